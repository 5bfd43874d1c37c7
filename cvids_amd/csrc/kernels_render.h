// kernels_render.h -- depth, normals and colours of the TSDF as a camera at a given pose sees it (chisel_hip_render_view).
//
// Not a kernel of the reference: a ray march whose every sample is ChunkManager::GetSDF (ChunkManager.cpp:476-499, as kernels_mesh.h:
// get_sdf<N> restates it) and whose hit is shaded by the mesher's own device functions.  DESIGN.md "Rendering a view" is the definition;
// in short, for pixel (col, row), all in fp32, in the order written, no FMA:
//     xc = ((float)col + 0.5f - cx) / fx,  yc = ((float)row + 0.5f - cy) / fy,  d_i = (r_i0 xc + r_i1 yc) + r_i2,  o_i = pose[i][3]
//     z_k = near + (float)k step  (k = 0 .. K-1: from k, never accumulated),  p_k = o + z_k d,  s_k = GetSDF(p_k) or "unobserved"
//     the ray ENDS at the first k with s_k observed and <= 0; it is a HIT iff sample k-1 is observed with s_{k-1} > 0; then
//     z* = z_{k-1} + step (s_{k-1} / (s_{k-1} - s_k)); every other pixel is NaN.
// The result is a function of that sample sequence alone.  What the kernel does NOT evaluate:
//   * Samples inside an absent chunk are unobserved by definition, so a lane that finds itself in one may jump over them.  Every step
//     from k to a chunk coordinate -- (float)k step, near + ., z d_i, o_i + ., . rf_chunk, floorf -- is a monotone function of its
//     argument under round-to-nearest, so each chunk coordinate is monotone in k: if samples k and k' > k lie in the same chunk, so does
//     every sample between them.  The lane estimates where the ray leaves the chunk, evaluates the chunk id of the sample just before
//     that, and jumps only when it equals the id it is in: the estimate may be as rough as it likes, the test is exact.  Because z_k comes
//     from k, the samples behind a jump have the bits they have in a march that took every step: skipped and full march agree bit for bit.
//     A jump leaves "the previous sample is unobserved" behind it, which is what the sample in front of the first observed one must say.
//   * For the same reason a ray that has left the box of all chunk ids ever created (MC_BBOX) on an axis along which it moves further
//     out meets absent chunks only: it never ends, and stops there.
//   * A lane keeps the id and slot of the chunk it was last in; the hash is probed when the id changes, about once per N samples.
// One sample per step: addressing the voxels of 2, 4 or 8 consecutive samples first and requesting their weights and distances together
// (as get_sdf_and_gradient does with its seven) was measured and is SLOWER here (EXPERIMENTS.md): at 7 waves per SIMD the other waves
// cover a lane's round trip, and the lanes of a batch address samples behind their ray's end.
// A wave is an 8 x 8 pixel tile (a 256-thread block: 16 x 16), so that its lanes walk the same chunks and neighbouring voxel rows, and
// leaves when all its lanes have ended.  No LDS, no atomics; the map is only read.
#pragma once
#include "kernels_mesh.h"

namespace chisel_hip {

#ifndef RENDER_SKIP
#define RENDER_SKIP 1  // jump over the samples of absent chunks (0: the full march, for the A/B of EXPERIMENTS.md -- same bits)
#endif
constexpr int RENDER_MAX_SAMPLES = 65536;

struct RenderCamera {
    float pose[12];  // camera -> world, row-major 3 x 4
    float fx, fy, cx, cy;
    float near_plane, step;
    int width, height;
    int n_samples;   // K
};

// the voxel GetSDF reads for `p`: ok = chunk resident and linear voxel id in range; (cix, ciy, ciz, cslot): the chunk this lane was last in
template <int N>
__device__ inline bool render_locate(const MapView &M, const MeshParams &P, f3v p, int &cix, int &ciy, int &ciz, int &cslot, size_t &off) {
    int ix, iy, iz;
    id_at(P, p, ix, iy, iz);
    if (ix != cix || iy != ciy || iz != ciz || cslot == -2) {
        cix = ix; ciy = iy; ciz = iz;
        const bool outside = ix < -ID_BIAS + 2 || ix > ID_BIAS - 2 || iy < -ID_BIAS + 2 || iy > ID_BIAS - 2 || iz < -ID_BIAS + 2 || iz > ID_BIAS - 2;  // chunk_at's guard
        cslot = outside ? -1 : hash_find_quiescent(M, ix, iy, iz);
    }
    off = 0;
    if (cslot < 0) return false;
    const f3v origin = mk3((float)(N * ix) * P.res, (float)(N * iy) * P.res, (float)(N * iz) * P.res);  // Chunk.cpp:43
    const f3v rel = sub3(p, origin);
    const int vx = (int)floorf(rel.x * P.rf_voxel), vy = (int)floorf(rel.y * P.rf_voxel), vz = (int)floorf(rel.z * P.rf_voxel);
    const int id = (vz * N + vy) * N + vx;
    if (id < 0 || id >= N * N * N) return false;  // (only the linear id is range-checked: Chunk.h:81-84)
    off = (size_t)cslot * (N * N * N) + id;
    return true;
}

template <int N>
__global__ __launch_bounds__(256) void render_view_kernel(MapView M, MeshParams P, RenderCamera C, float *__restrict__ depth, float *__restrict__ normals,
                                                          float *__restrict__ colors) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), row = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = col < C.width && row < C.height;
    const float xc = ((float)col + 0.5f - C.cx) / C.fx, yc = ((float)row + 0.5f - C.cy) / C.fy;
    const f3v d = mk3((C.pose[0] * xc + C.pose[1] * yc) + C.pose[2], (C.pose[4] * xc + C.pose[5] * yc) + C.pose[6], (C.pose[8] * xc + C.pose[9] * yc) + C.pose[10]);
    const f3v o = mk3(C.pose[3], C.pose[7], C.pose[11]);
    const int K = C.n_samples;
    const float step = C.step, near_plane = C.near_plane;
    auto z_of = [&](int k) -> float { return near_plane + (float)k * step; };
    auto p_of = [&](float z) -> f3v { return mk3(o.x + z * d.x, o.y + z * d.y, o.z + z * d.z); };
    // for the estimate of a chunk's far side only (never for a result): 1 / d_i, the chunk's edge
    const float big = 3.0e38f;
    const f3v inv = mk3(d.x != 0.0f ? __frcp_rn(d.x) : big, d.y != 0.0f ? __frcp_rn(d.y) : big, d.z != 0.0f ? __frcp_rn(d.z) : big);
    const float edge = (float)N * P.res, inv_step = __frcp_rn(step);

    // the box of every chunk id ever created (MC_BBOX: a superset of what is resident); every id where the map keeps none
    int bb[6] = {-ID_BIAS, -ID_BIAS, -ID_BIAS, ID_BIAS, ID_BIAS, ID_BIAS};
    if (M.mesh_ctl) {
#pragma unroll
        for (int i = 0; i < 6; i++) bb[i] = M.mesh_ctl[MC_BBOX + i];
    }

    bool done = !inside, hit = false;
    bool prev_obs = false;
    float prev_s = 0.0f, z_hit = 0.0f;
    int k = 0;
    int cix = 0, ciy = 0, ciz = 0, cslot = -2;  // -2: nothing looked up yet
    while (__any(!done)) {
        if (done) continue;
        const f3v p = p_of(z_of(k));
        size_t off;
        const bool ok = render_locate<N>(M, P, p, cix, ciy, ciz, cslot, off);
        if (cslot < 0) {
            // an absent chunk: this sample is unobserved, and so is every sample up to the last one that has this chunk id
            prev_obs = false;
            int next = k + 1;
#if RENDER_SKIP
            // beyond the box of all chunks on an axis along which the ray moves further out (the coordinate is monotone in k): absent
            // chunks from here on, the ray never ends
            if ((cix > bb[3] && d.x >= 0.0f) || (cix < bb[0] && d.x <= 0.0f) || (ciy > bb[4] && d.y >= 0.0f) || (ciy < bb[1] && d.y <= 0.0f) ||
                (ciz > bb[5] && d.z >= 0.0f) || (ciz < bb[2] && d.z <= 0.0f))
                next = K;
            const float tx = d.x > 0.0f ? ((float)(cix + 1) * edge - p.x) * inv.x : (d.x < 0.0f ? ((float)cix * edge - p.x) * inv.x : big);
            const float ty = d.y > 0.0f ? ((float)(ciy + 1) * edge - p.y) * inv.y : (d.y < 0.0f ? ((float)ciy * edge - p.y) * inv.y : big);
            const float tz = d.z > 0.0f ? ((float)(ciz + 1) * edge - p.z) * inv.z : (d.z < 0.0f ? ((float)ciz * edge - p.z) * inv.z : big);
            const float far_side = fminf(fminf(tx, ty), tz) * inv_step - 1.0f;  // samples to the chunk's far side, one held back
            const int jump = far_side > 1.0f ? (int)fminf(far_side, (float)(K - 1 - k)) : 0;
            if (next < K && jump > 0) {
                int jx, jy, jz;
                id_at(P, p_of(z_of(k + jump)), jx, jy, jz);
                if (jx == cix && jy == ciy && jz == ciz) next = k + jump + 1;  // samples k .. k + jump share the chunk (monotone in k)
            }
#endif
            k = next;
            done = k >= K;  // the ray never ends
            continue;
        }
        const float w = M.wgt[off], s = M.sdf[off];
        const bool obs = ok && (double)w > 1e-12;
        if (obs && s <= 0.0f) {
            done = true;
            if (prev_obs && prev_s > 0.0f) {
                hit = true;
                z_hit = z_of(k - 1) + step * (prev_s / (prev_s - s));
            }
            continue;
        }
        prev_obs = obs;
        prev_s = s;
        k++;
        done = k >= K;  // the ray never ends
    }
    if (!inside) return;
    const float nan = __builtin_nanf("");
    const size_t px = (size_t)row * C.width + col;
    depth[px] = hit ? z_hit : nan;
    f3v nrm = mk3(nan, nan, nan), rgb = mk3(nan, nan, nan);
    if (hit && (normals || colors)) {
        const f3v ps = p_of(z_hit);
        if (normals) {  // shade_vertices_kernel's normal for p*
            double dist;
            f3v grad;
            if (get_sdf_and_gradient<N>(M, P, ps, 0, 0, 0, nullptr, dist, grad)) {
                const float mag = sqrtf(sum3f(grad.x * grad.x, grad.y * grad.y, grad.z * grad.z));
                if ((double)mag > 1e-12) nrm = scl3(grad, 1.0f / mag);
            }
        }
        if (colors) rgb = interpolate_color<N>(M, P, ps, 0, 0, 0, nullptr);
    }
    if (normals) {
        normals[3 * px] = nrm.x;
        normals[3 * px + 1] = nrm.y;
        normals[3 * px + 2] = nrm.z;
    }
    if (colors) {
        colors[3 * px] = rgb.x;
        colors[3 * px + 1] = rgb.y;
        colors[3 * px + 2] = rgb.z;
    }
}

}  // namespace chisel_hip
