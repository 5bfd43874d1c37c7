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

// a pinhole camera at a pose, and the ray of a pixel as the header states it: the one text render_view_kernel and align_terms_kernel share
struct PixelCamera {
    float pose[12];  // camera -> world, row-major 3 x 4
    float fx, fy, cx, cy;
};
__device__ inline f3v pixel_ray(const PixelCamera &C, int col, int row, f3v &o) {
    const float xc = ((float)col + 0.5f - C.cx) / C.fx, yc = ((float)row + 0.5f - C.cy) / C.fy;
    o = mk3(C.pose[3], C.pose[7], C.pose[11]);
    return mk3((C.pose[0] * xc + C.pose[1] * yc) + C.pose[2], (C.pose[4] * xc + C.pose[5] * yc) + C.pose[6], (C.pose[8] * xc + C.pose[9] * yc) + C.pose[10]);
}

struct RenderCamera {
    PixelCamera cam;
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

__device__ inline bool finite3(f3v a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }

// the box of every chunk id ever created (MC_BBOX: a superset of what is resident); every id where the map keeps none
__device__ inline void load_chunk_box(const MapView &M, int bb[6]) {
#pragma unroll
    for (int i = 0; i < 6; i++) bb[i] = i < 3 ? -ID_BIAS : ID_BIAS;
    if (M.mesh_ctl) {
#pragma unroll
        for (int i = 0; i < 6; i++) bb[i] = M.mesh_ctl[MC_BBOX + i];
    }
}

// The march for one ray: t_k = t_near + (float)k step (from k, never accumulated), p_k = o + t_k d, the direction as given.  The state
// of a lane, so that the loop around it is free to hand a lane its ray whenever it likes.
struct RayMarch {
    f3v o, d, inv;  // inv: for the estimate of a chunk's far side only (never for a result): 1 / d_i
    float t_near;
    int K, k;
    int cix, ciy, ciz, cslot;  // the chunk this lane was last in (-2: nothing looked up yet)
    bool prev_obs;
    float prev_s;
    int status;   // CHISEL_HIP_RAY_*: 0 no end, 1 hit, 2 ended behind a surface
    float t_hit;
};

// a ray of K samples, none taken yet
__device__ inline void ray_reset(RayMarch &R, f3v o, f3v d, float t_near, int K) {
    R.o = o;
    R.d = d;
    const float big = 3.0e38f;
    R.inv = mk3(d.x != 0.0f ? __frcp_rn(d.x) : big, d.y != 0.0f ? __frcp_rn(d.y) : big, d.z != 0.0f ? __frcp_rn(d.z) : big);
    R.t_near = t_near;
    R.K = K;
    R.k = 0;
    R.cix = R.ciy = R.ciz = 0;
    R.cslot = -2;
    R.prev_obs = false;
    R.prev_s = 0.0f;
    R.status = 0;
    R.t_hit = 0.0f;
}

// one sample (or one jump over the samples of an absent chunk); true when the ray has ended or taken all its samples.  The argument
// of the header for the jump holds for any o, d.  NONFINITE_UNOBSERVED: a sample with a non-finite component is unobserved and no chunk
// id is taken from it (DESIGN.md "Querying points and rays"; not part of "Rendering a view").
template <int N, bool NONFINITE_UNOBSERVED>
__device__ inline bool ray_step(RayMarch &R, const MapView &M, const MeshParams &P, float step, float inv_step, const int *bb) {
    const int K = R.K;
    if (R.k >= K) return true;
    const f3v o = R.o, d = R.d;
    const float t_near = R.t_near;
    auto t_of = [&](int k) -> float { return t_near + (float)k * step; };
    auto p_of = [&](float t) -> f3v { return mk3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z); };
    const int k = R.k;
    const f3v p = p_of(t_of(k));
    if (NONFINITE_UNOBSERVED && !finite3(p)) {  // (t_k d overflowed: no voxel contains the sample)
        R.prev_obs = false;
        R.k = k + 1;
        return k + 1 >= K;
    }
    size_t off;
    const bool ok = render_locate<N>(M, P, p, R.cix, R.ciy, R.ciz, R.cslot, off);
    if (R.cslot < 0) {
        // an absent chunk: this sample is unobserved, and so is every sample up to the last one that has this chunk id
        R.prev_obs = false;
        int next = k + 1;
#if RENDER_SKIP
        const int cix = R.cix, ciy = R.ciy, ciz = R.ciz;
        const float big = 3.0e38f, edge = (float)N * P.res;
        // beyond the box of all chunks on an axis along which the ray moves further out (the coordinate is monotone in k): absent
        // chunks from here on, the ray never ends
        if ((cix > bb[3] && d.x >= 0.0f) || (cix < bb[0] && d.x <= 0.0f) || (ciy > bb[4] && d.y >= 0.0f) || (ciy < bb[1] && d.y <= 0.0f) ||
            (ciz > bb[5] && d.z >= 0.0f) || (ciz < bb[2] && d.z <= 0.0f))
            next = K;
        const float tx = d.x > 0.0f ? ((float)(cix + 1) * edge - p.x) * R.inv.x : (d.x < 0.0f ? ((float)cix * edge - p.x) * R.inv.x : big);
        const float ty = d.y > 0.0f ? ((float)(ciy + 1) * edge - p.y) * R.inv.y : (d.y < 0.0f ? ((float)ciy * edge - p.y) * R.inv.y : big);
        const float tz = d.z > 0.0f ? ((float)(ciz + 1) * edge - p.z) * R.inv.z : (d.z < 0.0f ? ((float)ciz * edge - p.z) * R.inv.z : big);
        const float far_side = fminf(fminf(tx, ty), tz) * inv_step - 1.0f;  // samples to the chunk's far side, one held back (an estimate)
        const int jump = far_side > 1.0f ? (int)fminf(far_side, (float)(K - 1 - k)) : 0;
        if (next < K && jump > 0) {
            int jx, jy, jz;
            id_at(P, p_of(t_of(k + jump)), jx, jy, jz);
            if (jx == cix && jy == ciy && jz == ciz) next = k + jump + 1;  // samples k .. k + jump share the chunk (monotone in k): exact
        }
#endif
        R.k = next;
        return next >= K;  // the ray never ends
    }
    const float w = M.wgt[off], s = M.sdf[off];
    const bool obs = ok && (double)w > 1e-12;
    if (obs && s <= 0.0f) {
        R.status = 2;
        if (R.prev_obs && R.prev_s > 0.0f) {
            R.status = 1;
            R.t_hit = t_of(k - 1) + step * (R.prev_s / (R.prev_s - s));
        }
        return true;
    }
    R.prev_obs = obs;
    R.prev_s = s;
    R.k = k + 1;
    return k + 1 >= K;  // the ray never ends
}

// what a finished ray writes: t_hit, status (where asked for) and, at p* = o + t_hit d, shade_vertices_kernel's normal and colour
// (NaN without a hit)
template <int N>
__device__ inline void ray_write(const RayMarch &R, const MapView &M, const MeshParams &P, long long i, float *__restrict__ t_hit,
                                 unsigned char *__restrict__ status, float *__restrict__ normals, float *__restrict__ colors) {
    const float nan = __builtin_nanf("");
    const bool hit = R.status == 1;
    t_hit[i] = hit ? R.t_hit : nan;
    if (status) status[i] = (unsigned char)R.status;
    f3v nrm = mk3(nan, nan, nan), rgb = mk3(nan, nan, nan);
    if (hit && (normals || colors)) {
        const f3v ps = mk3(R.o.x + R.t_hit * R.d.x, R.o.y + R.t_hit * R.d.y, R.o.z + R.t_hit * R.d.z);
        if (normals) gradient_normal<N>(M, P, ps, 0, 0, 0, nullptr, nrm);
        if (colors) rgb = interpolate_color<N>(M, P, ps, 0, 0, 0, nullptr);
    }
    if (normals) {
        normals[3 * i] = nrm.x;
        normals[3 * i + 1] = nrm.y;
        normals[3 * i + 2] = nrm.z;
    }
    if (colors) {
        colors[3 * i] = rgb.x;
        colors[3 * i + 1] = rgb.y;
        colors[3 * i + 2] = rgb.z;
    }
}

// One pixel per lane in the tiles of the header: the pixel's ray, then the march and the shading every ray gets.  z is the march's t.
template <int N>
__global__ __launch_bounds__(256) void render_view_kernel(MapView M, MeshParams P, RenderCamera C, float *__restrict__ depth, float *__restrict__ normals,
                                                          float *__restrict__ colors) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), row = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = col < C.width && row < C.height;
    f3v o;
    const f3v d = pixel_ray(C.cam, col, row, o);
    int bb[6];
    load_chunk_box(M, bb);
    const float step = C.step, inv_step = __frcp_rn(step);
    RayMarch R;
    ray_reset(R, o, d, C.near_plane, C.n_samples);
    bool done = !inside;
    while (__any(!done)) {
        if (done) continue;
        done = ray_step<N, false>(R, M, P, step, inv_step, bb);
    }
    if (inside) ray_write<N>(R, M, P, (long long)row * C.width + col, depth, nullptr, normals, colors);
}

}  // namespace chisel_hip
