// kernels_query.h -- the map read at a caller's own positions and along a caller's own rays (chisel_hip_query_points, chisel_hip_cast_rays).
//
// Not kernels of the reference.  Every value they return is one an existing device function defines: ChunkManager::GetSDF as
// kernels_mesh.h: get_sdf<N> restates it (through kernels_render.h: render_locate<N>, the same voxel with the weight beside it),
// get_sdf_and_gradient<N>, interpolate_color<N>, and the march of kernels_render.h with the ray handed in instead of derived from a
// pixel.  DESIGN.md "Querying points and rays" is the definition; the map is only read, no LDS, no atomics.
#pragma once
#include "kernels_render.h"

namespace chisel_hip {

struct QueryRay {  // = chisel_hip_ray: two 16-byte words
    float ox, oy, oz, dx;
    float dy, dz, t_near, t_far;
};
static_assert(sizeof(QueryRay) == 32, "chisel_hip_ray is 32 bytes");

__device__ inline bool finite3(f3v a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }

// One thread per position.  Which outputs are asked for is the same for every lane (kernel arguments): what is not asked for is not
// computed.  found: bit 0 GetSDF(p), bit 1 GetSDFAndGradient(p) (only with `gradient`); a position with a non-finite component is
// answered without touching the map (found 0, NaN everywhere) -- the device functions themselves are called unchanged.
template <int N>
__global__ __launch_bounds__(256) void query_points_kernel(MapView M, MeshParams P, const float *__restrict__ positions, long long n,
                                                           unsigned char *__restrict__ found, float *__restrict__ sdf, float *__restrict__ weight,
                                                           float *__restrict__ gradient, float *__restrict__ colors) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3v p = mk3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]);
    const float nan = __builtin_nanf("");
    const bool finite = finite3(p);
    unsigned f = 0;
    if (found || sdf || weight) {
        float s = nan, w = nan;
        if (finite) {
            int cix = 0, ciy = 0, ciz = 0, cslot = -2;
            size_t off;
            if (render_locate<N>(M, P, p, cix, ciy, ciz, cslot, off)) {  // chunk resident, linear voxel id in range
                w = M.wgt[off];
                if ((double)w > 1e-12) {
                    f |= 1u;
                    s = M.sdf[off];
                }
            }
        }
        if (sdf) sdf[i] = s;
        if (weight) weight[i] = w;
    }
    if (gradient) {
        f3v g = mk3(nan, nan, nan);
        if (finite) {
            double dist;
            f3v grad;
            if (get_sdf_and_gradient<N>(M, P, p, 0, 0, 0, nullptr, dist, grad)) {
                f |= 2u;
                g = grad;
            }
        }
        gradient[3 * i] = g.x;
        gradient[3 * i + 1] = g.y;
        gradient[3 * i + 2] = g.z;
    }
    if (colors) {
        const f3v c = finite ? interpolate_color<N>(M, P, p, 0, 0, 0, nullptr) : mk3(nan, nan, nan);
        colors[3 * i] = c.x;
        colors[3 * i + 1] = c.y;
        colors[3 * i + 2] = c.z;
    }
    if (found) found[i] = (unsigned char)f;
}

// The march of render_view_kernel for one ray: t_k = t_near + (float)k step (from k, never accumulated), p_k = o + t_k d, the direction
// as given.  The state of a lane, so that the loop around it is free to hand a lane its ray whenever it likes.
struct RayMarch {
    f3v o, d, inv;
    float t_near;
    int K, k;
    int cix, ciy, ciz, cslot;  // the chunk this lane was last in (-2: nothing looked up yet)
    bool prev_obs;
    float prev_s;
    int status;   // CHISEL_HIP_RAY_*: 0 no end, 1 hit, 2 ended behind a surface
    float t_hit;
};

// K_r = floorf((t_far - t_near) / step) + 1 capped at RENDER_MAX_SAMPLES, 0 where the quotient is negative or NaN -- and for a ray with
// a non-finite origin, direction or t_near, whose samples no voxel contains
__device__ inline void ray_begin(RayMarch &R, const QueryRay &r, float step) {
    R.o = mk3(r.ox, r.oy, r.oz);
    R.d = mk3(r.dx, r.dy, r.dz);
    const float big = 3.0e38f;
    R.inv = mk3(R.d.x != 0.0f ? __frcp_rn(R.d.x) : big, R.d.y != 0.0f ? __frcp_rn(R.d.y) : big, R.d.z != 0.0f ? __frcp_rn(R.d.z) : big);
    R.t_near = r.t_near;
    const float q = floorf((r.t_far - r.t_near) / step);
    R.K = q >= 0.0f ? (int)fminf(q, (float)(RENDER_MAX_SAMPLES - 1)) + 1 : 0;
    if (!finite3(R.o) || !finite3(R.d) || !__builtin_isfinite(r.t_near)) R.K = 0;
    R.k = 0;
    R.cix = R.ciy = R.ciz = 0;
    R.cslot = -2;
    R.prev_obs = false;
    R.prev_s = 0.0f;
    R.status = 0;
    R.t_hit = 0.0f;
}

// one sample (or one jump over the samples of an absent chunk); true when the ray has ended or taken all its samples.  The body is
// render_view_kernel's, with K, o, d and t_near the lane's own: the argument of DESIGN.md "Rendering a view" for the jump holds for any o, d.
template <int N>
__device__ inline bool ray_step(RayMarch &R, const MapView &M, const MeshParams &P, float step, float inv_step, const int *bb) {
    const int K = R.K;
    if (R.k >= K) return true;
    const f3v o = R.o, d = R.d;
    const float t_near = R.t_near;
    auto t_of = [&](int k) -> float { return t_near + (float)k * step; };
    auto p_of = [&](float t) -> f3v { return mk3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z); };
    const int k = R.k;
    const f3v p = p_of(t_of(k));
    if (!finite3(p)) {  // (t_k d overflowed: no voxel contains the sample, and no chunk id is taken from it)
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
        if ((cix > bb[3] && d.x >= 0.0f) || (cix < bb[0] && d.x <= 0.0f) || (ciy > bb[4] && d.y >= 0.0f) || (ciy < bb[1] && d.y <= 0.0f) ||
            (ciz > bb[5] && d.z >= 0.0f) || (ciz < bb[2] && d.z <= 0.0f))
            next = K;  // beyond the box of all chunks on an axis along which the ray moves further out: the ray never ends
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
        return next >= K;
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
    return k + 1 >= K;
}

// what a finished ray writes: t_hit, status and, at p* = o + t_hit d, render_view_kernel's normal and colour (NaN without a hit)
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
        if (normals) {
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

__device__ inline QueryRay load_ray(const QueryRay *__restrict__ rays, long long i) {
    const float4 a = reinterpret_cast<const float4 *>(rays)[2 * i], b = reinterpret_cast<const float4 *>(rays)[2 * i + 1];
    return QueryRay{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

// One ray per lane, in the caller's order; a wave leaves when all its lanes have ended.  A lane's result is a function of its ray and
// the map alone: the chunk it keeps is its own, and nothing is shared between lanes.
template <int N>
__global__ __launch_bounds__(256) void cast_rays_kernel(MapView M, MeshParams P, const QueryRay *__restrict__ rays, long long n, float step,
                                                        float *__restrict__ t_hit, unsigned char *__restrict__ status, float *__restrict__ normals,
                                                        float *__restrict__ colors) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = i < n;
    int bb[6] = {-ID_BIAS, -ID_BIAS, -ID_BIAS, ID_BIAS, ID_BIAS, ID_BIAS};  // the box of every chunk id ever created (MC_BBOX)
    if (M.mesh_ctl) {
#pragma unroll
        for (int a = 0; a < 6; a++) bb[a] = M.mesh_ctl[MC_BBOX + a];
    }
    const float inv_step = __frcp_rn(step);
    RayMarch R;
    ray_begin(R, load_ray(rays, inside ? i : 0), step);
    bool done = !inside;
    while (__any(!done)) {
        if (done) continue;
        done = ray_step<N>(R, M, P, step, inv_step, bb);
    }
    if (inside) ray_write<N>(R, M, P, i, t_hit, status, normals, colors);
}

}  // namespace chisel_hip
