// kernels_query.h -- the map read at a caller's own positions and along a caller's own rays (chisel_hip_query_points, chisel_hip_cast_rays).
//
// Not kernels of the reference.  Every value they return is one an existing device function defines: ChunkManager::GetSDF as
// kernels_mesh.h: get_sdf<N> restates it (through kernels_render.h: render_locate<N>, the same voxel with the weight beside it),
// get_sdf_and_gradient<N>, interpolate_color<N>, and the march of kernels_render.h itself (RayMarch, ray_step, ray_write) with the ray
// handed in instead of derived from a pixel.  DESIGN.md "Querying points and rays" is the definition; the map is only read, no LDS, no atomics.
#pragma once
#include "kernels_render.h"

namespace chisel_hip {

struct QueryRay {  // = chisel_hip_ray: two 16-byte words
    float ox, oy, oz, dx;
    float dy, dz, t_near, t_far;
};
static_assert(sizeof(QueryRay) == 32, "chisel_hip_ray is 32 bytes");

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

// The ray as given, with K_r = floorf((t_far - t_near) / step) + 1 capped at RENDER_MAX_SAMPLES, 0 where the quotient is negative or
// NaN -- and for a ray with a non-finite origin, direction or t_near, whose samples no voxel contains
__device__ inline void ray_begin(RayMarch &R, const QueryRay &r, float step) {
    const f3v o = mk3(r.ox, r.oy, r.oz), d = mk3(r.dx, r.dy, r.dz);
    const float q = floorf((r.t_far - r.t_near) / step);
    int K = q >= 0.0f ? (int)fminf(q, (float)(RENDER_MAX_SAMPLES - 1)) + 1 : 0;
    if (!finite3(o) || !finite3(d) || !__builtin_isfinite(r.t_near)) K = 0;
    ray_reset(R, o, d, r.t_near, K);
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
    int bb[6];
    load_chunk_box(M, bb);
    const float inv_step = __frcp_rn(step);
    RayMarch R;
    ray_begin(R, load_ray(rays, inside ? i : 0), step);
    bool done = !inside;
    while (__any(!done)) {
        if (done) continue;
        done = ray_step<N, true>(R, M, P, step, inv_step, bb);
    }
    if (inside) ray_write<N>(R, M, P, i, t_hit, status, normals, colors);
}

}  // namespace chisel_hip
