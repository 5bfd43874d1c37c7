// kernels_align.h -- the Gauss-Newton terms of a depth frame against the TSDF (chisel_hip_align_terms, chisel_hip_align_depth).
//
// Not kernels of the reference.  DESIGN.md "Aligning a frame to the map" is the definition; in short, per pixel i = row W + col with
// z = depth[i], fp32 in the order written, no FMA:
//     valid    z finite and near <= z <= far
//     p        o + z d, with o and d chisel_hip_render_view's ray of the pixel (kernels_render.h: pixel_ray)
//     ok, d0, g  get_sdf_and_gradient<N>(p), called unchanged (a p with a non-finite component is not looked up: not ok)
//     rho      d0 + ((g.x e.x + g.y e.y) + g.z e.z),  e = p - c,  c = floorf(p / r) r + r / 2 (the voxel centre the distance is read at)
//     used     valid and ok and (max_residual <= 0 or |rho| <= max_residual)
// and in double from the floats widened: J = (g, p x g), the 30 sums of ALIGN_SUMS below; a pixel that is not used adds +0.0.
// Every sum has ONE order, a pairwise tree over groups of 256 values in pixel order (padded with +0.0): neighbours x[2j] + x[2j+1]
// eight times, then the same over the group results.  The first level is a block of align_terms_kernel, every further level a launch
// of align_reduce_kernel; no atomics, so the 32 doubles are the same bits on every run.
//
// The tree inside a block goes through LDS instead of 30 x 6 cross-lane exchanges of a double: the block's values of up to 8 sums are
// written side by side, a thread adds 8 neighbours of one sum (three levels in registers), and one thread per sum adds the 32 results
// (five levels).  tree_sum is the tree of the definition because a group of 2^k neighbours is a subtree of it.
#pragma once
#include "kernels_query.h"

namespace chisel_hip {

constexpr int ALIGN_SUMS = 30;    // [0..20] upper triangle of J J^T, [21..26] J rho, [27] rho^2, [28] used pixels, [29] valid pixels
constexpr int ALIGN_TERMS = 32;   // chisel_hip_align_terms' output: the sums, then two zeros
constexpr int ALIGN_PASS = 8;     // sums that share the LDS at a time
constexpr int ALIGN_ROW = 320;    // doubles per sum in the LDS: 256 values, two doubles of padding after every 8 (a thread's 8 values
                                  // are read as four 16-byte words: with rows of 80 bytes the 16 lanes of a read hit 16 different slots)

struct AlignCamera {
    PixelCamera cam;
    float near_plane, far_plane, max_residual;
    int width;
};

// x[0] + ... + x[n-1] as the pairwise tree over neighbours (n a power of two)
template <int n>
__device__ inline double tree_sum(const double *x) {
    if constexpr (n == 1) {
        return x[0];
    } else {
        return tree_sum<n / 2>(x) + tree_sum<n / 2>(x + n / 2);
    }
}

// One thread per pixel, 256 pixels per block in pixel order; partials[s * n_groups + blockIdx.x] = the block's tree sum of sum s.
template <int N>
__global__ __launch_bounds__(256) void align_terms_kernel(MapView M, MeshParams P, AlignCamera C, const float *__restrict__ depth, int n,
                                                          double *__restrict__ partials, int n_groups) {
    __shared__ double buf[ALIGN_PASS][ALIGN_ROW];
    __shared__ double part[ALIGN_PASS][32];
    const int tid = threadIdx.x;
    const int i = (int)blockIdx.x * 256 + tid;
    const bool inside = i < n;
    const float z = inside ? depth[i] : __builtin_nanf("");
    const bool valid = __builtin_isfinite(z) && C.near_plane <= z && z <= C.far_plane;
    const int row = i / C.width, col = i - row * C.width;
    f3v o;
    const f3v d = pixel_ray(C.cam, col, row, o);
    const f3v p = mk3(o.x + z * d.x, o.y + z * d.y, o.z + z * d.z);
    bool used = false;
    float rho = 0.0f;
    f3v g = mk3(0.0f, 0.0f, 0.0f);
    if (valid && finite3(p)) {
        double dist;
        if (get_sdf_and_gradient<N>(M, P, p, 0, 0, 0, nullptr, dist, g)) {
            const float r = P.res;
            const f3v c = mk3(floorf(p.x / r) * r + r / 2.0f, floorf(p.y / r) * r + r / 2.0f, floorf(p.z / r) * r + r / 2.0f);  // get_sdf_and_gradient's posf
            const f3v e = sub3(p, c);
            rho = (float)dist + ((g.x * e.x + g.y * e.y) + g.z * e.z);
            used = !(C.max_residual > 0.0f) || fabsf(rho) <= C.max_residual;
        }
    }
    const double gx = (double)g.x, gy = (double)g.y, gz = (double)g.z, px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    double J[6] = {gx, gy, gz, py * gz - pz * gy, pz * gx - px * gz, px * gy - py * gx};
    const double rd = (double)rho;
    double T[ALIGN_SUMS];
    {
        int t = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) T[t++] = used ? J[a] * J[b] : 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) T[21 + a] = used ? J[a] * rd : 0.0;
        T[27] = used ? rd * rd : 0.0;
        T[28] = used ? 1.0 : 0.0;
        T[29] = valid ? 1.0 : 0.0;
    }
    const int slot = tid + 2 * (tid >> 3);  // < 256 + 2 * 31 + 2 = ALIGN_ROW
    const int k = tid >> 5, s = tid & 31;   // second step: sum k of the pass, values 8 s .. 8 s + 7
#pragma unroll
    for (int base = 0; base < ALIGN_SUMS; base += ALIGN_PASS) {
        const int count = ALIGN_SUMS - base < ALIGN_PASS ? ALIGN_SUMS - base : ALIGN_PASS;
#pragma unroll
        for (int t = 0; t < count; t++) buf[t][slot] = T[base + t];
        __syncthreads();
        if (k < count) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = buf[k][10 * s + j];
            part[k][s] = tree_sum<8>(v);
        }
        __syncthreads();  // (buf is free for the next pass; part is written again only behind that pass's first barrier)
        if (tid < count) {
            double v[32];
#pragma unroll
            for (int j = 0; j < 32; j++) v[j] = part[tid][j];
            partials[(size_t)(base + tid) * n_groups + blockIdx.x] = tree_sum<32>(v);
        }
    }
}

// One further level: block (g, s) adds values 256 g .. 256 g + 255 of sum s (in[s * n_in + .], +0.0 behind the end) as the same tree;
// out[s * n_out + g] with n_out = gridDim.x.
__global__ __launch_bounds__(256) void align_reduce_kernel(const double *__restrict__ in, int n_in, double *__restrict__ out) {
    __shared__ double buf[ALIGN_ROW];
    __shared__ double part[32];
    const int tid = threadIdx.x, sum = blockIdx.y;
    const int i = (int)blockIdx.x * 256 + tid;
    buf[tid + 2 * (tid >> 3)] = i < n_in ? in[(size_t)sum * n_in + i] : 0.0;
    __syncthreads();
    if (tid < 32) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = buf[10 * tid + j];
        part[tid] = tree_sum<8>(v);
    }
    __syncthreads();
    if (tid == 0) {
        double v[32];
#pragma unroll
        for (int j = 0; j < 32; j++) v[j] = part[j];
        out[(size_t)sum * gridDim.x + blockIdx.x] = tree_sum<32>(v);
    }
}

}  // namespace chisel_hip
