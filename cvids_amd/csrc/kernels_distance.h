// kernels_distance.h -- the distance to the nearest obstacle over a window of voxels (chisel_hip_distance_field): a truncated, exact
// Euclidean distance transform in squared voxel units, seeded from the chunk hash.
//
// Not kernels of the reference.  DESIGN.md 3.11 "Distance field" is the definition; in short, with g = chunk_id * N + voxel_coordinate
// the global index of a voxel per axis: a voxel is UNKNOWN (0) when its chunk is not resident, lies outside the ids the look-up
// accepts, or its weight fails GetSDF's rule, OCCUPIED (2) when it is observed with sdf < surface_offset (one fp32 compare), FREE (1)
// otherwise; obstacles are the occupied voxels, with the flag the unknown ones too; dist2[v] = min |v - o|^2 over the obstacles o of the
// MAP with |v - o|^2 <= R^2, -1 without one.  Integers throughout: any decomposition gives the same answer.  This one:
//   distance_seed_kernel<N>   classifies the window widened by R on every side.  A wave is a run of 64 voxels along x, so the chunk
//                             look-up is wave-uniform: one per chunk the run crosses (64 / N + 1 at most).  It writes the states of the
//                             window's own voxels and one obstacle bit per voxel of the widened window (__ballot: a 64-bit word per wave).
//   distance_x_kernel         g1(x) = d^2 to the nearest obstacle bit of the row within R, by count-leading / find-first on 64-bit
//                             extracts of the bit row: no loop over the radius.
//   distance_axis_kernel      g'(i) = min over |d| <= R of g(i + d) + d^2 along y, then along z (FINAL: thresholds at R^2, writes dist2
//                             and reads distance from the host's table).  A tile of 64 columns x (64 + 2 R) rows in LDS; a lane walks
//                             d = 0, 1, ... and stops at d^2 >= its best so far (exact: later terms cannot be smaller).
// 16-bit intermediates: a value above R^2 can never come back under the threshold, so every pass stores DIST_NONE for it and what is
// kept is at most 64^2.  No atomics; the map is only read.
#pragma once
#include "kernels_render.h"

namespace chisel_hip {

constexpr unsigned DIST_NONE = 0xFFFFu;  // "no obstacle within R so far"
constexpr int DIST_TILE = 64;            // outputs along the axis per workgroup of distance_axis_kernel

struct DistanceSeedArgs {
    int wo[3], wd[3];    // the widened window: first voxel (global index), extent
    int dims[3];         // the window itself; it starts at wo + R
    int R;
    int unknown_is_obstacle;
    float surface_offset;
    long long words_per_row;
};

template <int N>
struct DistanceLog2 {
    static constexpr int value = N == 8 ? 3 : N == 16 ? 4 : 5;
    static_assert(N == 8 || N == 16 || N == 32, "chunk edge");
};

// the slot of the chunk `id`, -1 where it is absent: outside the ids the look-up accepts (render_locate's guard), outside the box of
// every id ever created, or not in the hash
__device__ inline int distance_chunk_slot(const MapView &M, const int bb[6], int cx, int cy, int cz) {
    const bool outside = cx < -ID_BIAS + 2 || cx > ID_BIAS - 2 || cy < -ID_BIAS + 2 || cy > ID_BIAS - 2 || cz < -ID_BIAS + 2 || cz > ID_BIAS - 2;
    if (outside) return -1;
    if (cx < bb[0] || cy < bb[1] || cz < bb[2] || cx > bb[3] || cy > bb[4] || cz > bb[5]) return -1;
    return hash_find_quiescent(M, cx, cy, cz);
}

// One wave per run of 64 voxels along x of the widened window, four runs per workgroup.
template <int N>
__global__ __launch_bounds__(256) void distance_seed_kernel(MapView M, DistanceSeedArgs A, long long n_runs, unsigned char *__restrict__ state,
                                                            unsigned long long *__restrict__ bits) {
    constexpr int LOG = DistanceLog2<N>::value;
    const int lane = threadIdx.x & 63;
    const long long run = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (run >= n_runs) return;  // (the whole wave)
    const long long row = run / A.words_per_row;
    const int word = (int)(run - row * A.words_per_row);
    const int wy = (int)(row % A.wd[1]), wz = (int)(row / A.wd[1]);
    const int wx0 = word * 64, wx = wx0 + lane;
    const int gx0 = A.wo[0] + wx0, gx = gx0 + lane, gy = A.wo[1] + wy, gz = A.wo[2] + wz;  // (|g| <= 2^30 + 63: no overflow)
    const int cy = gy >> LOG, cz = gz >> LOG;  // floor division: the shift of a negative int is arithmetic
    const int last = min(wx0 + 63, A.wd[0] - 1) - wx0;
    const int c_first = gx0 >> LOG, c_last = (gx0 + last) >> LOG, c_mine = gx >> LOG;
    int bb[6];
    load_chunk_box(M, bb);
    int slot = -1;
    for (int c = c_first; c <= c_last; c++) {  // (wave-uniform: at most 64 / N + 1 look-ups)
        const int s = distance_chunk_slot(M, bb, c, cy, cz);
        if (c == c_mine) slot = s;
    }
    const bool inside = wx < A.wd[0];
    unsigned st = 0;
    if (inside && slot >= 0) {
        const size_t off = (size_t)slot * (N * N * N) + (size_t)((((gz & (N - 1)) * N) + (gy & (N - 1))) * N + (gx & (N - 1)));
        const float w = M.wgt[off];
        if ((double)w > 1e-12) st = M.sdf[off] < A.surface_offset ? 2u : 1u;
    }
    const bool obstacle = inside && (st == 2u || (A.unknown_is_obstacle && st == 0u));
    const unsigned long long mask = __ballot(obstacle);
    if (bits && lane == 0) bits[run] = mask;
    if (state) {
        const int x = wx - A.R, y = wy - A.R, z = wz - A.R;
        if (x >= 0 && x < A.dims[0] && y >= 0 && y < A.dims[1] && z >= 0 && z < A.dims[2])
            state[((size_t)z * A.dims[1] + y) * A.dims[0] + x] = (unsigned char)st;
    }
}

// 64 bits of a bit row from bit `pos` on (bit i of the result = bit pos + i of the row); bits outside the row read as 0
__device__ inline unsigned long long distance_row_bits(const unsigned long long *__restrict__ row, long long n_words, int pos) {
    const int w = pos >> 6, s = pos & 63;  // (floor and its remainder, also for pos < 0)
    const unsigned long long lo = (w >= 0 && w < n_words) ? row[w] : 0ull;
    const unsigned long long hi = (w + 1 >= 0 && w + 1 < n_words) ? row[w + 1] : 0ull;
    return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// One thread per (x of the window, row of the widened window): the squared distance along x to the nearest obstacle bit within R
__global__ __launch_bounds__(256) void distance_x_kernel(const unsigned long long *__restrict__ bits, long long words_per_row, int nx, long long n, int R,
                                                         unsigned short *__restrict__ g1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long row = i / nx;
    const int x = (int)(i - row * nx);
    const unsigned long long *r = bits + row * words_per_row;
    const int p = x + R;  // the voxel's x in the widened window
    const unsigned long long right = distance_row_bits(r, words_per_row, p);        // p ... p + 63: bit d is the voxel at distance d
    const unsigned long long left = distance_row_bits(r, words_per_row, p - 64);    // p - 64 ... p - 1: bit 63 - (d - 1) is the voxel at distance d
    const unsigned long long far = distance_row_bits(r, words_per_row, p + 64) & 1ull;  // p + 64 (R = 64 reaches it)
    int d = 65;
    if (far) d = 64;
    if (right) d = __builtin_ctzll(right);
    if (left) d = min(d, __builtin_clzll(left) + 1);
    g1[i] = (unsigned short)(d <= R ? (unsigned)(d * d) : DIST_NONE);
}

// g'(a) = min over |d| <= R of g(a + d) + d^2 along an axis whose stride is the length X of the contiguous dimension: the pass along y
// (X = nx, `outer` = the planes of the widened z) and the pass along z (X = nx * ny, one outer).  The input has `La + 2 R` entries
// along the axis, the output La.  A workgroup: 64 columns x DIST_TILE outputs, a wave per output row, the tile of DIST_TILE + 2 R input
// rows in LDS (dynamic: (DIST_TILE + 2 R) * 64 * 2 bytes, 24 KiB at R = 64).
template <bool FINAL>
__global__ __launch_bounds__(256) void distance_axis_kernel(const unsigned short *__restrict__ in, unsigned short *__restrict__ out, int *__restrict__ dist2,
                                                            float *__restrict__ distance, const float *__restrict__ table, long long X, int La,
                                                            long long blocks_x, long long blocks_a, int R) {
    extern __shared__ unsigned short distance_tile[];  // [rows][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.x;
    const long long bx = b % blocks_x, rest = b / blocks_x;
    const long long ba = rest % blocks_a, o = rest / blocks_a;
    const long long x = bx * 64 + lane;
    const int a0 = (int)(ba * DIST_TILE);
    const int Lin = La + 2 * R;
    const int rows = min(DIST_TILE, La - a0) + 2 * R;  // input rows a0 ... a0 + rows - 1 (< Lin)
    const unsigned short *src = in + (size_t)o * Lin * X;
    for (int j = wave; j < rows; j += 4) distance_tile[j * 64 + lane] = x < X ? src[(size_t)(a0 + j) * X + x] : (unsigned short)DIST_NONE;
    __syncthreads();
    if (x >= X) return;
    const int R2 = R * R;
    for (int i = wave; i < rows - 2 * R; i += 4) {
        const unsigned short *c = distance_tile + (i + R) * 64 + lane;
        int best = (int)DIST_NONE;
        for (int d = 0; d <= R; d++) {
            const int dd = d * d;
            if (dd >= best) break;  // (every later term is at least d^2)
            const int v = min((int)c[-d * 64], (int)c[d * 64]) + dd;
            best = min(best, v);
        }
        const size_t at = ((size_t)o * La + (size_t)(a0 + i)) * X + x;
        if (!FINAL) {
            out[at] = (unsigned short)(best <= R2 ? (unsigned)best : DIST_NONE);
        } else {
            const bool none = best > R2;
            if (dist2) dist2[at] = none ? -1 : best;
            if (distance) distance[at] = none ? __builtin_inff() : table[best];
        }
    }
}

}  // namespace chisel_hip
