// kernels_adjacency.h -- chisel_hip_mesh_adjacency, chisel_hip_mesh_vertex_normals and chisel_hip_smooth_mesh: the vertex -> triangle
// incidence and the vertex -> vertex neighbour rows of an indexed mesh's index array, and the two per-vertex passes that walk them (the
// host side: host_adjacency.h; the refusals, the valence limit and the scratch arithmetic: adjacency_checks.h; the definition:
// DESIGN.md 3.17).  Every step is a launch of its own on the map's stream, nothing crosses workgroups inside a kernel, and no float is
// ever added atomically: the rows are SORTED before a float is summed along them, so every sum has one order.
//
//   adjacency_count_kernel      a thread per triangle: a VALID triangle (mesh_triangle of kernels_workgroup.h) adds 1 to deg[] of each
//                               DISTINCT id it names (int32 vector atomics); the invalid are counted
//   adjacency_sums_kernel / adjacency_scan_sums_kernel / adjacency_prefix_kernel
//                               a reduce-then-scan over tiles of COMPONENTS_TILE (scan_tile_sums in the middle) of an int per element,
//                               V + 1 elements (the last one 0: its prefix is the total, offsets[V]); the maximum rides in the same two
//                               passes, a tile's maximum beside a tile's sum: no atomic
//   adjacency_fill_kernel       a thread per triangle: a slot of each named row through the row's atomic cursor; the order inside a
//                               row is whatever the scheduling made it
//   adjacency_rows_kernel       a thread per vertex, its row staged in LDS ([item][lane]: a lane's column, no two lanes on one bank):
//                               sorts the <= MESH_MAX_INCIDENT triangles ascending and writes them back, collects the <= 2 other ids
//                               of each into a sorted list, whose runs are the neighbours and their counts c(v, u): the neighbour row
//                               (un-compacted, at 2 x the row's incidence offset), its length, the flags.  A row above the limit is
//                               left alone: the call is refused behind the wait.
//   adjacency_compact_kernel    the neighbour rows to their offsets in the caller's array
//   mesh_vertex_normals_kernel  a thread per vertex: the face normals of its row, added in ascending triangle order, normalised
//   mesh_smooth_pass_kernel     a thread per vertex: one umbrella step with factor f from P into Q; a pinned vertex is copied
#pragma once
#include "kernels_workgroup.h"
#include "adjacency_checks.h"  // (the tile is components_checks.h's COMPONENTS_TILE: WORKGROUP_THREADS, as kernels_components.h asserts)

namespace chisel_hip {

struct AdjacencyView {
    int V, T;                  // (V <= 2^31 - 1, 6 T too: adjacency_size_refusal)
    const int *indices;        // [3 T] the caller's, or its staged copy
    int *deg, *cursor;         // [V] incident triangles | the slots of the row handed out so far
    int *tri_off, *nbr_off;    // [V + 1]
    int *nbr_count, *flags;    // [V]
    int *tri_items;            // [3 T] the incidence rows, row v at tri_off[v]
    int *nbr_rows;             // [6 T] the neighbour rows, row v at 2 tri_off[v]
    int *sums, *maxes;         // [tiles of V + 1] a scan's tile sums, then their exclusive prefix | its tile maxima
    unsigned long long *ctl;   // [ADJACENCY_HOST_WORDS] AC_*
    int pin_flags;             // what chisel_hip_smooth_mesh pins (the other entries: 0, and nothing is counted)
    int count_pinned;
};

__global__ __launch_bounds__(COMPONENTS_TILE) void adjacency_count_kernel(AdjacencyView X) {
    const long long t = tile_element();
    int a, b, c;
    const bool in = t < X.T;
    const bool valid = in && mesh_triangle(X.indices, X.V, t, a, b, c);
    if (valid) {
        atomicAdd(&X.deg[a], 1);
        if (b != a) atomicAdd(&X.deg[b], 1);
        if (c != a && c != b) atomicAdd(&X.deg[c], 1);
    }
    const int invalid = __syncthreads_count(in && !valid);
    if (threadIdx.x == 0 && invalid) atomicAdd(&X.ctl[AC_INVALID], (unsigned long long)invalid);
}

// values[n] and one 0 behind them: a tile's sum and a tile's maximum (not an atomicMax a wave into a control word: a million vertices
// queue 8 800 of them up at that one word, 11 ns each -- 100 of a launch's 103 microseconds when it was measured)
__global__ __launch_bounds__(COMPONENTS_TILE) void adjacency_sums_kernel(const int *__restrict__ values, int n, int *__restrict__ sums, int *__restrict__ maxes) {
    __shared__ int s_wave[COMPONENTS_TILE / 64];
    const long long i = tile_element();
    const int mine = i < n ? values[i] : 0;
    int total;
    (void)block_exclusive_scan(mine, s_wave, total);
    const int most = block_max(mine, s_wave);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total;
        maxes[blockIdx.x] = most;
    }
}

// One workgroup.  The tiles' maxima beside their sums: sums[b] = the sums of the tiles in front of b; ctl[total_word] = the total
// (<= 2^31 - 1), ctl[max_word] = the largest element.
__global__ __launch_bounds__(COMPONENTS_TILE) void adjacency_scan_sums_kernel(int *__restrict__ sums, const int *__restrict__ maxes, int n_tiles,
                                                                              unsigned long long *__restrict__ ctl, int total_word, int max_word) {
    __shared__ int s_wave[COMPONENTS_TILE / 64];
    int most = 0;
    const int run = scan_tile_sums<true>(sums, n_tiles, s_wave, maxes, &most);
    most = block_max(most, s_wave);
    if (threadIdx.x == 0) {
        ctl[total_word] = (unsigned long long)run;
        ctl[max_word] = (unsigned long long)most;
    }
}

// prefix[i] = the values in front of element i, for i = 0 ... n (prefix[n]: the total)
__global__ __launch_bounds__(COMPONENTS_TILE) void adjacency_prefix_kernel(const int *__restrict__ values, int n, const int *__restrict__ sums, int *__restrict__ prefix) {
    __shared__ int s_wave[COMPONENTS_TILE / 64];
    const long long i = tile_element();
    const int mine = i < n ? values[i] : 0;
    int total;
    const int at = sums[blockIdx.x] + block_exclusive_scan(mine, s_wave, total);
    if (i <= n) prefix[i] = at;
}

__global__ __launch_bounds__(COMPONENTS_TILE) void adjacency_fill_kernel(AdjacencyView X) {
    const long long t = tile_element();
    int a, b, c;
    if (t >= X.T || !mesh_triangle(X.indices, X.V, t, a, b, c)) return;
    // (the count kernel counted the same ids: a cursor stays below its row's length, a slot below 3 T)
    X.tri_items[X.tri_off[a] + atomicAdd(&X.cursor[a], 1)] = (int)t;
    if (b != a) X.tri_items[X.tri_off[b] + atomicAdd(&X.cursor[b], 1)] = (int)t;
    if (c != a && c != b) X.tri_items[X.tri_off[c] + atomicAdd(&X.cursor[c], 1)] = (int)t;
}

// u into the ascending list column[0 .. n) of this lane (equal ids stay: their run is c(v, u))
__device__ inline void adjacency_insert(int (*column)[ADJACENCY_ROWS_THREADS], int lane, int &n, int u) {
    int j = n++;
    for (; j > 0 && column[j - 1][lane] > u; j--) column[j][lane] = column[j - 1][lane];
    column[j][lane] = u;
}

__global__ __launch_bounds__(ADJACENCY_ROWS_THREADS) void adjacency_rows_kernel(AdjacencyView X) {
    __shared__ int s_tri[MESH_MAX_INCIDENT][ADJACENCY_ROWS_THREADS];
    __shared__ int s_nbr[MESH_MAX_NEIGHBORS][ADJACENCY_ROWS_THREADS];
    const int lane = (int)threadIdx.x;
    const long long v = (long long)blockIdx.x * ADJACENCY_ROWS_THREADS + lane;
    const bool in = v < X.V;
    int flags = 0, n_nbr = 0;
    if (in) {
        const int first = X.tri_off[v], d = X.tri_off[v + 1] - first;
        if (d == 0) flags = MESH_FLAG_ISOLATED;
        if (d > 0 && d <= MESH_MAX_INCIDENT) {  // (every loop below is bounded by the limit)
            int n = 0;
            for (int k = 0; k < d; k++) adjacency_insert(s_tri, lane, n, X.tri_items[first + k]);
            n = 0;
            for (int k = 0; k < d; k++) {
                const int t = s_tri[k][lane];
                X.tri_items[first + k] = t;
                int a, b, c;
                (void)mesh_triangle(X.indices, X.V, t, a, b, c);  // (a triangle of a row is valid)
                if (a != (int)v) adjacency_insert(s_nbr, lane, n, a);
                if (b != (int)v && b != a) adjacency_insert(s_nbr, lane, n, b);
                if (c != (int)v && c != a && c != b) adjacency_insert(s_nbr, lane, n, c);
            }
            int *row = X.nbr_rows + 2 * (size_t)first;
            for (int i = 0; i < n;) {
                const int u = s_nbr[i][lane];
                int j = i + 1;
                while (j < n && s_nbr[j][lane] == u) j++;
                if (j - i == 1) flags |= MESH_FLAG_BOUNDARY;
                if (j - i > 2) flags |= MESH_FLAG_NONMANIFOLD;
                row[n_nbr++] = u;
                i = j;
            }
        }
        X.nbr_count[v] = n_nbr;
        X.flags[v] = flags;
    }
    const int boundary = __syncthreads_count(in && (flags & MESH_FLAG_BOUNDARY)), nonmanifold = __syncthreads_count(in && (flags & MESH_FLAG_NONMANIFOLD)),
              isolated = __syncthreads_count(in && (flags & MESH_FLAG_ISOLATED)),
              pinned = __syncthreads_count(in && X.count_pinned && ((flags & X.pin_flags) || n_nbr == 0));
    if (threadIdx.x == 0) {
        if (boundary) atomicAdd(&X.ctl[AC_BOUNDARY], (unsigned long long)boundary);
        if (nonmanifold) atomicAdd(&X.ctl[AC_NONMANIFOLD], (unsigned long long)nonmanifold);
        if (isolated) atomicAdd(&X.ctl[AC_ISOLATED], (unsigned long long)isolated);
        if (pinned) atomicAdd(&X.ctl[AC_PINNED], (unsigned long long)pinned);
    }
}

__global__ __launch_bounds__(COMPONENTS_TILE) void adjacency_compact_kernel(AdjacencyView X, int *__restrict__ nbr_items) {
    const long long v = tile_element();
    if (v >= X.V) return;
    const int *row = X.nbr_rows + 2 * (size_t)X.tri_off[v];
    int *to = nbr_items + X.nbr_off[v];
    const int n = min(X.nbr_count[v], MESH_MAX_NEIGHBORS);
    for (int k = 0; k < n; k++) to[k] = row[k];
}

// DESIGN.md 3.17 VERTEX NORMALS: fp32, one operation per rounding (the library builds with -ffp-contract=off and IEEE divide / sqrt)
__global__ __launch_bounds__(COMPONENTS_TILE) void mesh_vertex_normals_kernel(AdjacencyView X, const float *__restrict__ P, float *__restrict__ normals) {
    const long long v = tile_element();
    if (v >= X.V) return;
    const int first = X.tri_off[v], d = min(X.tri_off[v + 1] - first, MESH_MAX_INCIDENT);
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (int k = 0; k < d; k++) {
        int i0, i1, i2;
        (void)mesh_triangle(X.indices, X.V, X.tri_items[first + k], i0, i1, i2);
        const float *p0 = P + 3 * (size_t)i0, *p1 = P + 3 * (size_t)i1, *p2 = P + 3 * (size_t)i2;
        const float pxx = p1[0] - p0[0], pxy = p1[1] - p0[1], pxz = p1[2] - p0[2];
        const float pyx = p2[0] - p0[0], pyy = p2[1] - p0[1], pyz = p2[2] - p0[2];
        ax = ax + (pxy * pyz - pxz * pyy);
        ay = ay + (pxz * pyx - pxx * pyz);
        az = az + (pxx * pyy - pxy * pyx);
    }
    const float len = sqrtf((ax * ax + ay * ay) + az * az);
    float *to = normals + 3 * (size_t)v;
    const bool some = len > 0.0f;
    to[0] = some ? ax / len : 0.0f;
    to[1] = some ? ay / len : 0.0f;
    to[2] = some ? az / len : 0.0f;
}

// DESIGN.md 3.17 SMOOTHING: one pass with factor f, P -> Q (never the same array)
__global__ __launch_bounds__(COMPONENTS_TILE) void mesh_smooth_pass_kernel(AdjacencyView X, const float *__restrict__ P, float *__restrict__ Q, float f) {
    const long long v = tile_element();
    if (v >= X.V) return;
    const int n = min(X.nbr_count[v], MESH_MAX_NEIGHBORS);
    const float *p = P + 3 * (size_t)v;
    float *q = Q + 3 * (size_t)v;
    if ((X.flags[v] & X.pin_flags) || n == 0) {  // pinned: the words as they are
        const unsigned *from = (const unsigned *)p;
        unsigned *to = (unsigned *)q;
        to[0] = from[0]; to[1] = from[1]; to[2] = from[2];
        return;
    }
    const int *row = X.nbr_rows + 2 * (size_t)X.tri_off[v];
    const float *u0 = P + 3 * (size_t)row[0];
    float mx = u0[0], my = u0[1], mz = u0[2];
    for (int k = 1; k < n; k++) {
        const float *u = P + 3 * (size_t)row[k];
        mx = mx + u[0]; my = my + u[1]; mz = mz + u[2];
    }
    const float count = (float)n;
    mx = mx / count; my = my / count; mz = mz / count;
    const float dx = mx - p[0], dy = my - p[1], dz = mz - p[2];
    const float sx = f * dx, sy = f * dy, sz = f * dz;
    q[0] = p[0] + sx; q[1] = p[1] + sy; q[2] = p[2] + sz;
}

}  // namespace chisel_hip
