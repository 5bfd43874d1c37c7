// kernels_workgroup.h -- what a workgroup of WORKGROUP_THREADS = 256 lanes does together, written once for the passes that need it:
// the exclusive scan and the maximum across the workgroup, a lane's element in a grid of 256-element tiles and the one-workgroup scan
// over such a grid's tile sums, the validity test of an indexed triangle, the wait-free union-find on an array in global memory with
// the per-wave counted add behind it, and report_words_kernel, the way of a few words to the host.  No pass's own kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace chisel_hip {

constexpr int WORKGROUP_THREADS = 256;  // (a multiple of 64: the scan and the maximum take one word of LDS a wave)

// The exclusive sum of `mine` over the lanes of a workgroup, and the workgroup's `total`.  EVERY lane of a WORKGROUP_THREADS workgroup
// calls it (a lane with nothing passes 0); s_wave: WORKGROUP_THREADS / 64 words of LDS.  The function owns both barriers around s_wave:
// one between the waves' sums and their readers, one behind the readers -- s_wave is free again on return, and what the workgroup
// wrote in front of the call can be read behind it.
template <class T>
__device__ inline T block_exclusive_scan(T mine, T *s_wave, T &total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    T incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WORKGROUP_THREADS / 64; w++) {
        before += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    __syncthreads();
    return before + incl - mine;
}

// the maximum of `mine` over the workgroup, in every lane (s_wave: one int a wave; both barriers are the function's, as above)
__device__ inline int block_max(int mine, int *s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine = max(mine, __shfl_xor(mine, o));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    int most = s_wave[0];
#pragma unroll
    for (int w = 1; w < WORKGROUP_THREADS / 64; w++) most = max(most, s_wave[w]);
    __syncthreads();
    return most;
}

// the element of this lane where a workgroup takes a tile of WORKGROUP_THREADS consecutive elements
__device__ inline long long tile_element() { return (long long)blockIdx.x * WORKGROUP_THREADS + (long long)threadIdx.x; }

// The middle step of a reduce-then-scan over such tiles, by every lane of its ONE workgroup: sums[b] = the sums of the tiles in front
// of b, exclusive and in place, WORKGROUP_THREADS tiles at a time with the sum carried from round to round. -> the grand total, in
// every lane.  With MAXES the largest of maxes[0 .. n_tiles) and 0 rides along, a lane's share of it into `most` (block_max makes
// it the workgroup's).  I: the type n_tiles is counted in.
template <bool MAXES = false, class T, class I>
__device__ inline T scan_tile_sums(T *__restrict__ sums, I n_tiles, T *s_wave, const T *__restrict__ maxes = nullptr, T *most = nullptr) {
    T run = 0;
    for (I base = 0; base < n_tiles; base += WORKGROUP_THREADS) {
        const I b = base + (I)threadIdx.x;
        const T mine = b < n_tiles ? sums[b] : 0;
        if constexpr (MAXES) *most = max(*most, b < n_tiles ? maxes[b] : 0);
        T total;
        const T before = block_exclusive_scan(mine, s_wave, total);
        if (b < n_tiles) sums[b] = run + before;
        run += total;
    }
    return run;
}

// the three ids of triangle t of an index array over V vertices, and whether all of them name a vertex -- the test every kernel
// makes before it uses one as an address
__device__ inline bool mesh_triangle(const int *indices, int V, long long t, int &a, int &b, int &c) {
    const int *p = indices + 3 * (size_t)t;
    a = p[0]; b = p[1]; c = p[2];
    return (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
}

// ---- a wait-free union-find on parent[] in global memory, while other workgroups unite in the same array ---------------------------
// find walks to the root; the link is a compare-and-swap on the LARGER root that expects the root itself and writes the smaller one,
// retried from fresh finds when it loses.  A link only ever points from a larger id to a smaller: every tree's root is its minimum,
// and the final partition and its roots do not depend on the order of execution.  EVERY access to parent[] here is an agent-scope
// relaxed atomic: a CU's L1 and another XCD's L2 are not refreshed by other CUs' stores, so a plain load could stay stale for the
// kernel's life.  No thread waits for another: the find walk is bounded by the tree's depth (ids strictly decrease along it) and a
// compare-and-swap fails only when another thread's has succeeded.  Behind the uniting kernel's end parent[] is read-only: plain loads.
__device__ inline int union_find_shared(int *parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;  // (p < x: bounded by the tree's depth)
    }
}
__device__ inline void union_unite(int *parent, int a, int b) {
    for (;;) {
        a = union_find_shared(parent, a);
        b = union_find_shared(parent, b);
        if (a == b) return;
        const int lo = min(a, b), hi = max(a, b);
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(&parent[hi], &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        // (lost: somebody else has linked hi, which is progress; a and b are still members of their sets)
    }
}

// + 1 to count[r] for every lane that is `active`; the lanes of a wave that name the same root add once between them (a mesh is mostly
// one component: a lane each would queue the whole array up at one word).  EVERY lane of the wave calls it.
__device__ inline void wave_count(int *count, int r, bool active) {
    unsigned long long todo = __ballot(active);
    while (todo) {  // (wave-uniform; every round retires its leader's lanes)
        const int leader = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(r, leader);
        const unsigned long long same = __ballot(active && r == r0);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&count[r0], (int)__popcll(same));
        todo &= ~same;
    }
}

// n words of device memory into pinned memory, by the lanes of one workgroup of any size: what the host reads after its wait
template <class T>
__global__ void report_words_kernel(const T *src, T *dst, int n) {
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) dst[i] = src[i];
}

}  // namespace chisel_hip
