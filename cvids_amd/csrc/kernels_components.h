// kernels_components.h -- chisel_hip_mesh_components and chisel_hip_filter_mesh: the connected components of an indexed mesh's
// vertex graph, and the mesh without its small ones (the host side: host_components.h; the refusals, the tile and the largest
// component's key: components_checks.h; the definition: DESIGN.md 3.16).  Integers only.  A wait-free union-find, then counts,
// three prefix sums and the compaction -- every step a launch of its own on the map's stream, no host round trip between them:
//
//   components_init_kernel          a thread per vertex: parent[v] = v, both counts 0
//   components_hook_kernel          a thread per triangle: a VALID triangle (all three ids in [0, V), tested before any is used as
//                                   an address) unites (a, b) and (a, c).  find walks to the root; the link is a compare-and-swap on
//                                   the LARGER root that expects the root itself and writes the smaller one, retried from fresh finds
//                                   when it loses.  A link only ever points from a larger id to a smaller: every tree's root is its
//                                   minimum, and the final partition and its roots do not depend on the order of execution.  EVERY
//                                   access to parent[] in this kernel is an agent-scope relaxed atomic: a CU's L1 and another XCD's
//                                   L2 are not refreshed by other CUs' stores, so a plain load could stay stale for the kernel's
//                                   life.  No thread waits for another: the find walk is bounded by the tree's depth (ids strictly
//                                   decrease along it) and a compare-and-swap fails only when another thread's has succeeded.
//   components_label_vertices_kernel   behind the hook's end parent[] is read-only: plain loads.  root_of[v], no path writes; + 1 to
//                                   vertex_count[root] (vector atomics on int32, one per wave and root: components_count)
//   components_label_triangles_kernel  + 1 to tri_count[root_of[first id]] of a valid triangle, likewise; the invalid ones are counted
//   components_sums_kernel<F> / components_scan_sums_kernel / components_prefix_kernel<F>
//                                   reduce-then-scan of a flag F per element, COMPONENTS_TILE elements a workgroup: the tiles' sums,
//                                   one workgroup over the sums (exclusive, in place; the total into a control word), the exclusive
//                                   prefix of every element.  F: is a root (the prefix is the component's NUMBER; the same pass takes
//                                   the 64-bit maximum of components_largest_key), is a kept vertex, is a kept triangle.  Nobody
//                                   waits for another workgroup's flag: no look-back.
//   components_write_*_kernel       vertex_component, triangle_component, the table (pinned memory)
//   filter_vertices_kernel / filter_triangles_kernel   the maps, the renumbered ids and the copied rows (32-bit words, bit for bit)
//   components_report_kernel        the control words into pinned memory: what the host reads after its one wait
#pragma once
#include "kernels_coarse.h"  // block_exclusive_scan
#include "components_checks.h"

namespace chisel_hip {

static_assert(COMPONENTS_TILE == COARSE_THREADS, "block_exclusive_scan is written for COARSE_THREADS lanes");

struct ComponentsView {
    int V, T;                    // (both <= 2^31 - 1, 3 T too: components_size_refusal)
    const int *indices;          // [3 T] the caller's, or its staged copy
    int *parent, *root_of;       // [V]
    int *vertex_count, *tri_count;  // [V] per root
    int *number;                 // [V] roots in front of v: the number of the component whose root v is
    int *vertex_prefix;          // [V] kept vertices in front of v
    int *tri_prefix;             // [T] kept triangles in front of t
    int *sums;                   // [tiles of max(V, T)] a scan's tile sums, then their exclusive prefix
    unsigned long long *ctl;     // [COMPONENTS_HOST_WORDS] CC_*
    int min_triangles, largest_only;
};

enum { FLAG_ROOT = 0, FLAG_KEPT_VERTEX = 1, FLAG_KEPT_TRIANGLE = 2 };

__device__ inline long long components_element() { return (long long)blockIdx.x * COMPONENTS_TILE + (long long)threadIdx.x; }

// the three ids of triangle t, and whether all of them name a vertex -- the test every kernel makes before it uses one as an address
__device__ inline bool components_triangle(const ComponentsView &X, long long t, int &a, int &b, int &c) {
    const int *p = X.indices + 3 * (size_t)t;
    a = p[0]; b = p[1]; c = p[2];
    return (unsigned)a < (unsigned)X.V && (unsigned)b < (unsigned)X.V && (unsigned)c < (unsigned)X.V;
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_init_kernel(ComponentsView X) {
    const long long v = components_element();
    if (v >= X.V) return;
    X.parent[v] = (int)v;
    X.vertex_count[v] = 0;
    X.tri_count[v] = 0;
}

__device__ inline int components_find_shared(int *parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;  // (p < x: bounded by the tree's depth)
    }
}
__device__ inline void components_unite(int *parent, int a, int b) {
    for (;;) {
        a = components_find_shared(parent, a);
        b = components_find_shared(parent, b);
        if (a == b) return;
        const int lo = min(a, b), hi = max(a, b);
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(&parent[hi], &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        // (lost: somebody else has linked hi, which is progress; a and b are still members of their sets)
    }
}
__global__ __launch_bounds__(COMPONENTS_TILE) void components_hook_kernel(ComponentsView X) {
    const long long t = components_element();
    if (t >= X.T) return;
    int a, b, c;
    if (!components_triangle(X, t, a, b, c)) return;
    components_unite(X.parent, a, b);
    components_unite(X.parent, a, c);
}

// + 1 to count[r] for every lane that is `active`; the lanes of a wave that name the same root add once between them (a mesh is mostly
// one component: a lane each would queue the whole array up at one word).  EVERY lane of the wave calls it.
__device__ inline void components_count(int *count, int r, bool active) {
    unsigned long long todo = __ballot(active);
    while (todo) {  // (wave-uniform; every round retires its leader's lanes)
        const int leader = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(r, leader);
        const unsigned long long same = __ballot(active && r == r0);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&count[r0], (int)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_label_vertices_kernel(ComponentsView X) {
    const long long v = components_element();
    const bool in = v < X.V;
    int r = 0;
    if (in) {
        r = (int)v;
        for (int p = X.parent[r]; p != r; p = X.parent[r]) r = p;
        X.root_of[v] = r;
    }
    components_count(X.vertex_count, r, in);
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_label_triangles_kernel(ComponentsView X) {
    const long long t = components_element();
    int a = 0, b, c;
    const bool in = t < X.T;
    const bool valid = in && components_triangle(X, t, a, b, c);
    components_count(X.tri_count, valid ? X.root_of[a] : 0, valid);
    const int invalid = __syncthreads_count(in && !valid);
    if (threadIdx.x == 0 && invalid) atomicAdd(&X.ctl[CC_INVALID], (unsigned long long)invalid);
}

// is the component of root r kept?  (number[] and the largest key are complete: launches behind the root scan)
__device__ inline bool components_root_kept(const ComponentsView &X, int r) {
    if (X.tri_count[r] < X.min_triangles) return false;
    return !X.largest_only || (long long)X.number[r] == components_key_number(X.ctl[CC_LARGEST_KEY]);
}

template <int F>
__device__ inline bool components_flag(const ComponentsView &X, long long i) {
    if (F == FLAG_ROOT) return i < X.V && X.parent[i] == (int)i;
    if (F == FLAG_KEPT_VERTEX) return i < X.V && components_root_kept(X, X.root_of[i]);
    int a, b, c;
    return i < X.T && components_triangle(X, i, a, b, c) && components_root_kept(X, X.root_of[a]);
}

template <int F>
__global__ __launch_bounds__(COMPONENTS_TILE) void components_sums_kernel(ComponentsView X) {
    const long long i = components_element();
    const bool flag = components_flag<F>(X, i);
    const int sum = __syncthreads_count(flag);
    if (threadIdx.x == 0) X.sums[blockIdx.x] = sum;
    if (F == FLAG_KEPT_VERTEX) {  // (the kept components: the kept vertices that are roots)
        const int roots = __syncthreads_count(flag && X.parent[i] == (int)i);
        if (threadIdx.x == 0 && roots) atomicAdd(&X.ctl[CC_KEPT_COMPONENTS], (unsigned long long)roots);
    }
}

// One workgroup.  sums[b] = the sums of the tiles in front of b; ctl[word] = the total (<= 2^31 - 1: an element counts once).
__global__ __launch_bounds__(COMPONENTS_TILE) void components_scan_sums_kernel(int *__restrict__ sums, int n_tiles, unsigned long long *__restrict__ ctl, int word) {
    __shared__ int s_wave[COMPONENTS_TILE / 64];
    int run = 0;
    for (int base = 0; base < n_tiles; base += COMPONENTS_TILE) {
        const int b = base + (int)threadIdx.x;
        const int mine = b < n_tiles ? sums[b] : 0;
        int total;
        const int before = block_exclusive_scan(mine, s_wave, total);
        if (b < n_tiles) sums[b] = run + before;
        run += total;
    }
    if (threadIdx.x == 0) ctl[word] = (unsigned long long)run;
}

template <int F>
__global__ __launch_bounds__(COMPONENTS_TILE) void components_prefix_kernel(ComponentsView X) {
    __shared__ int s_wave[COMPONENTS_TILE / 64];
    const long long i = components_element();
    const bool flag = components_flag<F>(X, i);
    int total;
    const int at = X.sums[blockIdx.x] + block_exclusive_scan((int)flag, s_wave, total);
    int *out = F == FLAG_ROOT ? X.number : (F == FLAG_KEPT_VERTEX ? X.vertex_prefix : X.tri_prefix);
    if (i < (F == FLAG_KEPT_TRIANGLE ? X.T : X.V)) out[i] = at;
    if (F == FLAG_ROOT) {  // the largest component: a wave's maximum, one vector atomic a wave
        unsigned long long key = flag ? components_largest_key(X.tri_count[i], at) : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned hi = __shfl_xor((unsigned)(key >> 32), o), lo = __shfl_xor((unsigned)key, o);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            key = other > key ? other : key;
        }
        if ((threadIdx.x & 63) == 0 && key) atomicMax(&X.ctl[CC_LARGEST_KEY], key);
    }
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_write_vertices_kernel(ComponentsView X, int *__restrict__ vertex_component) {
    const long long v = components_element();
    if (v < X.V) vertex_component[v] = X.number[X.root_of[v]];
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_write_triangles_kernel(ComponentsView X, int *__restrict__ triangle_component) {
    const long long t = components_element();
    if (t >= X.T) return;
    int a, b, c;
    triangle_component[t] = components_triangle(X, t, a, b, c) ? X.number[X.root_of[a]] : -1;
}

// table: 3 words a component -- root, vertices, valid triangles -- for the components below `rows`
__global__ __launch_bounds__(COMPONENTS_TILE) void components_write_table_kernel(ComponentsView X, long long *__restrict__ table, long long rows) {
    const long long v = components_element();
    if (v >= X.V || X.parent[v] != (int)v) return;
    const long long row = X.number[v];
    if (row >= rows) return;
    table[3 * row] = v;
    table[3 * row + 1] = X.vertex_count[v];
    table[3 * row + 2] = X.tri_count[v];
}

// rows of 3 32-bit words: floats are copied as the words they are
__global__ __launch_bounds__(COMPONENTS_TILE) void filter_vertices_kernel(ComponentsView X, const unsigned *__restrict__ vertices, const unsigned *__restrict__ normals,
                                                                          const unsigned *__restrict__ colors, unsigned *__restrict__ out_vertices,
                                                                          unsigned *__restrict__ out_normals, unsigned *__restrict__ out_colors, int *__restrict__ vertex_map) {
    const long long v = components_element();
    if (v >= X.V) return;
    const bool kept = components_root_kept(X, X.root_of[v]);
    const int to = kept ? X.vertex_prefix[v] : -1;
    if (vertex_map) vertex_map[v] = to;
    if (!kept) return;
    const size_t src = 3 * (size_t)v, dst = 3 * (size_t)to;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (out_vertices) out_vertices[dst + k] = vertices[src + k];
        if (out_normals) out_normals[dst + k] = normals[src + k];
        if (out_colors) out_colors[dst + k] = colors[src + k];
    }
}

__global__ __launch_bounds__(COMPONENTS_TILE) void filter_triangles_kernel(ComponentsView X, int *__restrict__ out_indices, int *__restrict__ triangle_map) {
    const long long t = components_element();
    if (t >= X.T) return;
    int a, b, c;
    const bool kept = components_triangle(X, t, a, b, c) && components_root_kept(X, X.root_of[a]);
    const int to = kept ? X.tri_prefix[t] : -1;
    if (triangle_map) triangle_map[t] = to;
    if (!kept || !out_indices) return;
    const size_t dst = 3 * (size_t)to;  // (a valid triangle's three vertices are in one component: all kept)
    out_indices[dst] = X.vertex_prefix[a];
    out_indices[dst + 1] = X.vertex_prefix[b];
    out_indices[dst + 2] = X.vertex_prefix[c];
}

__global__ void components_report_kernel(const unsigned long long *__restrict__ ctl, long long *__restrict__ host) {
    if (threadIdx.x < COMPONENTS_HOST_WORDS) host[threadIdx.x] = (long long)ctl[threadIdx.x];
}

}  // namespace chisel_hip
