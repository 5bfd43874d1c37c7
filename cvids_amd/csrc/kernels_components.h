// kernels_components.h -- chisel_hip_mesh_components and chisel_hip_filter_mesh: the connected components of an indexed mesh's
// vertex graph, and the mesh without its small ones (the host side: host_components.h; the refusals, the tile and the largest
// component's key: components_checks.h; the definition: DESIGN.md 3.16).  Integers only.  A wait-free union-find, then counts,
// three prefix sums and the compaction -- every step a launch of its own on the map's stream, no host round trip between them; what
// a workgroup does together, the union and the triangle test are kernels_workgroup.h's:
//
//   components_init_kernel          a thread per vertex: parent[v] = v, both counts 0
//   components_hook_kernel          a thread per triangle: a VALID triangle (mesh_triangle) unites (a, b) and (a, c): union_unite
//   components_label_vertices_kernel   behind the hook's end parent[] is read-only: plain loads.  root_of[v], no path writes; + 1 to
//                                   vertex_count[root] (vector atomics on int32, one per wave and root: wave_count)
//   components_label_triangles_kernel  + 1 to tri_count[root_of[first id]] of a valid triangle, likewise; the invalid ones are counted
//   components_sums_kernel<F> / components_scan_sums_kernel / components_prefix_kernel<F>
//                                   reduce-then-scan of a flag F per element, COMPONENTS_TILE elements a workgroup: the tiles' sums,
//                                   one workgroup over the sums (scan_tile_sums; the total into a control word), the exclusive
//                                   prefix of every element.  F: is a root (the prefix is the component's NUMBER; the same pass takes
//                                   the 64-bit maximum of components_largest_key), is a kept vertex, is a kept triangle.  Nobody
//                                   waits for another workgroup's flag: no look-back.
//   components_write_*_kernel       vertex_component, triangle_component, the table (pinned memory)
//   filter_vertices_kernel / filter_triangles_kernel   the maps, the renumbered ids and the copied rows (32-bit words, bit for bit)
#pragma once
#include "kernels_workgroup.h"
#include "components_checks.h"

namespace chisel_hip {

static_assert(COMPONENTS_TILE == WORKGROUP_THREADS, "a tile is what one workgroup of kernels_workgroup.h takes");

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

__global__ __launch_bounds__(COMPONENTS_TILE) void components_init_kernel(ComponentsView X) {
    const long long v = tile_element();
    if (v >= X.V) return;
    X.parent[v] = (int)v;
    X.vertex_count[v] = 0;
    X.tri_count[v] = 0;
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_hook_kernel(ComponentsView X) {
    const long long t = tile_element();
    if (t >= X.T) return;
    int a, b, c;
    if (!mesh_triangle(X.indices, X.V, t, a, b, c)) return;
    union_unite(X.parent, a, b);
    union_unite(X.parent, a, c);
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_label_vertices_kernel(ComponentsView X) {
    const long long v = tile_element();
    const bool in = v < X.V;
    int r = 0;
    if (in) {
        r = (int)v;
        for (int p = X.parent[r]; p != r; p = X.parent[r]) r = p;
        X.root_of[v] = r;
    }
    wave_count(X.vertex_count, r, in);
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_label_triangles_kernel(ComponentsView X) {
    const long long t = tile_element();
    int a = 0, b, c;
    const bool in = t < X.T;
    const bool valid = in && mesh_triangle(X.indices, X.V, t, a, b, c);
    wave_count(X.tri_count, valid ? X.root_of[a] : 0, valid);
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
    return i < X.T && mesh_triangle(X.indices, X.V, i, a, b, c) && components_root_kept(X, X.root_of[a]);
}

template <int F>
__global__ __launch_bounds__(COMPONENTS_TILE) void components_sums_kernel(ComponentsView X) {
    const long long i = tile_element();
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
    const int run = scan_tile_sums(sums, n_tiles, s_wave);
    if (threadIdx.x == 0) ctl[word] = (unsigned long long)run;
}

template <int F>
__global__ __launch_bounds__(COMPONENTS_TILE) void components_prefix_kernel(ComponentsView X) {
    __shared__ int s_wave[COMPONENTS_TILE / 64];
    const long long i = tile_element();
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
    const long long v = tile_element();
    if (v < X.V) vertex_component[v] = X.number[X.root_of[v]];
}

__global__ __launch_bounds__(COMPONENTS_TILE) void components_write_triangles_kernel(ComponentsView X, int *__restrict__ triangle_component) {
    const long long t = tile_element();
    if (t >= X.T) return;
    int a, b, c;
    triangle_component[t] = mesh_triangle(X.indices, X.V, t, a, b, c) ? X.number[X.root_of[a]] : -1;
}

// table: 3 words a component -- root, vertices, valid triangles -- for the components below `rows`
__global__ __launch_bounds__(COMPONENTS_TILE) void components_write_table_kernel(ComponentsView X, long long *__restrict__ table, long long rows) {
    const long long v = tile_element();
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
    const long long v = tile_element();
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
    const long long t = tile_element();
    if (t >= X.T) return;
    int a, b, c;
    const bool kept = mesh_triangle(X.indices, X.V, t, a, b, c) && components_root_kept(X, X.root_of[a]);
    const int to = kept ? X.tri_prefix[t] : -1;
    if (triangle_map) triangle_map[t] = to;
    if (!kept || !out_indices) return;
    const size_t dst = 3 * (size_t)to;  // (a valid triangle's three vertices are in one component: all kept)
    out_indices[dst] = X.vertex_prefix[a];
    out_indices[dst + 1] = X.vertex_prefix[b];
    out_indices[dst + 2] = X.vertex_prefix[c];
}

}  // namespace chisel_hip
