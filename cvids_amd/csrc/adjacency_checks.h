// adjacency_checks.h -- the host-side pieces of chisel_hip_mesh_adjacency, chisel_hip_mesh_vertex_normals and chisel_hip_smooth_mesh
// that call nothing of HIP (included by chisel_hip.hip for host_adjacency.h and kernels_adjacency.h and, on its own, by
// tests/adjacency_checks_check.cpp, which runs them under the address and undefined-behaviour sanitizers on the CPU): what the entries
// refuse about their arguments before the device is asked anything, the capacities and the valence limit against the totals, and the
// 64-bit arithmetic of the scratch against 2^31 - 1.  DESIGN.md 3.17 is the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "components_checks.h"  // components_size_refusal, COMPONENTS_TILE, COMPONENTS_MAX_INTS

namespace chisel_hip {

constexpr int MESH_MAX_INCIDENT = 32;        // the longest incidence row the entries take (marching cubes: at most 20)
constexpr int MESH_MAX_NEIGHBORS = 2 * MESH_MAX_INCIDENT;  // a triangle names at most two vertices beside v
constexpr int ADJACENCY_ROWS_THREADS = 64;   // vertices one workgroup of the row kernel stages in LDS (a lane each)
constexpr int MESH_FLAG_BOUNDARY = 1, MESH_FLAG_NONMANIFOLD = 2, MESH_FLAG_ISOLATED = 4, MESH_FLAGS_ALL = 7;
constexpr int ADJACENCY_HOST_WORDS = 16;     // 64-bit words the report kernel leaves in pinned memory (AC_*)
constexpr int AC_INVALID = 0, AC_INCIDENCES = 1, AC_MAX_INCIDENT = 2, AC_NEIGHBORS = 3, AC_MAX_NEIGHBORS = 4, AC_BOUNDARY = 5, AC_NONMANIFOLD = 6, AC_ISOLATED = 7,
              AC_PINNED = 8;

// a refusal: null = go on; *unsupported says which status the entry returns (CHISEL_HIP_ERR_UNSUPPORTED, else _INVALID)

// sizes and the index array, for all three entries: what the components refuse, and an index array whose un-compacted neighbour rows
// (two slots an incidence, three incidences a triangle) would not be addressed by an int
inline const char *adjacency_size_refusal(int64_t n_vertices, int64_t n_triangles, const void *indices, bool *unsupported) {
    if (const char *why = components_size_refusal(n_vertices, n_triangles, indices, unsupported)) return why;
    if (n_triangles > COMPONENTS_MAX_INTS / 6) {
        *unsupported = true;
        return "more than 2^31 - 1 neighbour slots";
    }
    return nullptr;
}

// chisel_hip_mesh_adjacency.  The size query: no output named.
inline bool adjacency_is_query(const void *tri_offsets, const void *tri_items, const void *nbr_offsets, const void *nbr_items, const void *vertex_flags) {
    return !tri_offsets && !tri_items && !nbr_offsets && !nbr_items && !vertex_flags;
}
inline const char *adjacency_request_refusal(int64_t n_vertices, int64_t n_triangles, const void *indices, const void *tri_offsets, int64_t capacity_incidence,
                                             const void *tri_items, const void *nbr_offsets, int64_t capacity_neighbors, const void *nbr_items,
                                             const void *vertex_flags, const void *totals, bool *unsupported) {
    if (const char *why = adjacency_size_refusal(n_vertices, n_triangles, indices, unsupported)) return why;
    if (capacity_incidence < 0 || capacity_neighbors < 0) return "a negative capacity";
    if (adjacency_is_query(tri_offsets, tri_items, nbr_offsets, nbr_items, vertex_flags) && !totals) return "the size query without totals";
    return nullptr;
}

// chisel_hip_mesh_vertex_normals: without normals it is the size query
inline const char *normals_request_refusal(int64_t n_vertices, int64_t n_triangles, const void *indices, const void *vertices, const void *normals, const void *totals,
                                           bool *unsupported) {
    if (const char *why = adjacency_size_refusal(n_vertices, n_triangles, indices, unsupported)) return why;
    if (!normals) return totals ? nullptr : "the size query without totals";
    if (n_vertices > 0 && !vertices) return "null vertices with normals asked for";
    return nullptr;
}

inline bool adjacency_finite(float x) { return x - x == 0.0f; }  // (neither an infinity nor a NaN)

// do [a, a + bytes) and [b, b + bytes) share a byte?
inline bool adjacency_overlap(const void *a, const void *b, uint64_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return bytes > 0 && (x <= y ? y - x < bytes : x - y < bytes);
}

// chisel_hip_smooth_mesh: without out_vertices (and out_normals) it is the size query
inline const char *smooth_request_refusal(int64_t n_vertices, int64_t n_triangles, const void *indices, const void *vertices, int64_t iterations, float lambda, float mu,
                                          int pin_flags, const void *out_vertices, const void *out_normals, const void *totals, bool *unsupported) {
    if (const char *why = adjacency_size_refusal(n_vertices, n_triangles, indices, unsupported)) return why;
    if (iterations < 0) return "negative iterations";
    if (!adjacency_finite(lambda) || !adjacency_finite(mu)) return "lambda and mu are finite";
    if (pin_flags < 0 || pin_flags > MESH_FLAGS_ALL) return "pin_flags outside 0 .. 7";
    if (out_normals && !out_vertices) return "normals out without vertices out";
    if (!out_vertices) return totals ? nullptr : "the size query without totals";
    if (n_vertices > 0 && !vertices) return "null vertices with vertices out";
    if (adjacency_overlap(vertices, out_vertices, (uint64_t)n_vertices * 12u)) return "out_vertices overlaps vertices";
    return nullptr;
}

// the valence limit, then the capacities: both are refused with the totals filled, so that the caller sees what was found
inline const char *adjacency_valence_refusal(int64_t max_incident) {
    return max_incident > MESH_MAX_INCIDENT ? "a vertex with more than MESH_MAX_INCIDENT = 32 incident triangles" : nullptr;
}
inline const char *adjacency_capacity_refusal(int64_t incidences, int64_t neighbors, int64_t capacity_incidence, const void *tri_items, int64_t capacity_neighbors,
                                              const void *nbr_items) {
    if (tri_items && capacity_incidence < incidences) return "the incidence capacity is below the incidences";
    if (nbr_items && capacity_neighbors < neighbors) return "the neighbour capacity is below the neighbours";
    return nullptr;
}

// launches of a smoothing call: a pass with lambda, and one with mu where mu is not 0, per iteration
constexpr int64_t smooth_passes(int64_t iterations, float mu) { return iterations * (mu != 0.0f ? 2 : 1); }
// does pass j of n (0-based) write the caller's array?  The last one does; the passes alternate backwards from it.
constexpr bool smooth_pass_writes_out(int64_t j, int64_t n) { return ((n - 1 - j) & 1) == 0; }

// the scratch of a call in ints: deg and cursor [V], both offset arrays [V + 1], the neighbour counts and the flags [V], the incidence
// items [3 T], the un-compacted neighbour rows [6 T], the tile sums and the tile maxima of a scan over V + 1 elements
constexpr int64_t adjacency_scan_tiles(int64_t n_vertices) { return components_tiles(n_vertices + 1); }
constexpr int64_t adjacency_scratch_ints(int64_t n_vertices, int64_t n_triangles) {
    return 4 * n_vertices + 2 * (n_vertices + 1) + 9 * n_triangles + 2 * adjacency_scan_tiles(n_vertices);
}

}  // namespace chisel_hip
