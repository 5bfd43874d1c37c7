// components_checks.h -- the host-side pieces of chisel_hip_mesh_components and chisel_hip_filter_mesh that call nothing of HIP
// (included by chisel_hip.hip for host_components.h and kernels_components.h and, on its own, by tests/components_checks_check.cpp,
// which runs them under the address and undefined-behaviour sanitizers on the CPU): what the entries refuse about their arguments
// before the device is asked anything, the capacities against the totals, and the 64-bit arithmetic of sizes, scan tiles and the
// largest component's key against 2^31 - 1.  DESIGN.md 3.16 is the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace chisel_hip {

constexpr int COMPONENTS_TILE = 256;       // elements one workgroup of the scans sums and prefixes (a lane each)
constexpr int COMPONENTS_HOST_WORDS = 8;   // 64-bit words the report kernel leaves in pinned memory (CC_*)
constexpr int CC_INVALID = 0, CC_COMPONENTS = 1, CC_LARGEST_KEY = 2, CC_KEPT_COMPONENTS = 3, CC_KEPT_VERTICES = 4, CC_KEPT_TRIANGLES = 5;
constexpr int64_t COMPONENTS_MAX_INTS = 0x7fffffffll;  // vertex ids, and entries of the index array

// a refusal: null = go on; *unsupported says which status the entry returns (CHISEL_HIP_ERR_UNSUPPORTED, else _INVALID)

// sizes and the index array, for both entries
inline const char *components_size_refusal(int64_t n_vertices, int64_t n_triangles, const void *indices, bool *unsupported) {
    *unsupported = false;
    if (n_vertices < 0 || n_triangles < 0) return "a negative size";
    *unsupported = true;
    if (n_vertices > COMPONENTS_MAX_INTS) return "more than 2^31 - 1 vertices";
    if (n_triangles > COMPONENTS_MAX_INTS / 3) return "more than 2^31 - 1 index entries";
    *unsupported = false;
    if (n_triangles > 0 && !indices) return "null indices with triangles";
    return nullptr;
}

// chisel_hip_mesh_components.  The size query: no label array and no table (a table with capacity 0 is none).
inline bool components_is_query(const void *vertex_component, const void *triangle_component, int64_t capacity_components, const void *component_table) {
    return !vertex_component && !triangle_component && !(component_table && capacity_components > 0);
}
inline const char *components_request_refusal(int64_t n_vertices, int64_t n_triangles, const void *indices, const void *vertex_component,
                                              const void *triangle_component, int64_t capacity_components, const void *component_table, const void *totals,
                                              bool *unsupported) {
    if (const char *why = components_size_refusal(n_vertices, n_triangles, indices, unsupported)) return why;
    if (capacity_components < 0) return "a negative capacity";
    if (capacity_components > 0 && !component_table) return "a table capacity without a table";
    if (components_is_query(vertex_component, triangle_component, capacity_components, component_table) && !totals) return "the size query without totals";
    return nullptr;
}

// chisel_hip_filter_mesh.  The size query: both capacities 0 -- nothing but totals is looked at behind it.
inline const char *filter_request_refusal(int64_t n_vertices, int64_t n_triangles, const void *indices, const void *vertices, const void *normals,
                                          const void *colors, int64_t min_triangles, int largest_only, int64_t capacity_vertices, int64_t capacity_triangles,
                                          const void *out_vertices, const void *out_indices, const void *out_normals, const void *out_colors, const void *totals,
                                          bool *unsupported) {
    if (const char *why = components_size_refusal(n_vertices, n_triangles, indices, unsupported)) return why;
    if (min_triangles < 1) return "min_triangles below 1";
    if (largest_only != 0 && largest_only != 1) return "largest_only is 0 or 1";
    if (capacity_vertices < 0 || capacity_triangles < 0) return "a negative capacity";
    if (capacity_vertices == 0 && capacity_triangles == 0) return totals ? nullptr : "the size query without totals";
    if (out_vertices && !vertices) return "vertices out without vertices in";
    if (out_normals && !normals) return "normals out without normals in";
    if (out_colors && !colors) return "colors out without colors in";
    if ((out_normals || out_colors || out_indices) && !out_vertices) return out_indices ? "indices out without vertices out" : "normals or colors out without vertices out";
    if (out_vertices && normals && !out_normals) return "normals in without normals out";
    if (out_vertices && colors && !out_colors) return "colors in without colors out";
    return nullptr;
}

// a capacity below its total is refused (the caller is told the totals all the same); a capacity nothing is written under is not looked at
inline const char *components_capacity_refusal(int64_t components, int64_t capacity_components, const void *component_table) {
    if (component_table && capacity_components > 0 && capacity_components < components) return "the table capacity is below the number of components";
    return nullptr;
}
inline const char *filter_capacity_refusal(int64_t kept_vertices, int64_t kept_triangles, int64_t capacity_vertices, int64_t capacity_triangles,
                                           const void *out_vertices, const void *out_indices) {
    if (out_vertices && capacity_vertices < kept_vertices) return "the vertex capacity is below the kept vertices";
    if (out_indices && capacity_triangles < kept_triangles) return "the triangle capacity is below the kept triangles";
    return nullptr;
}

// workgroups of a scan over n elements (n <= 2^31 - 1: at most 2^23)
constexpr int64_t components_tiles(int64_t n) { return (n + COMPONENTS_TILE - 1) / COMPONENTS_TILE; }

// The largest component by one 64-bit maximum: more triangles win, then the lower number.  0 is below every key (no component).
constexpr uint64_t components_largest_key(int64_t triangles, int64_t number) { return ((uint64_t)triangles << 32) | (uint64_t)(0xffffffffu - (uint32_t)number); }
constexpr int64_t components_key_triangles(uint64_t key) { return (int64_t)(key >> 32); }
constexpr int64_t components_key_number(uint64_t key) { return (int64_t)(0xffffffffu - (uint32_t)(key & 0xffffffffu)); }

}  // namespace chisel_hip
