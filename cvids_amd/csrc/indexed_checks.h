// indexed_checks.h -- the host-side pieces of chisel_hip_indexed_mesh that call nothing of HIP (included by chisel_hip.hip for
// host_indexed.h and kernels_indexed.h and, on its own, by tests/indexed_checks_check.cpp, which runs them under the address and
// undefined-behaviour sanitizers on the CPU): what the entry refuses about its request before the device is asked anything -- the
// coarse mesh's refusals (coarse_checks.h), the duplicate check of chunk_checks.h and its own --, the EXTRAS of a selection (the +
// neighbours that are not selected, once each, ascending), and the 64-bit arithmetic of rows, ids and index entries against
// 2^31 - 1.  DESIGN.md 3.15 is the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "coarse_checks.h"

namespace chisel_hip {

constexpr int INDEXED_HOST_WORDS = 8;  // 64-bit words the scan reports in front of the tables (IX_*)
constexpr int IX_CHUNKS = 0, IX_OWNERS = 1, IX_CUBES = 2, IX_VERTICES = 3, IX_TRIANGLES = 4, IX_ABSENT = 5;  // (IX_ABSENT: first listed id not resident, or -1)
constexpr int64_t INDEXED_MAX_INTS = 0x7fffffffll;  // vertex ids, and entries of the index array

// rows of one owner: one 32-bit mask per (axis, lk, lj), bit li -- M = N / s <= 32
inline int64_t indexed_rows(int chunk_edge, int stride) {
    const int64_t M = chunk_edge / stride;
    return 3 * M * M;
}

// the mask and prefix words of a call with `owners` owners, or -1 when they pass 2^31 - 1 (the kernels index them with 64 bits;
// the bound keeps the scratch below 16 GiB)
inline int64_t indexed_row_words(int64_t owners, int chunk_edge, int stride) {
    const int64_t rows = indexed_rows(chunk_edge, stride);
    if (owners < 0 || owners > INDEXED_MAX_INTS / rows) return -1;
    return owners * rows;
}

// a vertex id is an int32; the index array has 3 entries a triangle, indexed with ints by its readers.  Null = fine.
inline const char *indexed_size_refusal(int64_t vertices, int64_t triangles) {
    if (vertices < 0 || triangles < 0) return "a negative total";
    if (vertices > INDEXED_MAX_INTS) return "more than 2^31 - 1 vertices";
    if (triangles > INDEXED_MAX_INTS / 3) return "more than 2^31 - 1 index entries";
    return coarse_floats_refusal(vertices);
}

// What chisel_hip_indexed_mesh refuses about its request and its outputs before it asks the device; null = go on.  Request:
// chisel_hip_coarse_request.  *bad_id: the index of an id out of range or of the second of two equal ids, else -1.
template <class Request>
inline const char *indexed_request_refusal(const Request *r, int chunk_edge, int64_t capacity_vertices, int64_t capacity_triangles, const void *vertices,
                                           const void *indices, const void *normals, const void *colors, const void *chunk_table, const void *owner_table,
                                           const void *owner_ids_xyz, bool map_has_color, int id_limit, int64_t *bad_id) {
    *bad_id = -1;
    if (!r) return "null request";
    if (capacity_triangles < 0) return "a negative capacity";
    const bool query = capacity_vertices == 0 && capacity_triangles == 0;
    // everything the coarse mesh refuses; the tables stand in for each other as "an output"
    const void *table = chunk_table ? chunk_table : (owner_table ? owner_table : indices);
    if (const char *why = coarse_request_refusal(r, chunk_edge, query ? 0 : (capacity_vertices > 0 ? capacity_vertices : 1), vertices, normals, colors, table,
                                                 owner_ids_xyz, map_has_color, id_limit, bad_id))
        return why;
    if (capacity_vertices < 0) return "a negative capacity";
    if (r->chunks.ids_xyz) {  // an owner is unique
        *bad_id = chunk_first_duplicate(r->chunks.ids_xyz, r->chunks.n_ids);
        if (*bad_id >= 0) return "repeats an id earlier in the list";
    }
    if (query) return nullptr;  // the size query: nothing else is looked at
    if (normals && !(r->stages & 1)) return "normals without stage bit 0 (face normals have no per-vertex meaning)";
    if (indices && !vertices) return "indices without vertices";
    return nullptr;
}

// either capacity below its total is refused (the caller is told the totals all the same)
inline const char *indexed_capacity_refusal(int64_t vertices, int64_t triangles, int64_t capacity_vertices, int64_t capacity_triangles) {
    if (capacity_vertices < vertices) return "the vertex capacity is below the total";
    if (capacity_triangles < triangles) return "the triangle capacity is below the total";
    return nullptr;
}

// The extras of a selection of n distinct ids in range: the + neighbours (x + dx, y + dy, z + dz), d in {0, 1}^3 \ {0}, of the
// selected chunks that are not selected themselves, lie inside +-id_limit and satisfy keep(x, y, z) (the residency, where the
// caller knows it), each once, ascending by x, then y, then z.  -> their ids, 3 ints each.
template <class Keep>
inline std::vector<int> indexed_extras(const int *ids_xyz, int64_t n, int id_limit, Keep keep) {
    std::vector<uint64_t> selected((size_t)n);
    for (int64_t i = 0; i < n; i++) selected[(size_t)i] = chunk_order_key(ids_xyz[3 * i], ids_xyz[3 * i + 1], ids_xyz[3 * i + 2]);
    std::sort(selected.begin(), selected.end());
    std::vector<uint64_t> found;
    for (int64_t i = 0; i < n; i++)
        for (int d = 1; d < 8; d++) {
            const int x = ids_xyz[3 * i] + (d & 1), y = ids_xyz[3 * i + 1] + ((d >> 1) & 1), z = ids_xyz[3 * i + 2] + (d >> 2);
            if (x > id_limit || y > id_limit || z > id_limit) continue;
            const uint64_t key = chunk_order_key(x, y, z);
            if (std::binary_search(selected.begin(), selected.end(), key)) continue;
            if (keep(x, y, z)) found.push_back(key);
        }
    std::sort(found.begin(), found.end());
    found.erase(std::unique(found.begin(), found.end()), found.end());
    std::vector<int> out(found.size() * 3);
    for (size_t j = 0; j < found.size(); j++) {
        out[3 * j] = (int)(uint32_t)(found[j] >> 42) - CHUNK_ID_BIAS;
        out[3 * j + 1] = (int)(uint32_t)((found[j] >> 21) & 0x1fffff) - CHUNK_ID_BIAS;
        out[3 * j + 2] = (int)(uint32_t)(found[j] & 0x1fffff) - CHUNK_ID_BIAS;
    }
    return out;
}
inline std::vector<int> indexed_extras(const int *ids_xyz, int64_t n, int id_limit) {
    return indexed_extras(ids_xyz, n, id_limit, [](int, int, int) { return true; });
}

}  // namespace chisel_hip
