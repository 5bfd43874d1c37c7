// coarse_checks.h -- the host-side pieces of chisel_hip_coarse_mesh that call nothing of HIP (included by chisel_hip.hip for
// host_coarse.h and kernels_coarse.h and, on its own, by tests/coarse_checks_check.cpp, which runs them under the address and
// undefined-behaviour sanitizers on the CPU): the stride rule, the 64-bit arithmetic of vertices x 3 floats against 2^31 - 1, the
// grid of the count and emit launches, and what the entry refuses about its request before the device is asked anything -- the
// selection by chunk_checks.h.  DESIGN.md 3.14 is the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "chunk_checks.h"

namespace chisel_hip {

constexpr int COARSE_THREADS = 256;              // lanes of a count / emit workgroup
constexpr int COARSE_SLAB = 4;                   // layers of coarse cubes staged at a time: COARSE_SLAB + 1 layers of the lattice
constexpr int COARSE_MAX_GRID = 2048;            // workgroups of the count and emit launches (they stride over the chunks)
constexpr int64_t COARSE_MAX_FLOATS = 0x7fffffffll;  // floats of one output array
constexpr int COARSE_HOST_WORDS = 8;             // 64-bit words the scan reports in front of the table (CO_*)
constexpr int CO_CHUNKS = 0, CO_NONEMPTY = 1, CO_CUBES = 2, CO_VERTICES = 3, CO_ABSENT = 4;  // (CO_ABSENT: first listed id not resident, or -1)

// 1 <= s <= N and s divides N: null = fine
inline const char *coarse_stride_refusal(int chunk_edge, int stride) {
    if (stride < 1) return "a stride below 1";
    if (stride > chunk_edge) return "a stride above the chunk edge";
    if (chunk_edge % stride != 0) return "a stride that does not divide the chunk edge";
    return nullptr;
}

// samples of the lattice one workgroup stages at a time: (min(M, COARSE_SLAB) + 1) layers of (M + 1)^2, M = N / s
inline int64_t coarse_lattice_samples(int chunk_edge, int stride) {
    const int64_t M = chunk_edge / stride, layers = (M < COARSE_SLAB ? M : COARSE_SLAB) + 1;
    return layers * (M + 1) * (M + 1);
}

// an array of `vertices` x 3 floats is indexed with ints by its readers: at most 2^31 - 1 floats.  Null = fine.
inline const char *coarse_floats_refusal(int64_t vertices) {
    if (vertices < 0) return "a negative number of vertices";
    if (vertices > COARSE_MAX_FLOATS / 3) return "more than 2^31 - 1 floats in one array";
    return nullptr;
}

// workgroups of the count and emit launches for a selection of n chunks (n >= 1)
inline int coarse_grid(int64_t n_chunks) {
    if (n_chunks < 1) return 1;
    return (int)(n_chunks < COARSE_MAX_GRID ? n_chunks : COARSE_MAX_GRID);
}

// What chisel_hip_coarse_mesh refuses about its request and its outputs before it asks the device, in the order of the header;
// null = go on.  Request: chisel_hip_coarse_request (a template, so that this header goes on including nothing of the library's).
// *bad_id: the index of an id out of range, else -1.
template <class Request>
inline const char *coarse_request_refusal(const Request *r, int chunk_edge, int64_t capacity_vertices, const void *vertices, const void *normals,
                                          const void *colors, const void *chunk_table, const void *chunk_ids_xyz, bool map_has_color, int id_limit,
                                          int64_t *bad_id) {
    *bad_id = -1;
    if (!r) return "null request";
    if (const char *why = coarse_stride_refusal(chunk_edge, r->stride)) return why;
    if (r->stages < 0 || r->stages > 3) return "stages other than bit 0 (gradient normals) and bit 1 (colours)";
    if ((r->stages & 2) && !map_has_color) return "colour stage asked of a map without colour";
    // the selection: what chisel_hip_gather_chunks refuses of one (its outputs are not looked at: the size query's checks)
    if (const char *why = chunk_gather_refusal(&r->chunks, (int64_t)0, nullptr, nullptr, nullptr, nullptr, false, map_has_color, id_limit, bad_id)) return why;
    if (capacity_vertices < 0) return "a negative capacity";
    if (capacity_vertices == 0) return nullptr;  // the size query: nothing else is looked at
    if (!vertices && !normals && !colors && !chunk_table && !chunk_ids_xyz) return "no output asked for";
    if ((normals || colors) && !vertices) return "normals or colours without vertices";
    if (colors && !map_has_color) return "colours asked of a map without colour";
    return nullptr;
}

// a capacity below the total is refused (the caller is told the totals all the same)
inline const char *coarse_capacity_refusal(int64_t vertices, int64_t capacity_vertices) {
    return capacity_vertices < vertices ? "the capacity is below the total" : nullptr;
}

}  // namespace chisel_hip
