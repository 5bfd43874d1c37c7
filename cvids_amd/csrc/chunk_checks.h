// chunk_checks.h -- the host-side pieces of chisel_hip_gather_chunks and chisel_hip_scatter_chunks that call nothing of HIP (included by
// chisel_hip.hip for host_chunks.h and, on its own, by tests/chunk_checks_check.cpp, which runs them under the address and
// undefined-behaviour sanitizers on the CPU): what the two entries refuse about their requests before the device is asked anything,
// the duplicate and ownership checks of a scatter, the byte and grid arithmetic of a packed set in 64 bits, and the "every resident
// chunk" selection -- the box filter and the ascending order of chisel_hip_list_chunks.  DESIGN.md 3.13 is the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

namespace chisel_hip {

constexpr int CHUNK_COPY_THREADS = 256;      // lanes of a copy workgroup
constexpr int CHUNK_COPY_DEPTH = 4;          // 16-byte loads a lane has in flight before its first store
constexpr int CHUNK_TILE_QUADS = CHUNK_COPY_THREADS * CHUNK_COPY_DEPTH;  // 16-byte quads of ONE array one workgroup moves: 16 KiB
constexpr int64_t CHUNK_MAX_TILES = 0x7fffffffll;  // workgroups of one launch along x
constexpr int64_t CHUNK_MAX_CHUNKS = 0x7fffffffll; // chunks of one call (a slot table entry is an int)
constexpr int CHUNK_ID_BIAS = 1 << 20;       // = ID_BIAS (chisel_device.h)

// the key the selections sort by: x in the high bits, then y, then z -- ascending keys are chisel_hip_list_chunks' order (ids in range)
inline uint64_t chunk_order_key(int x, int y, int z) {
    return ((uint64_t)(uint32_t)(x + CHUNK_ID_BIAS) << 42) | ((uint64_t)(uint32_t)(y + CHUNK_ID_BIAS) << 21) | (uint64_t)(uint32_t)(z + CHUNK_ID_BIAS);
}

// the first id of the list with a coordinate outside +-id_limit, or -1
inline int64_t chunk_first_id_out_of_range(const int *ids_xyz, int64_t n, int id_limit) {
    for (int64_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (ids_xyz[3 * i + a] < -id_limit || ids_xyz[3 * i + a] > id_limit) return i;
    return -1;
}

// What the bytes and the grid of a packed set of n chunks of V voxels come to: bytes of one array (4 per voxel: a float, or four
// colour bytes), 16-byte quads per chunk and in all, workgroups per array.  Null = fine, else why the set is not served.
struct ChunkSizes {
    int64_t bytes_per_array, quads_per_chunk, quads, tiles;
    int quad_shift;  // log2(quads_per_chunk)
};
inline const char *chunk_sizes(int64_t n, int64_t voxels_per_chunk, ChunkSizes *out) {
    *out = ChunkSizes{0, 0, 0, 0, 0};
    if (voxels_per_chunk < 4 * (CHUNK_COPY_THREADS / 2) || (voxels_per_chunk & (voxels_per_chunk - 1)) != 0 || voxels_per_chunk > (1ll << 30))
        return "a chunk is not a power of two of at least 512 voxels";  // (the 256 quads of one access of a workgroup meet at most two chunks)
    out->quads_per_chunk = voxels_per_chunk / 4;
    while ((1ll << out->quad_shift) < out->quads_per_chunk) out->quad_shift++;
    if (n < 0 || n > CHUNK_MAX_CHUNKS) return "more chunks than one call takes (2^31 - 1)";
    // (n < 2^31 and V <= 2^30: n V 4 < 2^63)
    out->bytes_per_array = n * voxels_per_chunk * 4;
    out->quads = n * out->quads_per_chunk;
    out->tiles = (out->quads + CHUNK_TILE_QUADS - 1) / CHUNK_TILE_QUADS;
    if (out->tiles > CHUNK_MAX_TILES) return "the selection needs more workgroups than one launch takes (2^31 - 1 tiles of 16 KiB per array)";
    return nullptr;
}

// What chisel_hip_gather_chunks refuses about its request and its outputs before it asks the device, in the order of the header; null =
// go on.  Request: chisel_hip_chunk_request (a template, so that this header goes on including nothing of the library's).  *bad_id:
// the index of an id out of range, else -1.  Outputs: the three arrays and the id list as given.
template <class Request>
inline const char *chunk_gather_refusal(const Request *r, int64_t capacity_chunks, const void *sdf, const void *weight, const void *rgbw,
                                        const void *chunk_ids_xyz, bool on_device, bool map_has_color, int id_limit, int64_t *bad_id) {
    *bad_id = -1;
    if (!r) return "null request";
    if (r->n_ids < 0) return "a negative number of ids";
    if (r->ids_xyz && r->n_ids == 0) return "an id list without a count";
    if (!r->ids_xyz && r->n_ids > 0) return "a count without an id list";
    if (r->use_box && r->ids_xyz) return "a box together with an id list";
    if (r->use_box)
        for (int a = 0; a < 3; a++)
            if (r->box_lo[a] > r->box_hi[a]) return "a box with lo > hi on an axis";
    *bad_id = chunk_first_id_out_of_range(r->ids_xyz, r->n_ids, id_limit);
    if (*bad_id >= 0) return "a chunk id outside the addressable range";
    if (capacity_chunks < 0) return "a negative capacity";
    if (capacity_chunks == 0) return nullptr;  // the size query: nothing else is looked at
    if (!sdf && !weight && !rgbw && !chunk_ids_xyz) return "no output asked for";
    if (rgbw && !map_has_color) return "rgbw asked of a map without colour";
    if (on_device && ((((uintptr_t)sdf) | ((uintptr_t)weight) | ((uintptr_t)rgbw)) & 15)) return "a device pointer that is not 16-byte aligned";
    return nullptr;
}

// ... and chisel_hip_scatter_chunks, as far as the ids are not looked at (chunk_scatter_ids_refusal is next).  n == 0 is not refused.
inline const char *chunk_scatter_refusal(const int *ids_xyz, int64_t n, const void *sdf, const void *weight, const void *rgbw, bool on_device,
                                         bool map_has_color) {
    if (n < 0) return "a negative number of chunks";
    if (n == 0) return nullptr;
    if (!ids_xyz || !sdf || !weight) return "null ids, sdf or weight";
    if (rgbw && !map_has_color) return "rgbw given to a map without colour";
    if (on_device && ((((uintptr_t)sdf) | ((uintptr_t)weight) | ((uintptr_t)rgbw)) & 15)) return "a device pointer that is not 16-byte aligned";
    return nullptr;
}

// The second index of the first id that repeats an earlier one, or -1: the ids sorted with their indices (O(n log n)), equal
// neighbours compared.  The ids are in range (chunk_order_key).
inline int64_t chunk_first_duplicate(const int *ids_xyz, int64_t n) {
    std::vector<std::pair<uint64_t, int64_t>> keyed((size_t)n);
    for (int64_t i = 0; i < n; i++) keyed[(size_t)i] = {chunk_order_key(ids_xyz[3 * i], ids_xyz[3 * i + 1], ids_xyz[3 * i + 2]), i};
    std::sort(keyed.begin(), keyed.end());
    int64_t second = -1;
    for (size_t j = 1; j < keyed.size(); j++)
        if (keyed[j].first == keyed[j - 1].first && (second < 0 || keyed[j].second < second)) second = keyed[j].second;
    return second;
}

// The ids of a scatter, in the header's order: range, duplicates, ownership.  owner(x, y, z) -> the shard that owns the id
// (chisel_hip_chunk_owner with the map's configuration); rank: the map's own.  *bad_id: the index the message names.
template <class Owner>
inline const char *chunk_scatter_ids_refusal(const int *ids_xyz, int64_t n, int id_limit, Owner owner, int rank, int64_t *bad_id) {
    *bad_id = chunk_first_id_out_of_range(ids_xyz, n, id_limit);
    if (*bad_id >= 0) return "a chunk id outside the addressable range";
    *bad_id = chunk_first_duplicate(ids_xyz, n);
    if (*bad_id >= 0) return "repeats an id earlier in the list";
    for (int64_t i = 0; i < n; i++)
        if (owner(ids_xyz[3 * i], ids_xyz[3 * i + 1], ids_xyz[3 * i + 2]) != rank) {
            *bad_id = i;
            return "belongs to another shard";
        }
    return nullptr;
}

// The "every resident chunk" selection: of the n listed ids (any order, distinct, in range) those inside the box (lo <= id <= hi on
// every axis; use_box = false: all), ascending by x, then y, then z.  -> their indices into the listing, in that order.
inline std::vector<int64_t> chunk_select_sorted(const int *ids_xyz, int64_t n, bool use_box, const int lo[3], const int hi[3]) {
    std::vector<std::pair<uint64_t, int64_t>> keyed;
    keyed.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        bool inside = true;
        if (use_box)
            for (int a = 0; a < 3; a++) inside = inside && ids_xyz[3 * i + a] >= lo[a] && ids_xyz[3 * i + a] <= hi[a];
        if (inside) keyed.push_back({chunk_order_key(ids_xyz[3 * i], ids_xyz[3 * i + 1], ids_xyz[3 * i + 2]), i});
    }
    std::sort(keyed.begin(), keyed.end());
    std::vector<int64_t> order(keyed.size());
    for (size_t j = 0; j < keyed.size(); j++) order[j] = keyed[j].second;
    return order;
}

// a capacity below the selection is refused (the caller is told the count all the same)
inline const char *chunk_capacity_refusal(int64_t n_selected, int64_t capacity_chunks) {
    return capacity_chunks < n_selected ? "the capacity is below the selection" : nullptr;
}

// chunks per block of a save or a load: at most `block_bytes` of payload (sdf + weight [+ rgbw]), at least one chunk
inline int64_t chunk_block_chunks(int64_t voxels_per_chunk, bool color, int64_t block_bytes) {
    const int64_t per_chunk = voxels_per_chunk * 4 * (color ? 3 : 2);
    return std::max<int64_t>(1, block_bytes / per_chunk);
}

}  // namespace chisel_hip
