// kernels_chunks.h -- chisel_hip_gather_chunks and chisel_hip_scatter_chunks: many chunks copied between their pool slots and the
// caller's packed arrays by one launch (the host side: host_chunks.h; the request checks and the byte arithmetic: chunk_checks.h; the
// definition: DESIGN.md 3.13).
//
// A packed array is n chunks of V voxels, 4 bytes a voxel whichever array it is (sdf, weight, rgbw), chunk i of the selection at
// index i; the pool holds the same V voxels of chunk i at slot table[i].  The copy is cut into tiles of CHUNK_TILE_QUADS 16-byte
// quads of ONE packed array -- 16 KiB, whatever the chunk size: eight 8^3 chunks, one 16^3 chunk, an eighth of a 32^3 chunk -- and a
// workgroup owns one tile (blockIdx.x) of one array (blockIdx.y).  Each lane issues CHUNK_COPY_DEPTH 16-byte loads, 256 quads apart,
// and then their stores -- the loads unconditional and their values asked for behind the last of them, so that four are in flight
// per lane in the emitted code.  The 256 quads of one such access lie in one chunk (V / 4 >= 256) or in two (8^3: lanes 0-127 and 128-255),
// whose slots are read at addresses that depend on blockIdx alone -- scalar loads, once per wave -- and chosen by a compare.  No LDS,
// no atomics, no scratch.  Pool chunks start at multiples of V * 4 bytes and the packed arrays are 16-byte aligned (refused
// otherwise), so every access is a whole aligned quad.
//
// Around the copy of a scatter, the merge's pattern (kernels_merge.h): chunks_classify_kernel -- slot per id, the absent ones counted,
// the free slots reported; the host's one wait, the pool sized --, chunks_create_kernel -- create_chunk per absent id, safe for
// concurrent DISTINCT keys: duplicates are refused on the host --, and behind the copy chunks_note_kernel: one thread per chunk writes
// the slot's sign summary (SUM_ANY, chisel_hip_upload_chunk's rule) and, when asked, marks the slot as an integration that changed it
// does (note_slot_updated).
#pragma once
#include "kernels_integrate.h"  // create_chunk
#include "kernels_map.h"
#include "chunk_checks.h"

namespace chisel_hip {

// control words of a scatter (device ints): what the host reads after chunks_classify_kernel, through pinned memory
constexpr int CK_ABSENT = 0, CK_FREE = 1, CK_INTS = 4;

typedef unsigned ChunkQuad __attribute__((ext_vector_type(4)));  // (a native vector: HIP's uint4 is a struct, which takes no address space)
typedef __attribute__((address_space(1))) ChunkQuad ChunkGlobalQuad;

struct ChunkCopyArrays {  // the arrays of one launch: blockIdx.y picks one
    void *pool[3];        // the pool's array (MapView::sdf, wgt, rgbw)
    void *packed[3];      // the caller's; null (scatter only): zeros are written
};

template <bool SCATTER>
__global__ __launch_bounds__(CHUNK_COPY_THREADS) void chunk_copy_kernel(ChunkCopyArrays A, const int *__restrict__ table, long long n_chunks, int quad_shift) {
    const unsigned a = blockIdx.y;
    // (pointers taken from a struct are generic to the compiler: said to be global, the accesses are global_load / global_store)
    ChunkGlobalQuad *__restrict__ pool = (ChunkGlobalQuad *)(a == 0 ? A.pool[0] : (a == 1 ? A.pool[1] : A.pool[2]));
    ChunkGlobalQuad *__restrict__ packed = (ChunkGlobalQuad *)(a == 0 ? A.packed[0] : (a == 1 ? A.packed[1] : A.packed[2]));
    const bool zeros = SCATTER && packed == nullptr;
    const long long q0 = (long long)blockIdx.x * CHUNK_TILE_QUADS;
    const long long total = n_chunks << quad_shift;
    const long long in_chunk = (1ll << quad_shift) - 1;
    const int tid = (int)threadIdx.x;
    const bool second = quad_shift < 8 && (tid >> quad_shift) != 0;  // (quad_shift >= 7: chunk_sizes)
    // ---- the slots of the tile's accesses: every table entry is read at a clamped index, no branch between the reads (n_chunks >= 1)
    int s0[CHUNK_COPY_DEPTH], s1[CHUNK_COPY_DEPTH];
#pragma unroll
    for (int k = 0; k < CHUNK_COPY_DEPTH; k++) {
        const long long c0 = (q0 + k * CHUNK_COPY_THREADS) >> quad_shift;  // (the first quad of an access is a multiple of 256)
        s0[k] = table[c0 < n_chunks ? c0 : n_chunks - 1];
        s1[k] = table[c0 + 1 < n_chunks ? c0 + 1 : n_chunks - 1];
    }
    // ---- every quad's place in the pool, -1 = none (behind the selection's end, or a chunk that could not be created)
    long long at[CHUNK_COPY_DEPTH];
#pragma unroll
    for (int k = 0; k < CHUNK_COPY_DEPTH; k++) {
        const long long q = q0 + k * CHUNK_COPY_THREADS + tid;
        const int slot = second ? s1[k] : s0[k];
        at[k] = (q < total && slot >= 0) ? ((long long)slot << quad_shift) + (q & in_chunk) : -1;
    }
    if (zeros) {  // (block-uniform: a scatter without colours into a map with colour)
#pragma unroll
        for (int k = 0; k < CHUNK_COPY_DEPTH; k++)
            if (at[k] >= 0) pool[at[k]] = ChunkQuad{0u, 0u, 0u, 0u};
        return;
    }
    // ---- the four loads, unconditional: a lane without a quad reads quad 0 of its source (there is one: n_chunks >= 1, and slot 0 is
    // committed in every pool) and stores nothing, so that no load waits for a branch or for the load in front of it
    ChunkQuad r[CHUNK_COPY_DEPTH];
#pragma unroll
    for (int k = 0; k < CHUNK_COPY_DEPTH; k++) {
        const long long q = q0 + k * CHUNK_COPY_THREADS + tid;
        const long long from = at[k] >= 0 ? (SCATTER ? q : at[k]) : 0;
        r[k] = SCATTER ? packed[from] : pool[from];
    }
    // (the values are asked for here, in order, behind the last load: the compiler may not sink a load into the branch of its store)
#pragma unroll
    for (int k = 0; k < CHUNK_COPY_DEPTH; k++) asm volatile("" : "+v"(r[k]));
#pragma unroll
    for (int k = 0; k < CHUNK_COPY_DEPTH; k++) {
        if (at[k] < 0) continue;
        if (SCATTER) pool[at[k]] = r[k];
        else packed[q0 + k * CHUNK_COPY_THREADS + tid] = r[k];
    }
}

// one thread per id: its slot, or -1; the absent ones counted.  Nothing inserts into the hash while this runs: the map's stream is ours.
__global__ __launch_bounds__(256) void chunks_classify_kernel(MapView M, const int *__restrict__ ids, int n, int *__restrict__ slots, int *ctl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) ctl[CK_FREE] = *M.free_top;
    if (i >= n) return;
    const int slot = hash_find_quiescent(M, ids[3 * (size_t)i], ids[3 * (size_t)i + 1], ids[3 * (size_t)i + 2]);
    slots[i] = slot;
    if (slot < 0) atomicAdd(&ctl[CK_ABSENT], 1);
}

// one thread per absent id (-1 stays: pool or hash exhausted, the error is raised; the host has made room in the pool)
__global__ __launch_bounds__(256) void chunks_create_kernel(const MapView *__restrict__ Mc, const int *__restrict__ ids, int n, int *__restrict__ slots) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || slots[i] >= 0) return;
    slots[i] = create_chunk(Mc, ids[3 * (size_t)i], ids[3 * (size_t)i + 1], ids[3 * (size_t)i + 2]);
}

// behind the copy, one thread per chunk: voxels from outside -- the mesher looks at the chunk, whatever it held before
__global__ __launch_bounds__(256) void chunks_note_kernel(MapView M, const int *__restrict__ slots, int n, int mark_updated) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = slots[i];
    if (slot < 0) return;
    slot_summary(M)[slot] = SUM_ANY;
    if (mark_updated) note_slot_updated(M, slot, SUM_ANY);
}

}  // namespace chisel_hip
