// kernels_merge.h -- one TSDF map fused into another under a rigid transform (chisel_hip_merge_map; DESIGN.md 3.9 "Merging maps").
//
// Not a kernel of the reference: the server frees a keyframe's depth data once it is published (ServerKeyFrame::FreeSpace), so when the
// pose graph later moves an agent's trajectory by one rigid transform the frames cannot be integrated again; the dense equivalent is
// to move that agent's MAP by the transform and fuse it into the common one.  Every value comes from a device function that exists:
// the source voxel is the one ChunkManager::GetSDF reads (kernels_render.h: render_locate<N>), the update is DistVoxel::Integrate /
// ColorVoxel::Integrate (chisel_device.h), chunks appear through create_chunk (kernels_integrate.h) and what is left behind for an
// updated chunk is what integrate_kernel's epilogue leaves.  For voxel i = (x, y, z) of destination chunk `id`, all in fp32, one
// rounding per operation, no FMA:
//     c = ((float)i res + half_res) + (float)(N id) res            the reference's centroid (ChunkManager.cpp:50-66, Chunk.cpp:43)
//     p = ((m0 c.x + m1 c.y) + m2 c.z) + m3  per row of M          M = the inverse of src_to_dst, rounded to fp32 on the host
//     the source voxel at p, observed iff (double)weight > 1e-12   -> dist_integrate(dst, src.sdf, src.weight) [+ color_integrate]
// Four kernels on the destination's stream (host_merge.h):
//   merge_candidates_kernel   one thread per source slot: the chunk's cube taken through the inverse of M IN DOUBLE (the affine inverse of
//                             the very fp32 matrix the gather applies, so the argument does not depend on how good a rotation it is),
//                             its bounding box padded, the chunk ids the box meets entered ONCE into a scratch key table -> unique list
//   merge_classify_kernel     one thread per listed id: its slot in the destination, or "absent"; the absent ones are counted
//   (the host reads the two counts here, through report_words_kernel -- the one wait of a merge -- and sizes the pool: a fixed pool that cannot take the absent ids
//    refuses before anything is created)
//   merge_create_kernel       one thread per absent id: create_chunk (safe for concurrent DISTINCT keys: the list is unique)
//   merge_gather_kernel<N, COLOR>  one workgroup per listed id (the chunk pass of kernels_rewrite.h): the update above, then the chunk's
//                             bookkeeping -- or, for a chunk this merge created and did not touch, its removal (it still holds default
//                             voxels: nothing was stored)
#pragma once
#include "kernels_integrate.h"
#include "kernels_render.h"
#include "kernels_rewrite.h"

namespace chisel_hip {

// control words of a merge (device ints): what the host reads after merge_classify_kernel, through pinned memory
constexpr int MG_UNIQUE = 0, MG_ABSENT = 1, MG_OVERFLOW = 2, MG_SRC_CHUNKS = 3, MG_DST_FREE = 4, MG_INTS = 8;
// results of a merge (device 64-bit words): chisel_hip_merge_stats less src_chunks
constexpr int MS_CREATED = 0, MS_UPDATED = 1, MS_VOXELS = 2, MS_WORDS = 4;
constexpr int MERGE_CREATED = 1 << 30;  // in a list entry's slot word: this merge created the chunk

struct MergeView {
    unsigned long long *table;  // [table_capacity] packed ids, KEY_EMPTY = free
    unsigned long long *list;   // [table_capacity / 2] the unique ids in order of appearance
    int *slots;                 // [table_capacity / 2] destination slot per list entry (| MERGE_CREATED), -1 = absent
    int *ctl;                   // [MG_INTS]
    unsigned long long *stats;  // [MS_WORDS]
    unsigned table_capacity;    // power of two
};
struct MergeTransform {
    float m[12];    // M: destination -> source, row-major 3 x 4, what the gather applies
    double f[12];   // the affine inverse of M (source -> destination), for the candidate boxes only
    double pad;     // metres added to every side of a candidate box
};

__device__ inline void merge_list_id(const MergeView &G, int x, int y, int z) {
    const unsigned long long key = pack_id(x, y, z);
    const unsigned mask = G.table_capacity - 1u;
    unsigned h = (unsigned)(chunk_hash(x, y, z) * 0x9E3779B97F4A7C15ull >> 40) & mask;
    for (unsigned probe = 0; probe < G.table_capacity; probe++, h = (h + 1u) & mask) {
        const unsigned long long cur = G.table[h];
        if (cur == key) return;
        if (cur != KEY_EMPTY) continue;
        const unsigned long long old = atomicCAS(&G.table[h], (unsigned long long)KEY_EMPTY, key);
        if (old == key) return;
        if (old != KEY_EMPTY) continue;  // (somebody else's id: next bucket)
        const unsigned pos = (unsigned)atomicAdd(&G.ctl[MG_UNIQUE], 1);
        if (pos < G.table_capacity / 2) G.list[pos] = key;
        else G.ctl[MG_OVERFLOW] = 1;
        return;
    }
    G.ctl[MG_OVERFLOW] = 1;  // the table is full
}

// S: the SOURCE map.  edge = N res as a double.
__global__ __launch_bounds__(256) void merge_candidates_kernel(MapView S, MergeView G, MergeTransform T, double edge) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= S.committed) return;
    const uint64_t key = S.slot_key[slot];
    if (key == KEY_EMPTY) return;
    atomicAdd(&G.ctl[MG_SRC_CHUNKS], 1);
    int x, y, z;
    unpack_id(key, x, y, z);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, reach = 0.0;
    for (int c = 0; c < 8; c++) {
        const double px = (double)(x + (c & 1)) * edge, py = (double)(y + ((c >> 1) & 1)) * edge, pz = (double)(z + (c >> 2)) * edge;
        reach = fmax(reach, fmax(fabs(px), fmax(fabs(py), fabs(pz))));
        for (int a = 0; a < 3; a++) {
            const double q = ((T.f[4 * a] * px + T.f[4 * a + 1] * py) + T.f[4 * a + 2] * pz) + T.f[4 * a + 3];
            lo[a] = fmin(lo[a], q);
            hi[a] = fmax(hi[a], q);
            reach = fmax(reach, fabs(q));
        }
    }
    // The pad: one voxel, plus what fp32 rounding can move a position by on its way through the gather -- the centre, the three
    // products and sums of p, p * rf_chunk: a few ulp of the largest coordinate involved (4e-6 is more than 32 ulp) -- so that the
    // list holds every chunk with a voxel whose p lands in this source chunk, whatever the rounding.
    const double pad = T.pad + 4e-6 * reach;
    int i0[3], i1[3];
    const double limit = (double)(ID_BIAS - 2);
    for (int a = 0; a < 3; a++) {
        // (ids beyond the packed range hold no chunk and cannot be created: clipped away; a NaN bound fails both comparisons)
        const double f0 = floor((lo[a] - pad) / edge), f1 = floor((hi[a] + pad) / edge);
        if (!(f0 <= limit) || !(f1 >= -limit)) return;
        i0[a] = (int)fmax(f0, -limit);
        i1[a] = (int)fmin(f1, limit);
    }
    for (int cz = i0[2]; cz <= i1[2]; cz++)
        for (int cy = i0[1]; cy <= i1[1]; cy++)
            for (int cx = i0[0]; cx <= i1[0]; cx++) merge_list_id(G, cx, cy, cz);
}

// D: the DESTINATION map (nothing inserts into its hash while this runs: the map's stream is ours)
__global__ __launch_bounds__(256) void merge_classify_kernel(MapView D, MergeView G) {
    const int n = min(G.ctl[MG_UNIQUE], (int)(G.table_capacity / 2));
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) G.ctl[MG_DST_FREE] = *D.free_top;
    if (i >= n) return;
    int x, y, z;
    unpack_id(G.list[i], x, y, z);
    const int slot = hash_find_quiescent(D, x, y, z);
    G.slots[i] = slot;
    if (slot < 0) atomicAdd(&G.ctl[MG_ABSENT], 1);
}

__global__ __launch_bounds__(256) void merge_create_kernel(const MapView *__restrict__ Dc, MergeView G, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || G.slots[i] >= 0) return;
    int x, y, z;
    unpack_id(G.list[i], x, y, z);
    const int slot = create_chunk(Dc, x, y, z);  // (-1: pool or hash exhausted, the error is raised; the host has made room for the pool)
    G.slots[i] = slot >= 0 ? (slot | MERGE_CREATED) : -1;
}

// One workgroup per listed destination chunk, as the chunk pass of kernels_rewrite.h.  The source side is a gather: the lane keeps the
// source chunk it was last in (render_locate's cix ... cslot), so a hash probe is paid when a voxel's position enters another source
// chunk, not per voxel.
template <int N, bool COLOR>
__global__ __launch_bounds__(256) void merge_gather_kernel(MapView D, MapView S, MeshParams P, MergeView G, MergeTransform T, int n) {
    constexpr int V = N * N * N;
    __shared__ unsigned s_upd, s_col, s_signs;
    const int item = blockIdx.x;
    if (item >= n) return;
    const int entry = G.slots[item];  // block-uniform
    if (entry < 0) return;
    const int slot = entry & ~MERGE_CREATED;
    const bool created = (entry & MERGE_CREATED) != 0;
    int idx, idy, idz;
    unpack_id(G.list[item], idx, idy, idz);
    if (threadIdx.x == 0) s_upd = s_col = s_signs = 0u;
    __syncthreads();
    const ChunkCentres<N> C(P.res, P.half_res, idx, idy, idz);
    const size_t base = (size_t)slot * V;
    int cix = 0, ciy = 0, ciz = 0, cslot = -2;
    unsigned n_upd = 0, n_col = 0;
    bool pos = false, neg = false;
    for (int q = threadIdx.x; q < V / 4; q += 256) {
        const QuadIndex<N> Q(q);
        const float cy = C.y(Q.y), cz = C.z(Q.z);
        VoxelQuad<COLOR> vox;
        bool touched = false, painted = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float cx = C.x(Q.x0 + j);
            const f3v p = mk3(((T.m[0] * cx + T.m[1] * cy) + T.m[2] * cz) + T.m[3], ((T.m[4] * cx + T.m[5] * cy) + T.m[6] * cz) + T.m[7],
                              ((T.m[8] * cx + T.m[9] * cy) + T.m[10] * cz) + T.m[11]);
            if (!finite3(p)) continue;
            size_t off;
            if (!render_locate<N>(S, P, p, cix, ciy, ciz, cslot, off)) continue;
            const float w = S.wgt[off];
            if (!((double)w > 1e-12)) continue;
            const float s = S.sdf[off];
            vox.need(D, base, Q.v0);  // (most lanes of most chunks of a rotated map meet no source voxel)
            dist_integrate(vox.sdf(j), vox.weight(j), s, w);
            touched = true;
            n_upd++;
            note_sign(vox.sdf(j), vox.weight(j), pos, neg);
            if (COLOR) {
                const uchar4 sc = S.rgbw[off];
                if (sc.w > 0) {
                    unsigned &c = vox.rgbw(j);
                    uchar4 dc;
                    dc.x = (uint8_t)(c & 0xffu); dc.y = (uint8_t)((c >> 8) & 0xffu); dc.z = (uint8_t)((c >> 16) & 0xffu); dc.w = (uint8_t)(c >> 24);
                    dc = color_integrate(dc, sc.x, sc.y, sc.z, sc.w);
                    c = (unsigned)dc.x | ((unsigned)dc.y << 8) | ((unsigned)dc.z << 16) | ((unsigned)dc.w << 24);
                    painted = true;
                    n_col++;
                }
            }
        }
        vox.store(D, base, Q.v0, touched, painted);
    }
    tally_count(n_upd, &s_upd);
    tally_count(n_col, &s_col);
    tally_signs(pos, neg, &s_signs);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned upd = s_upd;
    if (upd) {
        note_slot_updated(D, slot, s_signs);
        unsigned long long *row = D.block_counters + (size_t)(blockIdx.x & (INTEGRATE_MAX_GRID - 1)) * 16;
        atomicAdd(&row[CHISEL_HIP_CNT_SDF], (unsigned long long)upd);
        if (s_col) atomicAdd(&row[CHISEL_HIP_CNT_COL], (unsigned long long)s_col);
        atomicAdd(&row[CHISEL_HIP_CNT_UPDATED_CHUNKS], 1ull);
        atomicAdd(&G.stats[MS_UPDATED], 1ull);
        atomicAdd(&G.stats[MS_VOXELS], (unsigned long long)upd);
        if (created) {
            atomicAdd(&row[CHISEL_HIP_CNT_NEW_CHUNKS], 1ull);
            atomicAdd(&G.stats[MS_CREATED], 1ull);
        }
    } else if (created) {
        // created and found untouched: out again (remove_chunks_kernel's unlinking; the slot holds default voxels still, no lane stored)
        uint64_t where = 0;
        if (hash_find(D, idx, idy, idz, &where) == slot) {
            D.hash_keys[where] = KEY_TOMB;
            D.slot_key[slot] = KEY_EMPTY;
            D.slot_dirty[slot] = 0;
            slot_summary(D)[slot] = 0;
            if (D.mesh_flag) D.mesh_flag[slot] = 0;
            __threadfence();
            const int at = atomicAdd(D.free_top, 1);
            D.free_list[at] = slot;
        }
    }
}

}  // namespace chisel_hip
