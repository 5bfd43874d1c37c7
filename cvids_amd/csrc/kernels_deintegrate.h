// kernels_deintegrate.h -- depth frames taken back out of the map (chisel_hip_deintegrate_depth, chisel_hip_deintegrate_batch; DESIGN.md
// 3.10 "Taking a frame out again" is the definition).
//
// Not a kernel of the reference: a pose graph moves keyframe poses after their depth maps were fused, and DistVoxel::Integrate is a
// weighted running mean that can be inverted per voxel.  A voxel is SELECTED when the frame's integration sent it down the in-band
// branch -- ProjectionIntegrator::Integrate / IntegrateColor (ProjectionIntegrator.h:51-99 / :101-183), all in fp32, one rounding per
// operation, no FMA:
//     c  = ((float)i res + half_res) + (float)(N id) res                    the reference's centroid (ChunkManager.cpp:50-66, Chunk.cpp:43)
//     q  = R^T (c - t), each row as r0 dx + (r3 dy + r6 dz);  u = fx qx (1 / qz) + cx, v likewise       (color_pixel's order)
//     on the image (0 <= u < W, 0 <= v < H) and qz >= 0;  depth = D[(int)v][(int)u], not NaN, not above max_depth (50 / 100)
//     sd = depth - qz,  |sd| < truncation(depth) + diag
// which depends on the frame and the geometry only.  With wu the weight of that update (1, or weight / (5 truncation) under the colour
// rules) a selected voxel (s, w) becomes
//     !(w > 0)                      left alone                                  (skipped)
//     w2 = w - wu, !(w2 > w 2^-16)  DistVoxel::Reset(): (99999, 0)              (cleared: an exact zero, a residue of rounding, a negative
//                                                                                remainder after a carve, NaN)
//     else                          ((w s - wu sd) / w2, w2)                    (updated)
// The carve branch is not undone and colour voxels are never written.  Two kernels on the map's stream (host_deintegrate.h), no host
// wait between them:
//   deintegrate_list_kernel      one thread per committed slot: the resident chunks whose bounding sphere reaches into the image pyramid,
//                                compacted into a list, one append per wave
//   deintegrate_apply_kernel<N, 256, DeintegrateView>  a fixed grid of workgroups strides over the list (its length is read from the
//                                device; the chunk pass of kernels_rewrite.h): the rule above, then the chunk's bookkeeping
// Many frames in one call (DESIGN.md 3.10 "Many frames in one call"): the frames are cut into launch sets of at most KMAX, in order, and
// each set is the same two launches with a 16-bit frame mask per listed chunk:
//   deintegrate_list_batch_kernel      a resident chunk is tested against every pyramid of the set and listed with the mask of those it reaches
//   deintegrate_apply_kernel<N, T, DeintegrateBatchView>  the same kernel template: per quad, the frames of the chunk's mask in ascending
//                                      order, the voxels kept in registers across them: loaded at first need, stored once; the chunk's
//                                      bookkeeping once per chunk and set; T threads per workgroup (deintegrate_batch_threads)
// The per-frame constants (camera, image, pyramid) are a table in device memory, indexed by the block-uniform frame number.
// What the two pairs do alike is written once: deintegrate_append (the list kernels' compaction), deintegrate_select (the frame's
// verdict), deintegrate_apply_kernel (one template for both apply kernels, the rule above in it), deintegrate_tally,
// deintegrate_chunk_end and deintegrate_flush (the chunk's bookkeeping).
#pragma once
#include "host_checks.h"
#include "kernels_rewrite.h"
#include <type_traits>

namespace chisel_hip {

// Results of a de-integration (device 64-bit words): chisel_hip_deintegrate_stats in its order; DS_LISTED: the list length of a single
// frame's call; from DS_WORDS on: the list lengths of a batch's launch sets, a word each.  One memset per call zeroes what it uses.
constexpr int DS_TESTED = 0, DS_TOUCHED = 1, DS_EMPTIED = 2, DS_UPDATED = 3, DS_CLEARED = 4, DS_SKIPPED = 5, DS_LISTED = 6, DS_WORDS = 8;
constexpr int DEINTEGRATE_GRID = 2048;  // workgroups of the apply kernel: what is resident at once
// threads per workgroup of the batched apply kernel for a chunk of n^3 voxels (n^3 / 4 quads: 128, 1024, 8192).  512 measured against 256
// and 1024 (EXPERIMENTS.md): 1024 is the fastest where few chunks are listed and the slowest where thousands are.
constexpr int deintegrate_batch_threads(int n) { return n >= 16 ? 512 : 256; }

// what differs from frame to frame of a batch: one entry of the call's table in device memory (320 bytes; 16 of them would not fit the
// kernel-argument segment beside MapView without scalar registers spilling)
struct DeintegrateBatchEntry {
    DeintegratePyramid Y;
    CameraParams cam;
    const float *depth;         // W x H on the device
};
// What the kernels take of the call's scratch (host_deintegrate.h: one set for both entries), and the frame source of the apply
// kernel: which of the two it is instantiated with decides whether it walks a mask of frames.  Two structs, not one: the single
// frame's kernels keep their 32 bytes of arguments.
struct DeintegrateView {
    int *list;                  // [committed slots] the listed slots
    unsigned long long *stats;  // [DS_WORDS]
    int *emptied;               // [3 max_ids] ids of the emptied chunks, or null
    int max_ids;
};
struct DeintegrateBatchView {
    int2 *list;                          // [committed slots] (listed slot, mask of the set's frames that may reach it): the same memory
    unsigned long long *stats;           // [DS_WORDS]: accumulated over the sets of a call (DS_LISTED is not used)
    unsigned long long *listed;          // this set's list length: a word of its own per set, behind the stats
    int *emptied;                        // [3 max_ids] ids of the emptied chunks, or null
    int max_ids;
    const DeintegrateBatchEntry *table;  // [frames of the call]
    int first;                           // the set's first frame in the table
};
// the frame, the integrator's settings and the map's constants
struct DeintegrateFrame {
    CameraParams cam;
    const float *depth;         // W x H on the device
    int trunc_kind;
    float trunc_param, weight;
    float res, half_res, diag, max_depth;
    int color_rules;            // IntegrateColor's rules: NaN depth skipped, max_depth 100, wu = constant_weight
};

// One append per wave with a survivor; the lanes of a wave keep their order.  The wave's resident chunks, `frames` times, go onto
// DS_TESTED; its survivors onto *length, each one's entry at its rank (at most one entry per committed slot: the list holds them all).
template <class Entry>
__device__ inline void deintegrate_append(bool resident, bool keep, Entry entry, Entry *list, unsigned long long *stats, int frames, unsigned long long *length) {
    const unsigned long long tested = __ballot(resident), kept = __ballot(keep);
    if (tested == 0ull) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) {
        atomicAdd(&stats[DS_TESTED], (unsigned long long)__popcll(tested) * (unsigned long long)frames);  // (each frame tests every resident chunk)
        if (kept) base = (int)atomicAdd(length, (unsigned long long)__popcll(kept));
    }
    base = __shfl(base, 0);
    if (keep) list[base + __popcll(kept & ((1ull << lane) - 1ull))] = entry;
}

__global__ __launch_bounds__(256) void deintegrate_list_kernel(MapView M, DeintegrateView G, DeintegratePyramid Y) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    bool resident = false, keep = false;
    if (slot < M.committed) {
        const uint64_t key = M.slot_key[slot];
        if (key != KEY_EMPTY) {
            resident = true;
            int x, y, z;
            unpack_id(key, x, y, z);
            keep = deintegrate_keeps(Y, x, y, z);
        }
    }
    deintegrate_append(resident, keep, slot, G.list, G.stats, 1, &G.stats[DS_LISTED]);
}

// frames first .. first + count - 1 of the table (count <= KMAX) against every resident chunk
__global__ __launch_bounds__(256) void deintegrate_list_batch_kernel(MapView M, DeintegrateBatchView G, int first, int count) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    bool resident = false;
    int x = 0, y = 0, z = 0;
    if (slot < M.committed) {
        const uint64_t key = M.slot_key[slot];
        if (key != KEY_EMPTY) {
            resident = true;
            unpack_id(key, x, y, z);
        }
    }
    unsigned mask = 0u;
    for (int k = 0; k < count; k++)  // (k is uniform: the pyramid comes in by scalar loads)
        if (deintegrate_keeps(G.table[first + k].Y, x, y, z)) mask |= 1u << k;
    if (!resident) mask = 0u;
    deintegrate_append(resident, mask != 0u, make_int2(slot, (int)mask), G.list, G.stats, count, G.listed);
}

// the frame's verdict on the voxel centred at (cx, cy, cz): selected -> sd and wu
__device__ inline bool deintegrate_select(const DeintegrateFrame &F, float cx, float cy, float cz, float &sd, float &wu) {
    const CameraParams &K = F.cam;
    const float dx = cx - K.t[0], dy = cy - K.t[1], dz = cz - K.t[2];
    const float qx = K.R[0] * dx + (K.R[3] * dy + K.R[6] * dz);
    const float qy = K.R[1] * dx + (K.R[4] * dy + K.R[7] * dz);
    const float qz = K.R[2] * dx + (K.R[5] * dy + K.R[8] * dz);
    const float iq = 1.0f / qz;
    const float u = K.fx * qx * iq + K.cx;
    const float v = K.fy * qy * iq + K.cy;
    if (!((u >= 0.0f) && (v >= 0.0f) && (u < (float)K.W) && (v < (float)K.H)) || qz < 0.0f) return false;
    const int iu = (int)u, iv = (int)v;
    if (iu >= K.W || iv >= K.H) return false;  // ((float)W rounds up from 2^24 on: no pixel there)
    const float depth = F.depth[(size_t)iv * K.W + iu];
    if (depth > F.max_depth || (F.color_rules && isnan(depth))) return false;
    const float tau = truncation_distance(F.trunc_kind, F.trunc_param, depth);
    sd = depth - qz;
    if (!(fabsf(sd) < tau + F.diag)) return false;
    wu = F.color_rules ? constant_weight(F.weight, tau) : 1.0f;
    return true;
}

// a lane's figures of one chunk: what the rule did to its voxels, and the signs it wrote
struct DeintegrateLane {
    unsigned upd = 0, clr = 0, skip = 0;
    bool pos = false, neg = false;
};

// ---- the chunk's bookkeeping ---------------------------------------------------------------------------------------------------------------
// The lanes' figures into the workgroup's LDS words (zeroed by thread 0 in front of a barrier); the caller's barrier follows.
__device__ inline void deintegrate_tally(const DeintegrateLane &L, unsigned *s_upd, unsigned *s_clr, unsigned *s_skip, unsigned *s_signs) {
    tally_count(L.upd, s_upd);
    tally_count(L.clr, s_clr);
    tally_count(L.skip, s_skip);
    tally_signs(L.pos, L.neg, s_signs);
}

// thread 0: this workgroup's share of the stats over the chunks it visits
struct DeintegrateTotals {
    unsigned long long touched = 0, upd = 0, clr = 0, skip = 0;
};

// Behind the barrier that follows the tallies, the end of one chunk of V voxels in a workgroup of T: `pairs` (block-uniform) is the
// number of (chunk, frame) pairs in which a voxel was updated or cleared -- what the single calls count as touched chunks; 0: the chunk
// was not touched.  A touched chunk is scanned for weight, noted (note_slot_updated) and, left without any, counted and reported as
// emptied (no later set touches a chunk without weight: once per call).
template <int V, int T, class View>
__device__ inline void deintegrate_chunk_end(const MapView &M, const View &G, int slot, size_t base, int idx, int idy, int idz, unsigned pairs,
                                             const unsigned *s_upd, const unsigned *s_clr, const unsigned *s_skip, const unsigned *s_signs, unsigned *s_live,
                                             DeintegrateTotals &t) {
    if (pairs) {
        // emptied?  Every weight of the chunk, each lane the quads it owns (what it stored itself, or nobody did)
        bool live = false;
        for (int q = threadIdx.x; q < V / 4; q += T) {
            const float4 w4 = *reinterpret_cast<const float4 *>(M.wgt + base + 4 * q);
            live = live || w4.x > 0.0f || w4.y > 0.0f || w4.z > 0.0f || w4.w > 0.0f;
        }
        if (__any(live) && (threadIdx.x & 63) == 0) atomicOr(s_live, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        t.skip += *s_skip;
        if (pairs) {
            note_slot_updated(M, slot, *s_signs);
            t.touched += pairs;
            t.upd += *s_upd;
            t.clr += *s_clr;
            if (!*s_live) {
                const unsigned long long at = atomicAdd(&G.stats[DS_EMPTIED], 1ull);
                if (G.emptied && at < (unsigned long long)G.max_ids) {
                    G.emptied[3 * at] = idx;
                    G.emptied[3 * at + 1] = idy;
                    G.emptied[3 * at + 2] = idz;
                }
            }
        }
    }
    // (thread 0 resets the LDS words for the next round behind its own reads; everybody else's were in front of the barrier above)
}

// behind the last chunk: the workgroup's share into the stats
template <class View>
__device__ inline void deintegrate_flush(const View &G, const DeintegrateTotals &t) {
    if (threadIdx.x != 0) return;
    if (t.touched) atomicAdd(&G.stats[DS_TOUCHED], t.touched);
    if (t.upd) atomicAdd(&G.stats[DS_UPDATED], t.upd);
    if (t.clr) atomicAdd(&G.stats[DS_CLEARED], t.clr);
    if (t.skip) atomicAdd(&G.stats[DS_SKIPPED], t.skip);
}

// Both apply kernels.  A fixed grid strides over the list, one workgroup of T per listed chunk at a time, as the chunk pass of
// kernels_rewrite.h; the depth image is gathered directly.  The view says where a chunk's frames come from.  DeintegrateView: the one
// frame is F as the kernel got it, and the list holds slots.  DeintegrateBatchView (BATCH): the list holds (slot, mask), and the frames
// of the mask are applied to every quad in ascending order before it is stored, F's camera and image filled from the table per frame;
// T threads per workgroup: a lane walks the frames of the mask once per quad it owns, each step behind a gather of the depth image, so
// the more lanes share a chunk, the shorter that chain.  The rule at the top of this file stands here, once, in the loop over a quad's
// voxels, and the kernel is a __global__ template, not two kernels around a __device__ body: a function of its own for the rule cost
// every instantiation some 35 instructions of control flow, a body function deintegrate_apply_kernel<32, 256> a VGPR (EXPERIMENTS.md).
template <int N, int T, class View>
__global__ __launch_bounds__(T) void deintegrate_apply_kernel(MapView M, View G, DeintegrateFrame F) {
    constexpr int V = N * N * N;
    constexpr bool BATCH = std::is_same<View, DeintegrateBatchView>::value;
    __shared__ unsigned s_upd, s_clr, s_skip, s_signs, s_live, s_frames;  // (s_frames: a batch's only)
    int n;  // block-uniform: written by the list kernel, which is over
    if constexpr (BATCH) n = (int)*G.listed; else n = (int)G.stats[DS_LISTED];
    DeintegrateTotals t;
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        int slot;           // block-uniform
        unsigned mask = 1u;  // (uniform by construction; said so, so that the table is read by scalar loads)
        if constexpr (BATCH) {
            const int2 entry = G.list[item];
            slot = __builtin_amdgcn_readfirstlane(entry.x);
            mask = (unsigned)__builtin_amdgcn_readfirstlane(entry.y);
        } else {
            slot = G.list[item];
        }
        int idx, idy, idz;
        unpack_id(M.slot_key[slot], idx, idy, idz);
        if (threadIdx.x == 0) {
            s_upd = s_clr = s_skip = s_signs = s_live = 0u;
            if constexpr (BATCH) s_frames = 0u;
        }
        __syncthreads();
        const ChunkCentres<N> C(F.res, F.half_res, idx, idy, idz);
        const size_t base = (size_t)slot * V;
        DeintegrateLane L;
        unsigned frames = 0u;  // a batch: the frames that updated or cleared a voxel of this lane's
        for (int q = threadIdx.x; q < V / 4; q += T) {
            const QuadIndex<N> Q(q);
            const float cy = C.y(Q.y), cz = C.z(Q.z);
            VoxelQuad<false> vox;
            bool changed = false;
            for (unsigned left = mask; left; left &= left - 1u) {
                const int k = __builtin_ctz(left);
                if constexpr (BATCH) {
                    const DeintegrateBatchEntry &E = G.table[G.first + k];
                    F.cam = E.cam;
                    F.depth = E.depth;
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float sd, wu;
                    if (!deintegrate_select(F, C.x(Q.x0 + j), cy, cz, sd, wu)) continue;
                    vox.need(M, base, Q.v0);  // (most quads of most listed chunks lie outside the band)
                    const float w = vox.weight(j);
                    if (!(w > 0.0f)) {
                        L.skip++;
                        continue;
                    }
                    const float w2 = w - wu;
                    if (!(w2 > w * 0x1p-16f)) {
                        vox.sdf(j) = 99999.0f;  // DistVoxel::Reset (DistVoxel.cpp:27-31)
                        vox.weight(j) = 0.0f;
                        L.clr++;
                    } else {
                        vox.sdf(j) = (w * vox.sdf(j) - wu * sd) / w2;
                        vox.weight(j) = w2;
                        L.upd++;
                        note_sign(vox.sdf(j), w2, L.pos, L.neg);  // (in a batch every intermediate value: the single calls would have stored it)
                    }
                    if constexpr (BATCH) frames |= 1u << k;
                    changed = true;
                }
            }
            vox.store(M, base, Q.v0, changed, false);
        }
        deintegrate_tally(L, &s_upd, &s_clr, &s_skip, &s_signs);
        if constexpr (BATCH) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) frames |= __shfl_down(frames, o);
            if ((threadIdx.x & 63) == 0 && frames) atomicOr(&s_frames, frames);
        }
        __syncthreads();
        const unsigned pairs = BATCH ? (unsigned)__popc(s_frames) : ((s_upd | s_clr) != 0u ? 1u : 0u);
        deintegrate_chunk_end<V, T>(M, G, slot, base, idx, idy, idz, pairs, &s_upd, &s_clr, &s_skip, &s_signs, &s_live, t);
    }
    deintegrate_flush(G, t);
}

}  // namespace chisel_hip
