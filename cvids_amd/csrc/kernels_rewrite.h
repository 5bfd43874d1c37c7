// kernels_rewrite.h -- the chunk pass: what merge_gather_kernel (kernels_merge.h) and the two de-integration apply
// kernels (kernels_deintegrate.h), which rewrite voxels outside the integration path, have in common.  One workgroup of T = 256 (512
// in the batched apply kernel from 16^3 on) per listed chunk at a time; a lane owns 4 consecutive x voxels (the map's lane layout:
// 16-byte accesses), quads q = thread, thread + T, ...; thread 0 ends with the chunk's note (chisel_device.h: note_slot_updated; for
// de-integration inside deintegrate_chunk_end).  The way of their few words to the host is report_words_kernel (kernels_workgroup.h).
#pragma once
#include "chisel_device.h"
#include "kernels_workgroup.h"

namespace chisel_hip {

// voxel i of chunk `id`, per axis, in the reference's order (ChunkManager.cpp:50-66, Chunk.cpp:43): ((float)i res + half_res) + (float)(N id) res
template <int N>
struct ChunkCentres {
    float res, half_res, ox, oy, oz;
    __device__ ChunkCentres(float res_, float half_res_, int idx, int idy, int idz)
        : res(res_), half_res(half_res_), ox((float)(N * idx) * res_), oy((float)(N * idy) * res_), oz((float)(N * idz) * res_) {}
    __device__ float x(int i) const { return ((float)i * res + half_res) + ox; }
    __device__ float y(int i) const { return ((float)i * res + half_res) + oy; }
    __device__ float z(int i) const { return ((float)i * res + half_res) + oz; }
};

// quad q of a chunk: the voxels v0 .. v0 + 3 = (x0 .. x0 + 3, y, z)
template <int N>
struct QuadIndex {
    int v0, x0, y, z;
    __device__ explicit QuadIndex(int q) : v0(4 * q), x0(v0 % N), y((v0 / N) % N), z(v0 / (N * N)) {}
};

// The voxels v0 .. v0 + 3 of the slot whose voxels begin at `base`: need() before the first is looked at (most quads of most listed
// chunks never are), store() behind the last.  (base and v0 apart: M.sdf + base is uniform; summed first they cost two spilled SGPRs.)
template <bool COLOR>
struct VoxelQuad {
    float4 s4, w4;
    uint4 c4 = make_uint4(0u, 0u, 0u, 0u);
    bool loaded = false;
    __device__ void need(const MapView &M, size_t base, int v0) {
        if (loaded) return;
        s4 = *reinterpret_cast<const float4 *>(M.sdf + base + v0);
        w4 = *reinterpret_cast<const float4 *>(M.wgt + base + v0);
        if (COLOR) c4 = *reinterpret_cast<const uint4 *>(M.rgbw + base + v0);
        loaded = true;
    }
    __device__ float &sdf(int j) { return (&s4.x)[j]; }
    __device__ float &weight(int j) { return (&w4.x)[j]; }
    __device__ unsigned &rgbw(int j) { return (&c4.x)[j]; }
    __device__ void store(const MapView &M, size_t base, int v0, bool dist, bool colour) const {
        if (dist) {
            *reinterpret_cast<float4 *>(M.sdf + base + v0) = s4;
            *reinterpret_cast<float4 *>(M.wgt + base + v0) = w4;
        }
        if (COLOR && colour) *reinterpret_cast<uint4 *>(M.rgbw + base + v0) = c4;
    }  // (dist / colour: one of the distance / colour voxels has changed)
};

// a voxel was written as (s, w): observed (w > 0.5: what a marching cube asks of a corner), its sign goes into the slot's summary
__device__ inline void note_sign(float s, float w, bool &pos, bool &neg) {
    if (w > 0.5f) (s < 0.0f ? neg : pos) = true;
}

// The chunk's figures: a per-lane counter, or the lanes' sign flags, across the wave, then one LDS atomic per wave into a word that
// thread 0 zeroed in front of a barrier; the caller's barrier follows.  (A word per figure: as one LDS array they cost four VGPRs.)
__device__ inline void tally_count(unsigned n, unsigned *s_word) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(s_word, n);
}
__device__ inline void tally_signs(bool pos, bool neg, unsigned *s_signs) {
    const unsigned signs = (__any(pos) ? SUM_POS : 0u) | (__any(neg) ? SUM_NEG : 0u);
    if ((threadIdx.x & 63) == 0 && signs) atomicOr(s_signs, signs);
}

}  // namespace chisel_hip
