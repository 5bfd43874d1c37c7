// kernels_coarse.h -- chisel_hip_coarse_mesh: a marching-cubes mesh over every s-th voxel of the selected chunks, packed in the
// selection's order (the host side: host_coarse.h; the stride rule and the request checks: coarse_checks.h; the definition:
// DESIGN.md 3.14).  Beside the mesher (kernels_mesh.h), whose kernels it does not touch: it shares their tables, interpolate_vertex and
// the face normal, and shade_vertices_kernel runs on its output unchanged.  The indexed mesh (kernels_indexed.h) is built from the
// pieces of this file: the lattice, the two walks and the chunk scan are written here once (the workgroup scan: kernels_workgroup.h).
//
// Chunk c of the selection has M^3 coarse cubes, M = N / s; cube (i, j, k) has its corners at the voxels s (i, j, k) + s offset_d, a
// component N meaning voxel 0 of the + neighbour.  All corners of a chunk's cubes are the (M + 1)^3 LATTICE of voxels s (li, lj, lk),
// li, lj, lk in [0, M], taken from the chunk and its up to seven + neighbours.  A walk stages the lattice into LDS (CoarseLattice) in
// slabs of COARSE_SLAB layers of cubes (COARSE_SLAB + 1 layers of samples): one float per sample and, beside it, one byte that says
// whether the sample's chunk is resident and its weight is above 0.5 -- beside it, not in the value: a NaN distance is legal input.  At
// N = 32, s = 1 that is 5 x 33^2 samples = 27 225 bytes a workgroup (five workgroups of 256 on a CU by LDS: 20 waves), at s >= 2 less
// than 8 KiB.  A layer's row is M + 1 samples, odd for every M > 1: lanes of consecutive i read consecutive words.
//
//   coarse_walk_strided     a chunk's meshed cubes, a cube per lane, strided: what the kernel does with one is its callable
//   coarse_walk_batched     the same cubes in batches of COARSE_THREADS in cube order, with the workgroup's exclusive sum of a per-cube
//                           count in front of the callable: every cube knows where its output begins
//
//   coarse_count_kernel<N>  a fixed grid strides over the chunks, a workgroup per chunk at a time: the strided walk (vertex count from
//                           c_mc_counts); the chunk's vertices and meshed cubes are summed across the workgroup and written as two ints
//   coarse_scan_kernel      one workgroup: the exclusive sum of the chunks' vertex counts (64-bit) for the emit kernel, and table,
//                           totals and the first absent id of a list into pinned memory -- what the host reads after its one wait
//   coarse_emit_kernel<N>   the batched walk over vertex counts: MeshCube's vertices (push order t + 2, t + 1, t) and the face normal
//                           thrice at first[chunk] + prefix[cube].  Not launched when the capacity is short or nothing is asked for.
#pragma once
#include "kernels_map.h"
#include "kernels_mesh.h"
#include "kernels_rewrite.h"  // ChunkCentres, tally_count
#include "kernels_workgroup.h"
#include "coarse_checks.h"

namespace chisel_hip {

static_assert(COARSE_THREADS == WORKGROUP_THREADS, "the walks and the scans take block_exclusive_scan's workgroup");

// One slab of a chunk's lattice in LDS, and the slots it is read from (trivially constructible: a kernel declares one __shared__).
template <int N>
struct CoarseLattice {
    static constexpr int SAMPLES = (COARSE_SLAB + 1) * (N + 1) * (N + 1);  // the largest staged slab: s = 1
    float val[SAMPLES];
    unsigned char ok[SAMPLES];
    int nb[8];

    // the slots of chunk (x, y, z) and its seven + neighbours, nb[dz * 4 + dy * 2 + dx]; lanes 0 .. 7 of the workgroup.  A neighbour
    // id beyond the addressable range is absent.
    __device__ void neighbours(const MapView &M, int slot) {
        if (threadIdx.x >= 8) return;
        const int d = (int)threadIdx.x;
        int ns = slot;
        if (slot >= 0 && d != 0) {
            int x, y, z;
            unpack_id(M.slot_key[slot], x, y, z);
            x += d & 1; y += (d >> 1) & 1; z += d >> 2;
            ns = (x > ID_BIAS - 2 || y > ID_BIAS - 2 || z > ID_BIAS - 2) ? -1 : hash_find_quiescent(M, x, y, z);
        }
        nb[d] = ns;
    }

    // the lattice layers lk = k0 .. k0 + layers - 1 of the chunk, sample (li, lj, lk) at ((lk - k0) L + lj) L + li, L = M + 1
    __device__ void stage(const MapView &M, int s, int Mc, int k0, int layers) {
        const int L = Mc + 1, n = layers * L * L;
        for (int t = (int)threadIdx.x; t < n; t += COARSE_THREADS) {
            const int li = t % L, lj = (t / L) % L, lz = t / (L * L);
            int vx = s * li, vy = s * lj, vz = s * (k0 + lz), d = 0;
            if (vx == N) { vx = 0; d |= 1; }
            if (vy == N) { vy = 0; d |= 2; }
            if (vz == N) { vz = 0; d |= 4; }
            const int slot = nb[d];
            float v = 0.0f;
            bool seen = false;
            if (slot >= 0) {
                const size_t o = (size_t)slot * (N * N * N) + (size_t)((vz * N + vy) * N + vx);
                seen = !(M.wgt[o] <= 0.5f);  // (weight <= 0.5 rejects: ChunkManager.cpp:273, :311, :351)
                v = M.sdf[o];
            }
            val[t] = v;
            ok[t] = seen ? 1 : 0;
        }
    }

    // cube (i, j, lz) of the staged slab: its corner distances and configuration (CalculateVertexConfiguration MarchingCubes.h:108-118),
    // or -1 when a corner is absent or unobserved
    __device__ int cube(int L, int i, int j, int lz, float sdf[8]) const {
        const int base = (lz * L + j) * L + i;
        bool observed = true;
        int index = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const int at = base + (corner_oz(d) * L + corner_oy(d)) * L + corner_ox(d);
            observed = observed && ok[at] != 0;
            sdf[d] = val[at];
            index |= (sdf[d] < 0.0f) ? (1 << d) : 0;
        }
        return observed ? index : -1;
    }
};

// The strided walk of one chunk, by every lane of the workgroup (slot: workgroup-uniform; < 0, a listed id that is not resident, has
// no cube): the neighbour look-up, begin() -- what else lanes 0 .. 7 look up per chunk --, then per slab barrier, stage, barrier, and
// cube(i, j, k, index, sdf) for every MESHED cube, a cube per lane.  The caller's barrier stands in front: the chunk before has been read.
// Mc = N / s, which the kernel divides once in front of its chunk loop (divided in here, per chunk, indexed_mark_kernel<8> came out with
// 96 registers for 57: EXPERIMENTS.md).
template <int N, class Begin, class Cube>
__device__ __forceinline__ void coarse_walk_strided(const MapView &M, CoarseLattice<N> &lat, int slot, int s, int Mc, Begin &&begin, Cube &&cube) {
    lat.neighbours(M, slot);
    begin();
    for (int k0 = 0; k0 < Mc && slot >= 0; k0 += COARSE_SLAB) {
        const int layers = min(COARSE_SLAB, Mc - k0);
        __syncthreads();  // the slots are there; the slab before has been read
        lat.stage(M, s, Mc, k0, layers + 1);
        __syncthreads();
        for (int t = (int)threadIdx.x; t < layers * Mc * Mc; t += COARSE_THREADS) {
            float sdf[8];
            const int i = t % Mc, j = (t / Mc) % Mc, lz = t / (Mc * Mc);
            const int index = lat.cube(Mc + 1, i, j, lz, sdf);
            if (index >= 0) cube(i, j, k0 + lz, index, sdf);
        }
    }
}

// The batched walk of one resident chunk: the same steps, the cubes in batches of COARSE_THREADS in cube order ((k M + j) M + i
// ascending).  count(index) is what a meshed cube will write (at most 15: a batch's sum fits an int); body(i, j, k, index, sdf, at) runs
// for every cube that writes, `at` = run + what the cubes in front of it write.  s_wave: block_exclusive_scan's.
template <int N, class Begin, class Count, class Body>
__device__ __forceinline__ void coarse_walk_batched(const MapView &M, CoarseLattice<N> &lat, int *s_wave, int slot, int s, int Mc, long long run, Begin &&begin,
                                                    Count &&count, Body &&body) {
    lat.neighbours(M, slot);
    begin();
    for (int k0 = 0; k0 < Mc; k0 += COARSE_SLAB) {
        const int layers = min(COARSE_SLAB, Mc - k0), cubes = layers * Mc * Mc;
        __syncthreads();  // the slots are there; the slab before has been read
        lat.stage(M, s, Mc, k0, layers + 1);
        __syncthreads();
        for (int base = 0; base < cubes; base += COARSE_THREADS) {
            const int t = base + (int)threadIdx.x;
            const int i = t % Mc, j = (t / Mc) % Mc, lz = t / (Mc * Mc);
            float sdf[8];
            const int index = t < cubes ? lat.cube(Mc + 1, i, j, lz, sdf) : -1;
            const int mine = index >= 0 ? count(index) : 0;
            int total;
            const int before = block_exclusive_scan(mine, s_wave, total);
            if (mine) body(i, j, k0 + lz, index, sdf, run + (long long)before);
            run += total;
        }
    }
}

// counts: two ints per chunk of the selection -- vertices, meshed cubes (a chunk whose slot is < 0, a listed id that is not resident: 0, 0)
template <int N>
__global__ __launch_bounds__(COARSE_THREADS) void coarse_count_kernel(MapView M, const int *__restrict__ slots, int n_chunks, int s, int *__restrict__ counts) {
    __shared__ CoarseLattice<N> lat;
    __shared__ unsigned s_vertices, s_cubes;
    const int Mc = N / s;
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        __syncthreads();  // (the chunk before: its slots, its sums and its last slab have been read)
        if (threadIdx.x == 8) { s_vertices = 0u; s_cubes = 0u; }
        unsigned nv = 0u, nc = 0u;
        coarse_walk_strided<N>(M, lat, slots[c], s, Mc, [] {}, [&](int, int, int, int index, const float *) {
            nv += c_mc_counts[index];
            nc++;
        });
        __syncthreads();  // (s_vertices, s_cubes are zero for everybody)
        tally_count(nv, &s_vertices);
        tally_count(nc, &s_cubes);
        __syncthreads();
        if (threadIdx.x == 0) {
            counts[2 * (size_t)c] = (int)s_vertices;  // (<= 15 N^3 = 491 520)
            counts[2 * (size_t)c + 1] = (int)s_cubes;
        }
    }
}

// The chunk half of a scan kernel, by every lane of its one workgroup: first[c] = counts[2 c] of the chunks in front of c, the same
// with the count as the chunk's row of the pinned table `rows`, and the first c whose slot is < 0 into *s_absent (atomicMin: the
// caller set it to INT_MAX in front of a barrier).  Chunks are taken COARSE_THREADS at a time, the sum carried from batch to batch.
// -> the sum; `cubes`, and `nonempty` unless null, take the lane's share of the meshed cubes and of the chunks with a count above 0.
__device__ inline long long scan_chunks(const int *__restrict__ slots, const int *__restrict__ counts, int n_chunks, long long *__restrict__ first, long long *rows,
                                        long long *s_wave, int *s_absent, long long &cubes, long long *nonempty) {
    long long run = 0;
    for (int base = 0; base < n_chunks; base += COARSE_THREADS) {
        const int c = base + (int)threadIdx.x;
        const long long mine = c < n_chunks ? (long long)counts[2 * (size_t)c] : 0;
        if (c < n_chunks) {
            cubes += counts[2 * (size_t)c + 1];
            if (nonempty) *nonempty += mine > 0 ? 1 : 0;
            if (slots[c] < 0) atomicMin(s_absent, c);
        }
        long long total;
        const long long at = run + block_exclusive_scan(mine, s_wave, total);
        if (c < n_chunks) {
            first[c] = at;
            rows[2 * (size_t)c] = at;
            rows[2 * (size_t)c + 1] = mine;
        }
        run += total;
    }
    return run;
}

// One workgroup.  first[c] = vertices of the chunks in front of c; host: COARSE_HOST_WORDS words (CO_*), then the table (first vertex,
// vertices) of every chunk -- pinned memory.
__global__ __launch_bounds__(COARSE_THREADS) void coarse_scan_kernel(const int *__restrict__ slots, const int *__restrict__ counts, int n_chunks, long long *__restrict__ first,
                                                                     long long *host) {
    __shared__ long long s_wave[COARSE_THREADS / 64];
    __shared__ long long s_cubes, s_nonempty;
    __shared__ int s_absent;
    if (threadIdx.x == 0) { s_cubes = 0; s_nonempty = 0; s_absent = 0x7fffffff; }
    __syncthreads();
    long long cubes = 0, nonempty = 0;
    const long long run = scan_chunks(slots, counts, n_chunks, first, host + COARSE_HOST_WORDS, s_wave, &s_absent, cubes, &nonempty);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cubes += __shfl_down(cubes, o);
        nonempty += __shfl_down(nonempty, o);
    }
    if (((int)threadIdx.x & 63) == 0) {
        atomicAdd((unsigned long long *)&s_cubes, (unsigned long long)cubes);
        atomicAdd((unsigned long long *)&s_nonempty, (unsigned long long)nonempty);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        host[CO_CHUNKS] = n_chunks;
        host[CO_NONEMPTY] = s_nonempty;
        host[CO_CUBES] = s_cubes;
        host[CO_VERTICES] = run;
        host[CO_ABSENT] = s_absent == 0x7fffffff ? -1 : s_absent;
        for (int w = CO_ABSENT + 1; w < COARSE_HOST_WORDS; w++) host[w] = 0;
    }
}

// vertices / normals: 3 floats per vertex, chunk c's at first[c]; normals may be null
template <int N>
__global__ __launch_bounds__(COARSE_THREADS) void coarse_emit_kernel(MapView M, MeshParams P, const int *__restrict__ slots, int n_chunks, int s, const long long *__restrict__ first,
                                                                     const int *__restrict__ counts, float *__restrict__ vertices, float *__restrict__ normals) {
    __shared__ CoarseLattice<N> lat;
    __shared__ int s_wave[COARSE_THREADS / 64];
    const int Mc = N / s;
    const float step = (float)s * P.res;  // rounded once
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        const int slot = slots[c];
        if (slot < 0 || counts[2 * (size_t)c] == 0) continue;  // (workgroup-uniform)
        __syncthreads();  // (the chunk before: its slots and its last slab have been read)
        int idx, idy, idz;
        unpack_id(M.slot_key[slot], idx, idy, idz);
        const ChunkCentres<N> C(P.res, P.half_res, idx, idy, idz);
        coarse_walk_batched<N>(
            M, lat, s_wave, slot, s, Mc, first[c], [] {}, [](int index) { return (int)c_mc_counts[index]; },
            [&](int i, int j, int k, int index, const float *sdf, long long at) {
                const int nv = (int)c_mc_counts[index];
                const unsigned long long row = c_mc_cases[index];
                // cube origin = centroid of the base voxel + chunk origin (ChunkManager.cpp:61, :404)
                const f3v coords = mk3(C.x(s * i), C.y(s * j), C.z(s * k));
                for (int tv = 0; tv < nv; tv += 3) {
                    f3v p[3];
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const int ed = (int)((row >> (4 * (tv + 2 - a))) & 0xF);
                        const int e0 = c_mc_edges[ed] & 0xF, e1 = c_mc_edges[ed] >> 4;
                        const f3v c0 = add3(coords, mk3((float)corner_ox(e0) * step, (float)corner_oy(e0) * step, (float)corner_oz(e0) * step));
                        const f3v c1 = add3(coords, mk3((float)corner_ox(e1) * step, (float)corner_oy(e1) * step, (float)corner_oz(e1) * step));
                        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
                        for (int d = 0; d < 8; d++) {  // (selects, not an indexed array: the distances stay in registers)
                            s0 = d == e0 ? sdf[d] : s0;
                            s1 = d == e1 ? sdf[d] : s1;
                        }
                        p[a] = interpolate_vertex(c0, c1, s0, s1);
                    }
                    const f3v fn = normalized3(cross3v(sub3(p[1], p[0]), sub3(p[2], p[0])));  // MarchingCubes.h:95-101
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        float *v = vertices + 3 * ((size_t)at + (size_t)(tv + a));
                        v[0] = p[a].x; v[1] = p[a].y; v[2] = p[a].z;
                        if (normals) {
                            float *nn = normals + 3 * ((size_t)at + (size_t)(tv + a));
                            nn[0] = fn.x; nn[1] = fn.y; nn[2] = fn.z;
                        }
                    }
                }
            });
    }
}

}  // namespace chisel_hip
