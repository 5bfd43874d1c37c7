// kernels_indexed.h -- chisel_hip_indexed_mesh: the coarse mesh's triangles (kernels_coarse.h) over ONE vertex per crossed lattice edge
// (the host side: host_indexed.h; the request checks, the extras and the size arithmetic: indexed_checks.h; the definition:
// DESIGN.md 3.15).  Built from the coarse mesh's pieces: CoarseLattice, coarse_walk_strided, coarse_walk_batched and scan_chunks are used
// as they are (the workgroup scan: kernels_workgroup.h), and shade_vertices_kernel runs on the vertices unchanged.  What this file adds is what a walk's
// callable does with a cube, the owners (indexed_owners) and the rows.
//
// A lattice point l = (li, lj, lk) in [0, M)^3 of an OWNER chunk owns the three edges l -> l + e_a.  An owner keeps R = 3 M^2 ROWS, row
// (a M + lk) M + lj, a 32-bit mask each (bit li: the edge is used) and an exclusive prefix each (used edges of the owner's rows in
// front).  The id of a used edge is first[owner] + prefix[row] + popcount(mask[row] below bit li): owners in the host's order, inside
// an owner ascending (a, lk, lj, li).  owner_of_slot turns a pool slot into the owner's index.
//
//   indexed_owner_kernel     a thread per owner: owner_of_slot[slot] = index
//   indexed_mark_kernel<N>   a workgroup per selected chunk at a time, the strided walk: every MESHED cube ORs the bits
//                            of its crossed edges into the owners' rows (global vector atomics; an edge has up to four cubes) and
//                            counts its triangles; per chunk two ints: triangles, meshed cubes
//   indexed_rows_kernel      a workgroup per owner at a time: the exclusive sum of its rows' popcounts, and the owner's vertices
//   indexed_scan_kernel      one workgroup: owners' first vertices, chunks' first triangles, totals and both tables into pinned memory
//   indexed_vertex_kernel<N> a workgroup per owner at a time, a lane per row: one position per set bit, interpolate_vertex from the
//                            lower end P (the owner's voxel s l) to the upper Q = P + step e_a, the two distances read from the
//                            owner and, for an upper end at N, from voxel 0 of its + neighbour along a
//   indexed_index_kernel<N>  the batched walk over triangle counts: three ids per
//                            triangle in MeshCube's push order (t + 2, t + 1, t), looked up through masks and prefixes
#pragma once
#include "kernels_coarse.h"
#include "kernels_workgroup.h"
#include "indexed_checks.h"

namespace chisel_hip {

// edge `ed` of cube (i, j, k): the lower lattice point of the edge, wrapped into its owner, and the axis.  d: which of the cube's
// eight chunks (CoarseLattice::nb's numbering) owns it.
struct LatticeEdge {
    int d, row, li;
};
__device__ inline LatticeEdge lattice_edge(int ed, int i, int j, int k, int Mc) {
    const int e0 = c_mc_edges[ed] & 0xF, e1 = c_mc_edges[ed] >> 4;
    const int x0 = corner_ox(e0), y0 = corner_oy(e0), z0 = corner_oz(e0);
    const int x1 = corner_ox(e1), y1 = corner_oy(e1), z1 = corner_oz(e1);
    const int a = x0 != x1 ? 0 : (y0 != y1 ? 1 : 2);
    int li = i + min(x0, x1), lj = j + min(y0, y1), lk = k + min(z0, z1), d = 0;
    if (li == Mc) { li = 0; d |= 1; }
    if (lj == Mc) { lj = 0; d |= 2; }
    if (lk == Mc) { lk = 0; d |= 4; }
    return LatticeEdge{d, (a * Mc + lk) * Mc + lj, li};
}

__global__ __launch_bounds__(256) void indexed_owner_kernel(const int *__restrict__ slots, int n_owners, int *__restrict__ owner_of_slot, int pool) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_owners) return;
    const int slot = slots[o];
    if (slot >= 0 && slot < pool) owner_of_slot[slot] = o;
}

// the owner index of each of the lattice's eight slots (-1: no owner), by lanes 0 .. 7 behind lat.neighbours without a barrier: lane d
// reads the word it wrote itself
template <int N>
__device__ inline void indexed_owners(const CoarseLattice<N> &lat, const int *__restrict__ owner_of_slot, int pool, int *s_owner) {
    if (threadIdx.x >= 8) return;
    const int ns = lat.nb[threadIdx.x];
    s_owner[threadIdx.x] = (ns >= 0 && ns < pool) ? owner_of_slot[ns] : -1;
}

// counts: two ints per selected chunk -- triangles, meshed cubes (a listed id that is not resident: 0, 0)
template <int N>
__global__ __launch_bounds__(COARSE_THREADS) void indexed_mark_kernel(MapView M, const int *__restrict__ slots, int n_chunks, int s, const int *__restrict__ owner_of_slot, int pool,
                                                                      unsigned *masks, int *__restrict__ counts) {
    __shared__ CoarseLattice<N> lat;
    __shared__ int s_owner[8];
    __shared__ unsigned s_triangles, s_cubes;
    const int Mc = N / s;
    const size_t R = (size_t)(3 * Mc * Mc);
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        __syncthreads();  // (the chunk before: its slots, its owners, its sums and its last slab have been read)
        if (threadIdx.x == 8) { s_triangles = 0u; s_cubes = 0u; }
        unsigned nt = 0u, nc = 0u;
        coarse_walk_strided<N>(
            M, lat, slots[c], s, Mc, [&] { indexed_owners(lat, owner_of_slot, pool, s_owner); },
            [&](int i, int j, int k, int index, const float *) {
                nc++;
                nt += c_mc_counts[index] / 3;
                if (index == 0 || index == 255) return;
#pragma unroll
                for (int ed = 0; ed < 12; ed++) {
                    const int e0 = c_mc_edges[ed] & 0xF, e1 = c_mc_edges[ed] >> 4;
                    if ((((index >> e0) ^ (index >> e1)) & 1) == 0) continue;  // (crossed: the corners' bits differ)
                    const LatticeEdge E = lattice_edge(ed, i, j, k, Mc);
                    const int owner = s_owner[E.d];
                    if (owner >= 0) atomicOr(&masks[(size_t)owner * R + (size_t)E.row], 1u << E.li);  // (a meshed cube's chunks are resident owners)
                }
            });
        __syncthreads();  // (s_triangles, s_cubes are zero for everybody)
        tally_count(nt, &s_triangles);
        tally_count(nc, &s_cubes);
        __syncthreads();
        if (threadIdx.x == 0) {
            counts[2 * (size_t)c] = (int)s_triangles;  // (<= 5 N^3 = 163 840)
            counts[2 * (size_t)c + 1] = (int)s_cubes;
        }
    }
}

// prefix[o R + r] = used edges of owner o in the rows in front of r; owner_counts[o] = its used edges (<= 3 M^3 = 98 304)
__global__ __launch_bounds__(COARSE_THREADS) void indexed_rows_kernel(const unsigned *__restrict__ masks, int n_owners, int rows, unsigned *__restrict__ prefix,
                                                                      int *__restrict__ owner_counts) {
    __shared__ long long s_wave[COARSE_THREADS / 64];
    for (int o = (int)blockIdx.x; o < n_owners; o += (int)gridDim.x) {
        const size_t at = (size_t)o * (size_t)rows;
        long long run = 0;
        for (int base = 0; base < rows; base += COARSE_THREADS) {
            const int r = base + (int)threadIdx.x;
            const long long mine = r < rows ? (long long)__popc(masks[at + r]) : 0;
            long long total;
            const long long before = block_exclusive_scan(mine, s_wave, total);
            if (r < rows) prefix[at + r] = (unsigned)(run + before);
            run += total;
        }
        if (threadIdx.x == 0) owner_counts[o] = (int)run;
    }
}

// One workgroup.  owner_first[o] = vertices of the owners in front of o, tri_first[c] = triangles of the chunks in front of c; host:
// INDEXED_HOST_WORDS words (IX_*), the chunk table (first triangle, triangles) of the n_chunks selected chunks, then the owner table
// (first vertex, vertices; vertices = -1 for an owner that is not resident) of the n_owners owners -- pinned memory.
__global__ __launch_bounds__(COARSE_THREADS) void indexed_scan_kernel(const int *__restrict__ slots, const int *__restrict__ counts, int n_chunks, const int *__restrict__ owner_counts,
                                                                      int n_owners, long long *__restrict__ owner_first, long long *__restrict__ tri_first, long long *host) {
    __shared__ long long s_wave[COARSE_THREADS / 64];
    __shared__ long long s_cubes;
    __shared__ int s_absent;
    if (threadIdx.x == 0) { s_cubes = 0; s_absent = 0x7fffffff; }
    __syncthreads();
    long long cubes = 0;
    const long long triangles = scan_chunks(slots, counts, n_chunks, tri_first, host + INDEXED_HOST_WORDS, s_wave, &s_absent, cubes, nullptr);
    long long *owner_rows = host + INDEXED_HOST_WORDS + 2 * (size_t)n_chunks;
    long long run = 0;
    for (int base = 0; base < n_owners; base += COARSE_THREADS) {
        const int o = base + (int)threadIdx.x;
        const long long mine = o < n_owners ? (long long)owner_counts[o] : 0;
        long long total;
        const long long at = run + block_exclusive_scan(mine, s_wave, total);
        if (o < n_owners) {
            owner_first[o] = at;
            owner_rows[2 * (size_t)o] = at;
            owner_rows[2 * (size_t)o + 1] = slots[o] < 0 ? -1 : mine;
        }
        run += total;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cubes += __shfl_down(cubes, o);
    if (((int)threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&s_cubes, (unsigned long long)cubes);
    __syncthreads();
    if (threadIdx.x == 0) {
        host[IX_CHUNKS] = n_chunks;
        host[IX_OWNERS] = n_owners;
        host[IX_CUBES] = s_cubes;
        host[IX_VERTICES] = run;
        host[IX_TRIANGLES] = triangles;
        host[IX_ABSENT] = s_absent == 0x7fffffff ? -1 : s_absent;
        for (int w = IX_ABSENT + 1; w < INDEXED_HOST_WORDS; w++) host[w] = 0;
    }
}

// vertices: 3 floats per used edge, owner o's at owner_first[o]
template <int N>
__global__ __launch_bounds__(COARSE_THREADS) void indexed_vertex_kernel(MapView M, MeshParams P, const int *__restrict__ slots, int n_owners, int s, const unsigned *__restrict__ masks,
                                                                        const unsigned *__restrict__ prefix, const int *__restrict__ owner_counts,
                                                                        const long long *__restrict__ owner_first, float *__restrict__ vertices) {
    __shared__ int s_up[3];  // the slots of the + neighbours along x, y, z
    const int Mc = N / s, rows = 3 * Mc * Mc;
    const float step = (float)s * P.res;  // rounded once
    for (int o = (int)blockIdx.x; o < n_owners; o += (int)gridDim.x) {
        const int slot = slots[o];
        if (slot < 0 || owner_counts[o] == 0) continue;  // (workgroup-uniform)
        __syncthreads();  // (the owner before: its neighbours have been read)
        int idx, idy, idz;
        unpack_id(M.slot_key[slot], idx, idy, idz);
        if (threadIdx.x < 3) {
            const int a = (int)threadIdx.x;
            const int x = idx + (a == 0), y = idy + (a == 1), z = idz + (a == 2);
            s_up[a] = (x > ID_BIAS - 2 || y > ID_BIAS - 2 || z > ID_BIAS - 2) ? -1 : hash_find_quiescent(M, x, y, z);
        }
        __syncthreads();
        const ChunkCentres<N> C(P.res, P.half_res, idx, idy, idz);
        const size_t at = (size_t)o * (size_t)rows;
        const long long first = owner_first[o];
        for (int r = (int)threadIdx.x; r < rows; r += COARSE_THREADS) {
            unsigned mask = masks[at + r];
            if (!mask) continue;
            const int a = r / (Mc * Mc), lk = (r / Mc) % Mc, lj = r % Mc;
            size_t id = (size_t)(first + (long long)prefix[at + r]);
            while (mask) {
                const int li = __ffs(mask) - 1;
                mask &= mask - 1u;
                const int v[3] = {s * li, s * lj, s * lk};
                int u[3] = {v[0], v[1], v[2]};
                u[a] += s;
                int upper = slot;
                if (u[a] == N) { u[a] = 0; upper = s_up[a]; }
                if (upper >= 0) {  // (a used edge's ends are observed voxels of resident chunks)
                    const float lo = M.sdf[(size_t)slot * (N * N * N) + (size_t)((v[2] * N + v[1]) * N + v[0])];
                    const float hi = M.sdf[(size_t)upper * (N * N * N) + (size_t)((u[2] * N + u[1]) * N + u[0])];
                    const f3v p = mk3(C.x(v[0]), C.y(v[1]), C.z(v[2]));
                    const f3v q = add3(p, mk3(a == 0 ? step : 0.0f, a == 1 ? step : 0.0f, a == 2 ? step : 0.0f));
                    const f3v w = interpolate_vertex(p, q, lo, hi);
                    float *out = vertices + 3 * id;
                    out[0] = w.x; out[1] = w.y; out[2] = w.z;
                }
                id++;
            }
        }
    }
}

// indices: 3 ints per triangle, chunk c's at tri_first[c]
template <int N>
__global__ __launch_bounds__(COARSE_THREADS) void indexed_index_kernel(MapView M, const int *__restrict__ slots, int n_chunks, int s, const int *__restrict__ owner_of_slot, int pool,
                                                                       const unsigned *__restrict__ masks, const unsigned *__restrict__ prefix,
                                                                       const long long *__restrict__ owner_first, const long long *__restrict__ tri_first,
                                                                       const int *__restrict__ counts, int *__restrict__ indices) {
    __shared__ CoarseLattice<N> lat;
    __shared__ int s_owner[8];
    __shared__ long long s_first[8];
    __shared__ int s_wave[COARSE_THREADS / 64];
    const int Mc = N / s;
    const size_t R = (size_t)(3 * Mc * Mc);
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        const int slot = slots[c];
        if (slot < 0 || counts[2 * (size_t)c] == 0) continue;  // (workgroup-uniform)
        __syncthreads();  // (the chunk before: its slots, its owners and its last slab have been read)
        coarse_walk_batched<N>(
            M, lat, s_wave, slot, s, Mc, tri_first[c],
            [&] {
                indexed_owners(lat, owner_of_slot, pool, s_owner);
                if (threadIdx.x < 8) s_first[threadIdx.x] = s_owner[threadIdx.x] >= 0 ? owner_first[s_owner[threadIdx.x]] : 0;
            },
            [](int index) { return (int)c_mc_counts[index] / 3; },
            [&](int i, int j, int k, int index, const float *, long long at) {
                int *out = indices + 3 * (size_t)at;
                const int nv = (int)c_mc_counts[index];
                const unsigned long long row = c_mc_cases[index];
                for (int tv = 0; tv < nv; tv += 3) {
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const int ed = (int)((row >> (4 * (tv + 2 - a))) & 0xF);
                        const LatticeEdge E = lattice_edge(ed, i, j, k, Mc);
                        const int owner = s_owner[E.d];
                        int id = -1;
                        if (owner >= 0) {
                            const size_t w = (size_t)owner * R + (size_t)E.row;
                            id = (int)(s_first[E.d] + (long long)prefix[w] + (long long)__popc(masks[w] & ((1u << E.li) - 1u)));
                        }
                        out[tv + a] = id;
                    }
                }
            });
    }
}

}  // namespace chisel_hip
