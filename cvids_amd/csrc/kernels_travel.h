// kernels_travel.h -- chisel_hip_travel_field: the least travel cost from seed voxels to every traversable voxel of a window, the step
// back towards a seed, and a row per group of target voxels (the host side: host_travel.h; the refusals, the tile grid, the scratch
// sizes and the walk of chisel_hip_travel_path: travel_checks.h; the definition: DESIGN.md 3.19).  Not kernels of the reference.  One
// fp32 compare per voxel in the seed (frontier_seed_kernel, as it is), integers after it: the costs are the unique fixed point of a
// relaxation in which values only fall, so the answer is a pure function of the map and the request, whatever the order of execution.
//
//   travel_plane_kernel     a wave per 64-bit word of the window: the TRAVERSABLE plane by ballot -- free, and with a clearance
//                           dist2 == -1 of the distance field's kernels --, every cost "infinite", the state totals.
//   travel_seed_kernel      a thread per seed: cost 0 on a traversable voxel and its tile flagged for round 0; else counted as ignored.
//   travel_round_kernel     a workgroup per 16 x 16 x 8 tile, 8 voxels of one row per lane.  A tile that is not flagged for this round
//                           leaves at once.  Otherwise: the tile and a one-voxel halo of costs into LDS (18 x 18 x 10 ints), a gather
//                           relaxation in LDS -- each lane computes its own eight voxels' minima over the moves from what LDS holds,
//                           the workgroup meets, each lane writes its own, __syncthreads_or tells whether anything fell --, the lowered
//                           voxels back to global memory, and a flag FOR THE NEXT ROUND on each neighbouring tile a lowered rim
//                           voxel has a move into.  A halo read that another workgroup lowers in the same round may be stale: that
//                           workgroup flags this tile.  Nobody waits for anybody; a kernel boundary is the only synchronisation
//                           between tiles.  The flags are double-buffered: a tile clears its own flag of this round, which is the
//                           next round's "next".
//   travel_count_kernel     one workgroup: the tiles flagged for the round after the batch, into a control word.
//   travel_finish_kernel    a lane per voxel: "infinite" -> -1, STEP from the converged costs alone, reached and the largest cost by
//                           wave sums, the outputs asked for.
//   travel_targets_kernel   a thread per target row: rows and reached by atomicAdd, (cost << 32) | linear index by one 64-bit
//                           atomicMin; a wave whose rows share a group adds once.  travel_table_kernel: the rows into pinned memory.
#pragma once
#include "kernels_frontier.h"  // frontier_seed_kernel, the wide planes, frontier_wave_sum
#include "travel_checks.h"

namespace chisel_hip {

static_assert(TRAVEL_TILE_X == FRONTIER_TILE_X && TRAVEL_TILE_Y == FRONTIER_TILE_Y && TRAVEL_TILE_Z == FRONTIER_TILE_Z && TRAVEL_THREADS == FRONTIER_THREADS,
              "the rounds' tile is the frontiers'");
static_assert(TRAVEL_TILE_X == 16 && TRAVEL_TILE_Y * TRAVEL_TILE_Z * 2 == TRAVEL_THREADS, "a thread of a tile takes 8 voxels of one of its 128 rows");

constexpr int TRAVEL_HALO_X = TRAVEL_TILE_X + 2, TRAVEL_HALO_Y = TRAVEL_TILE_Y + 2, TRAVEL_HALO_Z = TRAVEL_TILE_Z + 2;
constexpr int TRAVEL_HALO_VOXELS = TRAVEL_HALO_X * TRAVEL_HALO_Y * TRAVEL_HALO_Z;  // 3240 ints, 12 960 bytes

struct TravelView {
    int dims[3];
    int tiles[3];
    int level;          // 1, 2, 3 non-zero coordinates of a move for connectivity 6, 18, 26
    int step_cost[3];   // face, edge, corner
    int max_cost;
    int words_per_row;
    long long words, voxels;
    const unsigned long long *trav;  // [nz][ny][words_per_row]
    int *cost;                       // [voxels]
    int *flags;                      // [2][n_tiles]
    long long n_tiles;
    unsigned long long *ctl;         // [TRAVEL_HOST_WORDS] TC_*
};

// A wave per word of the window, a lane per voxel (FrontierLane's indexing).  X: the wide planes of the seed.
__global__ __launch_bounds__(TRAVEL_THREADS) void travel_plane_kernel(FrontierView X, const int *__restrict__ dist2, unsigned long long *__restrict__ trav,
                                                                      int *__restrict__ cost, unsigned long long *__restrict__ ctl) {
    const FrontierLane L(X);
    if (!L.in_word) return;  // (the whole wave)
    const int lane = (int)threadIdx.x & 63;
    const unsigned long long mask = frontier_word_mask(X, L.w);
    const unsigned long long free_bits = frontier_wide_bits(frontier_wide_row(X, X.wide_free, L.y, L.z), X.wide_words_per_row, L.w, 1) & mask;
    const unsigned long long unknown_bits = frontier_wide_bits(frontier_wide_row(X, X.wide_unknown, L.y, L.z), X.wide_words_per_row, L.w, 1) & mask;
    const bool inside = L.x < X.dims[0];
    bool ok = (free_bits >> lane) & 1ull;
    if (ok && dist2) ok = dist2[L.v] == -1;
    const unsigned long long bits = __ballot(ok);
    if (inside) cost[L.v] = TRAVEL_INFINITE;
    if (lane == 0) {
        trav[L.word] = bits;
        if (unknown_bits) atomicAdd(&ctl[TC_UNKNOWN], (unsigned long long)__popcll(unknown_bits));
        if (free_bits) atomicAdd(&ctl[TC_FREE], (unsigned long long)__popcll(free_bits));
        if (bits) atomicAdd(&ctl[TC_TRAVERSABLE], (unsigned long long)__popcll(bits));
    }
}

__device__ inline bool travel_bit(const TravelView &T, int x, int y, int z) {
    return (T.trav[((long long)z * T.dims[1] + y) * T.words_per_row + (x >> 6)] >> (x & 63)) & 1ull;
}
__device__ inline int travel_tile_of(const TravelView &T, int x, int y, int z) {
    return ((z / TRAVEL_TILE_Z) * T.tiles[1] + y / TRAVEL_TILE_Y) * T.tiles[0] + x / TRAVEL_TILE_X;
}

// seeds: [n][3] window-relative, every one inside the window (the host checked)
__global__ __launch_bounds__(TRAVEL_THREADS) void travel_seed_kernel(TravelView T, const int *__restrict__ seeds, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = seeds[3 * i], y = seeds[3 * i + 1], z = seeds[3 * i + 2];
    if (travel_bit(T, x, y, z)) {
        T.cost[((long long)z * T.dims[1] + y) * T.dims[0] + x] = 0;  // (duplicates store the same value)
        // the seed's tile, and every tile a move from the seed leads into: a round wakes the neighbours of what it LOWERED, and
        // nothing lowers a seed
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int ux = x + dx, uy = y + dy, uz = z + dz;
                    if ((unsigned)ux < (unsigned)T.dims[0] && (unsigned)uy < (unsigned)T.dims[1] && (unsigned)uz < (unsigned)T.dims[2])
                        T.flags[travel_tile_of(T, ux, uy, uz)] = 1;
                }
        atomicAdd(&T.ctl[TC_SEEDS_USED], 1ull);
    } else {
        atomicAdd(&T.ctl[TC_SEEDS_IGNORED], 1ull);
    }
}

// the cost of a move with k non-zero coordinates; 0 for no move of the connectivity
__device__ inline int travel_move_cost(const TravelView &T, int dx, int dy, int dz) {
    const int k = (dx != 0) + (dy != 0) + (dz != 0);
    return k >= 1 && k <= T.level ? T.step_cost[k - 1] : 0;
}

// One workgroup per tile; `round` picks the flags: [round & 1] is read and cleared, [(round + 1) & 1] is set.
__global__ __launch_bounds__(TRAVEL_THREADS) void travel_round_kernel(TravelView T, int round) {
    __shared__ int s_cost[TRAVEL_HALO_VOXELS];
    __shared__ unsigned s_wake;  // bit (tz + 1) * 9 + (ty + 1) * 3 + (tx + 1): the neighbouring tile at that offset is to be flagged
    const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
    int *mine_flag = T.flags + (long long)(round & 1) * T.n_tiles + tile;
    if (*mine_flag == 0) return;  // (uniform over the workgroup: the flag was written before this launch)
    __syncthreads();              // every lane has read the flag ...
    if (tid == 0) {
        *mine_flag = 0;           // ... which is the next round's "next"
        s_wake = 0u;
        atomicAdd(&T.ctl[TC_TILE_VISITS], 1ull);
        atomicMax(&T.ctl[TC_ROUNDS], (unsigned long long)(round + 1));
    }
    const int tx = tile % T.tiles[0], ty = (tile / T.tiles[0]) % T.tiles[1], tz = tile / (T.tiles[0] * T.tiles[1]);
    const int x0 = tx * TRAVEL_TILE_X, y0 = ty * TRAVEL_TILE_Y, z0 = tz * TRAVEL_TILE_Z;
    const int nx = T.dims[0], ny = T.dims[1], nz = T.dims[2];
    for (int i = tid; i < TRAVEL_HALO_VOXELS; i += TRAVEL_THREADS) {
        const int hx = i % TRAVEL_HALO_X, hy = (i / TRAVEL_HALO_X) % TRAVEL_HALO_Y, hz = i / (TRAVEL_HALO_X * TRAVEL_HALO_Y);
        const int x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
        const bool inside = (unsigned)x < (unsigned)nx && (unsigned)y < (unsigned)ny && (unsigned)z < (unsigned)nz;
        // (a voxel that is not traversable stays "infinite" for ever: the halo needs no bits.  Relaxed and agent-wide: another tile's
        // workgroup may be writing it.)
        s_cost[i] = inside ? __hip_atomic_load(&T.cost[((long long)z * ny + y) * nx + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : TRAVEL_INFINITE;
    }
    const int r = tid >> 1, ly = r % TRAVEL_TILE_Y, lz = r / TRAVEL_TILE_Y, b0 = (tid & 1) * 8;
    const int y = y0 + ly, z = z0 + lz;
    unsigned bits = 0u;  // the traversable ones of this lane's eight voxels
    if (y < ny && z < nz) bits = (unsigned)(T.trav[((long long)z * ny + y) * T.words_per_row + (x0 >> 6)] >> ((x0 & 63) + b0)) & 0xffu;
    const int at0 = ((lz + 1) * TRAVEL_HALO_Y + (ly + 1)) * TRAVEL_HALO_X + (b0 + 1);  // this lane's first voxel in s_cost
    __syncthreads();
    int first[8], now[8];
#pragma unroll
    for (int j = 0; j < 8; j++) first[j] = now[j] = s_cost[at0 + j];
    const int face = T.step_cost[0];
    for (;;) {
        int changed = 0;
        if (bits) {
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++) {
                    const int *row = s_cost + at0 + (dz * TRAVEL_HALO_Y + dy) * TRAVEL_HALO_X;
                    int v[10];  // the row's voxels b0 - 1 ... b0 + 8
#pragma unroll
                    for (int j = 0; j < 10; j++) v[j] = row[j - 1];
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const int c = travel_move_cost(T, dx, dy, dz);
                        if (!c) continue;
#pragma unroll
                        for (int j = 0; j < 8; j++) now[j] = min(now[j], v[j + 1 + dx] + c);
                    }
                }
            // along the lane's own eight voxels the faces at once, both ways
#pragma unroll
            for (int j = 1; j < 8; j++)
                if ((bits >> (j - 1)) & 1u) now[j] = min(now[j], now[j - 1] + face);
#pragma unroll
            for (int j = 6; j >= 0; j--)
                if ((bits >> (j + 1)) & 1u) now[j] = min(now[j], now[j + 1] + face);
        }
        __syncthreads();  // every lane has read what it needs of the others'
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int before = s_cost[at0 + j];
            if (((bits >> j) & 1u) && now[j] < before && now[j] <= T.max_cost) {
                s_cost[at0 + j] = now[j];
                changed = 1;
            } else {
                now[j] = before;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    // ---- what fell goes back; the rim voxels among it wake the neighbours
    unsigned wake = 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (now[j] >= first[j]) continue;
        const int lx = b0 + j;
        __hip_atomic_store(&T.cost[((long long)z * ny + y) * nx + (x0 + lx)], now[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lx != 0 && lx != TRAVEL_TILE_X - 1 && ly != 0 && ly != TRAVEL_TILE_Y - 1 && lz != 0 && lz != TRAVEL_TILE_Z - 1) continue;
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if (!travel_move_cost(T, dx, dy, dz)) continue;
                    const int jx = lx + dx, jy = ly + dy, jz = lz + dz;
                    const int ox = jx < 0 ? -1 : (jx >= TRAVEL_TILE_X ? 1 : 0), oy = jy < 0 ? -1 : (jy >= TRAVEL_TILE_Y ? 1 : 0), oz = jz < 0 ? -1 : (jz >= TRAVEL_TILE_Z ? 1 : 0);
                    if (ox | oy | oz) wake |= 1u << travel_code(ox, oy, oz);
                }
    }
    if (wake) atomicOr(&s_wake, wake);
    __syncthreads();
    if (tid < 27 && ((s_wake >> tid) & 1u)) {
        const int ux = tx + tid % 3 - 1, uy = ty + (tid / 3) % 3 - 1, uz = tz + tid / 9 - 1;
        if ((unsigned)ux < (unsigned)T.tiles[0] && (unsigned)uy < (unsigned)T.tiles[1] && (unsigned)uz < (unsigned)T.tiles[2])
            T.flags[(long long)((round + 1) & 1) * T.n_tiles + ((long long)uz * T.tiles[1] + uy) * T.tiles[0] + ux] = 1;
    }
}

// One workgroup: how many tiles are flagged for round `round`.
__global__ __launch_bounds__(TRAVEL_THREADS) void travel_count_kernel(TravelView T, int round) {
    __shared__ int s_wave[TRAVEL_THREADS / 64];
    const int *flags = T.flags + (long long)(round & 1) * T.n_tiles;
    int n = 0;
    for (long long i = threadIdx.x; i < T.n_tiles; i += TRAVEL_THREADS) n += flags[i] != 0;
    n = frontier_wave_sum(n);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < TRAVEL_THREADS / 64; w++) sum += s_wave[w];
        T.ctl[TC_FLAGGED] = (unsigned long long)sum;
    }
}

// A lane per voxel.  The scratch costs stay as they are (a neighbour reads them); X only for the state.
__global__ __launch_bounds__(TRAVEL_THREADS) void travel_finish_kernel(TravelView T, FrontierView X, int *__restrict__ cost, unsigned char *__restrict__ step,
                                                                       unsigned char *__restrict__ state) {
    const FrontierLane L(X);
    if (!L.in_word) return;  // (the whole wave)
    const int lane = (int)threadIdx.x & 63;
    const bool inside = L.x < T.dims[0];
    int c = TRAVEL_INFINITE;
    if (inside) c = T.cost[L.v];
    const bool reached = c != TRAVEL_INFINITE;
    if (inside) {
        if (cost) cost[L.v] = reached ? c : -1;
        if (step) {
            int code = reached ? TRAVEL_STEP_SEED : TRAVEL_STEP_NONE;
            if (reached && c > 0) {
                code = TRAVEL_STEP_NONE;
                for (int dz = 1; dz >= -1; dz--)  // (descending: the smallest code that fits is kept)
                    for (int dy = 1; dy >= -1; dy--)
                        for (int dx = 1; dx >= -1; dx--) {
                            const int m = travel_move_cost(T, dx, dy, dz);
                            const int x = L.x + dx, y = L.y + dy, z = L.z + dz;
                            if (!m || (unsigned)x >= (unsigned)T.dims[0] || (unsigned)y >= (unsigned)T.dims[1] || (unsigned)z >= (unsigned)T.dims[2]) continue;
                            if (T.cost[((long long)z * T.dims[1] + y) * T.dims[0] + x] + m == c) code = travel_code(dx, dy, dz);
                        }
            }
            step[L.v] = (unsigned char)code;
        }
        if (state) {
            const unsigned long long f = frontier_wide_bits(frontier_wide_row(X, X.wide_free, L.y, L.z), X.wide_words_per_row, L.w, 1);
            const unsigned long long u = frontier_wide_bits(frontier_wide_row(X, X.wide_unknown, L.y, L.z), X.wide_words_per_row, L.w, 1);
            state[L.v] = (unsigned char)((u >> lane) & 1ull ? 0 : ((f >> lane) & 1ull ? 1 : 2));
        }
    }
    const unsigned long long n = __ballot(reached);
    int largest = reached ? c + 1 : 0;  // (0: nothing reached)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, __shfl_xor(largest, o));
    if (lane == 0 && n) {
        atomicAdd(&T.ctl[TC_REACHED], (unsigned long long)__popcll(n));
        atomicMax(&T.ctl[TC_LARGEST], (unsigned long long)largest);
    }
}

// acc: TRAVEL_TABLE_WORDS per group: rows, reached, (least cost << 32) | smallest linear index with it
__global__ __launch_bounds__(TRAVEL_THREADS) void travel_table_init_kernel(long long *__restrict__ acc, long long groups) {
    const long long i = tile_element();
    if (i < groups * TRAVEL_TABLE_WORDS) acc[i] = (i % TRAVEL_TABLE_WORDS) == 2 ? 0x7fffffffffffffffll : 0ll;
}

__global__ __launch_bounds__(TRAVEL_THREADS) void travel_targets_kernel(TravelView T, const int *__restrict__ targets, long long n, long long n_groups,
                                                                        long long *__restrict__ acc) {
    const long long i = tile_element();
    int g = -1;
    long long key = 0x7fffffffffffffffll;
    bool ignored = false, reached = false;
    if (i < n) {
        const int x = targets[4 * i], y = targets[4 * i + 1], z = targets[4 * i + 2];
        g = targets[4 * i + 3];
        ignored = (unsigned)x >= (unsigned)T.dims[0] || (unsigned)y >= (unsigned)T.dims[1] || (unsigned)z >= (unsigned)T.dims[2] || g < 0 || g >= n_groups;
        if (ignored) {
            g = -1;
        } else {
            const long long v = ((long long)z * T.dims[1] + y) * T.dims[0] + x;
            const int c = T.cost[v];
            reached = c != TRAVEL_INFINITE;
            if (reached) key = ((long long)c << 32) | v;
        }
    }
    const unsigned long long n_ignored = __ballot(ignored), n_reached = __ballot(reached), live = __ballot(g >= 0);
    const int lane = (int)threadIdx.x & 63;
    if (lane == 0) {
        if (n_ignored) atomicAdd(&T.ctl[TC_TARGETS_IGNORED], (unsigned long long)__popcll(n_ignored));
        if (n_reached) atomicAdd(&T.ctl[TC_TARGETS_REACHED], (unsigned long long)__popcll(n_reached));
    }
    if (!live) return;  // (the whole wave)
    const int g0 = __shfl(g, __ffsll((long long)live) - 1);
    if (__ballot(g >= 0 && g != g0) == 0ull) {  // one group in the wave: it adds once
        long long least = key;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) least = min(least, __shfl_xor(least, o));
        if (lane == 0) {
            long long *row = acc + (size_t)g0 * TRAVEL_TABLE_WORDS;
            frontier_add(row, (long long)__popcll(live));
            if (n_reached) {
                frontier_add(row + 1, (long long)__popcll(n_reached));
                atomicMin(row + 2, least);
            }
        }
    } else if (g >= 0) {
        long long *row = acc + (size_t)g * TRAVEL_TABLE_WORDS;
        frontier_add(row, 1ll);
        if (reached) {
            frontier_add(row + 1, 1ll);
            atomicMin(row + 2, key);
        }
    }
}

// host: the rows as the caller reads them (pinned memory)
__global__ __launch_bounds__(TRAVEL_THREADS) void travel_table_kernel(const long long *__restrict__ acc, long long *__restrict__ host, long long groups) {
    const long long g = tile_element();
    if (g >= groups) return;
    const long long *row = acc + g * TRAVEL_TABLE_WORDS;
    const bool any = row[1] > 0;
    host[g * TRAVEL_TABLE_WORDS] = row[0];
    host[g * TRAVEL_TABLE_WORDS + 1] = row[1];
    host[g * TRAVEL_TABLE_WORDS + 2] = any ? row[2] >> 32 : -1ll;
    host[g * TRAVEL_TABLE_WORDS + 3] = any ? row[2] & 0xffffffffll : -1ll;
}

}  // namespace chisel_hip
