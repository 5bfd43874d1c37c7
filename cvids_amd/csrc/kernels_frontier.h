// kernels_frontier.h -- chisel_hip_frontiers: the free voxels of a window that border unknown space, their connected clusters and a
// table of the clusters (the host side: host_frontier.h; the refusals, the tile grid and the scratch sizes: frontier_checks.h; the
// definition: DESIGN.md 3.18).  Not kernels of the reference.  One fp32 compare per voxel in the seed, integers and bits after it: the
// answer is a pure function of the map and the window, whatever the order of execution.  Every step is a launch of its own on the
// map's stream, no host round trip between them until the report:
//
//   frontier_seed_kernel<N>   classifies the window widened by one voxel, as distance_seed_kernel does: a wave per run of 64 voxels
//                             along x, wave-uniform chunk look-ups, one __ballot word each into the FREE and the UNKNOWN plane.
//   frontier_mark_kernel      a thread per 64-bit word of the window: the free word and the six shifted / neighbouring unknown
//                             words, a bit-sliced count of the unknown faces, the frontier word.  Popcounts into the totals.
//   frontier_tile_kernel      a workgroup per tile of 16 x 16 x 8 voxels: the tile's 128 rows of 16 frontier bits and a tile-local
//                             parent array in LDS (8.5 KiB: 8 workgroups a CU, which is the 32-wave limit, in 68 of 160 KiB); the frontier
//                             voxels of the tile are united among themselves with LDS compare-and-swaps, always the larger index
//                             under the smaller, then every voxel's tile root goes to parent[] in global memory.
//   frontier_merge_kernel     the pairs of neighbours that straddle two tiles (faces, edges and corners alike: every forward offset
//                             of the connectivity that leaves the tile) are united in global memory by union_unite (kernels_workgroup.h) --
//                             every access to parent[] an agent-scope relaxed atomic, nobody waits for anybody.
//   frontier_label_kernel     behind the merge's end parent[] is read-only: plain loads to the root, root_of[v], the ROOT plane by
//                             ballot, + 1 to count[root] (wave_count: one atomic per wave and root).
//   frontier_keep_kernel      the KEPT and KEPT ROOT planes (count[root] >= min_voxels), the largest cluster.
//   frontier_sums_kernel / frontier_scan_sums_kernel / frontier_prefix_kernel
//                             reduce-then-scan over the words of both planes at once (two 32-bit counts in one 64-bit word;
//                             scan_tile_sums in the middle), no look-back: the kept roots and the kept voxels in front of every
//                             word.  A kept cluster's number is its root's word prefix plus the popcount below its bit; a kept
//                             voxel's row in the list likewise.  Then the control words go to the host and the host waits.
//   frontier_write_kernel     state (from the two planes), label and the voxel list, behind the wait and the capacity check.
//   frontier_table_*          the cluster table: 64-bit integer atomics (add, min, max) into a device accumulator; a wave walks a run
//                             of words and adds once per stretch of one cluster, its sums popcounts of wave-uniform words; then the
//                             rows into pinned memory.
#pragma once
#include "kernels_distance.h"    // distance_chunk_slot, DistanceLog2
#include "kernels_workgroup.h"
#include "frontier_checks.h"

namespace chisel_hip {

static_assert(FRONTIER_THREADS == WORKGROUP_THREADS, "a scan tile is what one workgroup of kernels_workgroup.h takes");
static_assert(FRONTIER_TILE_X == 16 && FRONTIER_TILE_ROWS * 2 == FRONTIER_THREADS, "a thread of a tile takes 8 bits of one of its 128 rows");

struct FrontierView {
    int wo[3], wd[3];   // the widened window: first voxel (global index), extent
    int dims[3];        // the window itself; it starts at wo + 1
    int tiles[3];
    int min_unknown_faces, level, min_voxels;  // level: 1, 2, 3 non-zero coordinates of an offset for connectivity 6, 18, 26
    float surface_offset;
    int wide_words_per_row, words_per_row;
    long long words;    // of one window plane
    unsigned long long *wide_free, *wide_unknown;          // [wd z][wd y][wide_words_per_row]
    unsigned long long *front, *roots, *kept, *kept_roots; // [nz][ny][words_per_row]
    unsigned long long *prefix;                            // [words] kept roots (high half) and kept voxels (low half) in front of the word
    unsigned long long *sums;                              // [scan tiles] a scan's tile sums, then their exclusive prefix
    int *parent, *root_of, *count;                         // [voxels]; count per root
    unsigned long long *ctl;                               // [FRONTIER_HOST_WORDS] FC_*
};

// One wave per run of 64 voxels along x of the widened window, four runs per workgroup (distance_seed_kernel's frame).
template <int N>
__global__ __launch_bounds__(256) void frontier_seed_kernel(MapView M, FrontierView X, long long n_runs) {
    constexpr int LOG = DistanceLog2<N>::value;
    const int lane = threadIdx.x & 63;
    const long long run = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (run >= n_runs) return;  // (the whole wave)
    const long long row = run / X.wide_words_per_row;
    const int word = (int)(run - row * X.wide_words_per_row);
    const int wy = (int)(row % X.wd[1]), wz = (int)(row / X.wd[1]);
    const int wx0 = word * 64, wx = wx0 + lane;
    const int gx0 = X.wo[0] + wx0, gx = gx0 + lane, gy = X.wo[1] + wy, gz = X.wo[2] + wz;  // (|g| <= 2^30 + 63: no overflow)
    const int cy = gy >> LOG, cz = gz >> LOG;  // floor division: the shift of a negative int is arithmetic
    const int last = min(wx0 + 63, X.wd[0] - 1) - wx0;
    const int c_first = gx0 >> LOG, c_last = (gx0 + last) >> LOG, c_mine = gx >> LOG;
    int bb[6];
    load_chunk_box(M, bb);
    int slot = -1;
    for (int c = c_first; c <= c_last; c++) {  // (wave-uniform: at most 64 / N + 1 look-ups)
        const int s = distance_chunk_slot(M, bb, c, cy, cz);
        if (c == c_mine) slot = s;
    }
    const bool inside = wx < X.wd[0];
    unsigned st = 0;
    if (inside && slot >= 0) {
        const size_t off = (size_t)slot * (N * N * N) + (size_t)((((gz & (N - 1)) * N) + (gy & (N - 1))) * N + (gx & (N - 1)));
        const float w = M.wgt[off];
        if ((double)w > 1e-12) st = M.sdf[off] < X.surface_offset ? 2u : 1u;
    }
    const unsigned long long free_bits = __ballot(inside && st == 1u), unknown_bits = __ballot(inside && st == 0u);
    if (lane == 0) {
        X.wide_free[run] = free_bits;
        X.wide_unknown[run] = unknown_bits;
    }
}

// bits [64 w + s, 64 w + s + 64) of a row of a wide plane, s = 0, 1, 2: for the window's word w its -x neighbours, itself, its +x
// neighbours (the window starts at bit 1 of the widened row).  w < words_per_row <= wide_words_per_row; bits beyond the row read 0
__device__ inline unsigned long long frontier_wide_bits(const unsigned long long *__restrict__ row, int wide_words_per_row, int w, int s) {
    const unsigned long long lo = row[w];
    const unsigned long long hi = w + 1 < wide_words_per_row ? row[w + 1] : 0ull;
    return s ? (lo >> s) | (hi << (64 - s)) : lo;
}
__device__ inline const unsigned long long *frontier_wide_row(const FrontierView &X, const unsigned long long *plane, int y, int z) {
    return plane + ((long long)(z + 1) * X.wd[1] + (y + 1)) * X.wide_words_per_row;
}
// the bits of the window's word w of row (y, z) that name a voxel of the window
__device__ inline unsigned long long frontier_word_mask(const FrontierView &X, int w) {
    const int n = X.dims[0] - 64 * w;
    return n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

// unknown_faces of the 64 voxels of word w of row (y, z), bit-sliced: the count of voxel b is bit b of b0 + 2 b1 + 4 b2 (0 ... 6)
struct FrontierFaces { unsigned long long b0, b1, b2; };
__device__ inline unsigned long long frontier_majority(unsigned long long a, unsigned long long b, unsigned long long c) { return (a & b) | (c & (a ^ b)); }
__device__ inline FrontierFaces frontier_faces(const FrontierView &X, int w, int y, int z) {
    const int P = X.wide_words_per_row;
    const unsigned long long *c = frontier_wide_row(X, X.wide_unknown, y, z);
    const long long dy = P, dz = (long long)X.wd[1] * P;
    const unsigned long long xm = frontier_wide_bits(c, P, w, 0), xp = frontier_wide_bits(c, P, w, 2);
    const unsigned long long ym = frontier_wide_bits(c - dy, P, w, 1), yp = frontier_wide_bits(c + dy, P, w, 1);
    const unsigned long long zm = frontier_wide_bits(c - dz, P, w, 1), zp = frontier_wide_bits(c + dz, P, w, 1);
    const unsigned long long s1 = xm ^ xp ^ ym, c1 = frontier_majority(xm, xp, ym), s2 = yp ^ zm ^ zp, c2 = frontier_majority(yp, zm, zp);
    const unsigned long long k = s1 & s2;  // the carry into bit 1
    FrontierFaces f;
    f.b0 = s1 ^ s2;
    f.b1 = c1 ^ c2 ^ k;
    f.b2 = frontier_majority(c1, c2, k);
    return f;
}
// the voxels with at least k = 1 ... 6 unknown faces
__device__ inline unsigned long long frontier_at_least(const FrontierFaces &f, int k) {
    switch (k) {
        case 1: return f.b0 | f.b1 | f.b2;
        case 2: return f.b1 | f.b2;
        case 3: return f.b2 | (f.b1 & f.b0);
        case 4: return f.b2;
        case 5: return f.b2 & (f.b1 | f.b0);
        default: return f.b2 & f.b1;
    }
}

// the sum of `mine` over the wave, in every lane
__device__ inline int frontier_wave_sum(int mine) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    return mine;
}

__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_mark_kernel(FrontierView X) {
    const long long i = tile_element();
    int n_unknown = 0, n_free = 0, n_front = 0;
    if (i < X.words) {
        const long long row = i / X.words_per_row;
        const int w = (int)(i - row * X.words_per_row), y = (int)(row % X.dims[1]), z = (int)(row / X.dims[1]);
        const unsigned long long mask = frontier_word_mask(X, w);
        const unsigned long long free_bits = frontier_wide_bits(frontier_wide_row(X, X.wide_free, y, z), X.wide_words_per_row, w, 1) & mask;
        const unsigned long long unknown_bits = frontier_wide_bits(frontier_wide_row(X, X.wide_unknown, y, z), X.wide_words_per_row, w, 1) & mask;
        const unsigned long long front = free_bits & frontier_at_least(frontier_faces(X, w, y, z), X.min_unknown_faces);
        X.front[i] = front;
        n_unknown = __popcll(unknown_bits);
        n_free = __popcll(free_bits);
        n_front = __popcll(front);
    }
    n_unknown = frontier_wave_sum(n_unknown);
    n_free = frontier_wave_sum(n_free);
    n_front = frontier_wave_sum(n_front);
    if ((threadIdx.x & 63) == 0) {  // (three vector atomics a wave of 4096 voxels)
        if (n_unknown) atomicAdd(&X.ctl[FC_UNKNOWN], (unsigned long long)n_unknown);
        if (n_free) atomicAdd(&X.ctl[FC_FREE], (unsigned long long)n_free);
        if (n_front) atomicAdd(&X.ctl[FC_FRONTIER], (unsigned long long)n_front);
    }
}

// ---- the tiles ---------------------------------------------------------------------------------------------------------------------
// A tile's voxel has the local index (lz * 16 + ly) * 16 + lx: ascending exactly as the linear index of the window ascends inside the
// tile, so "the larger under the smaller" means the same thing in LDS and in global memory.
struct FrontierTile {
    int x0, y0, z0;
    __device__ inline explicit FrontierTile(const FrontierView &X) {
        const int t = (int)blockIdx.x, tx = t % X.tiles[0], ty = (t / X.tiles[0]) % X.tiles[1], tz = t / (X.tiles[0] * X.tiles[1]);
        x0 = tx * FRONTIER_TILE_X; y0 = ty * FRONTIER_TILE_Y; z0 = tz * FRONTIER_TILE_Z;
    }
    __device__ inline int linear(const FrontierView &X, int local) const {  // the window's linear index of a local one
        const int lx = local % FRONTIER_TILE_X, ly = (local / FRONTIER_TILE_X) % FRONTIER_TILE_Y, lz = local / (FRONTIER_TILE_X * FRONTIER_TILE_Y);
        return ((z0 + lz) * X.dims[1] + (y0 + ly)) * X.dims[0] + (x0 + lx);
    }
    // the 16 frontier bits of the tile's row r = lz * 16 + ly; 0 where the row lies outside the window
    __device__ inline unsigned row_bits(const FrontierView &X, int r) const {
        const int y = y0 + r % FRONTIER_TILE_Y, z = z0 + r / FRONTIER_TILE_Y;
        if (y >= X.dims[1] || z >= X.dims[2]) return 0u;
        return (unsigned)(X.front[((long long)z * X.dims[1] + y) * X.words_per_row + (x0 >> 6)] >> (x0 & 63)) & ((1u << FRONTIER_TILE_X) - 1u);
    }
};

// is (dx, dy, dz) a forward offset of the connectivity?  (the order of frontier_forward_offsets)
__device__ inline bool frontier_forward(int dx, int dy, int dz, int level) {
    const bool forward = dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)));
    return forward && (dx != 0) + (dy != 0) + (dz != 0) <= level;
}

__device__ inline int frontier_find_lds(int *parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;  // (p < x: bounded by the tree's depth)
    }
}
__device__ inline void frontier_unite_lds(int *parent, int a, int b) {
    for (;;) {
        a = frontier_find_lds(parent, a);
        b = frontier_find_lds(parent, b);
        if (a == b) return;
        const int lo = min(a, b), hi = max(a, b);
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(&parent[hi], &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
        // (lost: another lane has linked hi, which is progress)
    }
}

// One workgroup per tile.  A thread takes 8 bits of one row.
__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_tile_kernel(FrontierView X) {
    __shared__ unsigned s_bits[FRONTIER_TILE_ROWS];
    __shared__ int s_parent[FRONTIER_TILE_VOXELS];
    const FrontierTile T(X);
    const int tid = (int)threadIdx.x;
    if (tid < FRONTIER_TILE_ROWS) s_bits[tid] = T.row_bits(X, tid);
    __syncthreads();
    const int r = tid >> 1, ly = r % FRONTIER_TILE_Y, lz = r / FRONTIER_TILE_Y, b0 = (tid & 1) * 8;
    const unsigned mine = (s_bits[r] >> b0) & 0xffu;
    for (unsigned m = mine; m; m &= m - 1) {
        const int i = r * FRONTIER_TILE_X + b0 + __builtin_ctz(m);
        s_parent[i] = i;
    }
    __syncthreads();
    for (unsigned m = mine; m; m &= m - 1) {
        const int lx = b0 + __builtin_ctz(m), i = r * FRONTIER_TILE_X + lx;
        for (int dz = 0; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if (!frontier_forward(dx, dy, dz, X.level)) continue;
                    const int jx = lx + dx, jy = ly + dy, jz = lz + dz;
                    if ((unsigned)jx >= (unsigned)FRONTIER_TILE_X || (unsigned)jy >= (unsigned)FRONTIER_TILE_Y || jz >= FRONTIER_TILE_Z) continue;  // (the merge's)
                    const int jr = jz * FRONTIER_TILE_Y + jy;
                    if ((s_bits[jr] >> jx) & 1u) frontier_unite_lds(s_parent, i, jr * FRONTIER_TILE_X + jx);
                }
    }
    __syncthreads();  // the tile's unions are over: plain reads
    for (unsigned m = mine; m; m &= m - 1) {
        const int i = r * FRONTIER_TILE_X + b0 + __builtin_ctz(m);
        int root = i;
        for (int p = s_parent[root]; p != root; p = s_parent[root]) root = p;
        const int v = T.linear(X, i);
        X.parent[v] = T.linear(X, root);
        X.count[v] = 0;
    }
}

// The same threads over the same voxels: the forward neighbours that lie in another tile (and in the window).
__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_merge_kernel(FrontierView X) {
    const FrontierTile T(X);
    const int tid = (int)threadIdx.x;
    const int r = tid >> 1, ly = r % FRONTIER_TILE_Y, lz = r / FRONTIER_TILE_Y, b0 = (tid & 1) * 8;
    const unsigned mine = (T.row_bits(X, r) >> b0) & 0xffu;
    const bool rim_row = ly == 0 || ly == FRONTIER_TILE_Y - 1 || lz == FRONTIER_TILE_Z - 1;
    for (unsigned m = mine; m; m &= m - 1) {
        const int lx = b0 + __builtin_ctz(m);
        if (!rim_row && lx != 0 && lx != FRONTIER_TILE_X - 1) continue;  // (no offset leaves the tile from here)
        const int i = r * FRONTIER_TILE_X + lx;
        for (int dz = 0; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if (!frontier_forward(dx, dy, dz, X.level)) continue;
                    const int jx = lx + dx, jy = ly + dy, jz = lz + dz;
                    if ((unsigned)jx < (unsigned)FRONTIER_TILE_X && (unsigned)jy < (unsigned)FRONTIER_TILE_Y && jz < FRONTIER_TILE_Z) continue;  // (the tile's)
                    const int x = T.x0 + jx, y = T.y0 + jy, z = T.z0 + jz;
                    if ((unsigned)x >= (unsigned)X.dims[0] || (unsigned)y >= (unsigned)X.dims[1] || z >= X.dims[2]) continue;  // outside the window: joins nothing
                    const unsigned long long there = X.front[((long long)z * X.dims[1] + y) * X.words_per_row + (x >> 6)];
                    if ((there >> (x & 63)) & 1ull) union_unite(X.parent, T.linear(X, i), (z * X.dims[1] + y) * X.dims[0] + x);
                }
    }
}

// ---- a lane per voxel: a wave per word of the window, four words a workgroup ----------------------------------------------------------
struct FrontierLane {
    long long word;  // of the window plane; wave-uniform
    bool in_word;    // word < words
    int w, x, y, z, v;
    __device__ inline explicit FrontierLane(const FrontierView &X) {
        const int lane = (int)threadIdx.x & 63;
        word = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        in_word = word < X.words;
        const long long row = in_word ? word / X.words_per_row : 0;
        w = in_word ? (int)(word - row * X.words_per_row) : 0;
        x = w * 64 + lane;
        y = (int)(row % X.dims[1]);
        z = (int)(row / X.dims[1]);
        v = (int)(row * X.dims[0]) + x;  // (an address only where the voxel's bit is set in a plane, or x < nx)
    }
    __device__ inline bool bit(const unsigned long long *plane) const { return in_word && ((plane[word] >> (threadIdx.x & 63)) & 1ull); }
};

__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_label_kernel(FrontierView X) {
    const FrontierLane L(X);
    const bool front = L.bit(X.front);
    int r = 0;
    if (front) {
        r = L.v;
        for (int p = X.parent[r]; p != r; p = X.parent[r]) r = p;
        X.root_of[L.v] = r;
    }
    const unsigned long long roots = __ballot(front && r == L.v);
    if (L.in_word && (threadIdx.x & 63) == 0) {
        X.roots[L.word] = roots;
        if (roots) atomicAdd(&X.ctl[FC_CLUSTERS], (unsigned long long)__popcll(roots));
    }
    wave_count(X.count, r, front);
}

__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_keep_kernel(FrontierView X) {
    const FrontierLane L(X);
    const bool front = L.bit(X.front);
    int r = 0, n = 0;
    if (front) {
        r = X.root_of[L.v];
        n = X.count[r];
    }
    const bool kept = front && n >= X.min_voxels;
    const unsigned long long kept_bits = __ballot(kept), kept_roots = __ballot(kept && r == L.v);
    int largest = front && r == L.v ? n : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, __shfl_xor(largest, o));
    if (L.in_word && (threadIdx.x & 63) == 0) {
        X.kept[L.word] = kept_bits;
        X.kept_roots[L.word] = kept_roots;
        if (largest) atomicMax(&X.ctl[FC_LARGEST], (unsigned long long)largest);
    }
}

// ---- the scans: kept roots in the high half, kept voxels in the low half (each <= 2^26: no carry between the halves) -------------------
__device__ inline unsigned long long frontier_word_counts(const FrontierView &X, long long i) {
    return i < X.words ? ((unsigned long long)__popcll(X.kept_roots[i]) << 32) | (unsigned long long)__popcll(X.kept[i]) : 0ull;
}
__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_sums_kernel(FrontierView X) {
    __shared__ unsigned long long s_wave[FRONTIER_THREADS / 64];
    unsigned long long total;
    (void)block_exclusive_scan(frontier_word_counts(X, tile_element()), s_wave, total);
    if (threadIdx.x == 0) X.sums[blockIdx.x] = total;
}
// One workgroup.  sums[b] = the sums of the tiles in front of b; the totals into their control words.
__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_scan_sums_kernel(unsigned long long *__restrict__ sums, long long n_tiles, unsigned long long *__restrict__ ctl) {
    __shared__ unsigned long long s_wave[FRONTIER_THREADS / 64];
    const unsigned long long run = scan_tile_sums(sums, n_tiles, s_wave);
    if (threadIdx.x == 0) {
        ctl[FC_KEPT_CLUSTERS] = run >> 32;
        ctl[FC_KEPT_VOXELS] = run & 0xffffffffull;
    }
}
__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_prefix_kernel(FrontierView X) {
    __shared__ unsigned long long s_wave[FRONTIER_THREADS / 64];
    const long long i = tile_element();
    unsigned long long total;
    const unsigned long long before = block_exclusive_scan(frontier_word_counts(X, i), s_wave, total);
    if (i < X.words) X.prefix[i] = X.sums[blockIdx.x] + before;
}

// ---- behind the wait ---------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned long long frontier_below(int bit) { return (1ull << bit) - 1ull; }  // bit < 64
// the number of the kept cluster whose root is r
__device__ inline int frontier_cluster_number(const FrontierView &X, int r) {
    const int row = r / X.dims[0], x = r - row * X.dims[0];
    const long long word = (long long)row * X.words_per_row + (x >> 6);
    return (int)(X.prefix[word] >> 32) + __popcll(X.kept_roots[word] & frontier_below(x & 63));
}

__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_write_kernel(FrontierView X, unsigned char *__restrict__ state, int *__restrict__ label, int *__restrict__ voxels) {
    const FrontierLane L(X);
    if (!L.in_word || L.x >= X.dims[0]) return;
    const int lane = (int)threadIdx.x & 63;
    if (state) {
        const unsigned long long f = frontier_wide_bits(frontier_wide_row(X, X.wide_free, L.y, L.z), X.wide_words_per_row, L.w, 1);
        const unsigned long long u = frontier_wide_bits(frontier_wide_row(X, X.wide_unknown, L.y, L.z), X.wide_words_per_row, L.w, 1);
        state[L.v] = (unsigned char)((u >> lane) & 1ull ? 0 : ((f >> lane) & 1ull ? 1 : 2));
    }
    if (!label && !voxels) return;
    const bool front = L.bit(X.front), kept = L.bit(X.kept);
    const int number = kept ? frontier_cluster_number(X, X.root_of[L.v]) : -2;
    if (label) label[L.v] = front ? number : -1;
    if (voxels && kept) {
        int *row = voxels + 4 * ((size_t)(X.prefix[L.word] & 0xffffffffull) + (size_t)__popcll(X.kept[L.word] & frontier_below(lane)));
        row[0] = L.x; row[1] = L.y; row[2] = L.z; row[3] = number;
    }
}

// acc: FRONTIER_TABLE_WORDS per kept cluster
__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_table_init_kernel(long long *__restrict__ acc, long long rows) {
    const long long i = tile_element();
    if (i >= rows * FRONTIER_TABLE_WORDS) return;
    const int k = (int)(i % FRONTIER_TABLE_WORDS);
    acc[i] = k >= FT_MIN && k < FT_MAX ? 0x7fffffffffffffffll : (k >= FT_MAX && k < FT_FACES ? -1ll : 0ll);
}

// the sum over the set bits of `bits` of their positions
__device__ inline int frontier_position_sum(unsigned long long bits) {
    return __popcll(bits & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(bits & 0xCCCCCCCCCCCCCCCCull) + 4 * __popcll(bits & 0xF0F0F0F0F0F0F0F0ull) +
           8 * __popcll(bits & 0xFF00FF00FF00FF00ull) + 16 * __popcll(bits & 0xFFFF0000FFFF0000ull) + 32 * __popcll(bits & 0xFFFFFFFF00000000ull);
}
__device__ inline void frontier_add(long long *p, long long v) { atomicAdd((unsigned long long *)p, (unsigned long long)v); }

// One cluster's share of a run of words, in wave-uniform values, and its flush: eleven 64-bit atomics by one lane.
struct FrontierRun {
    long long n, sx, sy, sz, faces;
    int x0, y0, z0, x1, y1, z1;
    __device__ inline void clear() {
        n = sx = sy = sz = faces = 0;
        x0 = y0 = z0 = 0x7fffffff;
        x1 = y1 = z1 = -1;
    }
    __device__ inline void flush(long long *__restrict__ acc, int c) const {
        long long *row = acc + (size_t)c * FRONTIER_TABLE_WORDS;
        frontier_add(row + FT_VOXELS, n);
        frontier_add(row + FT_SUM, sx);
        frontier_add(row + FT_SUM + 1, sy);
        frontier_add(row + FT_SUM + 2, sz);
        atomicMin(row + FT_MIN, (long long)x0);
        atomicMin(row + FT_MIN + 1, (long long)y0);
        atomicMin(row + FT_MIN + 2, (long long)z0);
        atomicMax(row + FT_MAX, (long long)x1);
        atomicMax(row + FT_MAX + 1, (long long)y1);
        atomicMax(row + FT_MAX + 2, (long long)z1);
        frontier_add(row + FT_FACES, faces);
    }
};

// A wave walks FRONTIER_TABLE_SPAN consecutive words of the window, a lane per voxel of the word at hand; a word without a kept voxel
// costs one load.  The lanes of a word share y and z, and every sum over the lanes of one cluster is a popcount of wave-uniform
// words, so the running sums are wave-uniform too: they are kept while the cluster stays the same and flushed when it changes (a
// window is mostly a few large clusters: as first written, a set of atomics per word and cluster, the waves queued up at one row).
__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_table_kernel(FrontierView X, long long *__restrict__ acc) {
    const int lane = (int)threadIdx.x & 63;
    const long long first = ((long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * FRONTIER_TABLE_SPAN;
    const long long last = min(first + (long long)FRONTIER_TABLE_SPAN, X.words);
    int cur = -1;
    FrontierRun R;
    R.clear();
    for (long long word = first; word < last; word++) {
        const unsigned long long bits = X.kept[word];
        const unsigned long long kept_bits = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(bits >> 32)) << 32) |
                                             (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)bits);
        if (!kept_bits) continue;
        const long long row = word / X.words_per_row;
        const int w = (int)(word - row * X.words_per_row), y = (int)(row % X.dims[1]), z = (int)(row / X.dims[1]), x0 = w * 64;
        const bool kept = (kept_bits >> lane) & 1ull;
        int c = 0;
        if (kept) {
            const int v = (int)(row * X.dims[0]) + x0 + lane, r = X.root_of[v];
            c = frontier_cluster_number(X, r);
            if (r == v) acc[(size_t)c * FRONTIER_TABLE_WORDS + FT_ROOT] = r;
        }
        const FrontierFaces F = frontier_faces(X, w, y, z);
        unsigned long long todo = kept_bits;
        while (todo) {  // (wave-uniform; every round retires its leader's lanes)
            const int c0 = __shfl(c, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(kept && c == c0);
            if (c0 != cur) {
                if (cur >= 0 && lane == 0) R.flush(acc, cur);
                cur = c0;
                R.clear();
            }
            const long long n = __popcll(same);
            R.n += n;
            R.sx += n * x0 + frontier_position_sum(same);
            R.sy += n * y;
            R.sz += n * z;
            R.faces += (long long)__popcll(same & F.b0) + 2 * __popcll(same & F.b1) + 4 * __popcll(same & F.b2);
            R.x0 = min(R.x0, x0 + (int)__ffsll((long long)same) - 1);
            R.x1 = max(R.x1, x0 + 63 - (int)__clzll((long long)same));
            R.y0 = min(R.y0, y); R.y1 = max(R.y1, y);
            R.z0 = min(R.z0, z); R.z1 = max(R.z1, z);
            todo &= ~same;
        }
    }
    if (cur >= 0 && lane == 0) R.flush(acc, cur);
}

__global__ __launch_bounds__(FRONTIER_THREADS) void frontier_table_rows_kernel(const long long *__restrict__ acc, long long *__restrict__ host, long long words) {
    const long long i = tile_element();
    if (i < words) host[i] = acc[i];
}

}  // namespace chisel_hip
