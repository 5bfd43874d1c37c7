// frontier_checks.h -- the host-side pieces of chisel_hip_frontiers that call nothing of HIP (included by chisel_hip.hip for
// host_frontier.h and kernels_frontier.h and, on its own, by tests/frontier_checks_check.cpp, which runs them under the address and
// undefined-behaviour sanitizers on the CPU): what the entry refuses about its arguments other than the map, in the order of the
// header; the window widened by one voxel; the tile grid of the labelling; every scratch size, in 64-bit arithmetic; the capacities
// against the totals.  DESIGN.md 3.18 is the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace chisel_hip {

constexpr int64_t FRONTIER_COORD_LIMIT = 1ll << 30;  // |global voxel index| of the widened window, per axis
constexpr int64_t FRONTIER_MAX_VOXELS = 1ll << 26;   // voxels of the window: a linear index, a rank and a count fit an int
constexpr int FRONTIER_TILE_X = 16, FRONTIER_TILE_Y = 16, FRONTIER_TILE_Z = 8;  // a labelling tile: a quarter of a 64-bit word per row, 128 rows
constexpr int FRONTIER_TILE_ROWS = FRONTIER_TILE_Y * FRONTIER_TILE_Z;
constexpr int FRONTIER_TILE_VOXELS = FRONTIER_TILE_X * FRONTIER_TILE_ROWS;
constexpr int FRONTIER_THREADS = 256;                // lanes of every workgroup: four words of a lane-per-voxel kernel, one scan tile
constexpr int FRONTIER_TABLE_WORDS = 12;             // int64 per row of the cluster table (FT_*)
constexpr int FRONTIER_TABLE_SPAN = 32;              // consecutive words of the window a wave of the table kernel walks
constexpr int FT_ROOT = 0, FT_VOXELS = 1, FT_SUM = 2, FT_MIN = 5, FT_MAX = 8, FT_FACES = 11;
constexpr int FRONTIER_HOST_WORDS = 8;               // 64-bit control words the report kernel leaves in pinned memory (FC_*)
constexpr int FC_UNKNOWN = 0, FC_FREE = 1, FC_FRONTIER = 2, FC_CLUSTERS = 3, FC_LARGEST = 4, FC_KEPT_CLUSTERS = 5, FC_KEPT_VOXELS = 6;
constexpr int FRONTIER_REFUSED_INVALID = 1, FRONTIER_REFUSED_UNSUPPORTED = 5;  // = CHISEL_HIP_ERR_INVALID, CHISEL_HIP_ERR_UNSUPPORTED

// The window widened by one voxel on every side (the seed classifies it), the window's own bit rows, the tile grid, and the scratch:
//   wide planes    free and unknown: one bit per voxel of the widened window, a row of x in 64-bit words    2 x [wd z][wd y][wide_words_per_row]
//   window planes  frontier, root, kept, kept root: one bit per voxel of the window                         4 x [nz][ny][words_per_row]
//   prefix         kept roots (high half) and kept voxels (low half) in front of every word of the window   [words] 64-bit words
//   sums           the scan's tile sums (FRONTIER_THREADS words a tile), packed likewise                     [scan_tiles] 64-bit words
//   per voxel      parent, root_of, count                                                                    3 x [voxels] ints
struct FrontierPlan {
    int wo[3], wd[3];  // first voxel and extent of the widened window
    int64_t voxels;    // of the window
    int64_t wide_words_per_row, wide_words;  // one wide plane
    int64_t words_per_row, words;            // one window plane
    int64_t tiles[3], n_tiles;               // the labelling's grid
    int64_t scan_tiles;
    int64_t plane_words;  // 64-bit words of the six planes, the prefix and the sums
    int64_t ints;         // ints of the per-voxel arrays
};

constexpr int64_t frontier_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The size query: no array is asked for (a list or a table with capacity 0 is none).
inline bool frontier_is_query(const void *state, const void *label, int64_t capacity_voxels, const void *voxels, int64_t capacity_clusters, const void *cluster_table) {
    return !state && !label && !(voxels && capacity_voxels > 0) && !(cluster_table && capacity_clusters > 0);
}

// what chisel_hip_frontiers refuses about its arguments other than the map, in the order of the header; null = go on, with *plan
// filled.  *code: FRONTIER_REFUSED_* of a refusal.  Window: chisel_hip_frontier_window (a template, so that this header goes on
// including nothing of the library's)
template <class Window>
inline const char *frontier_refusal(const Window *w, const void *totals, int64_t capacity_voxels, const void *voxels, int64_t capacity_clusters,
                                    const void *cluster_table, int *code, FrontierPlan *plan) {
    *code = FRONTIER_REFUSED_INVALID;
    if (!w) return "null window";
    if (!totals) return "null totals";
    for (int a = 0; a < 3; a++)
        if (w->dims[a] < 1) return "a window dimension below 1";
    if (w->min_unknown_faces < 1 || w->min_unknown_faces > 6) return "min_unknown_faces is outside 1 ... 6";
    if (w->connectivity != 6 && w->connectivity != 18 && w->connectivity != 26) return "the connectivity is 6, 18 or 26";
    if (w->min_voxels < 1) return "min_voxels below 1";
    if (w->surface_offset != w->surface_offset) return "the surface offset is NaN";
    if (capacity_voxels < 0 || capacity_clusters < 0) return "a negative capacity";
    if (capacity_voxels > 0 && !voxels) return "a voxel capacity without the voxel list";
    if (capacity_clusters > 0 && !cluster_table) return "a cluster capacity without the cluster table";
    int64_t wd[3];
    for (int a = 0; a < 3; a++) {
        const int64_t lo = (int64_t)w->origin[a] - 1, hi = (int64_t)w->origin[a] + (int64_t)w->dims[a];
        if (lo < -FRONTIER_COORD_LIMIT || hi > FRONTIER_COORD_LIMIT) return "the window widened by one voxel reaches beyond voxel index +-2^30";
        wd[a] = hi - lo + 1;  // (<= 2^31 + 1)
        plan->wo[a] = (int)lo;
    }
    *code = FRONTIER_REFUSED_UNSUPPORTED;
    const int64_t nx = w->dims[0], ny = w->dims[1], nz = w->dims[2];
    if (nx > FRONTIER_MAX_VOXELS || nx * ny > FRONTIER_MAX_VOXELS || nx * ny * nz > FRONTIER_MAX_VOXELS)  // (each product <= 2^26 * 2^31)
        return "the window holds more than 2^26 voxels";
    for (int a = 0; a < 3; a++) plan->wd[a] = (int)wd[a];
    plan->voxels = nx * ny * nz;
    plan->wide_words_per_row = frontier_ceil_div(wd[0], 64);
    plan->wide_words = plan->wide_words_per_row * wd[1] * wd[2];  // (<= 3 nx * 3 ny * 3 nz <= 27 * 2^26)
    plan->words_per_row = frontier_ceil_div(nx, 64);
    plan->words = plan->words_per_row * ny * nz;
    plan->tiles[0] = frontier_ceil_div(nx, FRONTIER_TILE_X);
    plan->tiles[1] = frontier_ceil_div(ny, FRONTIER_TILE_Y);
    plan->tiles[2] = frontier_ceil_div(nz, FRONTIER_TILE_Z);
    plan->n_tiles = plan->tiles[0] * plan->tiles[1] * plan->tiles[2];
    plan->scan_tiles = frontier_ceil_div(plan->words, FRONTIER_THREADS);
    plan->plane_words = 2 * plan->wide_words + 5 * plan->words + plan->scan_tiles;
    plan->ints = 3 * plan->voxels;
    *code = 0;
    return nullptr;
}

// a capacity below its total is refused (the caller is told the totals all the same); a capacity nothing is written under is not looked at
inline const char *frontier_capacity_refusal(int64_t kept_voxels, int64_t kept_clusters, int64_t capacity_voxels, const void *voxels, int64_t capacity_clusters,
                                             const void *cluster_table) {
    if (voxels && capacity_voxels > 0 && capacity_voxels < kept_voxels) return "the voxel capacity is below the kept voxels";
    if (cluster_table && capacity_clusters > 0 && capacity_clusters < kept_clusters) return "the cluster capacity is below the kept clusters";
    return nullptr;
}

// the offsets of a connectivity that point FORWARD in the linear index ((dz, dy, dx) above (0, 0, 0) in that order): 3, 9 or 13 of
// them, each with at most `level` = 1, 2, 3 non-zero coordinates.  Every pair of neighbours is united once, from its smaller voxel.
constexpr int frontier_level(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; }
inline int frontier_forward_offsets(int connectivity, int out[13][3]) {
    const int level = frontier_level(connectivity);
    int n = 0;
    for (int dz = 0; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const bool forward = dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)));
                if (!forward || (dx != 0) + (dy != 0) + (dz != 0) > level) continue;
                out[n][0] = dx; out[n][1] = dy; out[n][2] = dz;
                n++;
            }
    return n;
}

}  // namespace chisel_hip
