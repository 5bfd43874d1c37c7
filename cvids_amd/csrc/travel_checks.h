// travel_checks.h -- the host-side pieces of chisel_hip_travel_field and chisel_hip_travel_path that call nothing of HIP (included by
// chisel_hip.hip for host_travel.h and kernels_travel.h and, on its own, by tests/travel_checks_check.cpp, which runs them under the
// address and undefined-behaviour sanitizers on the CPU): what the entry refuses about its arguments other than the map, in the order
// of the header; the seed check; the tile grid of the rounds; every scratch size, in 64-bit arithmetic; the walk of
// chisel_hip_travel_path.  DESIGN.md 3.19 is the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace chisel_hip {

constexpr int64_t TRAVEL_COORD_LIMIT = 1ll << 30;  // |global voxel index| of the widened window, per axis
constexpr int64_t TRAVEL_MAX_VOXELS = 1ll << 26;   // voxels of the window: a linear index fits the low half of the table's 64-bit minimum
constexpr int64_t TRAVEL_MAX_SEEDS = 1ll << 20;
constexpr int TRAVEL_MAX_COST = 1 << 30;           // of max_cost; every candidate is at most 2^30 + 65535
constexpr int TRAVEL_MAX_STEP_COST = 65535;
constexpr int TRAVEL_MAX_CLEARANCE = 64;           // = DISTANCE_MAX_RADIUS
constexpr int TRAVEL_INFINITE = 0x7f000000;        // "not reached": above every max_cost, and + 65535 stays an int
constexpr int TRAVEL_TILE_X = 16, TRAVEL_TILE_Y = 16, TRAVEL_TILE_Z = 8;  // = FRONTIER_TILE_*: a thread takes 8 voxels of one of the 128 rows
constexpr int TRAVEL_THREADS = 256;
constexpr int TRAVEL_ROUNDS_PER_WAIT = 16;         // round launches the host queues between two looks at the flagged tiles
constexpr int TRAVEL_TABLE_WORDS = 4;              // int64 per row of the group table: rows, reached, least cost, its smallest linear index
constexpr int TRAVEL_STEP_SEED = 13, TRAVEL_STEP_NONE = 255;
constexpr int TRAVEL_HOST_WORDS = 12;              // 64-bit control words (TC_*)
constexpr int TC_UNKNOWN = 0, TC_FREE = 1, TC_TRAVERSABLE = 2, TC_SEEDS_USED = 3, TC_SEEDS_IGNORED = 4, TC_REACHED = 5, TC_LARGEST = 6, TC_TARGETS_REACHED = 7,
              TC_TARGETS_IGNORED = 8, TC_ROUNDS = 9, TC_TILE_VISITS = 10, TC_FLAGGED = 11;
constexpr int TRAVEL_REFUSED_INVALID = 1, TRAVEL_REFUSED_UNSUPPORTED = 5;  // = CHISEL_HIP_ERR_INVALID, CHISEL_HIP_ERR_UNSUPPORTED

// The window widened by one voxel on every side (frontier_seed_kernel classifies it: the layout of the frontiers' wide planes), the
// window's own bit rows, the tile grid of the rounds, and the scratch:
//   wide planes   free and unknown: one bit per voxel of the widened window            2 x [wd z][wd y][wide_words_per_row] 64-bit words
//   traversable   one bit per voxel of the window                                      [nz][ny][words_per_row] 64-bit words
//   cost          per voxel; with a clearance the distance field's dist2 beside it     (1 or 2) x [voxels] ints
//   flags         a tile is flagged for this round | for the next one                   2 x [n_tiles] ints
struct TravelPlan {
    int wo[3], wd[3];  // first voxel and extent of the window widened by one
    int64_t voxels;
    int64_t wide_words_per_row, wide_words;
    int64_t words_per_row, words;
    int64_t tiles[3], n_tiles;
    int64_t plane_words;  // 64-bit words of the three planes
    int64_t ints;         // ints of cost, dist2 and the flags
    int64_t max_rounds;   // the host loop's bound: no voxel's cheapest path crosses more tile borders than the window has voxels
};

constexpr int64_t travel_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int travel_level(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; }
constexpr int travel_code(int dx, int dy, int dz) { return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }

// what chisel_hip_travel_field refuses about its arguments other than the map, in the order of the header; null = go on, with *plan
// filled.  *code: TRAVEL_REFUSED_* of a refusal.  Window: chisel_hip_travel_window (a template, so that this header goes on including
// nothing of the library's).  The seeds are host memory: they are read here.
template <class Window>
inline const char *travel_refusal(const Window *w, const int32_t *seeds, int64_t n_seeds, const void *targets, int64_t n_targets, int64_t n_groups,
                                  const void *group_table, const void *totals, int *code, TravelPlan *plan) {
    *code = TRAVEL_REFUSED_INVALID;
    if (!w) return "null window";
    if (!seeds) return "null seeds";
    if (!totals) return "null totals";
    if (n_seeds < 1 || n_seeds > TRAVEL_MAX_SEEDS) return "n_seeds is outside 1 ... 2^20";
    for (int a = 0; a < 3; a++)
        if (w->dims[a] < 1) return "a window dimension below 1";
    for (int64_t i = 0; i < n_seeds; i++)
        for (int a = 0; a < 3; a++)
            if (seeds[3 * i + a] < 0 || seeds[3 * i + a] >= w->dims[a]) return "a seed outside the window";
    if (w->connectivity != 6 && w->connectivity != 18 && w->connectivity != 26) return "the connectivity is 6, 18 or 26";
    for (int k = 0; k < 3; k++)
        if (w->step_cost[k] < 1 || w->step_cost[k] > TRAVEL_MAX_STEP_COST) return "a step cost is outside 1 ... 65535";
    if (w->max_cost < 0 || w->max_cost > TRAVEL_MAX_COST) return "max_cost is outside 0 ... 2^30";
    if (w->clearance < 0 || w->clearance > TRAVEL_MAX_CLEARANCE) return "the clearance is outside 0 ... 64 voxels";
    if (w->surface_offset != w->surface_offset) return "the surface offset is NaN";
    if (n_targets < 0 || n_groups < 0) return "a negative count";
    if (n_targets > TRAVEL_MAX_VOXELS || n_groups > TRAVEL_MAX_VOXELS) return "more than 2^26 targets or groups";
    if (n_targets > 0 && !targets) return "a target count without the targets";
    if (n_targets > 0 && n_groups < 1) return "targets without n_groups >= 1";
    if (group_table && n_targets < 1) return "a group table without targets";
    const int64_t R = w->clearance > 1 ? w->clearance : 1;
    int64_t wd[3];
    for (int a = 0; a < 3; a++) {
        const int64_t lo = (int64_t)w->origin[a] - R, hi = (int64_t)w->origin[a] + (int64_t)w->dims[a] - 1 + R;
        if (lo < -TRAVEL_COORD_LIMIT || hi > TRAVEL_COORD_LIMIT) return "the window widened by the clearance reaches beyond voxel index +-2^30";
        wd[a] = (int64_t)w->dims[a] + 2;  // (<= 2^31 + 1)
        plan->wo[a] = (int)((int64_t)w->origin[a] - 1);
    }
    *code = TRAVEL_REFUSED_UNSUPPORTED;
    const int64_t nx = w->dims[0], ny = w->dims[1], nz = w->dims[2];
    if (nx > TRAVEL_MAX_VOXELS || nx * ny > TRAVEL_MAX_VOXELS || nx * ny * nz > TRAVEL_MAX_VOXELS)  // (each product <= 2^26 * 2^31)
        return "the window holds more than 2^26 voxels";
    for (int a = 0; a < 3; a++) plan->wd[a] = (int)wd[a];
    plan->voxels = nx * ny * nz;
    plan->wide_words_per_row = travel_ceil_div(wd[0], 64);
    plan->wide_words = plan->wide_words_per_row * wd[1] * wd[2];  // (<= 3 nx * 3 ny * 3 nz <= 27 * 2^26)
    plan->words_per_row = travel_ceil_div(nx, 64);
    plan->words = plan->words_per_row * ny * nz;
    plan->tiles[0] = travel_ceil_div(nx, TRAVEL_TILE_X);
    plan->tiles[1] = travel_ceil_div(ny, TRAVEL_TILE_Y);
    plan->tiles[2] = travel_ceil_div(nz, TRAVEL_TILE_Z);
    plan->n_tiles = plan->tiles[0] * plan->tiles[1] * plan->tiles[2];
    plan->plane_words = 2 * plan->wide_words + plan->words;
    plan->ints = (w->clearance > 0 ? 2 : 1) * plan->voxels + 2 * plan->n_tiles;
    plan->max_rounds = plan->voxels + 1;
    *code = 0;
    return nullptr;
}

// The size and reachability query: no array and no table is asked for.
inline bool travel_is_query(const void *cost, const void *step, const void *state, const void *group_table) { return !cost && !step && !state && !group_table; }

// is `code` a move of the connectivity?  -> its offset
inline bool travel_move(int code, int level, int d[3]) {
    if (code < 0 || code > 26 || code == TRAVEL_STEP_SEED) return false;
    d[0] = code % 3 - 1;
    d[1] = (code / 3) % 3 - 1;
    d[2] = code / 9 - 1;
    return (d[0] != 0) + (d[1] != 0) + (d[2] != 0) <= level;
}

// chisel_hip_travel_path: the walk along the steps from `from` to its seed, both ends included, (x, y, z) a row.  null = done, with
// *length filled; *length is also filled when the capacity is the only thing that is short, so that the caller can retry.
inline const char *travel_path_walk(const uint8_t *step, const int *dims, const int *from, int64_t capacity, int32_t *path, int64_t *length) {
    if (!step || !dims || !from || !path || !length) return "a null argument";
    if (capacity < 0) return "a negative capacity";
    for (int a = 0; a < 3; a++)
        if (dims[a] < 1) return "a window dimension below 1";
    const int64_t nx = dims[0], ny = dims[1], nz = dims[2];
    if (nx > TRAVEL_MAX_VOXELS || nx * ny > TRAVEL_MAX_VOXELS || nx * ny * nz > TRAVEL_MAX_VOXELS) return "the window holds more than 2^26 voxels";
    const int64_t voxels = nx * ny * nz;
    int64_t p[3] = {from[0], from[1], from[2]};
    for (int a = 0; a < 3; a++)
        if (p[a] < 0 || p[a] >= dims[a]) return "the start lies outside the window";
    if (step[(p[2] * ny + p[1]) * nx + p[0]] == TRAVEL_STEP_NONE) return "the start is not reached";
    int64_t n = 0;
    for (;;) {
        if (n >= voxels) return "the walk is longer than the window has voxels: the steps form a cycle";
        if (n < capacity) {
            path[3 * n] = (int32_t)p[0];
            path[3 * n + 1] = (int32_t)p[1];
            path[3 * n + 2] = (int32_t)p[2];
        }
        n++;
        const int code = step[(p[2] * ny + p[1]) * nx + p[0]];
        if (code == TRAVEL_STEP_SEED) break;
        int d[3];
        if (!travel_move(code, 3, d)) return "a step code that is no move";
        for (int a = 0; a < 3; a++) {
            p[a] += d[a];
            if (p[a] < 0 || p[a] >= dims[a]) return "a step leaves the window";
        }
    }
    *length = n;
    if (capacity < n) return "the capacity is below the path's length";
    return nullptr;
}

}  // namespace chisel_hip
