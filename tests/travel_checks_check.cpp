// Stand-alone check of cvids_amd/csrc/travel_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_travel_checks.py: every refusal of chisel_hip_travel_field's arguments with its code, in the order the header states; the
// seed check; the tile grid and the scratch sizes against brute force for small windows; the arithmetic at the limits (coordinates at
// +-2^30, 2^26 voxels in every shape), in 64 bits that must not overflow; chisel_hip_travel_path's walk on hand step volumes -- a
// straight walk, every refusal, a cyclic forgery that must stop at the length bound, a capacity one short.
#include <initializer_list>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <tuple>
#include <vector>

#include "travel_checks.h"

using namespace chisel_hip;

struct Window {  // = chisel_hip_travel_window
    int origin[3];
    int dims[3];
    int connectivity;
    int step_cost[3];
    int max_cost;
    int clearance;
    int unknown_is_obstacle;
    float surface_offset;
};
static_assert(sizeof(Window) == 56, "chisel_hip_travel_window is 56 bytes");

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s\n", __LINE__, #cond);                  \
            g_failed++;                                                \
        }                                                              \
    } while (0)

static Window window(int ox, int oy, int oz, int nx, int ny, int nz) { return Window{{ox, oy, oz}, {nx, ny, nz}, 26, {10, 14, 17}, 1 << 30, 0, 0, 0.0f}; }

static const int32_t kSeed[3] = {0, 0, 0};
static const int kSomething = 0;
struct Args {
    const int32_t *seeds;
    int64_t n_seeds;
    const void *targets;
    int64_t n_targets, n_groups;
    const void *table, *totals;
};
static const Args kPlain = {kSeed, 1, nullptr, 0, 0, nullptr, &kSomething};

// the refusal's code (0 = accepted); a refusal's text holds `word`
static int refused(const Window *w, const char *word, TravelPlan *plan = nullptr, const Args &a = kPlain) {
    TravelPlan local;
    int code = -1;
    const char *why = travel_refusal(w, a.seeds, a.n_seeds, a.targets, a.n_targets, a.n_groups, a.table, a.totals, &code, plan ? plan : &local);
    if (!why) {
        EXPECT(code == 0);
        return 0;
    }
    EXPECT(code == TRAVEL_REFUSED_INVALID || code == TRAVEL_REFUSED_UNSUPPORTED);
    if (word && !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why, word);
        g_failed++;
    }
    return code;
}

static int path_refused(const uint8_t *step, const int *dims, const int *from, int64_t capacity, int32_t *path, int64_t *length, const char *word) {
    const char *why = travel_path_walk(step, dims, from, capacity, path, length);
    if (!why) return 0;
    if (word && !strstr(why, word)) {
        printf("path refusal \"%s\" lacks \"%s\"\n", why, word);
        g_failed++;
    }
    return 1;
}

int main() {
    const int INV = TRAVEL_REFUSED_INVALID, UNS = TRAVEL_REFUSED_UNSUPPORTED, L = 1 << 30;
    // ---- refusals, each alone, in the order of the header
    Window ok = window(-5, 3, 100, 7, 9, 11);
    EXPECT(refused(&ok, nullptr) == 0);
    EXPECT(refused((const Window *)nullptr, "null window") == INV);
    {
        Args a = kPlain;
        a.seeds = nullptr;
        EXPECT(refused(&ok, "null seeds", nullptr, a) == INV);
        a = kPlain;
        a.totals = nullptr;
        EXPECT(refused(&ok, "null totals", nullptr, a) == INV);
        for (int64_t bad : {(int64_t)0, (int64_t)-1, TRAVEL_MAX_SEEDS + 1, (int64_t)INT64_MAX, (int64_t)INT64_MIN}) {
            a = kPlain;
            a.n_seeds = bad;
            EXPECT(refused(&ok, "n_seeds", nullptr, a) == INV);
        }
    }
    for (int a = 0; a < 3; a++)
        for (int bad : {0, -1, INT_MIN}) {
            Window w = ok;
            w.dims[a] = bad;
            EXPECT(refused(&w, "dimension") == INV);
        }
    {  // the seeds: the last voxel is one, one beyond it on any axis is none; all rows are read
        std::vector<int32_t> seeds(3 * TRAVEL_MAX_SEEDS, 0);
        Args a = kPlain;
        a.seeds = seeds.data();
        a.n_seeds = TRAVEL_MAX_SEEDS;
        seeds[3 * (TRAVEL_MAX_SEEDS - 1)] = 6;
        seeds[3 * (TRAVEL_MAX_SEEDS - 1) + 1] = 8;
        seeds[3 * (TRAVEL_MAX_SEEDS - 1) + 2] = 10;
        EXPECT(refused(&ok, nullptr, nullptr, a) == 0);
        for (int k = 0; k < 3; k++)
            for (int bad : {-1, ok.dims[k], INT_MAX, INT_MIN}) {
                const int32_t keep = seeds[3 * (TRAVEL_MAX_SEEDS - 1) + k];
                seeds[3 * (TRAVEL_MAX_SEEDS - 1) + k] = bad;
                EXPECT(refused(&ok, "seed outside", nullptr, a) == INV);
                seeds[3 * (TRAVEL_MAX_SEEDS - 1) + k] = keep;
            }
    }
    for (int bad : {0, 4, 7, 8, 27, -6}) {
        Window w = ok;
        w.connectivity = bad;
        EXPECT(refused(&w, "connectivity") == INV);
    }
    for (int connectivity : {6, 18, 26})
        for (int k = 0; k < 3; k++) {
            for (int bad : {0, -1, 65536, INT_MAX, INT_MIN}) {
                Window w = ok;
                w.connectivity = connectivity;
                w.step_cost[k] = bad;
                EXPECT(refused(&w, "step cost") == INV);  // (all three at every connectivity)
            }
            for (int good : {1, 65535}) {
                Window w = ok;
                w.connectivity = connectivity;
                w.step_cost[k] = good;
                EXPECT(refused(&w, nullptr) == 0);
            }
        }
    for (int bad : {-1, (1 << 30) + 1, INT_MAX, INT_MIN}) {
        Window w = ok;
        w.max_cost = bad;
        EXPECT(refused(&w, "max_cost") == INV);
    }
    for (int good : {0, 1 << 30}) {
        Window w = ok;
        w.max_cost = good;
        EXPECT(refused(&w, nullptr) == 0);
    }
    for (int bad : {-1, 65, INT_MAX}) {
        Window w = ok;
        w.clearance = bad;
        EXPECT(refused(&w, "clearance") == INV);
    }
    {
        Window w = ok;
        w.surface_offset = NAN;
        EXPECT(refused(&w, "NaN") == INV);
        w.surface_offset = INFINITY;
        EXPECT(refused(&w, nullptr) == 0);
    }
    {
        Args a = kPlain;
        a.n_targets = -1;
        EXPECT(refused(&ok, "negative", nullptr, a) == INV);
        a = kPlain;
        a.n_groups = -1;
        EXPECT(refused(&ok, "negative", nullptr, a) == INV);
        a = kPlain;
        a.targets = &kSomething;
        a.n_targets = TRAVEL_MAX_VOXELS + 1;
        a.n_groups = 1;
        EXPECT(refused(&ok, "2^26 targets", nullptr, a) == INV);
        a.n_targets = 3;
        a.n_groups = INT64_MAX;
        EXPECT(refused(&ok, "2^26 targets", nullptr, a) == INV);
        a.n_groups = 1;
        EXPECT(refused(&ok, nullptr, nullptr, a) == 0);
        a.targets = nullptr;
        EXPECT(refused(&ok, "without the targets", nullptr, a) == INV);
        a.targets = &kSomething;
        a.n_groups = 0;
        EXPECT(refused(&ok, "n_groups", nullptr, a) == INV);
        a = kPlain;
        a.table = &kSomething;
        EXPECT(refused(&ok, "table without targets", nullptr, a) == INV);
        a.targets = &kSomething;  // (targets without a count are no targets)
        EXPECT(refused(&ok, "table without targets", nullptr, a) == INV);
        a.n_targets = 1;
        a.n_groups = 1;
        EXPECT(refused(&ok, nullptr, nullptr, a) == 0);
    }
    // ---- the coordinates at +-2^30: the window widened by max(clearance, 1)
    for (int a = 0; a < 3; a++)
        for (int clearance : {0, 1, 2, 64}) {
            const int R = clearance > 1 ? clearance : 1;
            Window w = window(0, 0, 0, 4, 4, 4);
            w.clearance = clearance;
            w.origin[a] = L - 4 - R + 1;  // the last voxel widened: 2^30
            EXPECT(refused(&w, nullptr) == 0);
            w.origin[a]++;
            EXPECT(refused(&w, "2^30") == INV);
            w.origin[a] = -L + R;
            TravelPlan plan;
            EXPECT(refused(&w, nullptr, &plan) == 0);
            EXPECT(plan.wo[a] == -L + R - 1 && plan.wd[a] == 6);
            w.origin[a]--;
            EXPECT(refused(&w, "2^30") == INV);
            w.origin[a] = INT_MAX;
            EXPECT(refused(&w, "2^30") == INV);
            w.origin[a] = INT_MIN;
            EXPECT(refused(&w, "2^30") == INV);
        }
    // ---- 2^26 voxels in every shape, one more refused; no product overflows
    for (auto d : {std::make_tuple(1 << 26, 1, 1), std::make_tuple(1, 1 << 26, 1), std::make_tuple(1, 1, 1 << 26), std::make_tuple(512, 512, 256),
                   std::make_tuple(1 << 13, 1 << 13, 1)}) {
        Window w = window(-100, -100, -100, std::get<0>(d), std::get<1>(d), std::get<2>(d));
        TravelPlan plan;
        EXPECT(refused(&w, nullptr, &plan) == 0);
        EXPECT(plan.voxels == TRAVEL_MAX_VOXELS && plan.max_rounds == plan.voxels + 1);
        EXPECT(plan.words == travel_ceil_div(w.dims[0], 64) * w.dims[1] * w.dims[2]);
        EXPECT(plan.wide_words == travel_ceil_div((int64_t)w.dims[0] + 2, 64) * ((int64_t)w.dims[1] + 2) * ((int64_t)w.dims[2] + 2));
        EXPECT(plan.plane_words == 2 * plan.wide_words + plan.words && plan.ints == plan.voxels + 2 * plan.n_tiles);
        w.clearance = 1;
        EXPECT(refused(&w, nullptr, &plan) == 0 && plan.ints == 2 * plan.voxels + 2 * plan.n_tiles);
        w.dims[2]++;
        EXPECT(refused(&w, "2^26 voxels") == UNS);
    }
    {
        Window w = window(0, 0, 0, INT_MAX / 2, INT_MAX / 2, INT_MAX / 2);
        EXPECT(refused(&w, "2^26 voxels") == UNS);
        w = window(L - 3, 0, 0, 4, 1 << 13, 1 << 13);  // a coordinate (invalid) in front of the size (unsupported)
        EXPECT(refused(&w, "2^30") == INV);
        w = window(0, 0, 0, 0, 1 << 20, 1 << 20);  // a dimension in front of everything behind it
        w.connectivity = 5;
        EXPECT(refused(&w, "dimension") == INV);
    }
    // ---- the tile grid against brute force
    for (int nx : {1, 15, 16, 17, 33, 70})
        for (int ny : {1, 16, 17, 36})
            for (int nz : {1, 7, 8, 9, 12, 25}) {
                Window w = window(3, -4, 5, nx, ny, nz);
                TravelPlan plan;
                EXPECT(refused(&w, nullptr, &plan) == 0);
                std::set<std::tuple<int, int, int>> tiles;
                for (int z = 0; z < nz; z++)
                    for (int y = 0; y < ny; y++)
                        for (int x = 0; x < nx; x++) tiles.insert(std::make_tuple(x / TRAVEL_TILE_X, y / TRAVEL_TILE_Y, z / TRAVEL_TILE_Z));
                EXPECT((int64_t)tiles.size() == plan.n_tiles && plan.n_tiles == plan.tiles[0] * plan.tiles[1] * plan.tiles[2]);
                for (auto &t : tiles) EXPECT(std::get<0>(t) < plan.tiles[0] && std::get<1>(t) < plan.tiles[1] && std::get<2>(t) < plan.tiles[2]);
                EXPECT(plan.voxels == (int64_t)nx * ny * nz && plan.words_per_row == (nx + 63) / 64 && plan.wide_words_per_row == (nx + 2 + 63) / 64);
                for (int a = 0; a < 3; a++) EXPECT(plan.wo[a] == w.origin[a] - 1 && plan.wd[a] == w.dims[a] + 2);
            }
    // ---- the moves: 6, 18, 26 codes, none of them 13, the offsets back from the codes
    for (int level = 1; level <= 3; level++) {
        int n = 0;
        for (int code = 0; code < 256; code++) {
            int d[3];
            if (!travel_move(code, level, d)) continue;
            n++;
            EXPECT(travel_code(d[0], d[1], d[2]) == code && code != TRAVEL_STEP_SEED);
        }
        EXPECT(n == (level == 1 ? 6 : level == 2 ? 18 : 26));
    }
    EXPECT(travel_level(6) == 1 && travel_level(18) == 2 && travel_level(26) == 3);
    EXPECT((int64_t)TRAVEL_INFINITE > (int64_t)TRAVEL_MAX_COST && (int64_t)TRAVEL_INFINITE + TRAVEL_MAX_STEP_COST <= INT_MAX);
    // ---- chisel_hip_travel_path
    {
        const int dims[3] = {5, 3, 2};  // a straight walk along -x in row y = 1, z = 1, then a corner move down to the seed at (0, 0, 0)
        std::vector<uint8_t> step(30, TRAVEL_STEP_NONE);
        auto at = [&](int x, int y, int z) -> uint8_t & { return step[(z * 3 + y) * 5 + x]; };
        for (int x = 2; x < 5; x++) at(x, 1, 1) = (uint8_t)travel_code(-1, 0, 0);
        at(1, 1, 1) = (uint8_t)travel_code(-1, -1, -1);
        at(0, 0, 0) = TRAVEL_STEP_SEED;
        std::vector<int32_t> path(3 * 5, -7);
        int64_t length = -7;
        const int from[3] = {4, 1, 1};
        EXPECT(path_refused(step.data(), dims, from, 5, path.data(), &length, nullptr) == 0 && length == 5);
        const int32_t want[15] = {4, 1, 1, 3, 1, 1, 2, 1, 1, 1, 1, 1, 0, 0, 0};
        EXPECT(memcmp(path.data(), want, sizeof(want)) == 0);
        const int seed[3] = {0, 0, 0};
        length = -7;
        EXPECT(path_refused(step.data(), dims, seed, 1, path.data(), &length, nullptr) == 0 && length == 1 && path[0] == 0 && path[1] == 0 && path[2] == 0);
        // capacity one short: refused, the length filled, nothing written behind the capacity
        std::vector<int32_t> tight(3 * 4, -7);
        length = -7;
        EXPECT(path_refused(step.data(), dims, from, 4, tight.data(), &length, "capacity") == 1 && length == 5);
        EXPECT(memcmp(tight.data(), want, 12 * sizeof(int32_t)) == 0);
        length = -7;
        EXPECT(path_refused(step.data(), dims, from, 0, tight.data(), &length, "capacity") == 1 && length == 5);
        // every other refusal leaves the length alone
        length = -7;
        EXPECT(path_refused(nullptr, dims, from, 5, path.data(), &length, "null") == 1);
        EXPECT(path_refused(step.data(), nullptr, from, 5, path.data(), &length, "null") == 1);
        EXPECT(path_refused(step.data(), dims, nullptr, 5, path.data(), &length, "null") == 1);
        EXPECT(path_refused(step.data(), dims, from, 5, nullptr, &length, "null") == 1);
        EXPECT(path_refused(step.data(), dims, from, 5, path.data(), nullptr, "null") == 1);
        EXPECT(path_refused(step.data(), dims, from, -1, path.data(), &length, "negative") == 1);
        const int flat[3] = {5, 0, 2}, huge[3] = {1 << 20, 1 << 20, 1 << 20};
        EXPECT(path_refused(step.data(), flat, from, 5, path.data(), &length, "dimension") == 1);
        EXPECT(path_refused(step.data(), huge, from, 5, path.data(), &length, "2^26") == 1);
        for (int a = 0; a < 3; a++)
            for (int bad : {-1, dims[a], INT_MAX, INT_MIN}) {
                int start[3] = {4, 1, 1};
                start[a] = bad;
                EXPECT(path_refused(step.data(), dims, start, 5, path.data(), &length, "outside the window") == 1);
            }
        const int unreached[3] = {4, 2, 1};
        EXPECT(path_refused(step.data(), dims, unreached, 5, path.data(), &length, "not reached") == 1);
        for (int bad : {27, 100, 254}) {  // a code that is no move; 255 in the middle of a walk is none either
            at(2, 1, 1) = (uint8_t)bad;
            EXPECT(path_refused(step.data(), dims, from, 5, path.data(), &length, "no move") == 1);
        }
        at(2, 1, 1) = TRAVEL_STEP_NONE;
        EXPECT(path_refused(step.data(), dims, from, 5, path.data(), &length, "no move") == 1);
        at(2, 1, 1) = (uint8_t)travel_code(0, 0, 1);  // z = 2 is outside
        EXPECT(path_refused(step.data(), dims, from, 5, path.data(), &length, "leaves the window") == 1);
        at(2, 1, 1) = (uint8_t)travel_code(1, 0, 0);  // a forged cycle between x = 2 and x = 3: stops at the window's 30 voxels
        EXPECT(path_refused(step.data(), dims, from, 5, path.data(), &length, "cycle") == 1);
        std::vector<int32_t> roomy(3 * 64, -7);
        EXPECT(path_refused(step.data(), dims, from, 64, roomy.data(), &length, "cycle") == 1);
        for (int i = 3 * 30; i < 3 * 64; i++) EXPECT(roomy[i] == -7);  // no row behind the bound
        EXPECT(length == -7);
    }
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok: travel_checks.h\n");
    return 0;
}
