// Stand-alone check of cvids_amd/csrc/frontier_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_frontier_checks.py: every refusal of chisel_hip_frontiers' arguments with its code, in the order the header states; the
// widened window, the tile grid and the scratch sizes against brute force for small windows; the arithmetic at the limits
// (coordinates at +-2^30, 2^26 voxels in every shape), in 64 bits that must not overflow; the capacities against the totals; the
// forward offsets of the three connectivities.
#include <initializer_list>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <tuple>

#include "frontier_checks.h"

using namespace chisel_hip;

struct Window {  // = chisel_hip_frontier_window
    int origin[3];
    int dims[3];
    int min_unknown_faces;
    int connectivity;
    int min_voxels;
    float surface_offset;
};
static_assert(sizeof(Window) == 40, "chisel_hip_frontier_window is 40 bytes");

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s\n", __LINE__, #cond);                  \
            g_failed++;                                                \
        }                                                              \
    } while (0)

static Window window(int ox, int oy, int oz, int nx, int ny, int nz) { return Window{{ox, oy, oz}, {nx, ny, nz}, 1, 26, 1, 0.0f}; }

struct Args {
    const void *totals, *voxels, *table;
    int64_t capacity_voxels, capacity_clusters;
};
static const int kSomething = 0;
static const Args kPlain = {&kSomething, nullptr, nullptr, 0, 0};

// the refusal's code (0 = accepted); a refusal's text holds `word`
static int refused(const Window *w, const char *word, FrontierPlan *plan = nullptr, const Args &a = kPlain) {
    FrontierPlan local;
    int code = -1;
    const char *why = frontier_refusal(w, a.totals, a.capacity_voxels, a.voxels, a.capacity_clusters, a.table, &code, plan ? plan : &local);
    if (!why) {
        EXPECT(code == 0);
        return 0;
    }
    EXPECT(code == FRONTIER_REFUSED_INVALID || code == FRONTIER_REFUSED_UNSUPPORTED);
    if (word && !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why, word);
        g_failed++;
    }
    return code;
}

int main() {
    const int INV = FRONTIER_REFUSED_INVALID, UNS = FRONTIER_REFUSED_UNSUPPORTED, L = 1 << 30;
    // ---- refusals, each alone
    Window ok = window(-5, 3, 100, 7, 9, 11);
    EXPECT(refused(&ok, nullptr) == 0);
    EXPECT(refused((const Window *)nullptr, "null window") == INV);
    {
        Args a = kPlain;
        a.totals = nullptr;
        EXPECT(refused(&ok, "null totals", nullptr, a) == INV);
    }
    for (int a = 0; a < 3; a++)
        for (int bad : {0, -1, INT_MIN}) {
            Window w = ok;
            w.dims[a] = bad;
            EXPECT(refused(&w, "dimension") == INV);
        }
    for (int bad : {0, -1, 7, INT_MAX, INT_MIN}) {
        Window w = ok;
        w.min_unknown_faces = bad;
        EXPECT(refused(&w, "min_unknown_faces") == INV);
    }
    for (int good : {1, 2, 3, 4, 5, 6}) {
        Window w = ok;
        w.min_unknown_faces = good;
        EXPECT(refused(&w, nullptr) == 0);
    }
    for (int bad : {0, 1, 4, 8, 27, -6, INT_MAX}) {
        Window w = ok;
        w.connectivity = bad;
        EXPECT(refused(&w, "connectivity") == INV);
    }
    for (int good : {6, 18, 26}) {
        Window w = ok;
        w.connectivity = good;
        EXPECT(refused(&w, nullptr) == 0);
    }
    for (int bad : {0, -1, INT_MIN}) {
        Window w = ok;
        w.min_voxels = bad;
        EXPECT(refused(&w, "min_voxels") == INV);
    }
    {
        Window w = ok;
        w.min_voxels = INT_MAX;
        EXPECT(refused(&w, nullptr) == 0);
        w.surface_offset = NAN;
        EXPECT(refused(&w, "NaN") == INV);
        w.surface_offset = INFINITY;
        EXPECT(refused(&w, nullptr) == 0);
        w.surface_offset = -0.0f;
        EXPECT(refused(&w, nullptr) == 0);
    }
    {
        int64_t table[12];
        int rows[4];
        Args a = kPlain;
        a.capacity_voxels = -1;
        EXPECT(refused(&ok, "negative", nullptr, a) == INV);
        a = kPlain;
        a.capacity_clusters = INT64_MIN;
        EXPECT(refused(&ok, "negative", nullptr, a) == INV);
        a = kPlain;
        a.capacity_voxels = 1;
        EXPECT(refused(&ok, "voxel capacity without", nullptr, a) == INV);
        a.voxels = rows;
        EXPECT(refused(&ok, nullptr, nullptr, a) == 0);
        a.capacity_clusters = 1;
        EXPECT(refused(&ok, "cluster capacity without", nullptr, a) == INV);
        a.table = table;
        EXPECT(refused(&ok, nullptr, nullptr, a) == 0);
        a.capacity_voxels = a.capacity_clusters = 0;  // an array with capacity 0 is not asked for
        EXPECT(refused(&ok, nullptr, nullptr, a) == 0);
        EXPECT(frontier_is_query(nullptr, nullptr, 0, rows, 0, table) && frontier_is_query(nullptr, nullptr, 0, nullptr, 0, nullptr));
        EXPECT(!frontier_is_query(rows, nullptr, 0, nullptr, 0, nullptr) && !frontier_is_query(nullptr, rows, 0, nullptr, 0, nullptr));
        EXPECT(!frontier_is_query(nullptr, nullptr, 1, rows, 0, nullptr) && !frontier_is_query(nullptr, nullptr, 0, nullptr, 1, table));
    }
    // ---- the order of the header: each refusal in front of all later ones
    {
        Window w = ok;
        Args a = kPlain;
        w.origin[0] = L;                 // 11 a coordinate
        a.capacity_clusters = 1;         // 10 a capacity without its array
        EXPECT(refused(&w, "cluster capacity without", nullptr, a) == INV);
        a.capacity_voxels = -1;          // 9
        EXPECT(refused(&w, "negative", nullptr, a) == INV);
        w.surface_offset = NAN;          // 8
        EXPECT(refused(&w, "NaN", nullptr, a) == INV);
        w.min_voxels = 0;                // 7
        EXPECT(refused(&w, "min_voxels", nullptr, a) == INV);
        w.connectivity = 7;              // 6
        EXPECT(refused(&w, "connectivity", nullptr, a) == INV);
        w.min_unknown_faces = 0;         // 5
        EXPECT(refused(&w, "min_unknown_faces", nullptr, a) == INV);
        w.dims[2] = 0;                   // 4
        EXPECT(refused(&w, "dimension", nullptr, a) == INV);
        a.totals = nullptr;              // 3
        EXPECT(refused(&w, "null totals", nullptr, a) == INV);
        EXPECT(refused((const Window *)nullptr, "null window", nullptr, a) == INV);
        Window big = window(L - 2, 0, 0, 4, 1 << 13, 1 << 13);  // a coordinate (invalid) in front of the size (unsupported)
        EXPECT(refused(&big, "2^30") == INV);
    }
    // ---- coordinates: the widened window may touch +-2^30 and not pass it
    for (int a = 0; a < 3; a++) {
        Window w = window(0, 0, 0, 1, 1, 1);
        w.origin[a] = -L + 1;
        EXPECT(refused(&w, nullptr) == 0);
        w.origin[a] = -L;
        EXPECT(refused(&w, "2^30") == INV);
        w.origin[a] = L - 1;
        EXPECT(refused(&w, nullptr) == 0);
        w.origin[a] = L;
        EXPECT(refused(&w, "2^30") == INV);
        w.origin[a] = L - 10;
        w.dims[a] = 10;  // last voxel L - 1
        EXPECT(refused(&w, nullptr) == 0);
        w.dims[a] = 11;
        EXPECT(refused(&w, "2^30") == INV);
        for (int far : {INT_MAX, INT_MIN}) {  // (no overflow on the way to the verdict)
            w.origin[a] = far;
            w.dims[a] = INT_MAX;
            EXPECT(refused(&w, "2^30") == INV);
        }
    }
    // ---- sizes at the limit: 2^26 voxels pass in every shape, one row more does not
    {
        FrontierPlan p;
        Window w = window(-200, -200, -200, 512, 512, 256);
        EXPECT(refused(&w, nullptr, &p) == 0);
        EXPECT(p.voxels == (1ll << 26) && p.wo[0] == -201 && p.wd[0] == 514 && p.wd[1] == 514 && p.wd[2] == 258);
        EXPECT(p.wide_words_per_row == 9 && p.wide_words == 9ll * 514 * 258 && p.words_per_row == 8 && p.words == 8ll * 512 * 256);
        EXPECT(p.tiles[0] == 32 && p.tiles[1] == 32 && p.tiles[2] == 32 && p.n_tiles == 32768 && p.scan_tiles == 4096);
        EXPECT(p.plane_words == 2 * p.wide_words + 5 * p.words + p.scan_tiles && p.ints == 3ll << 26);
        w.dims[2] += 1;
        EXPECT(refused(&w, "more than 2^26 voxels") == UNS);
        for (int a = 0; a < 3; a++) {  // a line: the words of a row of one voxel, the widened window nine times the rows
            Window line = window(0, 0, 0, 1, 1, 1);
            line.dims[a] = 1 << 26;
            EXPECT(refused(&line, nullptr, &p) == 0);
            EXPECT(p.voxels == (1ll << 26) && p.words == (a == 0 ? 1ll << 20 : 1ll << 26));
            EXPECT(p.wide_words == (a == 0 ? ((1ll << 20) + 1) * 9 : 3 * ((1ll << 26) + 2)));
            EXPECT(p.n_tiles == (1ll << 26) / (a == 0 ? FRONTIER_TILE_X : a == 1 ? FRONTIER_TILE_Y : FRONTIER_TILE_Z));
            EXPECT(p.n_tiles < (1ll << 31) && p.wide_words / 4 < (1ll << 31) && p.plane_words * 8 < (1ll << 36));
            line.dims[a] += 1;
            EXPECT(refused(&line, "more than 2^26 voxels") == UNS);
        }
        Window all = window(-L + 1, -L + 1, -L + 1, INT_MAX, INT_MAX, INT_MAX);  // (2^31 - 1)^3 does not fit 64 bits: refused before it is formed
        EXPECT(refused(&all, "more than 2^26 voxels") == UNS);
        Window two = window(0, 0, 0, 1 << 14, 1 << 14, 1);
        EXPECT(refused(&two, "more than 2^26 voxels") == UNS);
    }
    // ---- small windows against brute force: every voxel of the window and of the widened window is counted where the plan says
    for (int nx : {1, 2, 15, 16, 17, 62, 63, 64, 65, 129})
        for (int ny : {1, 15, 16, 17, 33})
            for (int nz : {1, 7, 8, 9}) {
                FrontierPlan p;
                Window w = window(-7, 5, -3, nx, ny, nz);
                EXPECT(refused(&w, nullptr, &p) == 0);
                std::set<std::tuple<int, int, int>> tiles;
                std::set<std::tuple<int, int, int>> words, wide_words;
                for (int z = 0; z < nz; z++)
                    for (int y = 0; y < ny; y++)
                        for (int x = 0; x < nx; x++) {
                            tiles.insert(std::make_tuple(x / FRONTIER_TILE_X, y / FRONTIER_TILE_Y, z / FRONTIER_TILE_Z));
                            words.insert(std::make_tuple(x / 64, y, z));
                        }
                for (int z = 0; z < nz + 2; z++)
                    for (int y = 0; y < ny + 2; y++)
                        for (int x = 0; x < nx + 2; x++) wide_words.insert(std::make_tuple(x / 64, y, z));
                EXPECT(p.voxels == (int64_t)nx * ny * nz && p.n_tiles == (int64_t)tiles.size() && p.words == (int64_t)words.size());
                EXPECT(p.wide_words == (int64_t)wide_words.size() && p.wo[0] == -8 && p.wo[1] == 4 && p.wo[2] == -4);
                EXPECT(p.wd[0] == nx + 2 && p.wd[1] == ny + 2 && p.wd[2] == nz + 2);
                EXPECT(p.words_per_row <= p.wide_words_per_row);  // (the mark reads word w and w + 1 of a wide row for the window's word w)
                EXPECT(p.scan_tiles * FRONTIER_THREADS >= p.words && (p.scan_tiles - 1) * FRONTIER_THREADS < p.words);
                EXPECT(p.tiles[0] * p.tiles[1] * p.tiles[2] == p.n_tiles);
                EXPECT(p.plane_words == 2 * p.wide_words + 5 * p.words + p.scan_tiles && p.ints == 3 * p.voxels);
            }
    // ---- the capacities against the totals
    {
        int64_t table[12];
        int rows[4];
        EXPECT(!frontier_capacity_refusal(10, 3, 10, rows, 3, table));
        EXPECT(strstr(frontier_capacity_refusal(10, 3, 9, rows, 3, table), "voxel capacity"));
        EXPECT(strstr(frontier_capacity_refusal(10, 3, 10, rows, 2, table), "cluster capacity"));
        EXPECT(strstr(frontier_capacity_refusal(10, 3, 9, rows, 2, table), "voxel capacity"));  // the list first
        EXPECT(!frontier_capacity_refusal(10, 3, 0, rows, 0, table));  // (capacity 0: not asked for)
        EXPECT(!frontier_capacity_refusal(10, 3, 0, nullptr, 0, nullptr));
        EXPECT(!frontier_capacity_refusal(0, 0, 1, rows, 1, table));
    }
    // ---- the forward offsets: half of the neighbourhood, each pair once
    for (int connectivity : {6, 18, 26}) {
        int off[13][3];
        const int n = frontier_forward_offsets(connectivity, off);
        EXPECT(n == connectivity / 2 && frontier_level(connectivity) == (connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3));
        std::set<std::tuple<int, int, int>> seen;
        for (int i = 0; i < n; i++) {
            const int nonzero = (off[i][0] != 0) + (off[i][1] != 0) + (off[i][2] != 0);
            EXPECT(nonzero >= 1 && nonzero <= frontier_level(connectivity));
            EXPECT((off[i][2] * 3 + off[i][1]) * 3 + off[i][0] > 0);  // forward in the linear index of any window
            seen.insert(std::make_tuple(off[i][0], off[i][1], off[i][2]));
            seen.insert(std::make_tuple(-off[i][0], -off[i][1], -off[i][2]));
        }
        EXPECT((int)seen.size() == connectivity);
    }
    if (g_failed) {
        printf("FAILED: %d checks\n", g_failed);
        return 1;
    }
    printf("ok: refusals in order, the tile grid and scratch sizes against brute force, the limits\n");
    return 0;
}
