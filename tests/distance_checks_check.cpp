// Stand-alone check of cvids_amd/csrc/distance_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_distance_restated.py: every refusal of chisel_hip_distance_field's window with its code, in the order the header states;
// the widened window and the scratch sizes, at the limits too (coordinates at +-2^30, 2^30 voxels), in 64-bit arithmetic that must not
// overflow; and the distance table against sqrt in double.
#include <initializer_list>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "distance_checks.h"

using namespace chisel_hip;

struct Window {  // = chisel_hip_distance_window
    int origin[3];
    int dims[3];
    int radius;
    int unknown_is_obstacle;
    float surface_offset;
};
static_assert(sizeof(Window) == 36, "chisel_hip_distance_window is 36 bytes");

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s\n", __LINE__, #cond);                  \
            g_failed++;                                                \
        }                                                              \
    } while (0)

static Window window(int ox, int oy, int oz, int nx, int ny, int nz, int R, float offset = 0.0f) { return Window{{ox, oy, oz}, {nx, ny, nz}, R, 0, offset}; }

// the refusal's code (0 = accepted) and, in *why, a word of its text
static int refused(const Window *w, bool any_output, const char *word, DistancePlan *plan = nullptr) {
    DistancePlan local;
    int code = -1;
    const char *why = distance_refusal(w, any_output, &code, plan ? plan : &local);
    if (!why) {
        EXPECT(code == 0);
        return 0;
    }
    EXPECT(code == DISTANCE_REFUSED_INVALID || code == DISTANCE_REFUSED_UNSUPPORTED);
    if (word && !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why, word);
        g_failed++;
    }
    return code;
}

int main() {
    const int INV = DISTANCE_REFUSED_INVALID, UNS = DISTANCE_REFUSED_UNSUPPORTED, L = 1 << 30;
    // ---- refusals, each alone, then in the order of the header
    Window ok = window(-5, 3, 100, 7, 9, 11, 4);
    EXPECT(refused(&ok, true, nullptr) == 0);
    EXPECT(refused((const Window *)nullptr, true, "null window") == INV);
    EXPECT(refused(&ok, false, "output") == INV);
    for (int a = 0; a < 3; a++)
        for (int bad : {0, -1, INT_MIN}) {
            Window w = ok;
            w.dims[a] = bad;
            EXPECT(refused(&w, true, "dimension") == INV);
        }
    for (int bad : {0, -1, 65, INT_MAX, INT_MIN}) {
        Window w = ok;
        w.radius = bad;
        EXPECT(refused(&w, true, "radius") == INV);
    }
    for (int good : {1, 64}) {
        Window w = ok;
        w.radius = good;
        EXPECT(refused(&w, true, nullptr) == 0);
    }
    {
        Window w = ok;
        w.surface_offset = NAN;
        EXPECT(refused(&w, true, "NaN") == INV);
        w.surface_offset = INFINITY;
        EXPECT(refused(&w, true, nullptr) == 0);
        w.surface_offset = -0.0f;
        EXPECT(refused(&w, true, nullptr) == 0);
        w.dims[1] = 0;  // (a dimension is refused before the radius, the radius before the offset)
        w.radius = 0;
        w.surface_offset = NAN;
        EXPECT(refused(&w, true, "dimension") == INV);
        w.dims[1] = 1;
        EXPECT(refused(&w, true, "radius") == INV);
    }
    // ---- coordinates: the widened window may touch +-2^30 and not pass it
    for (int a = 0; a < 3; a++) {
        Window w = window(0, 0, 0, 1, 1, 1, 3);
        w.origin[a] = -L + 3;
        EXPECT(refused(&w, true, nullptr) == 0);
        w.origin[a] = -L + 2;
        EXPECT(refused(&w, true, "2^30") == INV);
        w.origin[a] = L - 3;
        EXPECT(refused(&w, true, nullptr) == 0);
        w.origin[a] = L - 2;
        EXPECT(refused(&w, true, "2^30") == INV);
        w.origin[a] = L - 12;
        w.dims[a] = 10;  // last voxel L - 3
        EXPECT(refused(&w, true, nullptr) == 0);
        w.dims[a] = 11;
        EXPECT(refused(&w, true, "2^30") == INV);
        for (int far : {INT_MAX, INT_MIN}) {  // (no overflow on the way to the verdict)
            w.origin[a] = far;
            w.dims[a] = INT_MAX;
            w.radius = 64;
            EXPECT(refused(&w, true, "2^30") == INV);
        }
    }
    {  // a coordinate is refused (invalid) before the size (unsupported)
        Window w = window(L - 2, 0, 0, 1, 4096, 4096, 64);
        EXPECT(refused(&w, true, "2^30") == INV);
    }
    // ---- sizes at the limit: 2^30 voxels of the widened window pass, one row more does not
    {
        DistancePlan p;
        Window w = window(-512 + 8, -512 + 8, -512 + 8, 1024 - 16, 1024 - 16, 1024 - 16, 8);
        EXPECT(refused(&w, true, nullptr, &p) == 0);
        EXPECT(p.widened == (1ll << 30) && p.voxels == 1008ll * 1008 * 1008);
        EXPECT(p.wo[0] == -512 && p.wd[0] == 1024 && p.wd[2] == 1024);
        EXPECT(p.words_per_row == 16 && p.bits_words == 16ll * 1024 * 1024);
        EXPECT(p.g1_elems == 1008ll * 1024 * 1024 && p.g2_elems == 1008ll * 1008 * 1024);
        w.dims[2] += 1;
        EXPECT(refused(&w, true, "more than 2^30 voxels") == UNS);
        Window line = window(-L + 64, 0, 0, 1, 1, 1, 64);  // widened: 129^3
        line.dims[0] = L - 128;  // widened x = 2^30: alone at the limit, times 129^2 beyond it
        EXPECT(refused(&line, true, "more than 2^30 voxels") == UNS);
        Window wide = window(-L + 64, 0, 0, L + (L - 127), 1, 1, 64);  // widened x = 2^31 + 1: beyond every product
        EXPECT(refused(&wide, true, "more than 2^30 voxels") == UNS);
        Window all = window(-L + 64, -L + 64, -L + 64, L + (L - 127), L + (L - 127), L + (L - 127), 64);  // (2^31 + 1)^3 does not fit 64 bits
        EXPECT(refused(&all, true, "more than 2^30 voxels") == UNS);
    }
    {  // odd sizes: the last word of a row is partial
        DistancePlan p;
        Window w = window(5, -7, 9, 1, 2, 3, 1);
        EXPECT(refused(&w, true, nullptr, &p) == 0);
        EXPECT(p.wo[0] == 4 && p.wo[1] == -8 && p.wo[2] == 8 && p.wd[0] == 3 && p.wd[1] == 4 && p.wd[2] == 5);
        EXPECT(p.voxels == 6 && p.widened == 60 && p.words_per_row == 1 && p.bits_words == 20 && p.g1_elems == 20 && p.g2_elems == 10);
        w = window(0, 0, 0, 63, 1, 1, 1);  // widened x = 65
        EXPECT(refused(&w, true, nullptr, &p) == 0);
        EXPECT(p.words_per_row == 2 && p.bits_words == 2 * 3 * 3);
        w = window(0, 0, 0, 62, 1, 1, 1);  // widened x = 64
        EXPECT(refused(&w, true, nullptr, &p) == 0);
        EXPECT(p.words_per_row == 1);
    }
    // ---- the table: every entry against sqrt in double, in a buffer of exactly R^2 + 1 floats
    for (int R : {1, 2, 5, 13, 64})
        for (float res : {0.0625f, 0.02f, 0.03f, 1.0f, 1e-3f}) {
            std::vector<float> t((size_t)R * R + 1);
            distance_table(R, res, t.data());
            for (int i = 0; i <= R * R; i++) EXPECT(t[i] == (float)(sqrt((double)i) * (double)res));
            EXPECT(t[0] == 0.0f && t[1] == res);
            if (res == 0.0625f) EXPECT(t[R * R] == (float)R * res);  // (exact: a power of two)
        }
    if (g_failed) {
        printf("FAILED: %d checks\n", g_failed);
        return 1;
    }
    printf("ok: refusals, sizes at the limits and the distance table\n");
    return 0;
}
