// Stand-alone check of cvids_amd/csrc/components_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_components_checks.py: every refusal of chisel_hip_mesh_components and chisel_hip_filter_mesh that needs no device, the
// capacities against the totals, and the size, tile and key arithmetic at and beside 2^31 - 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "components_checks.h"

using namespace chisel_hip;

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s\n", __LINE__, #cond);                  \
            g_failed++;                                                \
        }                                                              \
    } while (0)

static const int64_t MAX = 0x7fffffffll;
static int32_t g_x[8], g_vc[8], g_tc[8];
static int64_t g_table[8];
static float g_v[8], g_n[8], g_c[8], g_ov[8], g_on[8], g_oc[8];
static int32_t g_ox[8];
static char g_totals[64];

// true when `why` is a refusal with `word` in its text and the status `unsupported` (word null: accepted)
static bool is(const char *why, bool got_unsupported, const char *word, bool unsupported = false) {
    if (!word) return why == nullptr;
    if (!why || !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why ? why : "(none)", word);
        return false;
    }
    return got_unsupported == unsupported;
}

struct C {  // the arguments of chisel_hip_mesh_components, a good call
    int64_t V = 5, T = 2, cap = 5;
    const void *x = g_x, *vc = g_vc, *tc = g_tc, *table = g_table, *totals = g_totals;
};
static bool components(const C &a, const char *word, bool unsupported = false) {
    bool u = true;
    const char *why = components_request_refusal(a.V, a.T, a.x, a.vc, a.tc, a.cap, a.table, a.totals, &u);
    return is(why, u, word, unsupported);
}

struct F {  // the arguments of chisel_hip_filter_mesh, a good call
    int64_t V = 5, T = 2, min_triangles = 1, cap_v = 5, cap_t = 2;
    int largest_only = 0;
    const void *x = g_x, *v = g_v, *n = g_n, *c = g_c, *ov = g_ov, *ox = g_ox, *on = g_on, *oc = g_oc, *totals = g_totals;
};
static bool filter(const F &a, const char *word, bool unsupported = false) {
    bool u = true;
    const char *why = filter_request_refusal(a.V, a.T, a.x, a.v, a.n, a.c, a.min_triangles, a.largest_only, a.cap_v, a.cap_t, a.ov, a.ox, a.on, a.oc, a.totals, &u);
    return is(why, u, word, unsupported);
}

int main() {
    // ---- chisel_hip_mesh_components
    EXPECT(components(C(), nullptr));
    { C a; a.V = -1; EXPECT(components(a, "negative size")); }
    { C a; a.T = -1; EXPECT(components(a, "negative size")); }
    { C a; a.V = MAX; EXPECT(components(a, nullptr)); }
    { C a; a.V = MAX + 1; EXPECT(components(a, "2^31 - 1 vertices", true)); }
    { C a; a.V = INT64_MAX; EXPECT(components(a, "2^31 - 1 vertices", true)); }
    { C a; a.T = MAX / 3; EXPECT(components(a, nullptr)); }  // 715 827 882 triangles: 2 147 483 646 entries
    { C a; a.T = MAX / 3 + 1; EXPECT(components(a, "index entries", true)); }
    { C a; a.T = INT64_MAX; EXPECT(components(a, "index entries", true)); }
    { C a; a.x = nullptr; EXPECT(components(a, "null indices")); }
    { C a; a.x = nullptr; a.T = 0; EXPECT(components(a, nullptr)); }
    { C a; a.V = 0; a.T = 0; a.x = nullptr; EXPECT(components(a, nullptr)); }
    { C a; a.cap = -1; EXPECT(components(a, "negative capacity")); }
    { C a; a.table = nullptr; EXPECT(components(a, "capacity without a table")); }
    { C a; a.table = nullptr; a.cap = 0; EXPECT(components(a, nullptr)); }
    { C a; a.totals = nullptr; EXPECT(components(a, nullptr)); }  // (totals are optional beside an output)
    { C a; a.vc = a.tc = nullptr; a.cap = 0; EXPECT(components(a, nullptr)); }  // the size query
    { C a; a.vc = a.tc = nullptr; a.cap = 0; a.totals = nullptr; EXPECT(components(a, "size query without totals")); }
    { C a; a.vc = a.tc = a.table = nullptr; a.cap = 0; a.totals = nullptr; EXPECT(components(a, "size query without totals")); }
    { C a; a.vc = a.tc = nullptr; a.totals = nullptr; EXPECT(components(a, nullptr)); }  // (a table alone is an output)
    EXPECT(components_is_query(nullptr, nullptr, 0, g_table) && components_is_query(nullptr, nullptr, 0, nullptr));
    EXPECT(!components_is_query(g_vc, nullptr, 0, nullptr) && !components_is_query(nullptr, g_tc, 0, nullptr) && !components_is_query(nullptr, nullptr, 1, g_table));
    EXPECT(components_capacity_refusal(5, 5, g_table) == nullptr && components_capacity_refusal(5, 6, g_table) == nullptr);
    EXPECT(components_capacity_refusal(5, 4, g_table) != nullptr && components_capacity_refusal(MAX, MAX - 1, g_table) != nullptr);
    EXPECT(components_capacity_refusal(5, 0, g_table) == nullptr && components_capacity_refusal(5, 4, nullptr) == nullptr);  // (not asked for)

    // ---- chisel_hip_filter_mesh
    EXPECT(filter(F(), nullptr));
    { F a; a.V = -1; EXPECT(filter(a, "negative size")); }
    { F a; a.T = -2; EXPECT(filter(a, "negative size")); }
    { F a; a.V = MAX + 1; EXPECT(filter(a, "vertices", true)); }
    { F a; a.T = MAX / 3 + 1; EXPECT(filter(a, "index entries", true)); }
    { F a; a.x = nullptr; EXPECT(filter(a, "null indices")); }
    { F a; a.min_triangles = 0; EXPECT(filter(a, "min_triangles")); }
    { F a; a.min_triangles = -5; EXPECT(filter(a, "min_triangles")); }
    { F a; a.min_triangles = INT64_MAX; EXPECT(filter(a, nullptr)); }
    { F a; a.largest_only = 2; EXPECT(filter(a, "largest_only")); }
    { F a; a.largest_only = -1; EXPECT(filter(a, "largest_only")); }
    { F a; a.largest_only = 1; EXPECT(filter(a, nullptr)); }
    { F a; a.cap_v = -1; EXPECT(filter(a, "negative capacity")); }
    { F a; a.cap_t = -1; EXPECT(filter(a, "negative capacity")); }
    { F a; a.cap_v = a.cap_t = 0; EXPECT(filter(a, nullptr)); }  // the size query: nothing else is looked at
    { F a; a.cap_v = a.cap_t = 0; a.v = a.ov = nullptr; EXPECT(filter(a, nullptr)); }
    { F a; a.cap_v = a.cap_t = 0; a.totals = nullptr; EXPECT(filter(a, "size query without totals")); }
    { F a; a.cap_v = a.cap_t = 0; a.min_triangles = 0; EXPECT(filter(a, "min_triangles")); }  // (the knobs are refused in a query too)
    { F a; a.v = nullptr; EXPECT(filter(a, "vertices out without vertices in")); }
    { F a; a.n = nullptr; EXPECT(filter(a, "normals out without normals in")); }
    { F a; a.c = nullptr; EXPECT(filter(a, "colors out without colors in")); }
    { F a; a.on = nullptr; EXPECT(filter(a, "normals in without normals out")); }
    { F a; a.oc = nullptr; EXPECT(filter(a, "colors in without colors out")); }
    { F a; a.n = a.on = a.c = a.oc = nullptr; EXPECT(filter(a, nullptr)); }
    { F a; a.ov = nullptr; EXPECT(filter(a, "indices out without vertices out")); }
    { F a; a.ov = a.ox = nullptr; EXPECT(filter(a, "without vertices out")); }
    { F a; a.ov = a.ox = a.on = a.oc = nullptr; EXPECT(filter(a, nullptr)); }  // (the maps alone; inputs without outputs are not read)
    { F a; a.ox = nullptr; EXPECT(filter(a, nullptr)); }
    { F a; a.totals = nullptr; EXPECT(filter(a, nullptr)); }
    EXPECT(filter_capacity_refusal(5, 2, 5, 2, g_ov, g_ox) == nullptr && filter_capacity_refusal(5, 2, 6, 3, g_ov, g_ox) == nullptr);
    EXPECT(strstr(filter_capacity_refusal(5, 2, 4, 2, g_ov, g_ox), "vertex capacity") && strstr(filter_capacity_refusal(5, 2, 5, 1, g_ov, g_ox), "triangle capacity"));
    EXPECT(filter_capacity_refusal(5, 2, 4, 1, nullptr, nullptr) == nullptr && strstr(filter_capacity_refusal(5, 2, 5, 1, g_ov, g_ox), "triangle"));
    EXPECT(filter_capacity_refusal(MAX, MAX / 3, MAX, MAX / 3, g_ov, g_ox) == nullptr && filter_capacity_refusal(MAX, MAX / 3, MAX - 1, MAX / 3, g_ov, g_ox) != nullptr);

    // ---- the arithmetic
    EXPECT(components_tiles(0) == 0 && components_tiles(1) == 1 && components_tiles(COMPONENTS_TILE) == 1 && components_tiles(COMPONENTS_TILE + 1) == 2);
    EXPECT(components_tiles(MAX) == (1ll << 23) && components_tiles(MAX - 254) == (1ll << 23) && components_tiles(MAX - 255) == (1ll << 23) - 1);
    EXPECT(components_tiles(MAX) * COMPONENTS_TILE >= MAX && (components_tiles(MAX) - 1) * COMPONENTS_TILE < MAX);
    const int64_t most = MAX / 3;  // the most triangles of one component
    EXPECT(components_key_triangles(components_largest_key(most, 0)) == most && components_key_number(components_largest_key(most, 0)) == 0);
    EXPECT(components_key_triangles(components_largest_key(0, MAX - 1)) == 0 && components_key_number(components_largest_key(0, MAX - 1)) == MAX - 1);
    EXPECT(components_largest_key(0, MAX - 1) > 0);                                   // 0 is below every key
    EXPECT(components_largest_key(7, 3) > components_largest_key(7, 4));              // equal triangles: the lower number wins
    EXPECT(components_largest_key(8, MAX - 1) > components_largest_key(7, 0));        // more triangles win whatever the number
    EXPECT(components_largest_key(most, MAX - 1) > components_largest_key(most - 1, 0));
    EXPECT(components_largest_key(1, 0) == 0x1ffffffffull && components_largest_key(0, 0) == 0xffffffffull);
    static_assert(COMPONENTS_HOST_WORDS > CC_KEPT_TRIANGLES, "the control words fit");

    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok: components_checks.h\n");
    return 0;
}
