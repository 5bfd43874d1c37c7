// Stand-alone check of cvids_amd/csrc/gather_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_gather_checks.py: every refusal of chisel_hip_gather_meshes that needs no device; the segment table for 0 meshes, for one
// empty mesh, for meshes in three arenas with and without colour (every source offset, destination offset and length against a
// naive restatement of view_mesh's layout); the totals at the 2^31 - 1 limit and one past it; a capacity one short; the prefix and
// the tile count against a naive loop.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gather_checks.h"

using namespace chisel_hip;

struct Request {  // = chisel_hip_mesh_request
    const int *ids_xyz;
    int64_t n_ids;
    int marker_colors;
    float light0[3], light1[3];
    float diffuse, ambient;
};
static_assert(sizeof(Request) == 56, "chisel_hip_mesh_request is 56 bytes");

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s\n", __LINE__, #cond);                  \
            g_failed++;                                                \
        }                                                              \
    } while (0)

static const int LIMIT = (1 << 20) - 2;

static Request request(const int *ids, int64_t n, int marker = 0) { return Request{ids, n, marker, {0.6f, 0.0f, 0.8f}, {-0.5f, 0.2f, 0.2f}, 0.5f, 0.2f}; }
static GatherOutputs outputs(bool v, bool n, bool c, bool rgba, bool g) { return GatherOutputs{{v, n, c, rgba, g}}; }

// true when the request is refused with `word` in the text (word null: accepted)
static bool refused(const Request *r, const GatherOutputs &out, bool color, const char *word, int64_t want_bad = -1, bool check_outputs = true) {
    int64_t bad = -7;
    const char *why = gather_request_refusal(r, check_outputs, out, color, LIMIT, &bad);
    if (!word) return why == nullptr && bad == -1;
    if (!why || !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why ? why : "(none)", word);
        return false;
    }
    return bad == want_bad;
}

static void check_refusals() {
    const GatherOutputs all = outputs(true, true, false, false, true), none = outputs(false, false, false, false, false);
    const int ids[9] = {0, 0, 0, 1, -2, 3, LIMIT, -LIMIT, 0};
    Request ok = request(ids, 3);
    EXPECT(refused(&ok, all, false, nullptr));
    EXPECT(refused((const Request *)nullptr, all, false, "null request"));
    Request r = request(ids, -1);
    EXPECT(refused(&r, all, false, "negative"));
    r = request(ids, 0);
    EXPECT(refused(&r, all, false, "without a count"));
    r = request(nullptr, 2);
    EXPECT(refused(&r, all, false, "without an id list"));
    r = request(nullptr, 0);
    EXPECT(refused(&r, all, false, nullptr));
    for (int a = 0; a < 3; a++)
        for (int sign = -1; sign <= 1; sign += 2) {
            int bad[9];
            memcpy(bad, ids, sizeof(bad));
            bad[3 + a] = sign * (LIMIT + 1);
            r = request(bad, 3);
            EXPECT(refused(&r, all, false, "addressable range", 1));
        }
    EXPECT(refused(&ok, none, false, "no output"));
    EXPECT(refused(&ok, none, false, nullptr, -1, false));  // (the size call has no outputs)
    // lights: looked at only with marker_colors
    const float nan = nanf(""), inf = INFINITY;
    for (int k = 0; k < 8; k++)
        for (float bad : {nan, inf, -inf}) {
            Request m = request(ids, 3, 1);
            float *field = k < 3 ? &m.light0[k] : (k < 6 ? &m.light1[k - 3] : (k == 6 ? &m.diffuse : &m.ambient));
            *field = bad;
            EXPECT(refused(&m, outputs(true, false, false, true, false), false, "not finite"));
            m.marker_colors = 0;
            EXPECT(refused(&m, all, false, nullptr));
        }
    EXPECT(refused(&ok, outputs(true, false, false, true, false), false, "without marker_colors"));
    Request m = request(ids, 3, 1);
    EXPECT(refused(&m, outputs(false, false, false, true, false), false, nullptr));
    EXPECT(refused(&ok, outputs(true, false, true, false, false), false, "without colour"));
    EXPECT(refused(&ok, outputs(true, false, true, false, false), true, nullptr));
}

// view_mesh's layout restated: the arena is vertices | normals | colours (if any) | grids, 3 floats per entry
static int64_t naive_src(const GatherSource &s, int array) {
    const int64_t nv = s.arena_nv;
    switch (array) {
        case GATHER_VERTICES: return 3 * s.v_off;
        case GATHER_NORMALS: return 3 * nv + 3 * s.v_off;
        case GATHER_COLORS: return 6 * nv + 3 * s.v_off;
        case GATHER_RGBA: return (s.arena_color ? 6 * nv : 3 * nv) + 3 * s.v_off;
        default: return 3 * nv * (s.arena_color ? 3 : 2) + 3 * s.g_off;
    }
}

static void check_plan(const std::vector<GatherSource> &src, const GatherOutputs &out) {
    GatherPlan plan;
    int code = -1;
    const char *why = gather_plan(src.data(), (int64_t)src.size(), out, true, false, 0, 0, &plan, &code);
    EXPECT(why == nullptr && code == 0);
    // the table and the totals against a naive loop
    int64_t v = 0, g = 0, nonempty = 0;
    std::vector<int> arenas;
    for (size_t i = 0; i < src.size(); i++) {
        const GatherSource &s = src[i];
        const bool empty = s.arena < 0;
        EXPECT(plan.table[4 * i + 0] == (empty ? 0 : v) && plan.table[4 * i + 1] == (empty ? 0 : s.n_v));
        EXPECT(plan.table[4 * i + 2] == (empty ? 0 : g) && plan.table[4 * i + 3] == (empty ? 0 : s.n_g));
        if (empty) continue;
        v += s.n_v;
        g += s.n_g;
        nonempty++;
        bool seen = false;
        for (int a : arenas) seen = seen || a == s.arena;
        if (!seen) arenas.push_back(s.arena);
    }
    const GatherTotals &T = plan.totals;
    EXPECT(T.meshes == (int64_t)src.size() && T.meshes_nonempty == nonempty && T.vertices == v && T.grids == g && T.arenas_read == (int64_t)arenas.size());
    // the segments: array by array, mesh by mesh, none empty; the prefix and the tiles against a naive loop
    size_t k = 0;
    int64_t start = 0;
    for (int a = 0; a < GATHER_ARRAYS; a++) {
        if (!out.want[a]) continue;
        for (size_t i = 0; i < src.size(); i++) {
            const GatherSource &s = src[i];
            if (s.arena < 0) continue;
            const int64_t len = a == GATHER_GRIDS ? 3 * s.n_g : (a == GATHER_RGBA ? 4 * s.n_v : 3 * s.n_v);
            if (len == 0) continue;
            EXPECT(k < plan.segments.size());
            if (k >= plan.segments.size()) return;
            const GatherSegment &seg = plan.segments[k++];
            EXPECT(seg.array == a && seg.arena == s.arena && seg.len == len && seg.start == start);
            EXPECT(seg.src == naive_src(s, a));
            EXPECT(seg.dst == (a == GATHER_GRIDS ? 3 * plan.table[4 * i + 2] : (a == GATHER_RGBA ? 4 : 3) * plan.table[4 * i + 0]));
            EXPECT(seg.kind == (a != GATHER_RGBA ? GATHER_COPY : (s.arena_color ? GATHER_RGBA_FROM_COLOR : GATHER_RGBA_FROM_NORMAL)));
            start += len;
        }
    }
    EXPECT(k == plan.segments.size() && plan.floats == start);
    int64_t tiles = 0;
    for (int64_t at = 0; at < start; at += GATHER_TILE_FLOATS) tiles++;
    EXPECT(T.tiles == tiles);
}

static void check_plans() {
    const GatherOutputs every = outputs(true, true, false, true, true), every_c = outputs(true, true, true, true, true);
    check_plan({}, every);                                        // 0 meshes
    check_plan({GatherSource{-1, 0, 0, 0, 0, 0, false}}, every);  // one empty mesh
    for (int color = 0; color < 2; color++) {
        const bool c = color != 0;
        // three arenas (of 90, 3000 and 9 vertices), an empty mesh between them, a mesh with grids only, a duplicate
        std::vector<GatherSource> src = {
            GatherSource{0, 0, 27, 0, 5, 90, c},      GatherSource{2, 0, 9, 0, 1, 9, c},       GatherSource{-1, 0, 0, 0, 0, 0, false},
            GatherSource{1, 9, 2700, 3, 411, 3000, c}, GatherSource{0, 27, 63, 5, 20, 90, c},   GatherSource{1, 2709, 0, 414, 2, 3000, c},
            GatherSource{1, 9, 2700, 3, 411, 3000, c},
        };
        check_plan(src, c ? every_c : every);
        check_plan(src, outputs(false, false, false, false, true));
        check_plan(src, outputs(false, true, c, false, false));
        check_plan(src, outputs(false, false, false, true, false));
        // a capacity one short, in vertices and in grids: INVALID with the totals filled
        GatherPlan plan;
        int code = -1;
        const int64_t V = 27 + 9 + 2700 + 63 + 0 + 2700, G = 5 + 1 + 411 + 20 + 2 + 411;
        EXPECT(gather_plan(src.data(), (int64_t)src.size(), every, true, true, V, G, &plan, &code) == nullptr && code == 0);
        EXPECT(plan.totals.vertices == V && plan.totals.grids == G && plan.totals.arenas_read == 3 && plan.totals.meshes_nonempty == 6);
        const char *why = gather_plan(src.data(), (int64_t)src.size(), every, true, true, V - 1, G, &plan, &code);
        EXPECT(why && strstr(why, "capacity") && code == GATHER_REFUSED_INVALID && plan.totals.vertices == V && plan.totals.grids == G);
        why = gather_plan(src.data(), (int64_t)src.size(), every, true, true, V, G - 1, &plan, &code);
        EXPECT(why && strstr(why, "capacity") && code == GATHER_REFUSED_INVALID && plan.totals.vertices == V && plan.totals.grids == G);
        // a capacity speaks of the arrays asked for only
        EXPECT(gather_plan(src.data(), (int64_t)src.size(), outputs(true, true, false, false, false), true, true, V, 0, &plan, &code) == nullptr);
        EXPECT(gather_plan(src.data(), (int64_t)src.size(), outputs(false, false, false, false, true), true, true, 0, G, &plan, &code) == nullptr);
        EXPECT(gather_plan(src.data(), (int64_t)src.size(), outputs(false, false, false, true, false), true, true, V - 1, G, &plan, &code) != nullptr);
    }
}

// 2^31 - 1 floats in one array: 3 * 715827882 = 2^31 - 2 is the most an array of 3 per entry can hold, one entry more is refused;
// rgba holds 4 per vertex and reaches the limit first
static void check_limits() {
    const int64_t most3 = 715827882, most4 = 536870911;
    GatherPlan plan;
    int code = -1;
    // (several meshes of one huge arena: no segment is built, build = false, so nothing of that size is allocated)
    std::vector<GatherSource> src = {GatherSource{0, 0, most3 - 3, 0, most3 - 1, most3, false}, GatherSource{0, most3 - 3, 3, most3 - 1, 1, most3, false}};
    const GatherOutputs vg = outputs(true, true, false, false, true), with_rgba = outputs(true, false, false, true, false);
    EXPECT(gather_plan(src.data(), 2, vg, false, false, 0, 0, &plan, &code) == nullptr && code == 0);
    EXPECT(plan.totals.vertices == most3 && plan.totals.grids == most3);
    EXPECT(plan.totals.tiles == (3 * (3 * most3) + GATHER_TILE_FLOATS - 1) / GATHER_TILE_FLOATS);
    const char *why = gather_plan(src.data(), 2, with_rgba, false, false, 0, 0, &plan, &code);
    EXPECT(why && strstr(why, "2^31 - 1") && code == GATHER_REFUSED_UNSUPPORTED);
    src[1].n_v += 1;  // one vertex past the limit
    why = gather_plan(src.data(), 2, vg, false, false, 0, 0, &plan, &code);
    EXPECT(why && strstr(why, "2^31 - 1") && code == GATHER_REFUSED_UNSUPPORTED);
    src[1].n_v -= 1;
    src[1].n_g += 1;  // one grid entry past it
    why = gather_plan(src.data(), 2, vg, false, false, 0, 0, &plan, &code);
    EXPECT(why && strstr(why, "2^31 - 1") && code == GATHER_REFUSED_UNSUPPORTED);
    EXPECT(gather_plan(src.data(), 2, outputs(true, true, false, false, false), false, false, 0, 0, &plan, &code) == nullptr);  // (grids not asked for)
    // rgba at its own limit and one past
    std::vector<GatherSource> r = {GatherSource{0, 0, most4, 0, 0, most4 + 1, false}};
    EXPECT(gather_plan(r.data(), 1, with_rgba, false, false, 0, 0, &plan, &code) == nullptr && plan.totals.vertices == most4);
    r[0].n_v = most4 + 1;
    why = gather_plan(r.data(), 1, with_rgba, false, false, 0, 0, &plan, &code);
    EXPECT(why && code == GATHER_REFUSED_UNSUPPORTED);
    // one segment of the full length: its int32 length holds 2^31 - 2
    std::vector<GatherSource> one = {GatherSource{0, 0, most3, 0, 0, most3, false}};
    EXPECT(gather_plan(one.data(), 1, outputs(true, false, false, false, false), true, true, most3, 0, &plan, &code) == nullptr);
    EXPECT(plan.segments.size() == 1 && plan.segments[0].len == 2147483646 && plan.floats == 2147483646ll);
}

int main() {
    check_refusals();
    check_plans();
    check_limits();
    if (g_failed) {
        printf("FAILED: %d checks\n", g_failed);
        return 1;
    }
    printf("ok: gather_checks.h\n");
    return 0;
}
