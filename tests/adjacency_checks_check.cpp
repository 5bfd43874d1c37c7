// Stand-alone check of cvids_amd/csrc/adjacency_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_adjacency_checks.py: every refusal of chisel_hip_mesh_adjacency, chisel_hip_mesh_vertex_normals and chisel_hip_smooth_mesh
// that needs no device, the valence limit and the capacities against the totals, the order of the smoothing passes, and the size and
// scratch arithmetic at and beside 2^31 - 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "adjacency_checks.h"

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
static int32_t g_x[8], g_to[8], g_ti[8], g_no[8], g_ni[8], g_fl[8];
static float g_v[32], g_ov[32], g_on[32];
static char g_totals[96];

// true when `why` is a refusal with `word` in its text and the status `unsupported` (word null: accepted)
static bool is(const char *why, bool got_unsupported, const char *word, bool unsupported = false) {
    if (!word) return why == nullptr;
    if (!why || !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why ? why : "(none)", word);
        return false;
    }
    return got_unsupported == unsupported;
}

struct A {  // the arguments of chisel_hip_mesh_adjacency, a good call
    int64_t V = 5, T = 2, cap_i = 6, cap_n = 12;
    const void *x = g_x, *to = g_to, *ti = g_ti, *no = g_no, *ni = g_ni, *fl = g_fl, *totals = g_totals;
};
static bool adjacency(const A &a, const char *word, bool unsupported = false) {
    bool u = true;
    const char *why = adjacency_request_refusal(a.V, a.T, a.x, a.to, a.cap_i, a.ti, a.no, a.cap_n, a.ni, a.fl, a.totals, &u);
    return is(why, u, word, unsupported);
}

struct N {  // chisel_hip_mesh_vertex_normals
    int64_t V = 5, T = 2;
    const void *x = g_x, *v = g_v, *n = g_on, *totals = g_totals;
};
static bool normals(const N &a, const char *word, bool unsupported = false) {
    bool u = true;
    const char *why = normals_request_refusal(a.V, a.T, a.x, a.v, a.n, a.totals, &u);
    return is(why, u, word, unsupported);
}

struct S {  // chisel_hip_smooth_mesh
    int64_t V = 5, T = 2, iterations = 10;
    float lambda = 0.5f, mu = -0.53f;
    int pin = 3;
    const void *x = g_x, *v = g_v, *ov = g_ov, *on = g_on, *totals = g_totals;
};
static bool smooth(const S &a, const char *word, bool unsupported = false) {
    bool u = true;
    const char *why = smooth_request_refusal(a.V, a.T, a.x, a.v, a.iterations, a.lambda, a.mu, a.pin, a.ov, a.on, a.totals, &u);
    return is(why, u, word, unsupported);
}

template <class X, class Fn>
static X with(Fn &&fn) {
    X a;
    fn(a);
    return a;
}

int main() {
    // ---- sizes and indices, for all three
    EXPECT(adjacency(A(), nullptr) && normals(N(), nullptr) && smooth(S(), nullptr));
    EXPECT(adjacency(with<A>([](A &a) { a.V = -1; }), "negative size") && adjacency(with<A>([](A &a) { a.T = -1; }), "negative size"));
    EXPECT(adjacency(with<A>([](A &a) { a.V = MAX; a.T = 0; a.x = nullptr; }), nullptr));
    EXPECT(adjacency(with<A>([](A &a) { a.V = MAX + 1; }), "vertices", true));
    EXPECT(adjacency(with<A>([](A &a) { a.T = MAX / 6; }), nullptr));
    EXPECT(adjacency(with<A>([](A &a) { a.T = MAX / 6 + 1; }), "neighbour slots", true));
    EXPECT(adjacency(with<A>([](A &a) { a.T = MAX / 3 + 1; }), "index entries", true));
    EXPECT(adjacency(with<A>([](A &a) { a.T = INT64_MAX; }), "index entries", true) && adjacency(with<A>([](A &a) { a.V = INT64_MAX; }), "vertices", true));
    EXPECT(adjacency(with<A>([](A &a) { a.x = nullptr; }), "null indices") && adjacency(with<A>([](A &a) { a.x = nullptr; a.T = 0; }), nullptr));
    EXPECT(normals(with<N>([](N &a) { a.V = -1; }), "negative size") && normals(with<N>([](N &a) { a.T = MAX / 6 + 1; }), "neighbour slots", true));
    EXPECT(normals(with<N>([](N &a) { a.x = nullptr; }), "null indices"));
    EXPECT(smooth(with<S>([](S &a) { a.T = -1; }), "negative size") && smooth(with<S>([](S &a) { a.V = MAX + 1; }), "vertices", true));
    EXPECT(smooth(with<S>([](S &a) { a.x = nullptr; }), "null indices"));
    // ---- the adjacency's own
    EXPECT(adjacency(with<A>([](A &a) { a.cap_i = -1; }), "negative capacity") && adjacency(with<A>([](A &a) { a.cap_n = -1; }), "negative capacity"));
    EXPECT(adjacency(with<A>([](A &a) { a.to = a.ti = a.no = a.ni = a.fl = nullptr; }), nullptr));  // the size query
    EXPECT(adjacency(with<A>([](A &a) { a.to = a.ti = a.no = a.ni = a.fl = a.totals = nullptr; }), "size query without totals"));
    EXPECT(adjacency(with<A>([](A &a) { a.totals = nullptr; }), nullptr));
    EXPECT(adjacency_is_query(nullptr, nullptr, nullptr, nullptr, nullptr) && !adjacency_is_query(nullptr, nullptr, nullptr, nullptr, g_fl));
    // ---- the normals' own
    EXPECT(normals(with<N>([](N &a) { a.v = nullptr; }), "null vertices") && normals(with<N>([](N &a) { a.v = nullptr; a.V = 0; a.T = 0; }), nullptr));
    EXPECT(normals(with<N>([](N &a) { a.n = nullptr; a.v = nullptr; }), nullptr) && normals(with<N>([](N &a) { a.n = nullptr; a.totals = nullptr; }), "size query without totals"));
    // ---- the smoothing's own
    EXPECT(smooth(with<S>([](S &a) { a.iterations = -1; }), "negative iterations") && smooth(with<S>([](S &a) { a.iterations = 0; }), nullptr));
    EXPECT(smooth(with<S>([](S &a) { a.lambda = NAN; }), "finite") && smooth(with<S>([](S &a) { a.mu = INFINITY; }), "finite"));
    EXPECT(smooth(with<S>([](S &a) { a.lambda = -INFINITY; }), "finite") && smooth(with<S>([](S &a) { a.lambda = 3.0e38f; a.mu = 0.0f; }), nullptr));
    EXPECT(smooth(with<S>([](S &a) { a.pin = -1; }), "pin_flags") && smooth(with<S>([](S &a) { a.pin = 8; }), "pin_flags"));
    EXPECT(smooth(with<S>([](S &a) { a.pin = 0; }), nullptr) && smooth(with<S>([](S &a) { a.pin = 7; }), nullptr));
    EXPECT(smooth(with<S>([](S &a) { a.ov = nullptr; }), "normals out without vertices out"));
    EXPECT(smooth(with<S>([](S &a) { a.ov = a.on = nullptr; a.v = nullptr; }), nullptr));  // the size query
    EXPECT(smooth(with<S>([](S &a) { a.ov = a.on = a.totals = nullptr; }), "size query without totals"));
    EXPECT(smooth(with<S>([](S &a) { a.v = nullptr; }), "null vertices") && smooth(with<S>([](S &a) { a.on = nullptr; }), nullptr));
    EXPECT(smooth(with<S>([](S &a) { a.ov = g_v; }), "overlaps") && smooth(with<S>([](S &a) { a.ov = g_v + 14; }), "overlaps"));
    EXPECT(smooth(with<S>([](S &a) { a.ov = g_v + 15; }), nullptr) && smooth(with<S>([](S &a) { a.v = g_v + 15; a.ov = g_v; }), nullptr));
    EXPECT(smooth(with<S>([](S &a) { a.v = g_v + 14; a.ov = g_v; }), "overlaps"));
    EXPECT(!adjacency_overlap(g_v, g_v, 0) && adjacency_overlap(g_v, g_v, 1) && !adjacency_overlap(nullptr, (const void *)8, 8) && adjacency_overlap(nullptr, (const void *)7, 8));
    EXPECT(adjacency_finite(0.0f) && adjacency_finite(-3.4e38f) && adjacency_finite(1e-45f) && !adjacency_finite(NAN) && !adjacency_finite(INFINITY));
    // ---- behind the wait: the valence limit, then the capacities
    EXPECT(!adjacency_valence_refusal(0) && !adjacency_valence_refusal(MESH_MAX_INCIDENT) && adjacency_valence_refusal(MESH_MAX_INCIDENT + 1));
    EXPECT(adjacency_valence_refusal(MAX) && strstr(adjacency_valence_refusal(33), "32"));
    EXPECT(!adjacency_capacity_refusal(6, 12, 6, g_ti, 12, g_ni));
    EXPECT(strstr(adjacency_capacity_refusal(6, 12, 5, g_ti, 12, g_ni), "incidence capacity") && strstr(adjacency_capacity_refusal(6, 12, 6, g_ti, 11, g_ni), "neighbour capacity"));
    EXPECT(!adjacency_capacity_refusal(6, 12, 0, nullptr, 0, nullptr) && !adjacency_capacity_refusal(6, 12, 0, nullptr, 12, g_ni));
    EXPECT(strstr(adjacency_capacity_refusal(MAX, 2 * MAX, MAX - 1, g_ti, 2 * MAX, g_ni), "incidence") && !adjacency_capacity_refusal(0, 0, 0, g_ti, 0, g_ni));
    // ---- the passes: the last one writes the caller's array, none reads what it writes
    EXPECT(smooth_passes(0, -0.53f) == 0 && smooth_passes(10, -0.53f) == 20 && smooth_passes(10, 0.0f) == 10 && smooth_passes(10, -0.0f) == 10);
    EXPECT(smooth_passes(MAX, 1.0f) == 2 * MAX);
    for (int64_t n = 1; n <= 9; n++) {
        EXPECT(smooth_pass_writes_out(n - 1, n));
        for (int64_t j = 1; j < n; j++) EXPECT(smooth_pass_writes_out(j, n) != smooth_pass_writes_out(j - 1, n));
    }
    // ---- the scratch, in ints, below the size limits: no 32-bit intermediate
    EXPECT(adjacency_scan_tiles(0) == 1 && adjacency_scan_tiles(COMPONENTS_TILE - 1) == 1 && adjacency_scan_tiles(COMPONENTS_TILE) == 2);
    EXPECT(adjacency_scratch_ints(0, 0) == 4 && adjacency_scratch_ints(1, 1) == 4 + 4 + 9 + 2);
    EXPECT(adjacency_scratch_ints(MAX, MAX / 6) == 6 * MAX + 2 + 9 * (MAX / 6) + 2 * ((MAX + 1 + COMPONENTS_TILE - 1) / COMPONENTS_TILE));
    EXPECT(6 * (MAX / 6) <= MAX && MESH_MAX_NEIGHBORS == 2 * MESH_MAX_INCIDENT && MESH_FLAGS_ALL == (MESH_FLAG_BOUNDARY | MESH_FLAG_NONMANIFOLD | MESH_FLAG_ISOLATED));
    EXPECT(AC_PINNED < ADJACENCY_HOST_WORDS);
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok: the refusals, the capacities and the arithmetic of adjacency_checks.h\n");
    return 0;
}
