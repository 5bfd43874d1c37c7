// Stand-alone check of cvids_amd/csrc/coarse_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_coarse_checks.py: every refusal of chisel_hip_coarse_mesh that needs no device, in the header's order; the stride rule
// for N = 8, 16, 32 and every s from 0 to N + 1; the float arithmetic at and beside 2^31 - 1; the grid and the lattice sizes.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "coarse_checks.h"

using namespace chisel_hip;

struct ChunkRequest {  // = chisel_hip_chunk_request
    const int *ids_xyz;
    int64_t n_ids;
    int use_box;
    int box_lo[3], box_hi[3];
};
struct Request {  // = chisel_hip_coarse_request
    ChunkRequest chunks;
    int stride, stages;
};
static_assert(sizeof(Request) == 56, "chisel_hip_coarse_request is 56 bytes");

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s\n", __LINE__, #cond);                  \
            g_failed++;                                                \
        }                                                              \
    } while (0)

static const int LIMIT = (1 << 20) - 2;
static float g_f[8];
static int64_t g_t[8];
static int g_i[8];

// true when refused with `word` in the text and `want_bad` as the index (word null: accepted)
static bool refused(const Request *r, int N, int64_t cap, const void *v, const void *n, const void *c, const void *table, const void *ids, bool color, const char *word,
                    int64_t want_bad = -1) {
    int64_t bad = -7;
    const char *why = coarse_request_refusal(r, N, cap, v, n, c, table, ids, color, LIMIT, &bad);
    if (!word) return why == nullptr && bad == -1;
    if (!why || !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why ? why : "(none)", word);
        return false;
    }
    return bad == want_bad;
}

int main() {
    // ---- the stride rule
    for (int N : {8, 16, 32})
        for (int s = 0; s <= N + 1; s++) {
            const char *why = coarse_stride_refusal(N, s);
            const bool fine = s >= 1 && s <= N && N % s == 0;
            EXPECT((why == nullptr) == fine);
            if (s < 1) EXPECT(why && strstr(why, "below 1"));
            if (s > N) EXPECT(why && strstr(why, "above"));
            if (s >= 1 && s <= N && N % s) EXPECT(why && strstr(why, "divide"));
            if (fine) {
                const int64_t M = N / s, layers = (M < COARSE_SLAB ? M : COARSE_SLAB) + 1;
                EXPECT(coarse_lattice_samples(N, s) == layers * (M + 1) * (M + 1));
                EXPECT(coarse_lattice_samples(N, s) * 5 <= 64 * 1024);  // a float and a byte per sample: LDS of a workgroup
            }
        }
    EXPECT(coarse_stride_refusal(32, -5) != nullptr && coarse_stride_refusal(32, 1 << 30) != nullptr);
    EXPECT(coarse_lattice_samples(32, 1) == 5 * 33 * 33);

    // ---- vertices x 3 floats against 2^31 - 1
    const int64_t most = 0x7fffffffll / 3;  // 715 827 882 vertices = 2 147 483 646 floats
    EXPECT(coarse_floats_refusal(0) == nullptr && coarse_floats_refusal(most) == nullptr && coarse_floats_refusal(most - 1) == nullptr);
    EXPECT(most * 3 <= COARSE_MAX_FLOATS && (most + 1) * 3 > COARSE_MAX_FLOATS);
    EXPECT(coarse_floats_refusal(most + 1) != nullptr && strstr(coarse_floats_refusal(most + 1), "2^31 - 1"));
    EXPECT(coarse_floats_refusal(0x7fffffffll) != nullptr && coarse_floats_refusal(1ll << 40) != nullptr && coarse_floats_refusal(INT64_MAX) != nullptr);
    EXPECT(coarse_floats_refusal(-1) != nullptr);

    // ---- the grid
    EXPECT(coarse_grid(0) == 1 && coarse_grid(1) == 1 && coarse_grid(COARSE_MAX_GRID) == COARSE_MAX_GRID && coarse_grid(COARSE_MAX_GRID + 1) == COARSE_MAX_GRID);
    EXPECT(coarse_grid(0x7fffffffll) == COARSE_MAX_GRID && coarse_grid(-3) == 1);

    // ---- the capacity
    EXPECT(coarse_capacity_refusal(10, 9) != nullptr && coarse_capacity_refusal(10, 10) == nullptr && coarse_capacity_refusal(0, 1) == nullptr);

    // ---- the request, in the header's order
    const int ids[6] = {0, 0, 0, 1, 2, 3};
    const int far_ids[6] = {0, 0, 0, LIMIT + 1, 0, 0};
    Request all{};
    all.stride = 2;
    EXPECT(refused(nullptr, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "null request"));
    EXPECT(refused(&all, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, nullptr));  // the size query
    EXPECT(refused(&all, 16, 100, g_f, g_f, g_f, g_t, g_i, true, nullptr));
    for (int bad_stride : {0, -1, 3, 17, 32}) {
        Request r = all;
        r.stride = bad_stride;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "stride"));
    }
    {
        Request r = all;
        r.stages = 4;
        EXPECT(refused(&r, 16, 100, g_f, nullptr, nullptr, nullptr, nullptr, true, "stages"));
        r.stages = -1;
        EXPECT(refused(&r, 16, 100, g_f, nullptr, nullptr, nullptr, nullptr, true, "stages"));
        r.stages = 2;
        EXPECT(refused(&r, 16, 100, g_f, nullptr, nullptr, nullptr, nullptr, false, "without colour"));
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, false, "without colour"));  // (the size query too)
        EXPECT(refused(&r, 16, 100, g_f, nullptr, g_f, nullptr, nullptr, true, nullptr));
        r.stages = 1;
        EXPECT(refused(&r, 16, 100, g_f, g_f, nullptr, nullptr, nullptr, false, nullptr));
    }
    {  // whatever chisel_hip_gather_chunks refuses of a selection
        Request r = all;
        r.chunks.n_ids = -1;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "negative number of ids"));
        r = all;
        r.chunks.ids_xyz = ids;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "without a count"));
        r = all;
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "without an id list"));
        r = all;
        r.chunks.ids_xyz = ids;
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, nullptr));
        r.chunks.use_box = 1;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "box together"));
        r = all;
        r.chunks.use_box = 1;
        r.chunks.box_lo[1] = 1;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "lo > hi"));
        r.chunks.box_hi[1] = 1;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, nullptr));
        r = all;
        r.chunks.ids_xyz = far_ids;
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true, "addressable range", 1));
    }
    // the outputs
    EXPECT(refused(&all, 16, -1, g_f, nullptr, nullptr, nullptr, nullptr, true, "negative capacity"));
    EXPECT(refused(&all, 16, 5, nullptr, nullptr, nullptr, nullptr, nullptr, true, "no output"));
    EXPECT(refused(&all, 16, 5, nullptr, nullptr, nullptr, g_t, nullptr, true, nullptr));  // (the table alone)
    EXPECT(refused(&all, 16, 5, nullptr, nullptr, nullptr, nullptr, g_i, true, nullptr));
    EXPECT(refused(&all, 16, 5, nullptr, g_f, nullptr, nullptr, nullptr, true, "without vertices"));
    EXPECT(refused(&all, 16, 5, nullptr, nullptr, g_f, nullptr, nullptr, true, "without vertices"));
    EXPECT(refused(&all, 16, 5, g_f, nullptr, g_f, nullptr, nullptr, false, "without colour"));
    EXPECT(refused(&all, 16, 0, nullptr, g_f, g_f, nullptr, nullptr, false, nullptr));  // (the size query looks at nothing else)
    // the order: the stride in front of the selection, the selection in front of the outputs
    {
        Request r = all;
        r.stride = 5;
        r.chunks.n_ids = -1;
        EXPECT(refused(&r, 16, -1, nullptr, nullptr, nullptr, nullptr, nullptr, true, "stride"));
        r.stride = 4;
        EXPECT(refused(&r, 16, -1, nullptr, nullptr, nullptr, nullptr, nullptr, true, "negative number of ids"));
    }
    if (g_failed) {
        printf("FAILED: %d\n", g_failed);
        return 1;
    }
    printf("ok: coarse_checks\n");
    return 0;
}
