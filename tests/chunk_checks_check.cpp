// Stand-alone check of cvids_amd/csrc/chunk_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_chunk_checks.py: every refusal of chisel_hip_gather_chunks and chisel_hip_scatter_chunks that needs no device, in the
// header's order; duplicate detection (first and last pair, n = 2, none among 10^5 ids); the box filter at its edges; the ascending
// order against a plain sort of the triples; the 64-bit byte and grid arithmetic at its limits.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "chunk_checks.h"

using namespace chisel_hip;

struct Request {  // = chisel_hip_chunk_request
    const int *ids_xyz;
    int64_t n_ids;
    int use_box;
    int box_lo[3], box_hi[3];
};
static_assert(sizeof(Request) == 48, "chisel_hip_chunk_request is 48 bytes");

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s\n", __LINE__, #cond);                  \
            g_failed++;                                                \
        }                                                              \
    } while (0)

static const int LIMIT = (1 << 20) - 2;
alignas(16) static float g_f[8];
alignas(16) static unsigned char g_b[32];

// true when refused with `word` in the text and `want_bad` as the index (word null: accepted)
static bool said(const char *why, int64_t bad, const char *word, int64_t want_bad) {
    if (!word) return why == nullptr && bad == -1;
    if (!why || !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why ? why : "(none)", word);
        return false;
    }
    return bad == want_bad;
}
static bool gather_refused(const Request *r, int64_t cap, const void *s, const void *w, const void *c, const void *ids, bool dev, bool color, const char *word,
                           int64_t want_bad = -1) {
    int64_t bad = -7;
    const char *why = chunk_gather_refusal(r, cap, s, w, c, ids, dev, color, LIMIT, &bad);
    return said(why, bad, word, want_bad);
}

static void check_gather_refusals() {
    const int ids[9] = {0, 0, 0, 1, -2, 3, LIMIT, -LIMIT, 0};
    int out_ids[9];
    Request all{nullptr, 0, 0, {0, 0, 0}, {0, 0, 0}};
    EXPECT(gather_refused(&all, 4, g_f, g_f, nullptr, nullptr, false, false, nullptr));
    EXPECT(gather_refused((const Request *)nullptr, 4, g_f, g_f, nullptr, nullptr, false, false, "null request"));
    Request r{ids, -1, 0, {0, 0, 0}, {0, 0, 0}};
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, "negative number of ids"));
    r.n_ids = 0;
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, "without a count"));
    r = Request{nullptr, 2, 0, {0, 0, 0}, {0, 0, 0}};
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, "without an id list"));
    r = Request{ids, 3, 1, {0, 0, 0}, {1, 1, 1}};
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, "box together"));
    r = Request{nullptr, 0, 1, {0, 2, 0}, {1, 1, 1}};
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, "lo > hi"));
    r = Request{nullptr, 0, 0, {0, 2, 0}, {1, 1, 1}};  // (a box that is not used is not looked at)
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, nullptr));
    r = Request{nullptr, 0, 1, {3, 3, 3}, {3, 3, 3}};  // lo == hi is a box
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, nullptr));
    // ids at the limit pass, one beyond is named by its index
    r = Request{ids, 3, 0, {0, 0, 0}, {0, 0, 0}};
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, nullptr));
    int far_ids[9] = {0, 0, 0, 1, 1, 1, 0, LIMIT + 1, 0};
    r.ids_xyz = far_ids;
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, "outside the addressable range", 2));
    far_ids[7] = 0;
    far_ids[3] = -LIMIT - 1;
    EXPECT(gather_refused(&r, 4, g_f, nullptr, nullptr, nullptr, false, false, "outside the addressable range", 1));
    // ... also in the size query, which looks at nothing after it
    EXPECT(gather_refused(&r, 0, nullptr, nullptr, nullptr, nullptr, false, false, "outside the addressable range", 1));
    EXPECT(gather_refused(&all, 0, nullptr, nullptr, nullptr, nullptr, false, false, nullptr));
    EXPECT(gather_refused(&all, 0, nullptr, nullptr, g_b, nullptr, false, false, nullptr));
    EXPECT(gather_refused(&all, -1, g_f, nullptr, nullptr, nullptr, false, false, "negative capacity"));
    // outputs
    EXPECT(gather_refused(&all, 4, nullptr, nullptr, nullptr, nullptr, false, true, "no output"));
    EXPECT(gather_refused(&all, 4, nullptr, nullptr, nullptr, out_ids, false, true, nullptr));  // the ids alone are an output
    EXPECT(gather_refused(&all, 4, nullptr, nullptr, g_b, nullptr, false, false, "without colour"));
    EXPECT(gather_refused(&all, 4, nullptr, nullptr, g_b, nullptr, false, true, nullptr));
    // alignment speaks of device pointers only, of each of the three
    EXPECT(gather_refused(&all, 4, g_f + 1, g_f, nullptr, nullptr, false, true, nullptr));
    EXPECT(gather_refused(&all, 4, g_f + 1, g_f, nullptr, nullptr, true, true, "16-byte aligned"));
    EXPECT(gather_refused(&all, 4, g_f, g_f + 2, nullptr, nullptr, true, true, "16-byte aligned"));
    EXPECT(gather_refused(&all, 4, g_f, g_f, g_b + 8, nullptr, true, true, "16-byte aligned"));
    EXPECT(gather_refused(&all, 4, g_f, g_f + 4, g_b + 16, nullptr, true, true, nullptr));
    // the capacity
    EXPECT(chunk_capacity_refusal(5, 5) == nullptr && chunk_capacity_refusal(0, 1) == nullptr);
    EXPECT(chunk_capacity_refusal(5, 4) != nullptr && strstr(chunk_capacity_refusal(5, 4), "capacity"));
}

static int owner_mod2(int x, int, int) { return ((x % 2) + 2) % 2; }
static int owner_zero(int, int, int) { return 0; }
static bool ids_refused(const int *ids, int64_t n, int (*owner)(int, int, int), const char *word, int64_t want_bad = -1) {
    int64_t bad = -7;
    const char *why = chunk_scatter_ids_refusal(ids, n, LIMIT, owner, 0, &bad);
    return said(why, bad, word, want_bad);
}

static void check_scatter_refusals() {
    const int ids[9] = {0, 0, 0, 1, -2, 3, LIMIT, -LIMIT, 0};
    EXPECT(chunk_scatter_refusal(ids, 3, g_f, g_f, nullptr, false, false) == nullptr);
    EXPECT(chunk_scatter_refusal(nullptr, 0, nullptr, nullptr, nullptr, false, false) == nullptr);  // n == 0: a no-op, nothing looked at
    EXPECT(strstr(chunk_scatter_refusal(ids, -1, g_f, g_f, nullptr, false, false), "negative"));
    EXPECT(strstr(chunk_scatter_refusal(nullptr, 3, g_f, g_f, nullptr, false, false), "null"));
    EXPECT(strstr(chunk_scatter_refusal(ids, 3, nullptr, g_f, nullptr, false, false), "null"));
    EXPECT(strstr(chunk_scatter_refusal(ids, 3, g_f, nullptr, nullptr, false, false), "null"));
    EXPECT(strstr(chunk_scatter_refusal(ids, 3, g_f, g_f, g_b, false, false), "without colour"));
    EXPECT(chunk_scatter_refusal(ids, 3, g_f, g_f, g_b, false, true) == nullptr);
    EXPECT(chunk_scatter_refusal(ids, 3, g_f + 1, g_f, nullptr, false, true) == nullptr);
    EXPECT(strstr(chunk_scatter_refusal(ids, 3, g_f + 1, g_f, nullptr, true, true), "16-byte aligned"));
    EXPECT(strstr(chunk_scatter_refusal(ids, 3, g_f, g_f, g_b + 4, true, true), "16-byte aligned"));
    // the ids: range before duplicates before ownership
    EXPECT(ids_refused(ids, 3, owner_zero, nullptr));
    int both[12] = {5, 5, 5, 5, 5, 5, 0, 0, LIMIT + 1, 1, 0, 0};
    EXPECT(ids_refused(both, 4, owner_mod2, "outside the addressable range", 2));
    both[8] = 0;
    EXPECT(ids_refused(both, 4, owner_mod2, "repeats", 1));
    both[3] = 4;  // 5 5 5 | 4 5 5 | 0 0 0 | 1 0 0 with rank 0 of 2 by x: index 0 is another shard's
    EXPECT(ids_refused(both, 4, owner_mod2, "another shard", 0));
    EXPECT(ids_refused(both + 3, 1, owner_mod2, nullptr, -1));
    EXPECT(ids_refused(both + 3, 3, owner_mod2, "another shard", 2));
}

static void check_duplicates() {
    const int two_same[6] = {7, -3, 2, 7, -3, 2}, two_other[6] = {7, -3, 2, 7, -3, 3};
    EXPECT(chunk_first_duplicate(two_same, 2) == 1);
    EXPECT(chunk_first_duplicate(two_other, 2) == -1);
    EXPECT(chunk_first_duplicate(two_same, 1) == -1 && chunk_first_duplicate(nullptr, 0) == -1);
    // 10^5 distinct ids across the range, negative coordinates and the limits included
    const int64_t n = 100000;
    std::vector<int> ids((size_t)n * 3);
    for (int64_t i = 0; i < n; i++) {
        ids[3 * i] = (int)(i % 317) - 158;
        ids[3 * i + 1] = (int)((i / 317) % 317) - 158;
        ids[3 * i + 2] = (i & 1) ? LIMIT - (int)(i / (317 * 317)) : -LIMIT + (int)(i / (317 * 317));
    }
    EXPECT(chunk_first_duplicate(ids.data(), n) == -1);
    // the first pair: ids 0 and 1; the last pair: n - 2 and n - 1; a pair far apart; of several, the smallest second index
    std::vector<int> d = ids;
    for (int a = 0; a < 3; a++) d[3 + a] = d[a];
    EXPECT(chunk_first_duplicate(d.data(), n) == 1);
    d = ids;
    for (int a = 0; a < 3; a++) d[3 * (n - 1) + a] = d[3 * (n - 2) + a];
    EXPECT(chunk_first_duplicate(d.data(), n) == n - 1);
    for (int a = 0; a < 3; a++) d[3 * 5000 + a] = d[3 * 12 + a];
    EXPECT(chunk_first_duplicate(d.data(), n) == 5000);
    for (int a = 0; a < 3; a++) d[3 * 70000 + a] = d[3 * 12 + a];  // a third copy changes nothing
    EXPECT(chunk_first_duplicate(d.data(), n) == 5000);
    // ids that differ in one coordinate only, or are permutations of each other, are distinct
    const int near[12] = {1, 2, 3, 3, 2, 1, 1, 2, 4, -1, 2, 3};
    EXPECT(chunk_first_duplicate(near, 4) == -1);
}

static void check_selection() {
    // a listing in scrambled order over negative and positive ids
    std::vector<std::array<int, 3>> t;
    for (int x = -3; x <= 3; x++)
        for (int y = -2; y <= 2; y++)
            for (int z = -2; z <= 1; z++) t.push_back({x * 37 % 11 - 5 + x, y, z * 3});
    t.push_back({LIMIT, -LIMIT, 0});
    t.push_back({-LIMIT, LIMIT, LIMIT});
    for (size_t i = 0; i < t.size(); i++) std::swap(t[i], t[(i * 7919 + 13) % t.size()]);
    std::vector<int> ids;
    for (auto &p : t) ids.insert(ids.end(), p.begin(), p.end());
    const int64_t n = (int64_t)t.size();
    const int none[3] = {0, 0, 0};
    // all: a plain sort of the triples
    std::vector<int64_t> order = chunk_select_sorted(ids.data(), n, false, none, none);
    std::vector<std::array<int, 3>> sorted = t;
    std::sort(sorted.begin(), sorted.end());
    EXPECT((int64_t)order.size() == n);
    bool same = order.size() == sorted.size();
    for (size_t j = 0; same && j < order.size(); j++) same = t[(size_t)order[j]] == sorted[j];
    EXPECT(same);
    // boxes: every edge inclusive, against a naive filter of the sorted triples
    const int boxes[5][6] = {{-2, -1, -3, 2, 1, 3}, {-100, -100, -100, 100, 100, 100}, {0, 0, 0, 0, 0, 0}, {50, 50, 50, 60, 60, 60}, {-LIMIT, -LIMIT, -LIMIT, LIMIT, LIMIT, LIMIT}};
    for (const auto &b : boxes) {
        std::vector<std::array<int, 3>> want;
        for (auto &p : sorted)
            if (p[0] >= b[0] && p[0] <= b[3] && p[1] >= b[1] && p[1] <= b[4] && p[2] >= b[2] && p[2] <= b[5]) want.push_back(p);
        order = chunk_select_sorted(ids.data(), n, true, b, b + 3);
        bool ok = order.size() == want.size();
        for (size_t j = 0; ok && j < order.size(); j++) ok = t[(size_t)order[j]] == want[j];
        EXPECT(ok);
    }
    EXPECT(chunk_select_sorted(ids.data(), n, true, boxes[3], boxes[3] + 3).empty());  // a box holding nothing
    EXPECT((int64_t)chunk_select_sorted(ids.data(), n, true, boxes[4], boxes[4] + 3).size() == n);
    // lo == hi picks exactly the one chunk
    const int one[3] = {sorted[5][0], sorted[5][1], sorted[5][2]};
    order = chunk_select_sorted(ids.data(), n, true, one, one);
    EXPECT(order.size() == 1 && t[(size_t)order[0]] == sorted[5]);
    EXPECT(chunk_select_sorted(nullptr, 0, false, none, none).empty());
}

static void check_sizes() {
    ChunkSizes Z;
    // the three chunk sizes of the library
    EXPECT(chunk_sizes(1, 512, &Z) == nullptr && Z.bytes_per_array == 2048 && Z.quads_per_chunk == 128 && Z.quad_shift == 7 && Z.quads == 128 && Z.tiles == 1);
    EXPECT(chunk_sizes(8, 512, &Z) == nullptr && Z.tiles == 1);
    EXPECT(chunk_sizes(9, 512, &Z) == nullptr && Z.tiles == 2 && Z.bytes_per_array == 9 * 2048);
    EXPECT(chunk_sizes(3, 4096, &Z) == nullptr && Z.quad_shift == 10 && Z.tiles == 3 && Z.bytes_per_array == 3 * 16384);
    EXPECT(chunk_sizes(3, 32768, &Z) == nullptr && Z.quad_shift == 13 && Z.tiles == 24 && Z.bytes_per_array == 3 * 131072);
    EXPECT(chunk_sizes(0, 4096, &Z) == nullptr && Z.tiles == 0 && Z.bytes_per_array == 0);
    EXPECT(CHUNK_TILE_QUADS == 1024 && CHUNK_TILE_QUADS * 16 == 16384);
    // chunk sizes the copy's split cannot take
    EXPECT(chunk_sizes(1, 256, &Z) != nullptr && chunk_sizes(1, 1000, &Z) != nullptr && chunk_sizes(1, 0, &Z) != nullptr && chunk_sizes(1, -512, &Z) != nullptr);
    // the chunk count at its limit: 2^31 - 1 chunks of 8^3 are 2^28 tiles; one more chunk is refused
    EXPECT(chunk_sizes(CHUNK_MAX_CHUNKS, 512, &Z) == nullptr && Z.tiles == (1ll << 28) && Z.bytes_per_array == CHUNK_MAX_CHUNKS * 2048);
    EXPECT(chunk_sizes(CHUNK_MAX_CHUNKS + 1, 512, &Z) != nullptr && chunk_sizes(-1, 512, &Z) != nullptr);
    // the grid at its limit: 16^3 chunks are a tile each, 32^3 chunks eight: (2^31 - 1) / 8 of them fit, one more does not
    EXPECT(chunk_sizes(CHUNK_MAX_TILES, 4096, &Z) == nullptr && Z.tiles == CHUNK_MAX_TILES && Z.bytes_per_array == CHUNK_MAX_TILES * 16384);
    EXPECT(chunk_sizes(CHUNK_MAX_TILES / 8, 32768, &Z) == nullptr && Z.tiles == CHUNK_MAX_TILES / 8 * 8 && Z.bytes_per_array == (CHUNK_MAX_TILES / 8) * 131072);
    const char *why = chunk_sizes(CHUNK_MAX_TILES / 8 + 1, 32768, &Z);
    EXPECT(why != nullptr && strstr(why, "workgroups"));
    // bytes beyond 32 bits are kept whole
    EXPECT(chunk_sizes(40000, 32768, &Z) == nullptr && Z.bytes_per_array == 40000ll * 131072 && Z.bytes_per_array > (1ll << 32));
    // blocks of a save or a load
    EXPECT(chunk_block_chunks(4096, true, 64ll << 20) == (64ll << 20) / (3 * 16384));
    EXPECT(chunk_block_chunks(4096, false, 64ll << 20) == (64ll << 20) / (2 * 16384));
    EXPECT(chunk_block_chunks(32768, true, 64ll << 20) == 170);
    EXPECT(chunk_block_chunks(32768, true, 1000) == 1);
}

int main() {
    check_gather_refusals();
    check_scatter_refusals();
    check_duplicates();
    check_selection();
    check_sizes();
    if (g_failed) {
        printf("FAILED: %d checks\n", g_failed);
        return 1;
    }
    printf("ok: chunk_checks.h\n");
    return 0;
}
