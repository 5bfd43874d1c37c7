// Stand-alone check of cvids_amd/csrc/indexed_checks.h, built with -fsanitize=address,undefined and run on the CPU by
// tests/test_indexed_checks.py: every refusal of chisel_hip_indexed_mesh that needs no device; duplicates; the extras of lists and
// of boxes against a brute-force set; the row, id and index arithmetic at and beside 2^31 - 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <set>
#include <tuple>

#include "indexed_checks.h"

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
static int32_t g_x[8];
static int64_t g_t[8];
static int g_i[8];

struct Outputs {
    const void *v, *x, *n, *c, *table, *owners, *ids;
};

// true when refused with `word` in the text and `want_bad` as the index (word null: accepted)
static bool refused(const Request *r, int N, int64_t cap_v, int64_t cap_t, Outputs o, bool color, const char *word, int64_t want_bad = -1) {
    int64_t bad = -7;
    const char *why = indexed_request_refusal(r, N, cap_v, cap_t, o.v, o.x, o.n, o.c, o.table, o.owners, o.ids, color, LIMIT, &bad);
    if (!word) return why == nullptr && bad == -1;
    if (!why || !strstr(why, word)) {
        printf("refusal \"%s\" lacks \"%s\"\n", why ? why : "(none)", word);
        return false;
    }
    return bad == want_bad;
}

typedef std::tuple<int, int, int> Id;

// the definition, by brute force: every + neighbour of a selected id that is not selected, inside the limit and kept
template <class Keep>
static std::vector<int> brute_extras(const std::vector<int> &ids, Keep keep) {
    std::set<Id> chosen, found;
    for (size_t i = 0; i < ids.size() / 3; i++) chosen.insert(Id(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]));
    for (const Id &c : chosen)
        for (int dx = 0; dx < 2; dx++)
            for (int dy = 0; dy < 2; dy++)
                for (int dz = 0; dz < 2; dz++) {
                    const Id nb(std::get<0>(c) + dx, std::get<1>(c) + dy, std::get<2>(c) + dz);
                    if (!(dx | dy | dz) || chosen.count(nb)) continue;
                    if (std::get<0>(nb) > LIMIT || std::get<1>(nb) > LIMIT || std::get<2>(nb) > LIMIT) continue;
                    if (keep(std::get<0>(nb), std::get<1>(nb), std::get<2>(nb))) found.insert(nb);
                }
    std::vector<int> out;
    for (const Id &c : found) {  // (a set of tuples iterates ascending by x, then y, then z)
        out.push_back(std::get<0>(c));
        out.push_back(std::get<1>(c));
        out.push_back(std::get<2>(c));
    }
    return out;
}

int main() {
    const Outputs none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const Outputs full{g_f, g_x, g_f, g_f, g_t, g_t, g_i};
    const int ids[6] = {0, 0, 0, 1, 2, 3};
    const int far_ids[6] = {0, 0, 0, LIMIT + 1, 0, 0};
    Request all{};
    all.stride = 2;
    all.stages = 3;

    // ---- everything the coarse mesh refuses
    EXPECT(refused(nullptr, 16, 0, 0, none, true, "null request"));
    EXPECT(refused(&all, 16, 0, 0, none, true, nullptr));  // the size query
    EXPECT(refused(&all, 16, 100, 200, full, true, nullptr));
    for (int bad_stride : {0, -1, 3, 17, 32}) {
        Request r = all;
        r.stride = bad_stride;
        EXPECT(refused(&r, 16, 0, 0, none, true, "stride"));
        EXPECT(refused(&r, 16, 100, 200, full, true, "stride"));
    }
    {
        Request r = all;
        r.stages = 4;
        EXPECT(refused(&r, 16, 100, 200, full, true, "stages"));
        r.stages = -1;
        EXPECT(refused(&r, 16, 100, 200, full, true, "stages"));
        r.stages = 2;
        EXPECT(refused(&r, 16, 0, 0, none, false, "without colour"));
        r.stages = 1;
        EXPECT(refused(&r, 16, 100, 200, Outputs{g_f, g_x, g_f, g_f, nullptr, nullptr, nullptr}, false, "without colour"));  // colours of a map without
        EXPECT(refused(&r, 16, 100, 200, Outputs{g_f, g_x, g_f, nullptr, nullptr, nullptr, nullptr}, false, nullptr));
    }
    {  // the selection
        Request r = all;
        r.chunks.n_ids = -1;
        EXPECT(refused(&r, 16, 0, 0, none, true, "negative number of ids"));
        r = all;
        r.chunks.ids_xyz = ids;
        EXPECT(refused(&r, 16, 0, 0, none, true, "without a count"));
        r = all;
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 0, 0, none, true, "without an id list"));
        r = all;
        r.chunks.ids_xyz = ids;
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 0, 0, none, true, nullptr));
        r.chunks.use_box = 1;
        EXPECT(refused(&r, 16, 0, 0, none, true, "box together"));
        r = all;
        r.chunks.use_box = 1;
        r.chunks.box_lo[1] = 1;
        EXPECT(refused(&r, 16, 0, 0, none, true, "lo > hi"));
        r = all;
        r.chunks.ids_xyz = far_ids;
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 0, 0, none, true, "addressable range", 1));
    }
    EXPECT(refused(&all, 16, -1, 0, full, true, "negative capacity"));
    EXPECT(refused(&all, 16, 0, -1, full, true, "negative capacity"));
    EXPECT(refused(&all, 16, -1, -1, none, true, "negative capacity"));
    EXPECT(refused(&all, 16, 5, 5, none, true, "no output"));
    EXPECT(refused(&all, 16, 0, 5, none, true, "no output"));  // (one capacity zero is no size query)
    EXPECT(refused(&all, 16, 5, 5, Outputs{nullptr, nullptr, nullptr, nullptr, g_t, nullptr, nullptr}, true, nullptr));  // (a table alone)
    EXPECT(refused(&all, 16, 5, 5, Outputs{nullptr, nullptr, nullptr, nullptr, nullptr, g_t, nullptr}, true, nullptr));
    EXPECT(refused(&all, 16, 5, 5, Outputs{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, g_i}, true, nullptr));
    EXPECT(refused(&all, 16, 5, 5, Outputs{nullptr, nullptr, g_f, nullptr, nullptr, nullptr, nullptr}, true, "without vertices"));
    EXPECT(refused(&all, 16, 5, 5, Outputs{nullptr, nullptr, nullptr, g_f, nullptr, nullptr, nullptr}, true, "without vertices"));

    // ---- its own: duplicates, normals without their stage, indices without vertices
    {
        const int twice[12] = {4, 5, 6, 1, 2, 3, 4, 5, 6, 1, 2, 3};
        Request r = all;
        r.chunks.ids_xyz = twice;
        r.chunks.n_ids = 4;
        EXPECT(refused(&r, 16, 0, 0, none, true, "repeats", 2));  // (the size query too: an owner is unique)
        EXPECT(refused(&r, 16, 100, 200, full, true, "repeats", 2));
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 100, 200, full, true, nullptr));
        const int neg[6] = {-LIMIT, -LIMIT, -LIMIT, -LIMIT, -LIMIT, -LIMIT};
        r.chunks.ids_xyz = neg;
        EXPECT(refused(&r, 16, 0, 0, none, true, "repeats", 1));
    }
    {
        Request r = all;
        r.stages = 2;
        EXPECT(refused(&r, 16, 100, 200, full, true, "normals without stage bit 0"));
        EXPECT(refused(&r, 16, 0, 0, full, true, nullptr));  // (the size query looks at nothing else)
        r.stages = 0;
        EXPECT(refused(&r, 16, 100, 200, Outputs{g_f, g_x, nullptr, g_f, nullptr, nullptr, nullptr}, true, nullptr));  // (colours without their stage: zeros)
        EXPECT(refused(&all, 16, 100, 200, Outputs{nullptr, g_x, nullptr, nullptr, nullptr, nullptr, nullptr}, true, "indices without vertices"));
        EXPECT(refused(&all, 16, 100, 200, Outputs{g_f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, true, nullptr));
    }
    // the order: the stride in front of the selection, the selection in front of the duplicate, the duplicate in front of the outputs
    {
        const int twice[6] = {1, 1, 1, 1, 1, 1};
        Request r = all;
        r.stride = 5;
        r.chunks.ids_xyz = twice;
        r.chunks.n_ids = 2;
        EXPECT(refused(&r, 16, 5, 5, Outputs{nullptr, g_x, nullptr, nullptr, nullptr, nullptr, nullptr}, true, "stride"));
        r.stride = 4;
        EXPECT(refused(&r, 16, 5, 5, Outputs{g_f, g_x, nullptr, nullptr, nullptr, nullptr, nullptr}, true, "repeats", 1));
    }

    // ---- the capacities
    EXPECT(indexed_capacity_refusal(10, 20, 10, 20) == nullptr && indexed_capacity_refusal(0, 0, 1, 0) == nullptr);
    EXPECT(indexed_capacity_refusal(10, 20, 9, 20) != nullptr && strstr(indexed_capacity_refusal(10, 20, 9, 20), "vertex capacity"));
    EXPECT(indexed_capacity_refusal(10, 20, 10, 19) != nullptr && strstr(indexed_capacity_refusal(10, 20, 10, 19), "triangle capacity"));
    EXPECT(indexed_capacity_refusal(10, 20, 0, 20) != nullptr && indexed_capacity_refusal(10, 20, 10, 0) != nullptr);

    // ---- the arithmetic at 2^31 - 1
    const int64_t most_v = 0x7fffffffll / 3, most_t = 0x7fffffffll / 3;  // (3 floats a vertex bind first: 715 827 882)
    EXPECT(indexed_size_refusal(0, 0) == nullptr && indexed_size_refusal(most_v, most_t) == nullptr);
    EXPECT(indexed_size_refusal(most_v + 1, 0) != nullptr && strstr(indexed_size_refusal(most_v + 1, 0), "2^31 - 1"));
    EXPECT(indexed_size_refusal(0, most_t + 1) != nullptr && strstr(indexed_size_refusal(0, most_t + 1), "index entries"));
    EXPECT(indexed_size_refusal(0x80000000ll, 0) != nullptr && strstr(indexed_size_refusal(0x80000000ll, 0), "vertices"));
    EXPECT(indexed_size_refusal(-1, 0) != nullptr && indexed_size_refusal(0, -1) != nullptr && indexed_size_refusal(INT64_MAX, INT64_MAX) != nullptr);
    EXPECT(most_t * 3 <= INDEXED_MAX_INTS && (most_t + 1) * 3 > INDEXED_MAX_INTS);
    EXPECT(indexed_rows(32, 1) == 3072 && indexed_rows(16, 1) == 768 && indexed_rows(32, 32) == 3 && indexed_rows(8, 2) == 48);
    EXPECT(indexed_row_words(0, 32, 1) == 0 && indexed_row_words(10, 32, 1) == 30720);
    EXPECT(indexed_row_words(0x7fffffffll / 3072, 32, 1) == (0x7fffffffll / 3072) * 3072 && indexed_row_words(0x7fffffffll / 3072 + 1, 32, 1) == -1);
    EXPECT(indexed_row_words(0x7fffffffll / 3, 32, 32) > 0 && indexed_row_words(0x7fffffffll / 3 + 1, 32, 32) == -1);
    EXPECT(indexed_row_words(-1, 8, 1) == -1 && indexed_row_words(INT64_MAX, 8, 1) == -1);

    // ---- the extras against brute force
    {
        auto everything = [](int, int, int) { return true; };
        // a list: scattered ids, neighbours of each other among them, one at the upper limit
        const std::vector<int> list = {0, 0, 0, 1, 1, 1, 1, 0, 0, -5, 7, 2, -4, 8, 3, LIMIT, LIMIT, 3, 0, 1, 0, LIMIT - 1, -LIMIT, -LIMIT};
        const std::vector<int> got = indexed_extras(list.data(), (int64_t)list.size() / 3, LIMIT);
        EXPECT(got == brute_extras(list, everything) && got.size() / 3 > 20);
        std::set<Id> unique;
        for (size_t j = 0; j < got.size() / 3; j++) {
            unique.insert(Id(got[3 * j], got[3 * j + 1], got[3 * j + 2]));
            EXPECT(got[3 * j] <= LIMIT && got[3 * j + 1] <= LIMIT && got[3 * j + 2] <= LIMIT);
            if (j) EXPECT(chunk_order_key(got[3 * j - 3], got[3 * j - 2], got[3 * j - 1]) < chunk_order_key(got[3 * j], got[3 * j + 1], got[3 * j + 2]));
        }
        EXPECT(unique.size() == got.size() / 3);  // each once
        // a residency: every second id of a checkerboard
        auto resident = [](int x, int y, int z) { return ((x + y + z) & 1) == 0; };
        EXPECT(indexed_extras(list.data(), (int64_t)list.size() / 3, LIMIT, resident) == brute_extras(list, resident));
        // a box: every id inside it selected -- the extras are a shell on its + sides
        std::vector<int> box;
        for (int x = -2; x <= 1; x++)
            for (int y = 3; y <= 4; y++)
                for (int z = -1; z <= 1; z++) {
                    box.push_back(x);
                    box.push_back(y);
                    box.push_back(z);
                }
        const std::vector<int> shell = indexed_extras(box.data(), (int64_t)box.size() / 3, LIMIT);
        EXPECT(shell == brute_extras(box, everything));
        EXPECT((int64_t)shell.size() / 3 == 5 * 3 * 4 - 4 * 2 * 3);
        // one id, and none
        const int one[3] = {3, -2, 9};
        EXPECT(indexed_extras(one, 1, LIMIT).size() == 21);
        EXPECT(indexed_extras(one, 0, LIMIT).empty());
        const int corner[3] = {LIMIT, LIMIT, LIMIT};
        EXPECT(indexed_extras(corner, 1, LIMIT).empty());
    }
    if (g_failed) {
        printf("FAILED: %d\n", g_failed);
        return 1;
    }
    printf("ok: indexed_checks\n");
    return 0;
}
