// Stand-alone check of the batch argument check of cvids_amd/csrc/host_checks.h (deintegrate_batch_refusal: what
// chisel_hip_deintegrate_batch refuses before it touches anything), built with -fsanitize=address,undefined and run on the CPU by
// tests/test_host_checks_batch.py.  The frames live in heap arrays of exactly n elements, so that a look past the last one is seen.
#include <limits>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "chisel_hip.h"
#include "host_checks.h"

using namespace chisel_hip;

static float g_image[4] = {1.0f, 1.0f, 1.0f, 1.0f};

static chisel_hip_depth_frame good_frame() {
    chisel_hip_depth_frame f;
    memset(&f, 0, sizeof f);
    f.depth = g_image;
    f.width = 2;
    f.height = 2;
    const float pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(f.pose, pose, sizeof pose);
    f.fx = f.fy = 1.0f;
    f.cx = f.cy = 1.0f;
    return f;
}

static int g_bad = 0;
// the verdict on (n, frames, stats, ids, max_ids): refused or not, and the index the refusal names
static void expect(const char *what, int n, const chisel_hip_depth_frame *frames, bool stats, bool ids, int max_ids, bool refused, int index) {
    int at = 12345;
    const char *why = deintegrate_batch_refusal(n, frames, stats, ids, max_ids, &at);
    if ((why != nullptr) != refused || at != index) {
        printf("FAILED %s: %s, index %d (expected %s, index %d)\n", what, why ? why : "accepted", at, refused ? "a refusal" : "none", index);
        g_bad++;
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int n : {1, 2, 15, 16, 17, 40}) {
        std::vector<chisel_hip_depth_frame> frames((size_t)n, good_frame());
        expect("good frames", n, frames.data(), true, true, 4, false, -1);
        expect("good frames, nothing asked for", n, frames.data(), false, false, 0, false, -1);
        expect("ids without stats", n, frames.data(), false, true, 4, true, -1);
        expect("max_ids < 0", n, frames.data(), true, true, -1, true, -1);
        expect("null frames", n, nullptr, true, true, 4, true, -1);
        // one bad frame at the front, in the middle, at the end: the refusal names it; with two, the first
        for (int at : {0, n / 2, n - 1}) {
            for (int kind = 0; kind < 8; kind++) {
                std::vector<chisel_hip_depth_frame> f = frames;
                switch (kind) {
                    case 0: f[at].depth = nullptr; break;
                    case 1: f[at].width = 0; break;
                    case 2: f[at].height = -3; break;
                    case 3: f[at].width = 1 << 16; f[at].height = 1 << 15; break;
                    case 4: f[at].pose[0] = nan; break;
                    case 5: f[at].pose[11] = -inf; break;
                    case 6: f[at].fx = inf; break;
                    case 7: f[at].cy = nan; break;
                }
                expect("one bad frame", n, f.data(), true, true, 4, true, at);
                f[n - 1].width = -1;
                expect("two bad frames", n, f.data(), true, true, 4, true, at);
            }
        }
    }
    std::vector<chisel_hip_depth_frame> one(1, good_frame());
    expect("n < 0", -1, one.data(), true, true, 4, true, -1);
    expect("n < 0, null frames", -5, nullptr, true, true, 4, true, -1);
    expect("n == 0", 0, one.data(), true, true, 4, false, -1);
    expect("n == 0, null frames", 0, nullptr, true, true, 4, false, -1);
    expect("n == 0, nothing asked for", 0, nullptr, false, false, 0, false, -1);
    if (g_bad) return 1;
    printf("ok: the batch refusals\n");
    return 0;
}
