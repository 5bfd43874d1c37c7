// distance_checks.h -- the host-side pieces of chisel_hip_distance_field that call nothing of HIP (included by chisel_hip.hip for host_distance.h and, on its
// own, by tests/distance_checks_check.cpp, which runs them under the address and undefined-behaviour sanitizers on the CPU): what the
// entry refuses about its window, the window widened by the radius, the sizes of the scratch, and the table the distances are read from.
// DESIGN.md 3.11 is the definition.
#pragma once
#include <math.h>
#include <stdint.h>

namespace chisel_hip {

constexpr int DISTANCE_MAX_RADIUS = 64;                // 3 * 64^2 fits the 16-bit intermediates
constexpr int64_t DISTANCE_COORD_LIMIT = 1ll << 30;    // |global voxel index| of the widened window, per axis
constexpr int64_t DISTANCE_MAX_VOXELS = 1ll << 30;     // voxels of the widened window
constexpr int DISTANCE_REFUSED_INVALID = 1, DISTANCE_REFUSED_UNSUPPORTED = 5;  // = CHISEL_HIP_ERR_INVALID, CHISEL_HIP_ERR_UNSUPPORTED

// The window widened by the radius on every side (the seeds are read over it), and what the three passes keep between them:
//   bits  one obstacle bit per voxel of the widened window, a row of x in 64-bit words            [wd z][wd y][words_per_row]
//   g1    after the pass along x: window x, widened y and z, 16 bits per voxel                    [wd z][wd y][nx]
//   g2    after the pass along y: window x and y, widened z                                        [wd z][ny][nx]
struct DistancePlan {
    int wo[3], wd[3];         // first voxel and extent of the widened window
    int64_t voxels, widened;  // voxels of the window and of the widened window
    int64_t words_per_row, bits_words, g1_elems, g2_elems;
};

// what chisel_hip_distance_field refuses about its arguments other than the map, in the order of the header; null = go on, with *plan
// filled.  *code: DISTANCE_REFUSED_* of a refusal.  Window: chisel_hip_distance_window (a template, so that this header goes on
// including nothing of the library's)
template <class Window>
inline const char *distance_refusal(const Window *w, bool any_output, int *code, DistancePlan *plan) {
    *code = DISTANCE_REFUSED_INVALID;
    if (!w) return "null window";
    if (!any_output) return "no output asked for";
    for (int a = 0; a < 3; a++)
        if (w->dims[a] < 1) return "a window dimension below 1";
    if (w->radius < 1 || w->radius > DISTANCE_MAX_RADIUS) return "the radius is outside 1 ... 64 voxels";
    if (w->surface_offset != w->surface_offset) return "the surface offset is NaN";
    const int64_t R = w->radius;
    int64_t wd[3];
    for (int a = 0; a < 3; a++) {
        const int64_t lo = (int64_t)w->origin[a] - R, hi = (int64_t)w->origin[a] + (int64_t)w->dims[a] - 1 + R;
        if (lo < -DISTANCE_COORD_LIMIT || hi > DISTANCE_COORD_LIMIT) return "the window widened by the radius reaches beyond voxel index +-2^30";
        wd[a] = hi - lo + 1;  // (<= 2^31 + 1)
        plan->wo[a] = (int)lo;
    }
    *code = DISTANCE_REFUSED_UNSUPPORTED;
    if (wd[0] > DISTANCE_MAX_VOXELS || wd[0] * wd[1] > DISTANCE_MAX_VOXELS || wd[0] * wd[1] * wd[2] > DISTANCE_MAX_VOXELS)  // (each product <= 2^30 * (2^31 + 1))
        return "the window widened by the radius holds more than 2^30 voxels";
    for (int a = 0; a < 3; a++) plan->wd[a] = (int)wd[a];
    plan->voxels = (int64_t)w->dims[0] * w->dims[1] * w->dims[2];
    plan->widened = wd[0] * wd[1] * wd[2];
    plan->words_per_row = (wd[0] + 63) / 64;
    plan->bits_words = plan->words_per_row * wd[1] * wd[2];
    plan->g1_elems = (int64_t)w->dims[0] * wd[1] * wd[2];
    plan->g2_elems = (int64_t)w->dims[0] * w->dims[1] * wd[2];
    *code = 0;
    return nullptr;
}

// distance[dist2] for dist2 = 0 ... R^2: (float)(sqrt((double)dist2) * (double)voxel_resolution); out holds R^2 + 1 floats.  An entry
// does not depend on R: the table of a smaller radius is the front of this one
inline void distance_table(int radius, float voxel_resolution, float *out) {
    const int n = radius * radius;
    for (int i = 0; i <= n; i++) out[i] = (float)(sqrt((double)i) * (double)voxel_resolution);
}

}  // namespace chisel_hip
