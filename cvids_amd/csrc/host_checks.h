// host_checks.h -- the host-side pieces of the side entries (chisel_hip_align_terms / _align_depth, chisel_hip_deintegrate_depth / _batch)
// that call nothing of HIP (included by kernels_deintegrate.h and, on its own, by tests/host_checks_check.cpp and
// tests/host_checks_batch_check.cpp, which run them under the address and undefined-behaviour sanitizers on the CPU): what the entries
// refuse about a frame's image, what de-integration refuses
// about its other arguments, and the planes its list kernel rejects chunks by.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define CHISEL_HOST_DEVICE __host__ __device__
#else
#define CHISEL_HOST_DEVICE
#endif

namespace chisel_hip {

// What the list kernel rejects by, in double, camera frame: a chunk is dropped when its bounding sphere lies behind the camera plane or
// outside one of the four side planes of the image pyramid (normals pointing inwards, through the camera centre, the image widened by
// two pixels on every side).  Any superset of the chunks that hold a selected voxel is correct: the per-voxel rule is exact.
struct DeintegratePyramid {
    double R[9], t[3];          // the pose as the kernels take it, widened
    double plane[5][3];         // the camera plane, then left, right, top, bottom: n / |R n| (= the unit normal for a rotation R)
    double edge;                // N res
    double radius;              // half the chunk's diagonal
    double slack;               // per metre of the largest coordinate involved: what fp32 rounding moves a voxel centre and its q by
};

// With q = R^T (c - t) a voxel on the image has qz >= 0 and, multiplied through by qz, fx qx + cx qz >= 0, (W - cx) qz - fx qx > 0 and
// the same in y: five half-spaces through the camera centre, whatever the signs of fx and cx.  The image is widened by two pixels plus
// what fp32 rounding can move u and v by.  A voxel at world offset e from a chunk's centre moves n . q by (R n) . e <= |R n| |e|: the
// normals are divided by |R n|, so that the kernel compares against the chunk's radius also where R is not a rotation.
inline void deintegrate_pyramid(const float pose[12], float fx_, float fy_, float cx_, float cy_, int width, int height, int N, float res, DeintegratePyramid &Y) {
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) Y.R[3 * r + k] = (double)pose[4 * r + k];
        Y.t[r] = (double)pose[4 * r + 3];
    }
    const double fx = fx_, fy = fy_, cx = cx_, cy = cy_, W = width, H = height;
    const double mx = 2.0 + 1e-6 * (fabs(cx) + W), my = 2.0 + 1e-6 * (fabs(cy) + H);
    const double n[5][3] = {{0.0, 0.0, 1.0}, {fx, 0.0, cx + mx}, {-fx, 0.0, W + mx - cx}, {0.0, fy, cy + my}, {0.0, -fy, H + my - cy}};
    for (int p = 0; p < 5; p++) {
        double len2 = 0.0;
        for (int r = 0; r < 3; r++) {
            const double w = (Y.R[3 * r] * n[p][0] + Y.R[3 * r + 1] * n[p][1]) + Y.R[3 * r + 2] * n[p][2];
            len2 += w * w;
        }
        const double len = sqrt(len2);
        for (int k = 0; k < 3; k++) Y.plane[p][k] = len > 0.0 ? n[p][k] / len : 0.0;  // (a degenerate plane rejects nothing)
    }
    Y.edge = (double)N * (double)res;
    Y.radius = 0.5 * sqrt(3.0) * Y.edge;
    Y.slack = 4e-6;  // (more than 32 ulp of the largest coordinate: the centre's three operations, the difference, the products and sums of q)
}

// the list kernel's verdict on the chunk `id`, as the kernel computes it
CHISEL_HOST_DEVICE inline bool deintegrate_keeps(const DeintegratePyramid &Y, int x, int y, int z) {
    const double c[3] = {((double)x + 0.5) * Y.edge, ((double)y + 0.5) * Y.edge, ((double)z + 0.5) * Y.edge};
    const double d[3] = {c[0] - Y.t[0], c[1] - Y.t[1], c[2] - Y.t[2]};
    const double q[3] = {Y.R[0] * d[0] + Y.R[3] * d[1] + Y.R[6] * d[2], Y.R[1] * d[0] + Y.R[4] * d[1] + Y.R[7] * d[2],
                         Y.R[2] * d[0] + Y.R[5] * d[1] + Y.R[8] * d[2]};
    const double reach = fmax(fmax(fabs(c[0]), fabs(c[1])), fmax(fabs(c[2]), fmax(fabs(Y.t[0]), fmax(fabs(Y.t[1]), fabs(Y.t[2]))))) + Y.radius;
    const double r = Y.radius + Y.slack * reach;
    bool keep = true;  // (a NaN keeps the chunk)
    for (int p = 0; p < 5; p++) keep = keep && !(Y.plane[p][0] * q[0] + Y.plane[p][1] * q[1] + Y.plane[p][2] * q[2] + r < 0.0);
    return keep;
}

// what the entries that take a depth frame outside the integration path refuse about its image (check_frame of the integration path
// has limits of its own); null = go on
inline const char *frame_image_refusal(const float *depth, int width, int height) {
    if (!depth) return "null depth image";
    if (width < 1 || height < 1) return "non-positive image size";
    if ((int64_t)width * height > (int64_t)INT32_MAX) return "more than 2^31 - 1 pixels";
    return nullptr;
}

// what chisel_hip_deintegrate_depth refuses about its arguments other than the map; null = go on
inline const char *deintegrate_refusal(const float *depth, int width, int height, const float pose[12], float fx, float fy, float cx, float cy,
                                       bool want_stats, bool want_ids, int max_ids) {
    if (const char *why = frame_image_refusal(depth, width, height)) return why;
    for (int i = 0; i < 12; i++)
        if (!isfinite(pose[i])) return "the pose has an entry that is not finite";
    if (!isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return "intrinsics that are not finite";
    if (max_ids < 0) return "max_ids < 0";
    if (want_ids && !want_stats) return "emptied_ids_xyz without stats (the count of the ids is reported there)";
    return nullptr;
}

// what chisel_hip_deintegrate_batch refuses about its arguments other than the map, every frame looked at before anything is touched;
// null = go on (n == 0 included).  *bad_frame: the index of the frame the refusal is about, -1 when it is about the call.  Frame:
// chisel_hip_depth_frame (a template, so that this header goes on including nothing of the library's)
template <class Frame>
inline const char *deintegrate_batch_refusal(int n, const Frame *frames, bool want_stats, bool want_ids, int max_ids, int *bad_frame) {
    *bad_frame = -1;
    if (n < 0) return "n < 0";
    if (n > 0 && !frames) return "null frames with n > 0";
    if (max_ids < 0) return "max_ids < 0";
    if (want_ids && !want_stats) return "emptied_ids_xyz without stats (the count of the ids is reported there)";
    for (int i = 0; i < n; i++) {
        const Frame &f = frames[i];
        if (const char *why = deintegrate_refusal(f.depth, f.width, f.height, f.pose, f.fx, f.fy, f.cx, f.cy, want_stats, want_ids, max_ids)) {
            *bad_frame = i;
            return why;
        }
    }
    return nullptr;
}

}  // namespace chisel_hip
