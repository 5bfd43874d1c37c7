// kernels_stereo_prep.h -- the OpenCV work around the stereo matcher, on the device: what StereoMapper::InitReference, Update and
// Output do on the host in the reference (server_pose_graph/src/dense_mapping/sgm_stereo_mapper.cpp:55-123, :125-199, :219-422).
//   stereo_remap_kernel         cv::undistort's remap of the resized 8-bit image (fixed-point bilinear, BORDER_CONSTANT 0),
//                               written as the f32 image the cost kernel reads (convertTo(CV_32F), :70 / :170)
//   stereo_sobel_kernel         Sobel(5,5,9), Sobel(3,0,7), Sobel(0,3,7) of the undistorted image (:75, :92, :104) in int32, plus
//                               per-block int64 partial sums for cv::mean and cv::meanStdDev (:78, :93, :105)
//   stereo_prep_stats_kernel    the partials -> mean |Sobel(5,5,9)| and the two mean + stddev thresholds, in double
//   stereo_prep_finish_kernel   the P2 weight map (:79-83) and the two thresholded gradient maps as 1-byte masks (:96-114)
//   stereo_sparse_points_kernel Output's window loop (:231-357) per bound point: bounds from the masks, then the pixels it may write
//   stereo_sparse_raster_kernel the same loop per pixel: the points whose window covers it, in index order
//   stereo_resize_f32_kernel    the final cv::resize of the depth map to the camera size (:409)
// The undistort maps are built on the host (stereo_undistort_map in host_stereo.h) and the 8-bit resize is
// condition_color_kernel (kernels_map.h).  Every value is exact integer arithmetic or the reference's double / float operations
// in its order; the library builds with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_map.h"

namespace chisel_hip {

// ---- cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) with a CV_16SC2 + CV_16UC1 map (imgproc/imgwarp.cpp, remapBilinear) -----------
// map_xy: integer source position (u * 32 >> 5, v * 32 >> 5); map_f: (v * 32 & 31) * 32 + (u * 32 & 31).  Weights of the
// 32 x 32 table: 32 (32 - a)(32 - b), 32 a (32 - b), 32 (32 - a) b, 32 a b -- exact, summing to 32768.  The quad inside the image:
// all four taps; entirely outside (sx >= W, sx + 1 < 0, sy >= H or sy + 1 < 0): 0; otherwise taps outside read 0.
// Result (sum + 2^14) >> 15 (FixedPtCast<int, uchar, 15>).
__global__ void __launch_bounds__(256) stereo_remap_kernel(const uint8_t *__restrict__ src, int W, int H, const short2 *__restrict__ map_xy,
                                                           const uint16_t *__restrict__ map_f, float *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const short2 m = map_xy[i];
    const int sx = m.x, sy = m.y, f = map_f[i];
    const int a = f & 31, b = f >> 5;
    const int w0 = 32 * (32 - a) * (32 - b), w1 = 32 * a * (32 - b), w2 = 32 * (32 - a) * b, w3 = 32 * a * b;
    int sum;
    if ((unsigned)sx < (unsigned)(W - 1) && (unsigned)sy < (unsigned)(H - 1)) {
        const uint8_t *S = src + (size_t)sy * W + sx;
        sum = S[0] * w0 + S[1] * w1 + S[W] * w2 + S[W + 1] * w3;
    } else if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) {
        dst[i] = 0.0f;
        return;
    } else {
        const bool x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W, y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H;
        const int v0 = (x0 && y0) ? src[(size_t)sy * W + sx] : 0, v1 = (x1 && y0) ? src[(size_t)sy * W + sx + 1] : 0;
        const int v2 = (x0 && y1) ? src[(size_t)(sy + 1) * W + sx] : 0, v3 = (x1 && y1) ? src[(size_t)(sy + 1) * W + sx + 1] : 0;
        sum = v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3;
    }
    dst[i] = (float)min(max((sum + (1 << 14)) >> 15, 0), 255);
}

// ---- Sobel with BORDER_REFLECT_101 (getSobelKernels, sepFilter2D as correlation) ------------------------------------------
// The input is integer grey, so every Sobel value is an integer (|Sobel(5,5,9)| <= 255 * 22^2, |Sobel(3,0,7)| <= 255 * 8 * 64) and
// int32 gives the double result's bits.  One 16 x 16 tile per block with a 4-pixel apron in LDS; the apron index is reflected once
// (valid for W, H >= 5, which the host checks) and clamped so that tiles past the image edge stay in bounds.
constexpr int SOBEL_TILE = 16, SOBEL_R = 4, SOBEL_T = SOBEL_TILE + 2 * SOBEL_R;
constexpr int SOBEL_N_STATS = 5;  // sum |g59|, sum gx, sum gx^2, sum gy, sum gy^2

__device__ inline int reflect101(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p); }

__device__ inline long long wave_sum_ll(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(256) stereo_sobel_kernel(const float *__restrict__ img, int W, int H, int *__restrict__ g59abs,
                                                           int *__restrict__ gx, int *__restrict__ gy, long long *__restrict__ partials) {
    constexpr int K9[9] = {-1, 2, 2, -6, 0, 6, -2, -2, 1};  // order 5, size 9
    constexpr int D7[7] = {-1, 0, 3, 0, -3, 0, 1};          // order 3, size 7
    constexpr int S7[7] = {1, 6, 15, 20, 15, 6, 1};         // order 0, size 7
    __shared__ int t[SOBEL_T][SOBEL_T];
    __shared__ long long red[SOBEL_N_STATS][4];
    const int tx = threadIdx.x & (SOBEL_TILE - 1), ty = threadIdx.x / SOBEL_TILE;
    const int x0 = blockIdx.x * SOBEL_TILE, y0 = blockIdx.y * SOBEL_TILE;
    for (int k = threadIdx.x; k < SOBEL_T * SOBEL_T; k += 256) {
        const int r = k / SOBEL_T, c = k - r * SOBEL_T;
        const int sy = min(max(reflect101(y0 + r - SOBEL_R, H), 0), H - 1), sx = min(max(reflect101(x0 + c - SOBEL_R, W), 0), W - 1);
        t[r][c] = (int)img[(size_t)sy * W + sx];
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    long long v[SOBEL_N_STATS] = {0, 0, 0, 0, 0};
    if (x < W && y < H) {
        int s59 = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            int h = 0;
#pragma unroll
            for (int c = 0; c < 9; ++c) h += K9[c] * t[ty + r][tx + c];
            s59 += K9[r] * h;
        }
        int sx3 = 0, sy3 = 0;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            int hd = 0, hs = 0;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const int p = t[ty + 1 + r][tx + 1 + c];
                hd += D7[c] * p;
                hs += S7[c] * p;
            }
            sx3 += S7[r] * hd;  // Sobel(3,0,7): derivative along x, smoothing along y
            sy3 += D7[r] * hs;  // Sobel(0,3,7)
        }
        const int a = abs(s59);
        const size_t i = (size_t)y * W + x;
        g59abs[i] = a;
        gx[i] = sx3;
        gy[i] = sy3;
        v[0] = a;
        v[1] = sx3;
        v[2] = (long long)sx3 * sx3;
        v[3] = sy3;
        v[4] = (long long)sy3 * sy3;
    }
    // integer sums: exact and independent of the order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SOBEL_N_STATS; ++k) {
        const long long s = wave_sum_ll(v[k]);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < SOBEL_N_STATS) {
        const int k = threadIdx.x;
        partials[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * SOBEL_N_STATS + k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
    }
}

// the block partials -> the three scalars InitReference derives (one block).  cv::mean: sum * (1. / n); cv::meanStdDev:
// mean = sum * (1. / n), stddev = sqrt(max(sq * (1. / n) - mean^2, 0)).  The int64 sums convert to double exactly while below
// 2^53 (at 640 x 480 they are below 2^53: 307200 * (255 * 512)^2 < 2^53).
struct StereoPrepStats {
    double p2_scale;  // 1.5 * m * m * m, m = mean |Sobel(5,5,9)|
    double thr_x;     // mean + stddev of Sobel(3,0,7)
    double thr_y;     // mean + stddev of Sobel(0,3,7)
};
__global__ void __launch_bounds__(256) stereo_prep_stats_kernel(const long long *__restrict__ partials, int n_blocks, int n_pixels,
                                                                StereoPrepStats *__restrict__ out) {
    __shared__ long long red[SOBEL_N_STATS][4];
    long long v[SOBEL_N_STATS] = {0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < n_blocks; b += 256)
#pragma unroll
        for (int k = 0; k < SOBEL_N_STATS; ++k) v[k] += partials[(size_t)b * SOBEL_N_STATS + k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SOBEL_N_STATS; ++k) {
        const long long s = wave_sum_ll(v[k]);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long s[SOBEL_N_STATS];
    for (int k = 0; k < SOBEL_N_STATS; ++k) s[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
    const double inv_n = 1. / (double)n_pixels;
    const double m = (double)s[0] * inv_n;
    const double mx = (double)s[1] * inv_n, my = (double)s[3] * inv_n;
    const double dx = sqrt(fmax((double)s[2] * inv_n - mx * mx, 0.0)), dy = sqrt(fmax((double)s[4] * inv_n - my * my, 0.0));
    out->p2_scale = 1.5 * m * m * m;  // sgm_stereo_mapper.cpp:81, left to right
    out->thr_x = mx + dx;             // :98
    out->thr_y = my + dy;             // :110
}

// P2 weight map (:79-83): cv::pow(g, 3) is the integer-power loop g * (g * g) (exact: |g|^3 < 2^53); the MatExpr
// 0.8 + c / (1 + g^3) evaluates 1 + g^3 (exact), then c / that, then convertTo(alpha 1, beta 0.8): x * 1.0 + 0.8; then
// convertTo(CV_32F).  Masks (:96-114, read by Output as `> 0.0`): a pixel counts when g >= mean + stddev and g > 0.
__global__ void __launch_bounds__(256) stereo_prep_finish_kernel(const int *__restrict__ g59abs, const int *__restrict__ gx,
                                                                 const int *__restrict__ gy, const StereoPrepStats *__restrict__ st, int n,
                                                                 float *__restrict__ p2w, uint8_t *__restrict__ mask_x,
                                                                 uint8_t *__restrict__ mask_y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double g = (double)g59abs[i];
    const double g3 = g * (g * g);
    p2w[i] = (float)((st->p2_scale / (1.0 + g3)) * 1.0 + 0.8);
    const double vx = (double)gx[i], vy = (double)gy[i];
    mask_x[i] = (uint8_t)(!(vx < st->thr_x) && vx > 0.0);
    mask_y[i] = (uint8_t)(!(vy < st->thr_y) && vy > 0.0);
}

// ---- Output's sparse prior (sgm_stereo_mapper.cpp:229-357) ------------------------------------------------------------------
// Per point: (int) of the real-image position, then nX /= nScaleX with the reference's swapped scales (nScaleX = realH / H is
// applied to x, nScaleY = realW / W to y) and int truncation; the window's bounds from the two masks read at the flat index
// (nY + vs) * W + (nX + us) of the continuous map (a read outside [0, W * H) counts as 0: the reference reads out of its buffer
// there, undefined); the outward propagation; then the pixels (u, v) that pass the `(int)n + . >= W - 1 / < 1` skip and the bounds
// test as bit (u + 4) * 9 + (v + 4).  A point whose position does not fit an int (undefined in the reference) writes nothing.
constexpr int SPARSE_WIN = 4, SPARSE_SIDE = 2 * SPARSE_WIN + 1, SPARSE_CELLS = SPARSE_SIDE * SPARSE_SIDE;
struct SparsePoint {
    int x, y;      // nX, nY in work-image pixels
    float depth;   // (float)nDepth, as mSparseDepth.at<float>() = nDepth stores it
    unsigned bits[3];
};
// (1 - sqrt(u^2 + v^2) / (4 * 1.414))^2 per cell and the float its square narrows to (:346-350), computed on the host
struct SparseRatios {
    double ratio[SPARSE_CELLS];
    float stored[SPARSE_CELLS];
};

__global__ void __launch_bounds__(256) stereo_sparse_points_kernel(const double *__restrict__ depth, const double *__restrict__ xy, int n, int W,
                                                                   int H, double scale_x, double scale_y, const uint8_t *__restrict__ mask_x,
                                                                   const uint8_t *__restrict__ mask_y, SparsePoint *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SparsePoint p;
    p.depth = (float)depth[i];
    p.bits[0] = p.bits[1] = p.bits[2] = 0u;
    p.x = p.y = -(1 << 30);
    const double px = xy[2 * (size_t)i], py = xy[2 * (size_t)i + 1];
    const double lim = 1073741824.0;  // 2^30: beyond it no window pixel is in the image
    if (!(fabs(px) < lim && fabs(py) < lim)) {
        out[i] = p;
        return;
    }
    int nX = (int)px, nY = (int)py;
    const double qx = (double)nX / scale_x, qy = (double)nY / scale_y;
    if (!(fabs(qx) < lim && fabs(qy) < lim)) {
        out[i] = p;
        return;
    }
    nX = (int)qx;
    nY = (int)qy;
    int up[SPARSE_SIDE], bottom[SPARSE_SIDE], left[SPARSE_SIDE], right[SPARSE_SIDE];
    for (int k = 0; k < SPARSE_SIDE; ++k) {
        up[k] = SPARSE_WIN;
        bottom[k] = -SPARSE_WIN;
        left[k] = -SPARSE_WIN;
        right[k] = SPARSE_WIN;
    }
    const long long n_pix = (long long)W * H;
    for (int us = -SPARSE_WIN; us <= SPARSE_WIN; ++us) {
        for (int vs = -SPARSE_WIN; vs <= SPARSE_WIN; ++vs) {
            const long long k = (long long)(nY + vs) * W + (nX + us);
            const bool in = k >= 0 && k < n_pix;
            if (in && mask_x[k]) {
                if (left[vs + SPARSE_WIN] < us && us < 0) left[vs + SPARSE_WIN] = us;
                if (right[vs + SPARSE_WIN] > us && us > 0) right[vs + SPARSE_WIN] = us;
            }
            if (in && mask_y[k]) {
                if (up[us + SPARSE_WIN] > vs && vs > 0) up[us + SPARSE_WIN] = vs;
                if (bottom[us + SPARSE_WIN] < vs && vs < 0) bottom[us + SPARSE_WIN] = vs;
            }
        }
    }
    for (int us = 1; us <= SPARSE_WIN; ++us) {
        const int pi = us + SPARSE_WIN, ni = -us + SPARSE_WIN;
        if (up[pi] > up[pi - 1]) up[pi] = up[pi - 1];
        if (up[ni] > up[ni + 1]) up[ni] = up[ni + 1];
        if (bottom[pi] < bottom[pi - 1]) bottom[pi] = bottom[pi - 1];
        if (bottom[ni] < bottom[ni + 1]) bottom[ni] = bottom[ni + 1];
        if (left[pi] < left[pi - 1]) left[pi] = left[pi - 1];
        if (left[ni] < left[ni + 1]) left[ni] = left[ni + 1];
        if (right[pi] > right[pi - 1]) right[pi] = right[pi - 1];
        if (right[ni] > right[ni + 1]) right[ni] = right[ni + 1];
    }
    for (int u = -SPARSE_WIN; u <= SPARSE_WIN; ++u) {
        for (int v = -SPARSE_WIN; v <= SPARSE_WIN; ++v) {
            if (nY + v >= H - 1 || nY + v < 1 || nX + u >= W - 1 || nX + u < 1) continue;
            if (u >= left[v + SPARSE_WIN] && u <= right[v + SPARSE_WIN] && v >= bottom[u + SPARSE_WIN] && v <= up[u + SPARSE_WIN]) {
                const int b = (u + SPARSE_WIN) * SPARSE_SIDE + (v + SPARSE_WIN);
                p.bits[b >> 5] |= 1u << (b & 31);
            }
        }
    }
    p.x = nX;
    p.y = nY;
    out[i] = p;
}

// Per pixel of a 16 x 16 tile: the points are scanned in chunks of 256 in index order; those whose window meets the tile are
// compacted into LDS in the same order (ballot + prefix), then every pixel replays the writes that reach it.  A pixel's final
// value depends only on its own ordered writes, so this equals the sequential loop over the points.
__global__ void __launch_bounds__(256) stereo_sparse_raster_kernel(const SparsePoint *__restrict__ pts, int n, int W, int H, SparseRatios R,
                                                                   float *__restrict__ sparse_depth, float *__restrict__ sparse_dist) {
    __shared__ SparsePoint list[256];
    __shared__ int wave_count[4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16, x = x0 + tx, y = y0 + ty;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float d = -1.0f, dist = 0.0f;  // cv::Mat(HEIGHT, WIDTH, CV_32F, -1.0) and (..., 0.0)
    for (int base = 0; base < n; base += 256) {
        const int j = base + (int)threadIdx.x;
        SparsePoint p;
        bool hit = false;
        if (j < n) {
            p = pts[j];
            hit = (p.bits[0] | p.bits[1] | p.bits[2]) != 0u && p.x - SPARSE_WIN <= x0 + 15 && p.x + SPARSE_WIN >= x0 &&
                  p.y - SPARSE_WIN <= y0 + 15 && p.y + SPARSE_WIN >= y0;
        }
        const unsigned long long ballot = __ballot(hit);
        const int rank = __popcll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) wave_count[wave] = __popcll(ballot);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += wave_count[w];
            total += wave_count[w];
        }
        if (hit) list[off + rank] = p;
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const SparsePoint &q = list[k];
            const int u = x - q.x, v = y - q.y;
            if (u < -SPARSE_WIN || u > SPARSE_WIN || v < -SPARSE_WIN || v > SPARSE_WIN) continue;
            const int b = (u + SPARSE_WIN) * SPARSE_SIDE + (v + SPARSE_WIN);
            if (!((q.bits[b >> 5] >> (b & 31)) & 1u)) continue;
            if ((double)dist < R.ratio[b]) {
                d = q.depth;
                dist = R.stored[b];
            }
        }
        __syncthreads();
    }
    if (x < W && y < H) {
        sparse_depth[(size_t)y * W + x] = d;
        sparse_dist[(size_t)y * W + x] = dist;
    }
}

// ---- the final cv::resize of the depth map (sgm_stereo_mapper.cpp:409): CV_32F, INTER_LINEAR ---------------------------------
// The taps of condition_depth_kernel (resize_tap_x / resize_tap_y); the float type's work type is float: float weights, float
// products and sums (S[s] * a0 + S[s + 1] * a1, then r0 * b0 + r1 * b1; S[s] * 1.0f at the right edge).  Exact halving: INTER_AREA,
// (((a + b) + c) + d) * 0.25f.  Equal sizes: a copy.  The rejected value 1000 is interpolated like any other.
__global__ void stereo_resize_f32_kernel(const float *__restrict__ src, int w0, int h0, float *__restrict__ dst, int w, int h) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    float v;
    if (w == w0 && h == h0) {
        v = src[(size_t)y * w0 + x];
    } else if (w0 == 2 * w && h0 == 2 * h) {
        const float *s = src + (size_t)(2 * y) * w0 + 2 * x;
        v = (((s[0] + s[1]) + s[w0]) + s[w0 + 1]) * 0.25f;
    } else {
        const ResizeTap tx = resize_tap_x(x, resize_scale(w, w0), w0);
        int y0, y1;
        float fy;
        resize_tap_y(y, resize_scale(h, h0), h0, y0, y1, fy);
        const float a0 = 1.0f - tx.f, a1 = tx.f, b0 = 1.0f - fy, b1 = fy;
        const float *s0 = src + (size_t)y0 * w0 + tx.s, *s1 = src + (size_t)y1 * w0 + tx.s;
        const float r0 = tx.edge ? s0[0] * 1.0f : s0[0] * a0 + s0[1] * a1;
        const float r1 = tx.edge ? s1[0] * 1.0f : s1[0] * a0 + s1[1] * a1;
        v = r0 * b0 + r1 * b1;
    }
    dst[(size_t)y * w + x] = v;
}

}  // namespace chisel_hip
