// kernels_stereo.h -- the plane-sweep stereo matcher in front of the depth filter (StereoMapper, the reference's only GPU code).
// Reference: server_pose_graph/src/dense_mapping/calc_cost.cu -- ADCalcCostKernel :20-233 (launch :284-332), filterCostKernel
// :235-282, sgm2<...> :365-505 (launches :507-546), FuseSparseInfoKernel :684-736; driven by sgm_stereo_mapper.cpp:55-422.
// Every fp32 operation is the reference's, in its order (the library builds with -ffp-contract=off and IEEE division).  The one
// deviation: the match image is sampled bilinearly in software (stereo_sample) where the reference uses a CUDA texture with
// linear filtering and 1.8 fixed-point weights; reference-image reads sit on texel centres and are exact in both.
// Volumes are [height][width][STEREO_DEP_CNT] floats, depth fastest (calc_cost.cu:19, INDEX with ALIGN_WIDTH = width).
#pragma once
#include <hip/hip_runtime.h>

namespace chisel_hip {

constexpr int STEREO_DEP_CNT = 128;  // DEP_CNT, dense_mapping_parameters.h:28

struct StereoParams {
    float pi1, pi2, tau_so, sgm_q1, sgm_q2, var_scale, sparse_ratio, dep_sample;
};

struct StereoView {
    int w, h;
    const float *ref;    // m_mRefImage (undistorted, CV_32F)
    const float *match;  // m_mMatchImage
    const float *p2w;    // m_mGradient: the P2 weight map
    float *cost;         // m_mPhotometricCost
    float *sgm;          // m_mSgmCost
    float *depth;        // m_mDepthMap
};

// texel (i, j) of an image with border addressing: 0 outside (cudaAddressModeBorder)
__device__ inline float stereo_texel(const float *img, int w, int h, int i, int j) {
    return (i >= 0 && i < w && j >= 0 && j < h) ? img[(size_t)j * w + i] : 0.0f;
}

// bilinear sample at unnormalised position (u, v) in texel-centre coordinates (tex2D(t, u + 0.5f, v + 0.5f)), weights exact in
// fp32: (1-a)(1-b) T00 + a(1-b) T10 + (1-a) b T01 + a b T11 in that order.  A NaN coordinate reads 0.
__device__ inline float stereo_sample(const float *img, int w, int h, float u, float v) {
    if (u != u || v != v) return 0.0f;
    const float fu = floorf(u), fv = floorf(v);
    const int i = (int)fu, j = (int)fv;
    const float a = u - fu, b = v - fv;
    const float t00 = stereo_texel(img, w, h, i, j), t10 = stereo_texel(img, w, h, i + 1, j);
    const float t01 = stereo_texel(img, w, h, i, j + 1), t11 = stereo_texel(img, w, h, i + 1, j + 1);
    return (1.0f - a) * (1.0f - b) * t00 + a * (1.0f - b) * t10 + (1.0f - a) * b * t01 + a * b * t11;
}

// ---- ADCalcCostKernel (calc_cost.cu:20-233): one thread per (pixel, depth), depth fastest -------------------------------
// Block of 256 threads = 2 pixels x 128 depths, so each wave64 sees one pixel: its homography rows and the nine reference
// texels are wave-uniform (readfirstlane keeps them scalar); only the per-depth divisions and the match-image samples are
// per lane.
struct StereoPose {
    float r[9], t[3];
};

__global__ void __launch_bounds__(256) stereo_cost_kernel(StereoView S, StereoPose P, int measurement_cnt, float dep_sample) {
    const int pix = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 2 + (threadIdx.x >> 7)));
    if (pix >= S.w * S.h) return;
    const int d = threadIdx.x & (STEREO_DEP_CNT - 1);
    const int tidy = pix / S.w, tidx = pix - tidy * S.w;
    float *cost_ptr = S.cost + (size_t)pix * STEREO_DEP_CNT + d;
    if (measurement_cnt == 1 && (tidx == 0 || tidx == S.w - 1 || tidy == 0 || tidy == S.h - 1)) {
        *cost_ptr = -1.0f;
        return;
    }
    const float last_cost = *cost_ptr;
    if (measurement_cnt != 1 && last_cost < 0) return;

    const float r11 = P.r[0], r12 = P.r[1], r13 = P.r[2], r21 = P.r[3], r22 = P.r[4], r23 = P.r[5], r31 = P.r[6], r32 = P.r[7],
                r33 = P.r[8];
    const float x = r11 * tidx + r12 * tidy + r13 * 1.0f;
    const float y = r21 * tidx + r22 * tidy + r23 * 1.0f;
    const float z = r31 * tidx + r32 * tidy + r33 * 1.0f;
    const float xu = x - r12, yu = y - r22, zu = z - r32;
    const float xd = x + r12, yd = y + r22, zd = z + r32;
    const float xl = x - r11, yl = y - r21, zl = z - r31;
    const float xr = x + r11, yr = x + r21, zr = x + r31;  // sic: yr, zr from the x row (calc_cost.cu:56-57)
    // tap order of the reference: centre, u, d, l, r, ul, dr, ld, ru; homography numerators and the reference texel each reads
    // (u and d sample the reference image mirrored: calc_cost.cu:121, :135)
    const float hx[9] = {x, xu, xd, xl, xr, xu - r11, xd + r11, xl + r12, xr - r12};
    const float hy[9] = {y, yu, yd, yl, yr, yu - r21, yd + r21, yl + r22, xr - r22};  // sic: yru = xr - r22 (:72)
    const float hz[9] = {z, zu, zd, zl, zr, zu - r31, zd + r31, zl + r32, xr - r32};  // sic: zru = xr - r32 (:73)
    const int ox[9] = {0, 0, 0, -1, 1, -1, 1, -1, 1};
    const int oy[9] = {0, 1, -1, 0, 0, -1, 1, 1, -1};

    const float idep = d * dep_sample;
    const float t1 = P.t[0] * idep, t2 = P.t[1] * idep, t3 = P.t[2] * idep;
    const float wmax = (float)(S.w - 1), hmax = (float)(S.h - 1);
    float tmp = 0.0f;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float w = hz[k] + t3;
        const float u = (hx[k] + t1) / w;
        const float v = (hy[k] + t2) / w;
        bad |= w < 0 || u < 0 || u > wmax || v < 0 || v > hmax;
        if (bad) break;  // the entry is -1 whatever the remaining taps give (the reference's `continue`)
        const float left = stereo_texel(S.ref, S.w, S.h, tidx + ox[k], tidy + oy[k]);
        tmp += fabsf(left - stereo_sample(S.match, S.w, S.h, u, v) - 0.0f);  // nMeanDiscrepancy = 0 (sgm_stereo_mapper.cpp:195)
    }
    if (bad) *cost_ptr = -1.0f;
    else if (measurement_cnt == 1) *cost_ptr = tmp / 9.0f;
    else *cost_ptr = (last_cost * (measurement_cnt - 1) + tmp / 9.0f) / measurement_cnt;
}

// ---- FuseSparseInfoKernel (calc_cost.cu:684-736): the keyframe's sparse depth as a prior on the cost, in place -------------
__global__ void __launch_bounds__(256) stereo_fuse_sparse_kernel(StereoView S, const float *__restrict__ sparse_depth,
                                                                 const float *__restrict__ sparse_dist, float ratio, float dep_sample) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)S.w * S.h * STEREO_DEP_CNT) return;
    const size_t pix = e / STEREO_DEP_CNT;
    const int d = (int)(e % STEREO_DEP_CNT);
    const float nDepth = sparse_depth[pix];
    if (!(nDepth > 0.0)) return;
    const float nDist = sparse_dist[pix];
    const float nInvDepth = 1.0 / nDepth;  // a double division, narrowed
    const float nCurrentInvDepth = dep_sample * d;
    float nDiff = 0.0;
    if (nCurrentInvDepth < nInvDepth) nDiff = nInvDepth - nCurrentInvDepth;
    else nDiff = -nInvDepth + nCurrentInvDepth;
    nDiff /= dep_sample;
    if (S.cost[e] > 0.0) S.cost[e] += nDiff * ratio * nDist;
}

// ---- sgm2<idx, start, dx, dy, n> (calc_cost.cu:365-505): one wave64 per scanline, depths 2l and 2l+1 in lane l ------------
// The reference's block-wide tree minima become wave reductions (a minimum is exact in any order: no NaN, no -0 reaches here);
// its "min over the input < 0" becomes __any().  FIRST: the pass that runs on the zeroed volume writes instead of adding
// (0 + x == x for the x >= +0 this produces).  Every load of a step is issued PF steps ahead.
struct SgmScan {
    int n_lines;    // scanlines of this pass
    int n_steps;    // pixels per scanline
    int line_px;    // pixel step between scanlines
    int step_px;    // pixel step along a scanline (signed): the reference's (dx, dy); D1's previous pixel is p - step_px
    int start_px;   // first pixel of scanline 0
};

__device__ inline float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

template <bool FIRST>
__global__ void __launch_bounds__(256) stereo_sgm_kernel(StereoView S, SgmScan Q, StereoParams prm) {
    constexpr int PF = 8;
    const int line = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (line >= Q.n_lines) return;
    const int lane = threadIdx.x & 63;
    const float *__restrict__ input = S.cost;
    float *__restrict__ output = S.sgm;
    const int p0 = Q.start_px + line * Q.line_px;

    // the ring: everything step k reads from memory -- the cost slice, the old sums, D1's two texels (pixel p and the previous
    // pixel p - step_px along the scan) and the P2 weight -- is loaded PF steps ahead, unconditionally and at one address each
    // (indices clamped, no select between loads), so the step body itself waits on no load
    float2 in_buf[PF], out_buf[PF];
    float rc_buf[PF], rp_buf[PF], g_buf[PF];
    auto load = [&](int k, int slot) {
        const int kk = min(k, Q.n_steps - 1);
        const int p = p0 + kk * Q.step_px;
        const size_t off = (size_t)p * STEREO_DEP_CNT + 2 * lane;
        in_buf[slot] = *reinterpret_cast<const float2 *>(input + off);
        if (!FIRST) out_buf[slot] = *reinterpret_cast<const float2 *>(output + off);
        rc_buf[slot] = S.ref[p];
        rp_buf[slot] = S.ref[p0 + (max(kk, 1) - 1) * Q.step_px];  // (step 0 has none: it reads its own, unused)
        g_buf[slot] = S.p2w[p];
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) load(s, s);

    float2 prev = make_float2(0.0f, 0.0f);
    for (int k0 = 0; k0 < Q.n_steps; k0 += PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            // no early exit from the unrolled steps (an exit edge makes the compiler copy, and so wait for, the ring's freshly
            // loaded registers): steps past the scanline's end recompute its last pixel and store nothing
            const int k = k0 + s;
            const int p = p0 + min(k, Q.n_steps - 1) * Q.step_px;
            float2 in = in_buf[s];
            const float2 old = out_buf[s];
            const float rc = rc_buf[s], rp = rp_buf[s], g = g_buf[s];
            load(k + PF, s);
            const bool invalid = __any(in.x < 0.0f || in.y < 0.0f);
            if (invalid) in = make_float2(0.0f, 0.0f);
            float2 val;
            if (k == 0) {
                val = in;
            } else {
                const float m = wave_min(fminf(prev.x, prev.y));
                const float D1 = fabsf(rc - rp);  // the reference image at (x, y) and (x - dx, y - dy)
                float P1 = prm.pi1, P2 = prm.pi2;
                if (D1 < prm.tau_so) {
                    P1 /= prm.sgm_q1;
                    P2 /= prm.sgm_q2;
                    P2 *= g;
                }
                const float left = __shfl_up(prev.y, 1);   // depth 2l - 1
                const float right = __shfl_down(prev.x, 1);  // depth 2l + 2
                float c0 = fminf(prev.x, m + P2);
                if (lane > 0) c0 = fminf(c0, left + P1);
                c0 = fminf(c0, prev.y + P1);
                float c1 = fminf(prev.y, m + P2);
                c1 = fminf(c1, prev.x + P1);
                if (lane < 63) c1 = fminf(c1, right + P1);
                val.x = in.x + c0 - m;
                val.y = in.y + c1 - m;
            }
            float2 o;
            if (invalid) o = make_float2(0.0f, 0.0f);
            else if (FIRST) o = val;
            else o = make_float2(old.x + val.x, old.y + val.y);
            if (k < Q.n_steps) *reinterpret_cast<float2 *>(output + (size_t)p * STEREO_DEP_CNT + 2 * lane) = o;
            prev = val;
        }
    }
}

// ---- filterCostKernel (calc_cost.cu:235-282): winner-takes-all with parabola sub-sample, one wave64 per pixel ------------
// Depths l and l + 64 in lane l: the reference's first tree level (i = 64) is in-lane, the others go through __shfl_down with
// its strict '<' so the tie-break is the tree's (smallest bit-reversed index among equal minima).
__global__ void __launch_bounds__(256) stereo_wta_kernel(StereoView S, float var_scale, float dep_sample) {
    const int pix = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (pix >= S.w * S.h) return;
    const int lane = threadIdx.x & 63;
    const float *c = S.sgm + (size_t)pix * STEREO_DEP_CNT;
    const float lo = c[lane], hi = c[lane + 64];
    float cm = lo;
    int ci = lane;
    if (hi < cm) {
        cm = hi;
        ci = lane + 64;
    }
#pragma unroll
    for (int i = 32; i > 0; i >>= 1) {
        const float om = __shfl_down(cm, i);
        const int oi = __shfl_down(ci, i);
        if (lane < i && om < cm) {
            cm = om;
            ci = oi;
        }
    }
    if (lane != 0) return;
    const float min_cost = cm;
    const int min_idx = ci;
    float dep;
    if (min_cost == 0 || min_idx == 0 || min_idx == STEREO_DEP_CNT - 1 || c[min_idx - 1] + c[min_idx + 1] < 2 * min_cost * var_scale) {
        dep = 1000.0f;
    } else {
        const float cost_pre = c[min_idx - 1];
        const float cost_post = c[min_idx + 1];
        const float a = cost_pre - 2.0f * min_cost + cost_post;
        const float b = -cost_pre + cost_post;
        const float subpixel_idx = min_idx - b / (2.0f * a);
        dep = 1.0f / (subpixel_idx * dep_sample);
    }
    S.depth[pix] = dep;
}

// read-out 3: the depth map widened to double (depth_estimator.cpp:283, mRawResultMap.convertTo(CV_64FC1))
__global__ void stereo_widen_kernel(const float *__restrict__ src, double *__restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (double)src[i];
}

}  // namespace chisel_hip
