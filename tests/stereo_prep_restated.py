"""CPU restatement (numpy) of the OpenCV work around the stereo matcher -- StereoMapper::InitIntrinsic, InitReference, Update,
BindSparsePoints and Output (server_pose_graph/src/dense_mapping/sgm_stereo_mapper.cpp:20-422) -- for the tests of the library's
raw-image path (chisel_hip_stereo_set_camera and after).  Not a test module; only tests/ imports it.

OpenCV is a third-party dependency of the reference and is not installed here; its published algorithms (OpenCV 4, scalar paths,
no IPP) are restated:
  * cv::resize of the 8-bit frame: oracle/publish_dense.py's resize_u8 (the rules chisel_hip_condition_color follows);
  * cv::undistort(src, dst, K, D, K): stripes of min(max(1, 4096 / cols), rows) rows, each with Ar(1,2) = v0 - y and its own
    iR = Ar^-1 (cv::invert's 3 x 3 closed form); initUndistortRectifyMap's scalar loop (_x, _y, _w accumulated column by column,
    the k1 k2 p1 p2 k3 polynomial, u and v from the unmodified A) into a CV_16SC2 + CV_16UC1 map (cvRound(u * 32), 5 fraction
    bits); remap with the fixed-point bilinear table (weights 32 (32 - a)(32 - b) ... summing to 32768, (sum + 2^14) >> 15),
    BORDER_CONSTANT 0 per tap and 0 for a quad entirely outside;
  * cv::Sobel with the kernels of getSobelKernels as correlation with BORDER_REFLECT_101, in int64 (exact: the input is integer);
  * cv::mean = sum * (1. / n), cv::meanStdDev = (mean, sqrt(max(sq * (1. / n) - mean^2, 0))) of exact integer sums;
  * cv::pow(g, 3) = g * (g * g) (the integer-power loop) and the MatExpr 0.8 + c / (1 + g^3) as (c / (1 + g^3)) * 1.0 + 0.8;
  * the final cv::resize of the CV_32F depth: the taps of oracle/publish_dense.py with float weights, products and sums.
PARITY WITH THE REAL OPENCV IS UNPINNED: no OpenCV build was available to generate vectors; tests/test_stereo_prep_restated.py holds
hand-computed cases of the rules above.

sparse_maps() is Output's window loop (:229-357) kept literally close to the reference, one point and one pixel at a time;
sparse_maps_vectorised() computes every point's bounds at once and is what the chained restatement uses."""
import math

import numpy as np

from oracle import publish_dense as pd

f32 = np.float32
WINDOW = 4                     # nWindowSize, sgm_stereo_mapper.cpp:240
INT_MIN = -2 ** 31
FIT_LIMIT = 2.0 ** 30          # kernels_stereo_prep.h: a point at or beyond it (or at NaN) does not fit an int and writes nothing


def sobel_kernel(order, ksize):
    """getSobelKernels' 1-D kernel (imgproc/deriv.cpp) of derivative `order` and size `ksize`, as integers"""
    k = [1] + [0] * ksize
    for _ in range(ksize - order - 1):
        old = k[0]
        for j in range(1, ksize + 1):
            new = k[j] + k[j - 1]
            k[j - 1] = old
            old = new
    for _ in range(order):
        old = -k[0]
        for j in range(1, ksize + 1):
            new = k[j - 1] - k[j]
            k[j - 1] = old
            old = new
    return k[:ksize]


def sobel(img, dx, dy, ksize):
    """cv::Sobel(img, CV_64F, dx, dy, ksize) of an integer image, as int64: correlation, BORDER_REFLECT_101 (numpy's 'reflect')"""
    kx, ky = np.array(sobel_kernel(dx, ksize), np.int64), np.array(sobel_kernel(dy, ksize), np.int64)
    a = ksize // 2
    p = np.pad(np.asarray(img).astype(np.int64), a, mode="reflect")
    H, W = np.asarray(img).shape
    rows = sum(kx[c] * p[:, c:c + W] for c in range(ksize))
    return sum(ky[r] * rows[r:r + H, :] for r in range(ksize))


def mean_dev(g):
    """cv::meanStdDev of an integer map: exact integer sums, then mean = s * (1. / n), sqrt(max(sq * (1. / n) - mean^2, 0))"""
    g = np.asarray(g, np.int64)
    inv = 1.0 / float(g.size)
    m = float(int(g.sum())) * inv
    return m, math.sqrt(max(float(int((g * g).sum())) * inv - m * m, 0.0))


def p2_weight(g59):
    """InitReference's P2 weight map (:75-83) from the Sobel(5,5,9) map"""
    g = np.abs(np.asarray(g59, np.int64))
    m = float(int(g.sum())) * (1.0 / float(g.size))
    c = 1.5 * m * m * m
    gd = g.astype(np.float64)
    return ((c / (1.0 + gd * (gd * gd))) * 1.0 + 0.8).astype(np.float32)


def gradient_mask(g):
    """the thresholded gradient map (:92-114) as Output reads it (> 0.0): g >= mean + stddev and g > 0"""
    m, d = mean_dev(g)
    gd = np.asarray(g, np.int64).astype(np.float64)
    return (~(gd < m + d) & (gd > 0.0)).astype(np.uint8)


def invert3(m):
    """cv::invert(DECOMP_LU)'s closed form for a 3 x 3 CV_64F matrix (row-major list of 9 floats) -> list, or None if det == 0"""
    m = [float(v) for v in m]
    M = lambda i, j: m[i * 3 + j]
    d = M(0, 0) * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) - M(0, 1) * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0)) + \
        M(0, 2) * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0))
    if d == 0.0:
        return None
    d = 1.0 / d
    return [(M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * d, (M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * d,
            (M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * d, (M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * d,
            (M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * d, (M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * d,
            (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * d, (M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * d,
            (M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * d]


def _mul3(a, b, cols, bt=False):
    out = []
    for i in range(3):
        for j in range(cols):
            b0, b1, b2 = (b[j * 3], b[j * 3 + 1], b[j * 3 + 2]) if bt else (b[j], b[cols + j], b[2 * cols + j])
            out.append(a[i * 3] * b0 + a[i * 3 + 1] * b1 + a[i * 3 + 2] * b2)
    return out


def homography(K1, K2, Rr, tr, Rm, tm):
    """Update's R = K2 Rm^T Rr K1^-1, t = K2 Rm^T (tr - tm) (:179-182): K = (fx, fy, cx, cy), products left to right in double,
    K1^-1 by invert3; narrowed to float32"""
    k = lambda K: [float(K[0]), 0.0, float(K[2]), 0.0, float(K[1]), float(K[3]), 0.0, 0.0, 1.0]
    fl = lambda a: [float(v) for v in np.asarray(a, np.float64).reshape(-1)]
    Rr, tr, Rm, tm = fl(Rr), fl(tr), fl(Rm), fl(tm)
    a = _mul3(k(K2), Rm, 3, bt=True)
    r = _mul3(_mul3(a, Rr, 3), invert3(k(K1)), 3)
    t = _mul3(a, [tr[0] - tm[0], tr[1] - tm[1], tr[2] - tm[2]], 1)
    return np.array(r, np.float64).astype(np.float32).reshape(3, 3), np.array(t, np.float64).astype(np.float32)


def scale_intrinsics(K, real_w, real_h, W, H):
    """InitIntrinsic (:31-45): fx, cx / (real_w / W), fy, cy / (real_h / H)"""
    sx, sy = float(real_w) / float(W), float(real_h) / float(H)
    return (float(K[0]) / sx, float(K[1]) / sy, float(K[2]) / sx, float(K[3]) / sy)


def _cv_round(v):
    """cvRound as x86-64 computes it: half to even; NaN or outside int -> INT_MIN"""
    ok = (v >= -2147483648.5) & (v < 2147483647.5)
    return np.where(ok, np.rint(np.where(ok, v, 0.0)), INT_MIN).astype(np.int64)


def undistort_map(W, H, K, D):
    """cv::undistort's CV_16SC2 + CV_16UC1 map for a W x H image: (x, y) int16 arrays and the fraction index, uint16"""
    fx, fy, u0, v0 = (float(v) for v in K)
    k1, k2, p1, p2, k3 = (float(v) for v in D)
    k4 = k5 = k6 = 0.0
    mx, my, mf = np.empty((H, W), np.int16), np.empty((H, W), np.int16), np.empty((H, W), np.uint16)
    stripe0 = min(max(1, 4096 // max(W, 1)), H)
    for y in range(0, H, stripe0):
        rows = min(stripe0, H - y)
        ir = invert3([fx, 0.0, u0, 0.0, fy, v0 - y, 0.0, 0.0, 1.0]) or [0.0] * 9
        for i in range(rows):
            acc = lambda start, step: np.cumsum(np.concatenate([[start], np.full(W - 1, step)]))  # sequential += (numpy's cumsum)
            _x, _y, _w = acc(i * ir[1] + ir[2], ir[0]), acc(i * ir[4] + ir[5], ir[3]), acc(i * ir[7] + ir[8], ir[6])
            with np.errstate(all="ignore"):
                w = 1.0 / _w
                x, yy = _x * w, _y * w
                x2, y2 = x * x, yy * yy
                r2 = x2 + y2
                _2xy = 2 * x * yy
                kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
                xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
                yd = yy * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
                u, v = fx * xd + u0, fy * yd + v0
                iu, iv = _cv_round(u * 32), _cv_round(v * 32)
            mx[y + i] = (iu >> 5).astype(np.int16)
            my[y + i] = (iv >> 5).astype(np.int16)
            mf[y + i] = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return mx, my, mf


def remap(src, mx, my, mf):
    """cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) of an 8-bit image with a CV_16SC2 + CV_16UC1 map -> uint8"""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    sx, sy, f = mx.astype(np.int64), my.astype(np.int64), mf.astype(np.int64)
    a, b = f & 31, f >> 5
    w = [32 * (32 - a) * (32 - b), 32 * a * (32 - b), 32 * (32 - a) * b, 32 * a * b]

    def tap(dx, dy):
        x, y = sx + dx, sy + dy
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), 0)

    s = tap(0, 0) * w[0] + tap(1, 0) * w[1] + tap(0, 1) * w[2] + tap(1, 1) * w[3]
    out = np.clip((s + (1 << 14)) >> 15, 0, 255)
    outside = (sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)
    return np.where(outside, 0, out).astype(np.uint8)


def prepare(raw, W, H, K_scaled, D):
    """cv::resize to W x H, cv::undistort, convertTo(CV_32F) (:66-70, :162-170) -> float32 image"""
    small = pd.resize_u8(np.asarray(raw, np.uint8), W, H)
    return remap(small, *undistort_map(W, H, K_scaled, D)).astype(np.float32)


def reference_maps(ref32):
    """InitReference's maps from the prepared reference image: (P2 weight map, x mask, y mask)"""
    g = ref32.astype(np.int64)
    return p2_weight(sobel(g, 5, 5, 9)), gradient_mask(sobel(g, 3, 0, 7)), gradient_mask(sobel(g, 0, 3, 7))


def _ratio(u, v):
    r = 1.0 - (math.sqrt(u * u + v * v) / (WINDOW * 1.414))
    return r * r


def sparse_maps(depths, points, mask_x, mask_y, W, H, real_w, real_h):
    """Output's window loop (sgm_stereo_mapper.cpp:229-357), literally: -> (sparse depth, sparse distance) float32 (H, W).
    The masks are read at the flat index of the continuous map; outside [0, W * H) a read counts as 0 (the reference reads out of
    its buffer there: undefined).  A point whose position does not fit an int -- NaN, +-inf or |.| >= 2^30, before or after the
    scale -- writes nothing: the reference's (int) of such a double is undefined, and the library's stated rule
    (kernels_stereo_prep.h, the sparse prior's header comment) is the contract."""
    nScaleX = float(real_h) / float(H)     # sic: the x scale is the height ratio (:226-227)
    nScaleY = float(real_w) / float(W)
    mSparseDepth = np.full((H, W), -1.0, np.float32)
    mSparseDistance = np.zeros((H, W), np.float32)
    gx, gy = np.asarray(mask_x).reshape(-1), np.asarray(mask_y).reshape(-1)

    def at(m, r, c):
        k = r * W + c
        return int(m[k]) if 0 <= k < W * H else 0

    for i in range(len(depths)):
        nDepth = float(depths[i])
        fX, fY = float(points[i][0]), float(points[i][1])
        if not (abs(fX) < FIT_LIMIT and abs(fY) < FIT_LIMIT):      # (false for NaN too)
            continue
        nX = int(fX)
        nY = int(fY)
        if not (abs(nX / nScaleX) < FIT_LIMIT and abs(nY / nScaleY) < FIT_LIMIT):
            continue
        nX = int(nX / nScaleX)
        nY = int(nY / nScaleY)
        n = WINDOW
        up, bottom, left, right = [n] * (2 * n + 1), [-n] * (2 * n + 1), [-n] * (2 * n + 1), [n] * (2 * n + 1)
        for us in range(-n, n + 1):
            for vs in range(-n, n + 1):
                if at(gx, nY + vs, nX + us) > 0.0:
                    if left[vs + n] < us and us < 0:
                        left[vs + n] = us
                    if right[vs + n] > us and us > 0:
                        right[vs + n] = us
                if at(gy, nY + vs, nX + us) > 0.0:
                    if up[us + n] > vs and vs > 0:
                        up[us + n] = vs
                    if bottom[us + n] < vs and vs < 0:
                        bottom[us + n] = vs
        for us in range(1, n + 1):
            p, q = us + n, -us + n
            if up[p] > up[p - 1]:
                up[p] = up[p - 1]
            if up[q] > up[q + 1]:
                up[q] = up[q + 1]
            if bottom[p] < bottom[p - 1]:
                bottom[p] = bottom[p - 1]
            if bottom[q] < bottom[q + 1]:
                bottom[q] = bottom[q + 1]
            if left[p] < left[p - 1]:
                left[p] = left[p - 1]
            if left[q] < left[q + 1]:
                left[q] = left[q + 1]
            if right[p] > right[p - 1]:
                right[p] = right[p - 1]
            if right[q] > right[q + 1]:
                right[q] = right[q + 1]
        for u in range(-n, n + 1):
            for v in range(-n, n + 1):
                if nY + v >= H - 1 or nY + v < 1 or nX + u >= W - 1 or nX + u < 1:
                    continue
                if left[v + n] <= u <= right[v + n] and bottom[u + n] <= v <= up[u + n]:
                    nDistRatio = _ratio(u, v)
                    if float(mSparseDistance[nY + v, nX + u]) < nDistRatio:
                        mSparseDepth[nY + v, nX + u] = f32(nDepth)
                        mSparseDistance[nY + v, nX + u] = f32(nDistRatio * nDistRatio)
    return mSparseDepth, mSparseDistance


def sparse_maps_vectorised(depths, points, mask_x, mask_y, W, H, real_w, real_h):
    """the same maps: every point's bounds computed at once (arrays over the points), then the writes replayed per point in
    index order on its 9 x 9 window"""
    n = WINDOW
    S = 2 * n + 1
    depths = np.asarray(depths, np.float64).reshape(-1)
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    sd, sdist = np.full((H, W), -1.0, np.float32), np.zeros((H, W), np.float32)
    if len(depths) == 0:
        return sd, sdist
    # the does-not-fit-an-int rule, before any cast: such a point is parked at the origin here and skipped in the replay below
    fits = (np.abs(pts[:, 0]) < FIT_LIMIT) & (np.abs(pts[:, 1]) < FIT_LIMIT)      # (false for NaN too)
    pts = np.where(fits[:, None], pts, 0.0)
    qx, qy = np.trunc(pts[:, 0]) / (float(real_h) / float(H)), np.trunc(pts[:, 1]) / (float(real_w) / float(W))
    fits &= (np.abs(qx) < FIT_LIMIT) & (np.abs(qy) < FIT_LIMIT)
    nX = np.trunc(np.where(fits, qx, 0.0)).astype(np.int64)
    nY = np.trunc(np.where(fits, qy, 0.0)).astype(np.int64)
    off = np.arange(-n, n + 1)
    # masks at [point, us, vs]
    k = (nY[:, None, None] + off[None, None, :]) * W + (nX[:, None, None] + off[None, :, None])
    ok = (k >= 0) & (k < W * H)
    kc = np.clip(k, 0, W * H - 1)
    mx = ok & (np.asarray(mask_x).reshape(-1)[kc] > 0)
    my = ok & (np.asarray(mask_y).reshape(-1)[kc] > 0)
    us = np.broadcast_to(off[None, :, None], mx.shape)
    vs = np.broadcast_to(off[None, None, :], mx.shape)
    # the loop's updates keep the us / vs nearest to 0 on each side: left = max negative us with a mask (per vs), and so on
    left = np.where(mx & (us < 0), us, -n).max(axis=1)            # [point, vs]
    right = np.where(mx & (us > 0), us, n).min(axis=1)
    up = np.where(my & (vs > 0), vs, n).min(axis=2)               # [point, us]
    bottom = np.where(my & (vs < 0), vs, -n).max(axis=2)
    for s in range(1, n + 1):
        p, q = s + n, -s + n
        up[:, p] = np.minimum(up[:, p], up[:, p - 1])
        up[:, q] = np.minimum(up[:, q], up[:, q + 1])
        bottom[:, p] = np.maximum(bottom[:, p], bottom[:, p - 1])
        bottom[:, q] = np.maximum(bottom[:, q], bottom[:, q + 1])
        left[:, p] = np.maximum(left[:, p], left[:, p - 1])
        left[:, q] = np.maximum(left[:, q], left[:, q + 1])
        right[:, p] = np.minimum(right[:, p], right[:, p - 1])
        right[:, q] = np.minimum(right[:, q], right[:, q + 1])
    U, V = np.meshgrid(off, off, indexing="ij")                    # [u, v]
    ratio = np.array([[_ratio(int(u), int(v)) for v in off] for u in off])
    stored = (ratio * ratio).astype(np.float32)
    for i in np.flatnonzero(fits):
        px, py = nX[i] + U, nY[i] + V
        allowed = ((py < H - 1) & (py >= 1) & (px < W - 1) & (px >= 1) & (U >= left[i][V + n]) & (U <= right[i][V + n]) &
                   (V >= bottom[i][U + n]) & (V <= up[i][U + n]))
        if not allowed.any():
            continue
        yy, xx = py[allowed], px[allowed]
        take = sdist[yy, xx].astype(np.float64) < ratio[allowed]
        sd[yy[take], xx[take]] = np.float32(depths[i])
        sdist[yy[take], xx[take]] = stored[allowed][take]
    return sd, sdist


def resize_f32(src, w, h):
    """cv::resize(CV_32FC1, Size(w, h)) with INTER_LINEAR (:409): float weights, float products and sums"""
    src = np.asarray(src, np.float32)
    h0, w0 = src.shape
    if (w, h) == (w0, h0):
        return src.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if w0 == 2 * w and h0 == 2 * h:
            return (((src[0::2, 0::2] + src[0::2, 1::2]) + src[1::2, 0::2]) + src[1::2, 1::2]) * f32(0.25)
        x0, x1, fx, edge = pd._taps_x(w, w0)
        y0, y1, fy = pd._taps_y(h, h0)
        one = f32(1.0)
        a0, a1, b0, b1 = one - fx, fx, one - fy, fy
        rows = src[:, x0] * a0 + src[:, x1] * a1
        rows[:, edge] = src[:, x0[edge]] * one
        return rows[y0, :] * b0[:, None] + rows[y1, :] * b1[:, None]


class RawStereo:
    """the raw-image path chained into a float-input restatement (stereo_restated.VectorisedStereo or ScalarStereo): the same
    calls as chisel_hip_stereo_set_camera / set_reference_image / update_image / bind_sparse_points / output_image, with every
    intermediate kept (ref, match, p2w, mask_x, mask_y, sparse_depth, sparse_dist, depth_real)"""

    def __init__(self, matcher, W, H):
        self.m, self.W, self.H = matcher, W, H
        self.depths, self.points = np.zeros(0), np.zeros((0, 2))

    def set_camera(self, real_w, real_h, K1, D1, K2, D2):
        self.real_w, self.real_h = real_w, real_h
        self.K1, self.K2 = scale_intrinsics(K1, real_w, real_h, self.W, self.H), scale_intrinsics(K2, real_w, real_h, self.W, self.H)
        self.D1, self.D2 = [float(v) for v in D1], [float(v) for v in D2]

    def set_reference_image(self, raw):
        self.ref = prepare(raw, self.W, self.H, self.K1, self.D1)
        self.p2w, self.mask_x, self.mask_y = reference_maps(self.ref)
        self.m.set_reference(self.ref, self.p2w)

    def update_image(self, raw, ref_pose, match_pose):
        self.match = prepare(raw, self.W, self.H, self.K2, self.D2)
        R, t = homography(self.K1, self.K2, ref_pose[0], ref_pose[1], match_pose[0], match_pose[1])
        self.m.update(self.match, R, t)

    def bind_sparse_points(self, depths, points):
        self.depths, self.points = np.asarray(depths, np.float64), np.asarray(points, np.float64).reshape(-1, 2)

    def output_image(self):
        self.sparse_depth, self.sparse_dist = sparse_maps_vectorised(self.depths, self.points, self.mask_x, self.mask_y, self.W,
                                                                     self.H, self.real_w, self.real_h)
        if len(self.depths):
            self.m.output(self.sparse_depth, self.sparse_dist)
        else:
            self.m.output()
        self.depth_real = resize_f32(self.m.depth, self.real_w, self.real_h)
        return self.depth_real

    def clear(self):
        self.m.clear()

    depth = property(lambda self: self.m.depth)   # the W x H depth map of the last output
