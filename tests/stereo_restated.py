"""CPU restatement of the stereo matcher (StereoMapper, server_pose_graph/src/dense_mapping/calc_cost.cu and
sgm_stereo_mapper.cpp), written from the algorithm for the tests of chisel_hip_stereo_*.  Not a test module.

Two forms of the same computation:
  ScalarStereo      one CUDA thread at a time: ADCalcCostKernel's early `continue`s, sgm2's and filterCostKernel's shared-memory
                    tree reductions, all in np.float32 scalars.  Slow: small images only.
  VectorisedStereo  the same numbers as whole-array float32 numpy, the cost chunked by rows so 640 x 480 x 128 fits in memory.
Both sample the match image bilinearly with exact fp32 weights (the library's stated deviation from the CUDA texture) and read
the reference image on texel centres (0 outside the image, as the texture's border addressing gives).  Every fp32 operation is
the reference's in its order; numpy keeps float32 throughout because every constant here is an np.float32 (NEP 50)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

f32 = np.float32
DEP_CNT = 128                                                    # dense_mapping_parameters.h:28
DEP_SAMPLE = f32(1.0) / (f32(0.11) * f32((461.6 + 460.3) / 2))   # dense_mapping_parameters.h:24,36-37: 0.019722115f
DEP_INF = f32(1000.0)                                            # dense_mapping_parameters.h:50
THREADS = max(1, min(8, os.cpu_count() or 1))  # the vectorised cost's row chunks run side by side
DEFAULTS = dict(pi1=16.0, pi2=64.0, tau_so=8.0, sgm_q1=1.0, sgm_q2=1.0, var_scale=1.0, sparse_ratio=15.0, dep_sample=float(DEP_SAMPLE))

# ADCalcCostKernel's nine taps in its order (calc_cost.cu:96-221): the reference-image offset each reads.  u and d read the
# reference image mirrored against the match-image homography (:121, :135).
TAP_REF_OFFSETS = ((0, 0), (0, 1), (0, -1), (-1, 0), (1, 0), (-1, -1), (1, 1), (-1, 1), (1, -1))


def tap_numerators(R, X, Y):
    """homography rows of the nine taps at pixel (X, Y) (arrays or scalars, float32), calc_cost.cu:39-73, quirks included:
    tap r takes y and z from the x row, tap ru takes them from xr (:56-57, :72-73)"""
    r11, r12, r13, r21, r22, r23, r31, r32, r33 = (f32(v) for v in np.asarray(R, np.float32).reshape(9))
    x = r11 * X + r12 * Y + r13 * f32(1.0)
    y = r21 * X + r22 * Y + r23 * f32(1.0)
    z = r31 * X + r32 * Y + r33 * f32(1.0)
    xu, yu, zu = x - r12, y - r22, z - r32
    xd, yd, zd = x + r12, y + r22, z + r32
    xl, yl, zl = x - r11, y - r21, z - r31
    xr, yr, zr = x + r11, x + r21, x + r31
    return [(x, y, z), (xu, yu, zu), (xd, yd, zd), (xl, yl, zl), (xr, yr, zr), (xu - r11, yu - r21, zu - r31),
            (xd + r11, yd + r21, zd + r31), (xl + r12, yl + r22, zl + r32), (xr - r12, xr - r22, xr - r32)]


def tree_argmin(c):
    """filterCostKernel's reduction (calc_cost.cu:254-262) over the last axis of a (..., 128) float32 array -> (min, index).
    Strict '<' at every level: among equal minima the index with the smallest bit-reversed value wins (1 vs 2 -> 2)."""
    cm = np.array(c, np.float32, copy=True)
    ci = np.broadcast_to(np.arange(DEP_CNT), cm.shape).copy()
    i = DEP_CNT // 2
    while i > 0:
        take = cm[..., i:2 * i] < cm[..., :i]
        cm[..., :i] = np.where(take, cm[..., i:2 * i], cm[..., :i])
        ci[..., :i] = np.where(take, ci[..., i:2 * i], ci[..., :i])
        i //= 2
    return cm[..., 0], ci[..., 0]


def same_bits(a, b):
    """bit-equality of float arrays, NaN == NaN whatever its sign or payload (x86 and the GPU make different default NaNs)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8 if a.dtype.itemsize == 1 else a.dtype.str.replace("f", "u")),
                                                          b[~nb].view(np.uint8 if b.dtype.itemsize == 1 else b.dtype.str.replace("f", "u"))))


class _Base:
    def __init__(self, width, height, **params):
        p = dict(DEFAULTS)
        p.update(params)
        self.W, self.H = int(width), int(height)
        self.p = {k: f32(v) for k, v in p.items()}
        self.count = 0
        self.ref = np.zeros((self.H, self.W), np.float32)
        self.p2w = np.zeros((self.H, self.W), np.float32)
        self.cost = np.zeros((self.H, self.W, DEP_CNT), np.float32)
        self.sgm = np.zeros_like(self.cost)
        self.depth = np.zeros((self.H, self.W), np.float32)

    def set_reference(self, ref, p2_weight):          # InitReference, sgm_stereo_mapper.cpp:55-123
        self.ref = np.ascontiguousarray(ref, np.float32).copy()
        self.p2w = np.ascontiguousarray(p2_weight, np.float32).copy()
        self.count = 0

    def clear(self):                                  # ClearRawCost, :202-216 (the count stays)
        self.cost[:] = 0
        self.sgm[:] = 0
        self.depth[:] = 0

    def update(self, match, R, t):                    # Update, :125-199
        self.count += 1
        self._cost(np.ascontiguousarray(match, np.float32), np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3))

    def output(self, sparse_depth=None, sparse_dist=None):   # Output, :219-385
        if sparse_depth is not None:
            self._fuse(np.asarray(sparse_depth, np.float32), np.asarray(sparse_dist, np.float32))
        self.sgm[:] = 0                               # :371
        self._sgm()
        self._wta()
        return self.depth


# ---------------------------------------------------------------------------------------------------------------------------
class ScalarStereo(_Base):
    """per-thread restatement: loops over (pixel, depth) and over the 128 threads of a block"""

    def _texel(self, img, i, j):
        return img[j, i] if 0 <= i < self.W and 0 <= j < self.H else f32(0.0)

    def _sample(self, img, u, v):
        if np.isnan(u) or np.isnan(v):
            return f32(0.0)
        fu, fv = np.floor(u), np.floor(v)
        i, j = int(fu), int(fv)
        a, b = u - fu, v - fv
        one = f32(1.0)
        return ((one - a) * (one - b) * self._texel(img, i, j) + a * (one - b) * self._texel(img, i + 1, j)
                + (one - a) * b * self._texel(img, i, j + 1) + a * b * self._texel(img, i + 1, j + 1))

    def _cost(self, match, R, t):
        W, H, cnt = self.W, self.H, self.count
        t1, t2, t3 = (f32(v) for v in t)
        wmax, hmax = f32(W - 1), f32(H - 1)
        for tidy in range(H):
            for tidx in range(W):
                taps = tap_numerators(R, f32(tidx), f32(tidy))
                for i in range(DEP_CNT):
                    if cnt == 1 and (tidx == 0 or tidx == W - 1 or tidy == 0 or tidy == H - 1):
                        self.cost[tidy, tidx, i] = -1.0
                        continue
                    last = self.cost[tidy, tidx, i]
                    if cnt != 1 and last < 0:
                        continue
                    tmp = f32(0.0)
                    idep = f32(i) * self.p["dep_sample"]
                    bad = False
                    for (hx, hy, hz), (ox, oy) in zip(taps, TAP_REF_OFFSETS):
                        w = hz + t3 * idep
                        u = (hx + t1 * idep) / w
                        v = (hy + t2 * idep) / w
                        if w < 0 or u < 0 or u > wmax or v < 0 or v > hmax:
                            bad = True
                            break
                        tmp += abs(self._texel(self.ref, tidx + ox, tidy + oy) - self._sample(match, u, v) - f32(0.0))
                    if bad:
                        self.cost[tidy, tidx, i] = -1.0
                    elif cnt == 1:
                        self.cost[tidy, tidx, i] = tmp / f32(9.0)
                    else:
                        self.cost[tidy, tidx, i] = (last * f32(cnt - 1) + tmp / f32(9.0)) / f32(cnt)

    def _fuse(self, sd, sdist):
        ds, ratio = self.p["dep_sample"], self.p["sparse_ratio"]
        for y in range(self.H):
            for x in range(self.W):
                nDepth, nDist = sd[y, x], sdist[y, x]
                if not float(nDepth) > 0.0:
                    continue
                inv = f32(1.0 / float(nDepth))        # a double division, narrowed (calc_cost.cu:697)
                for d in range(DEP_CNT):
                    cur = ds * f32(d)
                    diff = inv - cur if cur < inv else -inv + cur
                    diff = diff / ds
                    if float(self.cost[y, x, d]) > 0.0:
                        self.cost[y, x, d] = self.cost[y, x, d] + diff * ratio * nDist

    def _tree_min(self, a):
        a = list(a)
        i = DEP_CNT // 2
        while i > 0:
            for d in range(i):
                if a[d + i] < a[d]:
                    a[d] = a[d + i]
            i //= 2
        return a[0]

    def _sgm(self):
        W, H, p = self.W, self.H, self.p
        passes = ((0, 0, 1, 0, W, H), (0, W - 1, -1, 0, W, H), (1, 0, 0, 1, H, W), (1, H - 1, 0, -1, H, W))  # sgm2<idx, start, dx, dy, n>
        for idx, start, dx, dy, n, blocks in passes:
            for blk in range(blocks):
                xy = [blk, blk]
                xy[idx] = start
                x, y = xy
                inp = [self.cost[y, x, d] for d in range(DEP_CNT)]
                if self._tree_min(inp) < 0:
                    inp = [f32(0.0)] * DEP_CNT
                    for d in range(DEP_CNT):
                        self.sgm[y, x, d] = 0.0
                else:
                    for d in range(DEP_CNT):
                        self.sgm[y, x, d] = self.sgm[y, x, d] + inp[d]
                out_s = list(inp)
                for _ in range(1, n):
                    x, y = x + dx, y + dy
                    inp = [self.cost[y, x, d] for d in range(DEP_CNT)]
                    out_min = self._tree_min(out_s)
                    invalid = self._tree_min(inp) < 0
                    if invalid:
                        inp = [f32(0.0)] * DEP_CNT
                    D1 = abs(self.ref[y, x] - self.ref[y - dy, x - dx])
                    P1, P2 = p["pi1"], p["pi2"]
                    if D1 < p["tau_so"]:
                        P1 = P1 / p["sgm_q1"]
                        P2 = P2 / p["sgm_q2"]
                        P2 = P2 * self.p2w[y, x]
                    val = []
                    for d in range(DEP_CNT):
                        c = min(out_s[d], out_min + P2)
                        if d - 1 >= 0:
                            c = min(c, out_s[d - 1] + P1)
                        if d + 1 < DEP_CNT:
                            c = min(c, out_s[d + 1] + P1)
                        v = inp[d] + c - out_min
                        self.sgm[y, x, d] = 0.0 if invalid else self.sgm[y, x, d] + v
                        val.append(v)
                    out_s = val

    def _wta(self):
        p = self.p
        for y in range(self.H):
            for x in range(self.W):
                c = [self.sgm[y, x, d] for d in range(DEP_CNT)]
                c_min, c_idx = list(c), list(range(DEP_CNT))
                i = 64
                while i > 0:
                    for d in range(i):
                        if d + i < DEP_CNT and c_min[d + i] < c_min[d]:
                            c_min[d], c_idx[d] = c_min[d + i], c_idx[d + i]
                    i //= 2
                mc, mi = c_min[0], c_idx[0]
                if mc == 0 or mi == 0 or mi == DEP_CNT - 1 or c[mi - 1] + c[mi + 1] < f32(2) * mc * p["var_scale"]:
                    self.depth[y, x] = DEP_INF
                else:
                    pre, post = c[mi - 1], c[mi + 1]
                    a = pre - f32(2.0) * mc + post
                    b = -pre + post
                    with np.errstate(all="ignore"):
                        sub = f32(mi) - b / (f32(2.0) * a)
                        self.depth[y, x] = f32(1.0) / (sub * p["dep_sample"])

    def update(self, match, R, t):
        with np.errstate(all="ignore"):
            super().update(match, R, t)


# ---------------------------------------------------------------------------------------------------------------------------
class VectorisedStereo(_Base):
    """whole-array float32 form of the same computation"""
    ROWS = 16  # cost rows per chunk: 16 x 640 x 128 entries

    def __init__(self, width, height, **params):
        super().__init__(width, height, **params)

    @staticmethod
    def _padded(img):
        P = np.zeros((img.shape[0] + 2, img.shape[1] + 2), np.float32)
        P[1:-1, 1:-1] = img
        return P

    def _sample(self, Pm, u, v):
        """bilinear fp32 sample of the zero-padded match image Pm at (u, v), each within [-1, W] x [-1, H] or NaN"""
        nan = np.isnan(u) | np.isnan(v)
        u = np.where(nan, f32(0.0), u)
        v = np.where(nan, f32(0.0), v)
        fu, fv = np.floor(u), np.floor(v)
        i, j = fu.astype(np.int64) + 1, fv.astype(np.int64) + 1
        a, b = u - fu, v - fv
        one = f32(1.0)
        i1, j1 = np.minimum(i + 1, Pm.shape[1] - 1), np.minimum(j + 1, Pm.shape[0] - 1)
        s = (one - a) * (one - b) * Pm[j, i] + a * (one - b) * Pm[j, i1] + (one - a) * b * Pm[j1, i] + a * b * Pm[j1, i1]
        return np.where(nan, f32(0.0), s)

    def _cost(self, match, R, t):
        Pm, Pr = self._padded(match), self._padded(self.ref)
        idep = np.arange(DEP_CNT, dtype=np.float32) * self.p["dep_sample"]
        tt = [f32(v) * idep for v in t]
        chunks = range(0, self.H, self.ROWS)
        with ThreadPoolExecutor(THREADS) as ex:   # row chunks are independent; numpy releases the GIL
            list(ex.map(lambda y0: self._cost_rows(y0, Pm, Pr, R, tt), chunks))

    def _cost_rows(self, y0, Pm, Pr, R, tt):
        W, H, cnt = self.W, self.H, self.count
        t1, t2, t3 = tt
        wmax, hmax = f32(W - 1), f32(H - 1)
        ys = np.arange(y0, min(H, y0 + self.ROWS))
        Xg, Yg = np.meshgrid(np.arange(W, dtype=np.float32), ys.astype(np.float32))
        taps = tap_numerators(R, Xg, Yg)
        tmp = np.zeros((len(ys), W, DEP_CNT), np.float32)
        bad = np.zeros(tmp.shape, bool)
        with np.errstate(all="ignore"):
            for (hx, hy, hz), (ox, oy) in zip(taps, TAP_REF_OFFSETS):
                w = hz[..., None] + t3
                u = (hx[..., None] + t1) / w
                v = (hy[..., None] + t2) / w
                bad |= (w < 0) | (u < 0) | (u > wmax) | (v < 0) | (v > hmax)
                u = np.where(bad, f32(0.0), u)           # entries already -1: any in-range position will do
                v = np.where(bad, f32(0.0), v)
                left = Pr[ys[:, None] + oy + 1, np.arange(W)[None, :] + ox + 1][..., None]
                tmp = tmp + np.abs(left - self._sample(Pm, u, v) - f32(0.0))
        last = self.cost[y0:y0 + len(ys)]
        if cnt == 1:
            new = np.where(bad, f32(-1.0), tmp / f32(9.0))
            border = np.zeros((len(ys), W), bool)
            border[:, 0] = border[:, W - 1] = True
            border[ys == 0] = True
            border[ys == H - 1] = True
            new[border] = -1.0
        else:
            mean = (last * f32(cnt - 1) + tmp / f32(9.0)) / f32(cnt)
            new = np.where(last < 0, last, np.where(bad, f32(-1.0), mean))
        self.cost[y0:y0 + len(ys)] = new

    def _fuse(self, sd, sdist):
        ds, ratio = self.p["dep_sample"], self.p["sparse_ratio"]
        has = sd > 0
        with np.errstate(all="ignore"):
            inv = (1.0 / sd.astype(np.float64)).astype(np.float32)[..., None]
        cur = ds * np.arange(DEP_CNT, dtype=np.float32)
        diff = np.where(cur < inv, inv - cur, -inv + cur) / ds
        add = diff * ratio * sdist[..., None]
        upd = has[..., None] & (self.cost > 0)
        self.cost[upd] = (self.cost + add)[upd]

    def _lines(self, idx):
        """per scan step the (lines, 128) slice views of cost / sgm and the pixels it touches"""
        if idx == 0:   # horizontal passes: a step is a column
            return lambda vol, s: vol[:, s]
        return lambda vol, s: vol[s]

    def _sgm(self):
        W, H, p = self.W, self.H, self.p
        passes = ((0, 0, 1, 0, W), (0, W - 1, -1, 0, W), (1, 0, 0, 1, H), (1, H - 1, 0, -1, H))
        for idx, start, dx, dy, n in passes:
            sl = self._lines(idx)
            step = dx if idx == 0 else dy
            prev = None
            for k in range(n):
                s = start + k * step
                inp = sl(self.cost, s).copy()
                invalid = inp.min(axis=1) < 0
                inp[invalid] = 0.0
                if k == 0:
                    val = inp
                else:
                    m = prev.min(axis=1, keepdims=True)
                    D1 = np.abs(sl(self.ref, s) - sl(self.ref, s - step))
                    g = sl(self.p2w, s)
                    soft = D1 < p["tau_so"]
                    P1 = np.where(soft, p["pi1"] / p["sgm_q1"], p["pi1"]).astype(np.float32)[:, None]
                    P2 = np.where(soft, p["pi2"] / p["sgm_q2"] * g, p["pi2"]).astype(np.float32)[:, None]
                    c = np.minimum(prev, m + P2)
                    c[:, 1:] = np.minimum(c[:, 1:], prev[:, :-1] + P1)
                    c[:, :-1] = np.minimum(c[:, :-1], prev[:, 1:] + P1)
                    val = inp + c - m
                out = sl(self.sgm, s)
                out[:] = np.where(invalid[:, None], f32(0.0), out + val)
                prev = val

    def _wta(self):
        p = self.p
        c = self.sgm.reshape(-1, DEP_CNT)
        mc, mi = tree_argmin(c)
        rows = np.arange(c.shape[0])
        pre = c[rows, np.clip(mi - 1, 0, DEP_CNT - 1)]
        post = c[rows, np.clip(mi + 1, 0, DEP_CNT - 1)]
        reject = (mc == 0) | (mi == 0) | (mi == DEP_CNT - 1) | (pre + post < f32(2) * mc * p["var_scale"])
        with np.errstate(all="ignore"):
            a = pre - f32(2.0) * mc + post
            b = -pre + post
            sub = mi.astype(np.float32) - b / (f32(2.0) * a)
            dep = f32(1.0) / (sub * p["dep_sample"])
        self.depth = np.where(reject, DEP_INF, dep).astype(np.float32).reshape(self.H, self.W)
