"""Inputs that drive the stereo matcher (kernels_stereo.h) and its raw-image preparation (kernels_stereo_prep.h) into the
branches that random textures, random poses and default parameters never reach: WTA ties, the variance rejection, the soft
SGM penalties with non-default parameters, homographies whose denominator is negative or exactly zero, sparse depths at 0, -0,
inf, NaN, a denormal and the largest float, a cost of exactly 0 under a prior, twelve measurements, and point sets at the
rasteriser's chunk boundaries, piled on one pixel or placed where no int holds them.  Not a test module and not a conftest:
tests/test_stereo_cases.py asserts on the CPU restatement alone that every input reaches its branch, and the GPU tests
(test_gpu_stereo_edges.py, test_gpu_stereo_prep_edges.py) compare the library with the restatement on the same inputs.

A float-path case is a script of the restatement's calls (stereo_restated._Base): run_case() plays it on any object with that
interface and returns every state it passes through."""
import numpy as np

import stereo_restated as sr
from test_stereo_restated import random_pose, scene

f32 = np.float32
DS64 = 2.0 ** -6                       # a dep_sample whose multiples 0 .. 127 are exact, so i * dep_sample carries no rounding
IDENTITY = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))


class Case:
    def __init__(self, name, W, H, params, steps, **notes):
        self.name, self.W, self.H, self.params, self.steps = name, W, H, dict(params), steps
        self.__dict__.update(notes)

    def __repr__(self):
        return "%s-%dx%d" % (self.name, self.W, self.H)


def run_case(factory, case, upto=None):
    """plays case.steps on factory(W, H, **params) -> [(name, array)]: the cost after every update, and the cost (the prior is
    fused into it), the SGM volume and the depth after every output"""
    s = factory(case.W, case.H, **case.params)
    states = []
    for op in case.steps[:upto]:
        if op[0] == "ref":
            s.set_reference(op[1], op[2])
        elif op[0] == "update":
            s.update(op[1], op[2], op[3])
            states.append(("cost", np.array(s.cost, copy=True)))
        elif op[0] == "clear":
            s.clear()
        elif op[0] == "output":
            with np.errstate(invalid="ignore", over="ignore"):      # (prior_edges: 1 / denormal = inf, then inf - inf, are meant)
                s.output(*op[1:])
            states += [("cost", np.array(s.cost, copy=True)), ("sgm", np.array(s.sgm, copy=True)), ("depth", np.array(s.depth, copy=True))]
        else:
            raise ValueError(op[0])
    return states


def last(states, name):
    return [x for n, x in states if n == name][-1]


def _textures(rng, W, H):
    ref = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    match = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    p2w = (0.8 + rng.uniform(0.0, 1.5, (H, W))).astype(np.float32)
    return ref, match, p2w


# ---- (a) WTA ties --------------------------------------------------------------------------------------------------------------
TIE_ODD, TIE_EVEN = (1, 5, 63, 125), (2, 64, 100)
TIE_EDGE = 0     # a tie of depths 0 and 1: the tree keeps 0, which filterCostKernel rejects; any rule that takes 1 accepts it


def tie_depth(k):
    """the sparse depth 64 / (k + 0.5) as float32, checked to invert to exactly (k + 0.5) / 64: with dep_sample = 2^-6 the
    prior's |1 / depth - d / 64| * 64 is then exactly |k + 0.5 - d|, equal at d = k and d = k + 1"""
    sd = f32(64.0 / (k + 0.5))
    assert (f32(1.0) / sd) * f32(64.0) == f32(k + 0.5), k
    assert (1.0 / np.float64(sd)).astype(np.float32) == f32(1.0) / sd
    return sd


def ties(W, H, k, seed=1):
    """R = identity and t = 0: every hypothesis samples the same positions, so a pixel's cost is one value 128 times.  The prior
    (one depth everywhere, a per-pixel distance) then puts the minimum on the pair (k, k + 1), exactly tied."""
    rng = np.random.default_rng(seed)
    ref, match, p2w = _textures(rng, W, H)
    sd = np.full((H, W), tie_depth(k), np.float32)
    dist = rng.uniform(0.05, 1.0, (H, W)).astype(np.float32)
    steps = [("ref", ref, p2w), ("update", match) + IDENTITY, ("output", sd, dist)]
    return Case("ties-k%d" % k, W, H, dict(dep_sample=DS64), steps, k=k)


# Adjacent ties cannot tell two tie-breaks apart by the DEPTH: with c[k] == c[k + 1] == min the parabola's vertex is k + 1/2
# from either index ((k + 1) - 1/2 or k + 1/2).  The split ties below put the two equal minima eight indices apart.
SPLIT_UPPER, SPLIT_LOWER = (16, 64, 96), (8, 24)      # centres m where the tree takes m + 4 / takes m - 4 (a first minimum: m - 4)


def split_ties(W, H, m, seed=2):
    """R = identity, t = (8, 0, 0) and dep_sample = 2^-6: hypothesis d samples the match image at x + d / 8.  Its columns
    alternate 0, 128 (rows 0 and 1, which the quirky taps r and ru read, are 0), so every tap's sample is a triangle wave in d,
    exact in fp32 and even about every multiple of 8; the reference is 64 +- 8.  The cost of a pixel is then even about m, with
    dips at m +- 4, m +- 12, ...; the prior (depth 64 / m everywhere, sparse_ratio 2) adds |m - d| * 2 * dist, which leaves the
    pair m - 4, m + 4 as the minimum, exactly tied; the SGM's operations are the same at d and 2 m - d, so its volume stays even about m and the tie survives it."""
    assert m % 8 == 0 and (f32(1.0) / f32(64.0 / m)) * f32(64.0) == f32(m)
    rng = np.random.default_rng(seed)
    match = np.broadcast_to(np.where(np.arange(W) % 2 == 0, 0.0, 128.0), (H, W)).astype(np.float32).copy()
    match[:2] = 0.0
    ref = (64 + rng.integers(-8, 9, (H, W))).astype(np.float32)
    p2w = (0.8 + rng.uniform(0.0, 1.5, (H, W))).astype(np.float32)
    sd = np.full((H, W), f32(64.0 / m), np.float32)
    dist = rng.uniform(0.05, 1.0, (H, W)).astype(np.float32)
    steps = [("ref", ref, p2w), ("update", match, np.eye(3, dtype=np.float32), np.array([8.0, 0.0, 0.0], np.float32)), ("output", sd, dist)]
    return Case("split-m%d" % m, W, H, dict(dep_sample=DS64, sparse_ratio=2.0), steps, m=m)


def wta_with(argmin, sgm, params):
    """filterCostKernel's accept / reject and parabola (calc_cost.cu:264-281) on top of any (min, index) rule, as
    VectorisedStereo._wta computes it -> (depth, min, index, index accepted)"""
    p = {k: f32(v) for k, v in dict(sr.DEFAULTS, **params).items()}
    c = sgm.reshape(-1, sr.DEP_CNT)
    mc, mi = argmin(c)
    rows = np.arange(c.shape[0])
    pre, post = c[rows, np.clip(mi - 1, 0, 127)], c[rows, np.clip(mi + 1, 0, 127)]
    reject = (mc == 0) | (mi == 0) | (mi == 127) | (pre + post < f32(2) * mc * p["var_scale"])
    with np.errstate(all="ignore"):
        sub = mi.astype(np.float32) - (-pre + post) / (f32(2.0) * (pre - f32(2.0) * mc + post))
        dep = f32(1.0) / (sub * p["dep_sample"])
    shape = sgm.shape[:2]
    return np.where(reject, sr.DEP_INF, dep).astype(np.float32).reshape(shape), mc.reshape(shape), mi.reshape(shape), ~reject.reshape(shape)


def first_argmin(c):
    """the rule the tree is NOT: the first of equal minima"""
    mi = np.argmin(c, axis=-1)
    return np.take_along_axis(c, mi[..., None], axis=-1)[..., 0], mi


# ---- (b) the variance rejection ------------------------------------------------------------------------------------------------
VAR_SCALE = 1.02


def variance(W, H, seed=7, var_scale=VAR_SCALE):
    """the random scene of test_stereo_restated after three updates, with a var_scale above 1: pre + post < 2 min var_scale now
    rejects the shallow minima and keeps the deep ones"""
    ref, match, p2w, _, _ = scene(W, H, seed)
    steps = [("ref", ref, p2w)]
    for k in range(3):
        steps.append(("update", np.roll(match, k, axis=1) + f32(k)) + tuple(random_pose(W, H, seed * 10 + k)))
    steps.append(("output",))
    return Case("variance", W, H, dict(var_scale=var_scale), steps)


# ---- (c) a smooth reference and non-default SGM parameters --------------------------------------------------------------------------
SGM_SETS = (
    dict(pi1=10.0, pi2=40.0, tau_so=5.0, sgm_q1=2.0, sgm_q2=3.0, sparse_ratio=7.0, dep_sample=DS64),
    dict(pi1=24.0, pi2=96.0, tau_so=12.0, sgm_q1=0.75, sgm_q2=0.4, sparse_ratio=22.5, dep_sample=0.0173),
    dict(pi1=20.0, pi2=50.0, tau_so=6.5, sgm_q1=-2.0, sgm_q2=1.5, sparse_ratio=7.0, dep_sample=DS64),   # a negative q: P1 < 0
)
SGM_NEUTRAL = dict(pi1=16.0, pi2=64.0, tau_so=8.0, sgm_q1=1.0, sgm_q2=1.0)   # the defaults these sets move away from


def smooth(W, H, params, seed=5):
    """a reference image that is a gentle ramp (neighbour differences 3 and 2, below every tau_so used) with one pixel in
    eight lifted by 40 .. 120, so both sides of `D1 < tau_so` are taken on every scanline; two updates and a sparse prior"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    ref = (20.0 + (3.0 * x + 2.0 * y) % 96.0 + np.where(rng.random((H, W)) < 0.125, rng.uniform(40.0, 120.0, (H, W)), 0.0)).astype(np.float32)
    match = (ref * f32(0.9) + rng.uniform(0.0, 25.0, (H, W)).astype(np.float32)).astype(np.float32)
    _, _, p2w, sd, dist = scene(W, H, seed)
    steps = [("ref", ref, p2w)]
    for k in range(2):
        steps.append(("update", np.roll(match, k + 1, axis=1)) + tuple(random_pose(W, H, seed * 10 + k, shift=0.05)))
    steps.append(("output", sd, dist))
    return Case("smooth", W, H, params, steps, ref=ref)


# ---- (d) degenerate homographies --------------------------------------------------------------------------------------------------
# small integers, dep_sample = 2^-6: every numerator and denominator is exact, so the zeros are exact zeros.
#   pose 0: w = x + y plus the taps' offsets, t = 0: the zeros and the sign changes sit on the image's diagonals.  tap_report
#           counts what the pose reaches rather than arguing it.
#   pose 1: t3 = -2, so w = 1 - d / 32 changes sign at depth index 32 at every pixel; t1 and t2 keep u and v inside the image
#           beyond it, which leaves `w < 0` as the only reason to reject.
DEGENERATE_POSES = (
    (np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32), np.zeros(3, np.float32)),
    (np.eye(3, dtype=np.float32), np.array([-16.0, -12.0, -2.0], np.float32)),
)


def degenerate(W, H, pose, seed=9):
    rng = np.random.default_rng(seed)
    ref, match, p2w = _textures(rng, W, H)
    R, t = DEGENERATE_POSES[pose]
    # a second update with the same pose runs the `count != 1` form of the same divisions (entries at -1 stay); the update after
    # a ClearRawCost meets a zeroed cost whose border is unmarked, so the border pixels' taps are evaluated as well
    steps = [("ref", ref, p2w), ("update", match, R, t), ("update", np.roll(match, 1, axis=0), R, t), ("clear",),
             ("update", np.roll(match, 2, axis=1), R, t), ("output",)]
    return Case("degenerate%d" % pose, W, H, dict(dep_sample=DS64), steps, R=R, t=t)


def tap_report(R, t, W, H, dep_sample, border=False):
    """what ADCalcCostKernel's nine taps meet at every (pixel, depth) that an update evaluates -- the interior for a first update,
    the border too (border=True) for one on a cleared cost -- taps taken in order until the first that rejects
    (calc_cost.cu:96-221) -> counts:
      valid        entries that keep a cost
      nan_valid    valid entries one of whose taps had a NaN coordinate (0 / 0: the sample reads 0)
      w_only       entries whose rejecting tap had w < 0 and both coordinates inside the image
      w_zero       entries whose rejecting tap had w == 0 with a non-zero numerator (+-inf)
      w_negative   entries that evaluated a tap with w < 0 at all"""
    Xg, Yg = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    idep = np.arange(sr.DEP_CNT, dtype=np.float32) * f32(dep_sample)
    t1, t2, t3 = (f32(v) * idep for v in t)
    wmax, hmax = f32(W - 1), f32(H - 1)
    shape = (H, W, sr.DEP_CNT)
    bad, nan_used, w_only, w_zero, w_neg = (np.zeros(shape, bool) for _ in range(5))
    with np.errstate(all="ignore"):
        for hx, hy, hz in sr.tap_numerators(R, Xg, Yg):
            w, nx, ny = hz[..., None] + t3, hx[..., None] + t1, hy[..., None] + t2
            u, v = nx / w, ny / w
            outside = (u < 0) | (u > wmax) | (v < 0) | (v > hmax)
            live = ~bad
            w_only |= live & (w < 0) & ~outside
            w_neg |= live & (w < 0)
            w_zero |= live & (w == 0) & ((nx != 0) | (ny != 0)) & outside
            nan_used |= live & ~(w < 0) & ~outside & (np.isnan(u) | np.isnan(v))
            bad |= (w < 0) | outside
    inner = np.ones(shape, bool) if border else np.zeros(shape, bool)
    inner[1:-1, 1:-1] = True
    return dict(valid=int((~bad & inner).sum()), nan_valid=int((nan_used & ~bad & inner).sum()), w_only=int((w_only & inner).sum()),
                w_zero=int((w_zero & inner).sum()), w_negative=int((w_neg & inner).sum()), entries=int(inner.sum()))


# ---- (e) the prior's edge values -------------------------------------------------------------------------------------------------
PRIOR_CLASSES = ("zero", "minus_zero", "inf", "nan", "denormal", "largest", "negative", "ordinary")
PRIOR_VALUES = dict(zero=f32(0.0), minus_zero=f32(-0.0), inf=f32(np.inf), nan=f32(np.nan), denormal=f32(1e-40),
                    largest=np.finfo(np.float32).max, negative=f32(-2.5), ordinary=f32(1.75))


def prior_edges(W, H, seed=13):
    """the left half of both images is 0 and R = identity, t = 0: there every tap reads equal values, and the interior costs are
    exact zeros; the right half is random.  After a ClearRawCost the second update (count 2) unmarks the border.  The prior
    puts every class of sparse depth on pixels of both halves, each with a distance > 0.  A denormal depth inverts to +inf
    (a double division narrowed to float) and makes every positive cost of its pixel +inf; the SGM turns such a pixel into NaN
    for the rest of its four scanlines -- all 128 entries alike, so no minimum depends on the order of its operands."""
    rng = np.random.default_rng(seed)
    ref, match, p2w = _textures(rng, W, H)
    half = W // 2
    ref[:, :half] = 0.0
    match[:, :half] = 0.0
    sd = np.full((H, W), -1.0, np.float32)
    dist = rng.uniform(0.1, 1.0, (H, W)).astype(np.float32)
    where = {}
    for n, name in enumerate(PRIOR_CLASSES):
        # two columns of the zero half and two of the random half per class, every third row; the denormal on two pixels only
        cols = [1 + n % (half - 2), half + 1 + n % (W - half - 2)]
        rows = np.arange(1 + n % 3, H - 1, 3)
        if name == "denormal":
            rows = rows[:1]
        m = np.zeros((H, W), bool)
        m[np.ix_(rows, cols)] = True
        m &= sd == -1.0
        sd[m] = PRIOR_VALUES[name]
        where[name] = m
    steps = [("ref", ref, p2w), ("update", match) + IDENTITY, ("clear",), ("update", match) + IDENTITY, ("output", sd, dist)]
    return Case("prior-edges", W, H, dict(dep_sample=DS64), steps, where=where, half=half, sd=sd, dist=dist)


# ---- (f) twelve measurements ------------------------------------------------------------------------------------------------------
def count12(W, H, seed=17):
    """twelve updates on one reference, ClearRawCost after the seventh: counts 2 .. 7 average into the cost, 8 .. 12 into a
    zeroed one (the count stays, sgm_stereo_mapper.cpp:202-216)"""
    ref, match, p2w, sd, dist = scene(W, H, seed)
    rng = np.random.default_rng(seed + 1)
    steps = [("ref", ref, p2w)]
    for k in range(12):
        img = np.roll(match, k, axis=k % 2) * f32(0.95) + rng.uniform(0, 8, match.shape).astype(np.float32)
        steps.append(("update", img) + tuple(random_pose(W, H, seed * 20 + k, shift=0.03)))
        if k == 6:
            steps.append(("clear",))
    steps.append(("output", sd, dist))
    return Case("count12", W, H, {}, steps)


def float_cases(W, H):
    """every float-path case at one work size"""
    return ([ties(W, H, k) for k in TIE_ODD + TIE_EVEN + (TIE_EDGE,)] + [split_ties(W, H, m) for m in SPLIT_UPPER + SPLIT_LOWER] + [variance(W, H)] + [smooth(W, H, p) for p in SGM_SETS] +
            [degenerate(W, H, 0), degenerate(W, H, 1), prior_edges(W, H), count12(W, H)])


# ---- (g) point sets for the raw path ------------------------------------------------------------------------------------------------
CHUNK = 256                                      # stereo_sparse_raster_kernel scans the points in chunks of this many
COUNTS = (0, 1, 255, 256, 257, 513)
PILE_OFFSETS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def ordinary_points(rng, n, real_w, real_h):
    return rng.uniform(0.8, 6.0, n), np.stack([rng.uniform(-3, real_w + 3, n), rng.uniform(-3, real_h + 3, n)], axis=1)


def quiet_pixel(mask_x, mask_y):
    """the interior pixel (x, y) with the fewest gradient-mask pixels within 6 of it: a point's window around it is least cut"""
    m = (np.asarray(mask_x) > 0).astype(np.int64) + (np.asarray(mask_y) > 0)
    H, W = m.shape
    c = np.pad(m, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
    r = 6
    ys, xs = np.arange(r + 2, H - r - 2), np.arange(r + 2, W - r - 2)
    box = c[ys[:, None] + r + 1, xs[None, :] + r + 1] - c[ys[:, None] - r, xs[None, :] + r + 1] - c[ys[:, None] + r + 1, xs[None, :] - r] + \
        c[ys[:, None] - r, xs[None, :] - r]
    j, i = np.unravel_index(np.argmin(box), box.shape)
    return int(xs[i]), int(ys[j])


def pile_steps(W, H, real_w, real_h):
    """the spacing of the work pixels that camera positions can reach: 1 unless the camera is smaller than the work image (a scale
    below 1 skips pixels)"""
    sx, sy = float(real_h) / float(H), float(real_w) / float(W)
    return max(1, int(np.ceil(1.0 / sx - 1e-9))), max(1, int(np.ceil(1.0 / sy - 1e-9)))


def to_real(px, py, frac, W, H, real_w, real_h):
    """a camera-image position that Output's (int) and its swapped scales (x by realH / H, y by realW / W) bring to work pixel
    (px, py); frac in [0.2, 0.8) moves it inside that camera pixel"""
    sx, sy = float(real_h) / float(H), float(real_w) / float(W)
    x, y = np.ceil(px * sx) + frac, np.ceil(py * sy) + frac
    assert (np.trunc(np.trunc(x) / sx) == px).all() and (np.trunc(np.trunc(y) / sy) == py).all(), "work pixel out of the camera's reach"
    return np.stack([x, y], axis=-1)


def pile(centre, W, H, real_w, real_h, n=320, seed=23):
    """-> (depths, points, the piled pixel): n >= 300 points, each one reachable pixel (straight or diagonal; two work pixels where
    the camera is half the work size) away from the pixel at or next to `centre`, with distinct depths and positions.  At that
    pixel their ratios are 0.678 or 0.5625 and the stored squares at most 0.459 (0.418, 0.25 and 0.175 at two pixels), so every
    point overwrites the one before: the pixel ends with the LAST point's depth, a point of the second chunk, and any other order
    of the chunks ends elsewhere."""
    rng = np.random.default_rng(seed)
    assert n > CHUNK + 32
    kx, ky = pile_steps(W, H, real_w, real_h)
    assert kx <= 2 and ky <= 2
    cx, cy = centre[0] - centre[0] % kx, centre[1] - centre[1] % ky
    off = np.array(PILE_OFFSETS)[rng.integers(0, 8, n)] * (kx, ky)
    frac = 0.2 + 0.6 * (np.arange(n) + 0.5) / n
    pts = to_real(cx + off[:, 0], cy + off[:, 1], rng.permutation(frac), W, H, real_w, real_h)
    depths = 1.0 + np.arange(n) / 64.0                                 # distinct, exact in float32
    assert len({(a, b) for a, b in pts.tolist()}) == n
    return depths, pts, (cx, cy)


UNFIT = (np.nan, np.inf, -np.inf, 1e12, -1e12, 2.0 ** 31, -2.0 ** 31, 2.0 ** 30, -2.0 ** 30)   # (2^30 is the kernel's own limit)


def unfit_mix(W, H, real_w, real_h, n=90, seed=29):
    """ordinary points with every third one at a position that fits no int in x, in y or in both; the ordinary points just before
    and after each are in reach of it, so a stray write would show"""
    rng = np.random.default_rng(seed)
    depths, pts = ordinary_points(rng, n, real_w, real_h)
    unfit = np.zeros(n, bool)
    for j, i in enumerate(range(1, n, 3)):
        v = UNFIT[j % len(UNFIT)]
        pts[i] = [(v, pts[i, 1]), (pts[i, 0], v), (v, v)][j % 3]
        unfit[i] = True
    pts[4] = (2.0 ** 30 - 1.0, 5.0)      # the largest position that fits: its window is far outside, it writes nothing either
    return depths, pts, unfit


def odd_depths(W, H, real_w, real_h, n=60, seed=31):
    """ordinary positions; depths 0, -0.0, negative, NaN, +inf and -inf between ordinary ones"""
    rng = np.random.default_rng(seed)
    depths, pts = ordinary_points(rng, n, real_w, real_h)
    pts[:, 0] = np.clip(pts[:, 0], 0.25 * real_w, 0.75 * real_w)       # clustered: the windows overlap and overwrite
    pts[:, 1] = np.clip(pts[:, 1], 0.25 * real_h, 0.75 * real_h)
    odd = (0.0, -0.0, -3.0, np.nan, np.inf, -np.inf)
    for j, i in enumerate(range(0, n, 2)):
        depths[i] = odd[j % len(odd)]
    return depths, pts


def point_sets(mask_x, mask_y, W, H, real_w, real_h):
    """-> [(name, depths, points)]: the counts around the chunk size, the pile, the positions that fit no int, the odd depths"""
    rng = np.random.default_rng(37)
    sets = [("count%d" % n,) + ordinary_points(rng, n, real_w, real_h) for n in COUNTS]
    sets.append(("pile",) + pile(quiet_pixel(mask_x, mask_y), W, H, real_w, real_h)[:2])
    sets.append(("unfit",) + unfit_mix(W, H, real_w, real_h)[:2])
    sets.append(("odd-depths",) + odd_depths(W, H, real_w, real_h))
    return sets
