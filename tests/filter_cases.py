"""Cases, scalar restatement and comparison for the inverse-depth filter tests (tests/test_filter_cases.py on the CPU,
tests/test_gpu_filter_cases.py on the GPU).  No GPU is needed to import or run anything here.

A case is a size (H, W), a list of updates and a table of marks.  An update is (array, covariance, reciprocal): the array is the
inverse-depth reading, or the DEPTH where `reciprocal` is set (the filter and the oracle then use 1.0 / array); the covariance is
a scalar on odd updates and a map on even ones.  A mark (k, i) says that update k holds a named class at flat pixel i.

Pixel roles, by flat index i modulo 8 (a single-pixel case has the one "exact" pixel, with a few events on it):
  0-4  converging   a fixed truth, log-uniform in [0.011, 99]; readings truth * (1 + rel * noise), rel in 1e-2 .. 1e-5, noise
                    clipped at three sigma; covariance max((rel * truth)^2, floor) with a floor in 1e-3 .. 1e-2.  The floor is there
                    because NormPdf is a PRODUCT with sqrt(2 PI s2) (depth_filter.cpp:10-16): a reading with a standard deviation
                    far below 0.01 loses against the uniform term however well it fits, and the reference filter never
                    converges on it.  The first update's covariance also covers (truth - 0.5)^2 / 2, the distance from the
                    prior mean: otherwise truths beyond about 35 are taken for outliers for good and the mean never gets near
                    100, where the variance's cancelling terms are of order 1e4.
  5    underflow    converging, half of them with a truth in [90, 99]; the last update but one reads 60 away from the truth: the
                    oracle's exp() argument is below -746, c1 is exactly 0, the mean is kept bit for bit and the variance is
                    (s_old + mu^2) - mu^2, which collapses to exactly 0 where s_old is below half an ulp of mu^2.
  6    exact        truth 0.5 and the first reading exactly 0.5 from the constructor state: exp(-0.0), pure IEEE arithmetic.
  7    hostile      converging readings with events on top, from update 1 on: a reading class on any update, a covariance class
                    or the outlier-with-NaN-covariance pair on map updates, at pixels drawn afresh for every update.
Scalar covariances: updates 7, 17, .. and 9, 19, .. take two different ones of -1, NaN, +inf (every pixel is skipped or, for an
outlier reading, still counted), update 1 takes 0 and updates 5, 15, .. one of 1e-300, 1e300; updates 3, 13, .. take 4.05e-3.  A
10-update case has five scalar updates and so holds four of the six scalar classes, chosen by its pixel count; all six are
held across the sizes and by the 60-update run.  1e-300 and 1e300 stay off the last update: either leaves every variance at
exactly 0.
A covariance of exactly 0, as the scalar or in the map, comes at updates 1 and 2 only, while every variance is still far above its
rounding residue (below).  Later, 0 onto a collapsed variance gives m = 0 / 0 and the pixel is skipped where the variance is
exactly 0, but fused with c1 = 0 where it is 1e-17: which of the two happens depends on the last bit of exp() many updates earlier,
in the reference as much as here, and no tolerance can cover it.

What a converged pixel's variance is: the filter stores the SQUARE of the fused variance and takes its square root as the next
standard deviation (depth_filter.cpp:190, :251), so the variance squares itself with every update and after five or six of them
is the rounding residue of c1 (s + m^2) + c2 (s_old + mu^2) - mu'^2, about 1e-16 mu^2 or exactly 0.  About half of the converged
pixels of a case therefore end with a variance of exactly 0; the cases' seeds are chosen, on the oracle alone, so that at least
a third of every case's pixels end with ratio > 0.5 AND a variance above 0.

Tolerances (both from the project, neither measured on the code under test): a, b, mu relative 1e-9; the variance (square root
of the stored covariance) absolute 1e-12 * max(1, mu_before^2, reading^2).  tests/test_filter_cases.py runs the oracle with exp()
as numpy has it and moved one ulp up and down, and asserts 100 x the largest spread inside each tolerance.  Measured over all
cases (the worst is the 60-update run or 16 x 16): a 1.2e-12, b 1.4e-12, mu 4e-14 relative, variance 9e-16 x its scale; the CPU
test prints what it measures.  The variance is compared with that absolute tolerance alone, no relative term on top."""
import functools

import numpy as np

from oracle.depth_filter import DepthFilter as Oracle

RTOL = 1e-9
VAR_ATOL = 1e-12

SIZES = ((1, 1), (1, 255), (16, 16), (1, 257), (7, 37), (17, 31), (3, 171), (2, 256))
UPDATES = 10
LONG_SIZE, LONG_UPDATES = (7, 37), 60
DEFAULT_COV = 4.05e-3               # the (3 * DEP_SAMPLE)^2-like constant of depth_estimator.cpp:293
LO, HI = 0.01, 100.0
BELOW_LO, ABOVE_HI = float(np.nextafter(0.01, 0.0)), float(np.nextafter(100.0, np.inf))
INF, NAN = float("inf"), float("nan")

# reading classes: name -> inverse depth.  The first two are kept (fused), the NaN is skipped, the rest are outliers (b + 1)
READINGS = (("bound_lo", LO), ("bound_hi", HI), ("below_lo", BELOW_LO), ("above_hi", ABOVE_HI), ("out_zero", 0.0), ("out_neg", -1.0),
            ("out_pinf", INF), ("out_ninf", -INF), ("out_300", 300.0), ("nan_reading", NAN))
# covariance classes: name -> covariance.  -1, NaN and +inf make c1 * m NaN (skipped); 0, 1e-300 and 1e300 are fused
COVS = (("cov_zero", 0.0), ("cov_neg", -1.0), ("cov_nan", NAN), ("cov_inf", INF), ("cov_tiny", 1e-300), ("cov_huge", 1e300))
OUTLIER_NAN_COV = "outlier_nan_cov"  # reading 300 with covariance NaN: the outlier test comes first, b + 1 still happens
KEPT = ("bound_lo", "bound_hi", "cov_zero", "cov_tiny", "cov_huge")
OUTLIERS = ("below_lo", "above_hi", "out_zero", "out_neg", "out_pinf", "out_ninf", "out_300", OUTLIER_NAN_COV)
SKIPPED = ("nan_reading", "cov_neg", "cov_nan", "cov_inf")
SCALAR_SKIP = (-1.0, NAN, INF)
SCALAR_KEPT = (0.0, 1e-300, 1e300)
# reciprocal form: name -> depth; the filter reads 1.0 / depth.  +-0 -> +-inf, 5e-324 -> +inf, -2 -> -0.5, +inf -> 0: outliers; NaN:
# skipped; 0.01 -> 100.0 and 100.0 -> 0.01: kept; their neighbours: nextafter(0.01, 0) -> above 100 (outlier), nextafter(100, inf)
# -> below 0.01 (outlier)
RECIPROCALS = (("rcp_zero", 0.0), ("rcp_negzero", -0.0), ("rcp_subnormal", 5e-324), ("rcp_neg", -2.0), ("rcp_inf", INF), ("rcp_nan", NAN),
               ("rcp_lo", 0.01), ("rcp_hi", 100.0), ("rcp_below_lo", BELOW_LO), ("rcp_above_hi", ABOVE_HI))
RCP_KEPT = ("rcp_lo", "rcp_hi")
RCP_OUTLIERS = ("rcp_zero", "rcp_negzero", "rcp_subnormal", "rcp_neg", "rcp_inf", "rcp_below_lo", "rcp_above_hi")
RCP_SKIPPED = ("rcp_nan",)

# one seed per case, chosen on the oracle alone (see the module docstring)
SEEDS = {(1, 1, 10): 3, (16, 16, 10): 1}      # every other case: 0


class Case:
    def __init__(self, H, W, n_updates, seed):
        self.H, self.W, self.n, self.n_updates, self.seed = H, W, H * W, n_updates, seed
        self.name = "%dx%d_%d" % (H, W, n_updates)
        self.updates = []      # (array (H, W), covariance: float or (H, W), reciprocal: bool)
        self.marks = {}        # class name -> [(k, flat pixel)]
        self.scalars = {}      # k -> hostile scalar covariance of that update
        self.role = {}         # role name -> flat pixel indices
        self._build()

    def reading(self, k):
        """what the filter sees at update k: the inverse depth"""
        arr, _, rcp = self.updates[k]
        with np.errstate(all="ignore"):
            return 1.0 / arr if rcp else arr

    def cov_map(self, k):
        return np.broadcast_to(np.asarray(self.updates[k][1], np.float64), (self.H, self.W))

    def marked(self, names, k=None):
        return [(kk, i) for name in names for kk, i in self.marks.get(name, ()) if k is None or kk == k]

    def _build(self):
        n, K = self.n, self.n_updates
        rng = np.random.default_rng(self.seed)
        idx = np.arange(n)
        r = idx % 8 if n > 1 else np.array([6])
        truth = np.exp(rng.uniform(np.log(0.011), np.log(99.0), n))
        under = np.flatnonzero(r == 5)
        truth[under[::2]] = rng.uniform(90.0, 99.0, len(under[::2]))
        truth[under[1::2]] = np.exp(rng.uniform(np.log(0.011), np.log(30.0), len(under[1::2])))
        truth[r == 6] = 0.5
        rel = 10.0 ** -rng.integers(2, 6, n).astype(np.float64)
        rel[under[::2]] = 1e-5
        floor = 10.0 ** rng.uniform(-3.0, -2.0, n)
        hostile = np.flatnonzero(r == 7) if n > 1 else np.array([0])
        self.role = {"converging": np.flatnonzero(r <= 4), "underflow": under, "exact": np.flatnonzero(r == 6), "hostile": hostile}
        self.truth = truth
        placed = {}            # (k, pixel) -> class name; a later event at the same place replaces the earlier one
        for k in range(K):
            x = truth * (1.0 + rel * np.clip(rng.normal(0.0, 1.0, n), -3.0, 3.0))
            cov = np.maximum((rel * truth) ** 2, floor)
            if k == 0:
                cov = np.maximum(cov, (truth - 0.5) ** 2 / 2.0)
                x[r == 6] = 0.5
                cov[r == 6] = rng.uniform(1e-4, 1e-2, int((r == 6).sum()))
            if k == K - 2:
                x[under] = np.where(truth[under] > 50.0, truth[under] - 60.0, truth[under] + 60.0)
                for i in under:
                    placed[(k, int(i))] = "underflow"
            use_map = k % 2 == 0
            rcp = k % 5 == 4                      # updates 4, 9, 14, ..: the depth form
            if k >= 1 and len(hostile) and (n > 1 or k in (3, 5, 7)):
                events = [(name, v, None) for name, v in READINGS]
                if rcp:
                    events = [(name, None, None) for name, _ in RECIPROCALS]
                if use_map:
                    events += [(name, None, v) for name, v in COVS if v != 0.0 or k == 2] + [(OUTLIER_NAN_COV, 300.0, NAN)]
                events = events[k % len(events):] + events[:k % len(events)]
                slots = rng.permutation(hostile)
                for j, (name, v, c) in enumerate(events):
                    i = int(slots[j % len(slots)])
                    if j >= len(slots) and n > 1:
                        break                      # more events than hostile pixels: the rest get their turn on another update
                    placed[(k, i)] = name
                    if v is not None:
                        x[i] = v
                    if c is not None:
                        cov[i] = c
                    if n == 1:
                        break
            with np.errstate(all="ignore"):
                arr = 1.0 / x if rcp else x
            if rcp:
                depth_of = dict(RECIPROCALS)
                for (kk, i), name in placed.items():
                    if kk == k and name in depth_of:
                        arr[i] = depth_of[name]
                    elif kk == k and name == OUTLIER_NAN_COV:
                        arr[i] = 1.0 / 300.0
            if use_map:
                c_out = cov.reshape(self.H, self.W)
            elif k == 1:
                c_out = self.scalars[k] = 0.0
            elif k % 10 == 7:
                c_out = self.scalars[k] = SCALAR_SKIP[(k // 10 + n) % 3]
            elif k % 10 == 5:
                c_out = self.scalars[k] = SCALAR_KEPT[1 + (k // 10 + n) % 2]
            elif k % 10 == 9:
                c_out = self.scalars[k] = SCALAR_SKIP[(k // 10 + n + 1) % 3]
            else:
                c_out = DEFAULT_COV
            self.updates.append((arr.reshape(self.H, self.W), c_out, rcp))
        for (k, i), name in placed.items():
            self.marks.setdefault(name, []).append((k, i))
        for i in self.role["exact"]:
            self.marks.setdefault("exact", []).append((0, int(i)))


@functools.lru_cache(maxsize=None)
def case(H, W, n_updates=UPDATES):
    return Case(H, W, n_updates, SEEDS.get((H, W, n_updates), 0))


def all_cases():
    return [case(H, W) for H, W in SIZES] + [case(*LONG_SIZE, LONG_UPDATES)]


def shifted_exp(ulps):
    """numpy's exp moved by `ulps` (+1 / -1) units in the last place"""
    def f(x):
        y = np.exp(x)
        return np.nextafter(y, np.inf if ulps > 0 else -np.inf)
    return np.exp if ulps == 0 else f


@functools.lru_cache(maxsize=None)
def oracle_states(H, W, n_updates=UPDATES, ulps=0):
    """-> [state before update 0, state after update 0, ...]; a state is the read-only tuple (a, b, mu, cov) of (H, W) arrays"""
    c = case(H, W, n_updates)
    f = Oracle(H, W)
    f.exp = shifted_exp(ulps)
    states = []
    for k in range(n_updates + 1):
        st = tuple(np.array(v) for v in (f.a, f.b, f.mu, f.cov))
        for v in st:
            v.setflags(write=False)
        states.append(st)
        if k < n_updates:
            f.update(c.reading(k), c.updates[k][1])
    return states


def ratio_of(a, b):
    with np.errstate(all="ignore"):
        return a / (a + b)


def masked_inv_depth(a, b, mu):
    """depth_estimator.cpp:387-398: 1e-5 where the ratio is below 0.5 (a NaN ratio is not below: mu)"""
    return np.where(ratio_of(a, b) < 0.5, 0.00001, mu)


def scalar_update(a, b, mu, cov, new_mu, new_cov, inv_range=100 - 0.01):
    """depth_filter.cpp:186-253 for one pixel, statement by statement, in numpy.float64 scalars (IEEE double like the reference's
    `double`s; sqrt of a negative number, overflow and inf - inf give NaN or inf as in C, they do not raise); -> (a, b, mu, cov)"""
    f8 = np.float64
    a, b, mu, cov, new_mu, new_cov, inv_range = f8(a), f8(b), f8(mu), f8(cov), f8(new_mu), f8(new_cov), f8(inv_range)
    with np.errstate(all="ignore"):
        n_a = a                                                        # :186
        n_b = b
        old_mu = mu
        old_sigma = np.sqrt(cov)                                       # :190
        old_sq = old_sigma * old_sigma
        new_sigma = np.sqrt(new_cov)
        if new_mu < f8(0.01) or new_mu > f8(100):                      # :203 the outlier test comes first
            n_b = n_b + f8(1)
            return n_a, n_b, mu, cov
        new_sq = new_sigma * new_sigma
        m = (new_sq * old_mu + old_sq * new_mu) / (old_sq + new_sq)
        s = (new_sq * old_sq) / (new_sq + old_sq)
        ssum = new_sq + old_sq
        pdf = np.exp(-(new_mu - old_mu) * (new_mu - old_mu) / (f8(2.0) * ssum)) * np.sqrt(f8(2.0) * f8(3.14159) * ssum)   # :10-16
        c1 = (n_a / (n_a + n_b)) * pdf
        c2 = (n_b / (n_a + n_b)) * f8(1.0) / inv_range
        norm = c1 + c2
        c1 = c1 / norm
        c2 = c2 / norm
        f = c1 * ((n_a + f8(1.0)) / (n_a + n_b + f8(1.0))) + c2 * (n_a / (n_a + n_b + f8(1.0)))
        e = (c1 * ((n_a + f8(1.0)) * (n_a + f8(2.0))) / ((n_a + n_b + f8(1.0)) * (n_a + n_b + f8(2.0))) +
             c2 * (n_a * (n_a + f8(1.0))) / ((n_a + n_b + f8(1.0)) * (n_a + n_b + f8(2.0))))
        if np.isnan(c1 * m):                                           # :238 `continue`
            return a, b, mu, cov
        fused_mu = c1 * m + c2 * old_mu
        fused_sigma = c1 * (s + m * m) + c2 * (old_sq + old_mu * old_mu) - fused_mu * fused_mu      # :245
        fused_a = (e - f) / (f - e / f)
        fused_b = fused_a * (f8(1.0) - f) / f
        return fused_a, fused_b, fused_mu, fused_sigma * fused_sigma   # :251 the square of the variance is what is stored


def close(got, want, what, rtol=RTOL, atol=0.0):
    """got against want, every element: NaNs in the same places, infinities in the same places with the same sign, finite values
    within |got - want| <= atol + rtol * |want|; atol may be an array (a tolerance per element).  Nothing is left out."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %s against %s" % (what, got.shape, want.shape)
    assert (np.isnan(got) == np.isnan(want)).all(), "%s: NaN at other places, first %s" % (what, _first(np.isnan(got) != np.isnan(want)))
    ginf, winf = np.isinf(got), np.isinf(want)
    assert (ginf == winf).all(), "%s: infinity at other places, first %s" % (what, _first(ginf != winf))
    assert (np.signbit(got[winf]) == np.signbit(want[winf])).all(), "%s: infinity of the other sign" % what
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    atol = np.broadcast_to(np.asarray(atol, np.float64), want.shape)
    err = np.abs(got[ok] - want[ok]) - atol[ok]
    rel = err / np.maximum(np.abs(want[ok]), 1e-300)
    assert rel.max() <= rtol, "%s: relative error %g beyond the absolute tolerance, at %s" % (what, rel.max(), _first(ok, int(rel.argmax())))
    return float(rel.max())


def _first(mask, nth=0):
    return tuple(int(v[nth]) for v in np.nonzero(mask))


def variance_atol(mu_before, reading):
    """absolute tolerance of the variance after an update: 1e-12 times the size of the terms that cancel in depth_filter.cpp:245.
    Non-finite readings (outliers, skipped) change nothing and count as 1."""
    with np.errstate(all="ignore"):
        x2 = np.where(np.isfinite(reading), reading * reading, 1.0)
        m2 = np.where(np.isfinite(mu_before), mu_before * mu_before, 1.0)
    return VAR_ATOL * np.maximum(1.0, np.maximum(m2, x2))


def close_state(got, want, before, reading, what):
    """the four maps after an update: (a, b, mu, cov) `got` against the oracle's `want`; `before` is the oracle's state before it"""
    for name, g, w in zip(("a", "b", "mu"), got, want):
        close(g, w, "%s %s" % (what, name))
    with np.errstate(all="ignore"):
        close(np.sqrt(got[3]), np.sqrt(want[3]), "%s variance" % what, rtol=0.0, atol=variance_atol(before[2], reading))


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()
