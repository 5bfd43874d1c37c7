"""CPU checks of the inverse-depth filter cases (tests/filter_cases.py): the vectorised oracle against the scalar restatement on
every case and update, every named class reached, the +-1 ulp-of-exp() margin of the GPU tolerances, and the cap on what the
masked read-outs may leave out.  Nothing here runs the code under test."""
import numpy as np
import pytest

from tests import filter_cases as fc

CASES = fc.all_cases()
IDS = [c.name for c in CASES]


def _states(c, ulps=0):
    return fc.oracle_states(c.H, c.W, c.n_updates, ulps)


def _pixel(state, i):
    return tuple(v.reshape(-1)[i] for v in state)


def _same(x, y):
    return fc.bits(x) == fc.bits(y)


def _sq(cov):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(cov, np.float64)) * np.sqrt(np.asarray(cov, np.float64))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_matches_the_scalar_statements(c):
    """equal, both NaN, or within 4e-15 relative; infinities equal with their sign"""
    states = _states(c)
    for k in range(c.n_updates):
        x, cov = c.reading(k).reshape(-1), c.cov_map(k).reshape(-1)
        for i in range(c.n):
            want = fc.scalar_update(*_pixel(states[k], i), x[i], cov[i])
            got = _pixel(states[k + 1], i)
            for g, w in zip(got, want):
                assert g == w or (np.isnan(g) and np.isnan(w)) or (np.isfinite(g) and np.isfinite(w) and abs(g - w) <= 4e-15 * abs(w)), \
                    (c.name, k, i, got, want)


def check_classes(c):
    states = _states(c)
    held = set(c.marks)
    if c.n >= 255:      # every class fits
        want = {n for n, _ in fc.READINGS + fc.COVS + fc.RECIPROCALS} | {fc.OUTLIER_NAN_COV, "underflow", "exact"}
        assert want <= held, (c.name, sorted(want - held))
        assert 0.0 in c.scalars.values() and len(c.scalars) >= 4 and len({repr(v) for v in c.scalars.values()}) >= 4
    reached = 0
    for name, places in c.marks.items():
        for k, i in places:
            before, after = _pixel(states[k], i), _pixel(states[k + 1], i)
            x = c.reading(k).reshape(-1)[i]
            scalar = c.scalars.get(k)
            skipping_scalar = scalar is not None and not scalar >= 0.0 or scalar == fc.INF
            if name in fc.OUTLIERS + fc.RCP_OUTLIERS:
                assert x < 0.01 or x > 100, (c.name, name, k, i, x)
                assert after[1] == before[1] + 1 and _same(after[0::2] + after[3:], before[0::2] + before[3:]), (c.name, name, k, i)
                assert _same(after[0], before[0]) and _same(after[2], before[2]) and _same(after[3], before[3])
            elif name in fc.SKIPPED + fc.RCP_SKIPPED or (skipping_scalar and name != "underflow"):
                assert _same(after, before), (c.name, name, k, i)
            elif name in fc.KEPT + fc.RCP_KEPT:
                assert 0.01 <= x <= 100
                outlier_result = (before[0], before[1] + 1, before[2], before[3])
                assert not _same(after, before) and not _same(after, outlier_result), (c.name, name, k, i)
                if name == "rcp_lo":
                    assert x == 100.0
                if name == "rcp_hi":
                    assert x == 0.01
            elif name == "exact":
                assert k == 0 and x == 0.5 and before == (15.0, 15.0, 0.5, 100.0) and after[0] > 15.0 and abs(after[2] - 0.5) < 1e-15
            elif name == "underflow":
                with np.errstate(all="ignore"):
                    arg = -(x - before[2]) * (x - before[2]) / (2.0 * (c.cov_map(k).reshape(-1)[i] + before[3]))
                assert arg < -746 and np.exp(arg) == 0.0, (c.name, k, i, arg)
                assert _same(after[2], before[2]) and after[1] > before[1], (c.name, k, i)      # c1 == 0: the mean is kept
            else:
                raise AssertionError("unknown class %s" % name)
            reached += 1
    # hostile scalar covariances: the whole image at once
    for k, scalar in c.scalars.items():
        x = c.reading(k)
        outlier = (x < 0.01) | (x > 100)
        a0, b0, m0, c0 = states[k]
        a1, b1, m1, c1 = states[k + 1]
        assert _same(b1[outlier], b0[outlier] + 1)
        if scalar in fc.SCALAR_KEPT:
            assert (_sq(c0) + _sq(scalar) > 0.0).all()                   # never 0 onto a collapsed variance (m = 0 / 0)
            fused = ~outlier & ~np.isnan(x)
            assert not fused.any() or (a1[fused] != a0[fused]).mean() > 0.9, (c.name, k)
        else:
            assert _same(a1, a0) and _same(m1, m0) and _same(c1, c0) and _same(b1[~outlier], b0[~outlier])
    # the collapse: among the underflow pixels with a truth near 100, the variance ends exactly 0 right after the far reading
    if c.n >= 255:
        k = c.n_updates - 2
        high = [i for i in c.role["underflow"] if c.truth[i] > 50]
        assert high and all(states[k + 1][3].reshape(-1)[i] == 0.0 for i in high), c.name
        assert max(abs(states[k][2].reshape(-1)[i]) for i in high) > 89.0       # the mean did get near 100
    # converged: ratio above 0.5 and a variance above 0, at a third of the pixels at least; the pixels that never get a valid
    # reading (none here by construction) would sit below 0.5
    a, b, mu, cov = states[-1]
    ratio = fc.ratio_of(a, b).reshape(-1)
    conv = (ratio > 0.5) & (np.sqrt(cov.reshape(-1)) > 0)
    assert conv.sum() * 3 >= c.n, (c.name, int(conv.sum()), c.n)
    steady = np.concatenate([c.role["converging"], c.role["exact"]]).astype(int)
    assert (ratio[steady] > 0.5).all(), c.name
    assert np.allclose(mu.reshape(-1)[steady], c.truth[steady], rtol=0.05), c.name
    return reached


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_named_class_is_reached(c):
    assert check_classes(c) >= (3 if c.n == 1 else 30)


def spreads(c):
    """largest difference between the oracle runs with exp() as it is, one ulp up and one ulp down, over all updates: a, b, mu
    relative, the variance as a multiple of its scale max(1, mu_before^2, reading^2)"""
    runs = [_states(c, u) for u in (0, 1, -1)]
    out = {"a": 0.0, "b": 0.0, "mu": 0.0, "variance": 0.0}
    for k in range(c.n_updates):
        for other in runs[1:]:
            for j, name in enumerate(("a", "b", "mu")):
                w, g = runs[0][k + 1][j], other[k + 1][j]
                assert (np.isnan(w) == np.isnan(g)).all() and (np.isinf(w) == np.isinf(g)).all()
                ok = np.isfinite(w)
                out[name] = max(out[name], float((np.abs(g[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1e-300)).max()))
            with np.errstate(all="ignore"):
                vw, vg = np.sqrt(runs[0][k + 1][3]), np.sqrt(other[k + 1][3])
            assert (np.isfinite(vw) == np.isfinite(vg)).all()
            ok = np.isfinite(vw)
            scale = fc.variance_atol(runs[0][k][2], c.reading(k)) / fc.VAR_ATOL
            out["variance"] = max(out["variance"], float((np.abs(vg[ok] - vw[ok]) / scale[ok]).max()))
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_one_ulp_of_exp_stays_a_hundred_times_inside_the_tolerances(c):
    s = spreads(c)
    print(c.name, s)
    assert 100 * s["a"] <= fc.RTOL and 100 * s["b"] <= fc.RTOL and 100 * s["mu"] <= fc.RTOL, s
    assert 100 * s["variance"] <= fc.VAR_ATOL, s


def undecided(c, k):
    """pixels whose ratio is within 1e-9 of 0.5 after update k (k = -1: the constructor state)"""
    a, b = _states(c)[k + 1][:2]
    return np.abs(fc.ratio_of(a, b) - 0.5) <= 1e-9


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_masked_readouts_leave_out_one_percent_at_most(c):
    for k in range(c.n_updates):
        assert undecided(c, k).sum() <= 0.01 * c.n, (c.name, k, int(undecided(c, k).sum()))


def test_close_compares_infinities_and_leaves_nothing_out():
    inf, nan = np.inf, np.nan
    want = np.array([1.0, inf, -inf, nan, 0.0])
    fc.close(want.copy(), want, "same")
    fc.close(want * (1 + 5e-10), want, "within")
    for bad in ([1.0, 1e308, -inf, nan, 0.0], [1.0, -inf, -inf, nan, 0.0], [1.0, inf, -inf, 0.0, 0.0], [1.0, inf, -inf, nan, 1e-20],
                [1.0 + 2e-9, inf, -inf, nan, 0.0], [inf, inf, -inf, nan, 0.0]):
        with pytest.raises(AssertionError):
            fc.close(np.array(bad), want, "bad")
    fc.close(np.array([1.0, inf, -inf, nan, 1e-13]), want, "atol", atol=np.array([0, 0, 0, 0, 1e-12]))
    with pytest.raises(AssertionError):
        fc.close(np.array([1e-13, 1.0]), np.array([0.0, 1.0]), "atol of another element", atol=np.array([0.0, 1e-12]))


def test_scalar_update_survives_what_math_raises_on():
    assert fc.scalar_update(15.0, 15.0, 0.5, 100.0, 0.7, -1.0) == (15.0, 15.0, 0.5, 100.0)         # sqrt(-1): NaN, skipped
    assert fc.scalar_update(15.0, 15.0, 0.5, 100.0, 300.0, np.nan) == (15.0, 16.0, 0.5, 100.0)     # outlier first
    assert fc.scalar_update(15.0, 15.0, 0.5, 100.0, 0.7, 1e300)[0] > 15.0                          # no overflow error
    a, b, mu, cov = fc.scalar_update(15.0, 15.0, 0.5, 100.0, 0.5, 4e-3)
    assert mu == 0.5 and a > 15.0
