"""The inputs of tests/stereo_cases.py checked on the CPU restatement alone: each really reaches the branch it is there for (so
that a GPU test passing on it means something), and the scalar per-thread form and the vectorised form of the restatement agree
bit for bit on every one of them, as do the two restated rasterisers on the point sets.  No GPU needed."""
import warnings

import numpy as np
import pytest

import stereo_cases as sc
import stereo_prep_restated as pr
import stereo_restated as sr

f32 = np.float32
SIZES = [(48, 32), (45, 27)]     # the work sizes the GPU tests run the cases at: a multiple of 8, and odd with W * H odd


def run(case):
    return sc.run_case(sr.VectorisedStereo, case)


def valid_pixels(cost):
    return ~(cost < 0).any(axis=2)


def tie_figures(case):
    """-> (tied, depth, tree's depth / index, a first minimum's depth / index): tied = valid pixels whose SGM minimum is non-zero
    and held by more than one depth"""
    st = run(case)
    sgm, depth = sc.last(st, "sgm"), sc.last(st, "depth")
    d_tree, mc, mi, _ = sc.wta_with(sr.tree_argmin, sgm, case.params)
    d_first, _, mi_first, _ = sc.wta_with(sc.first_argmin, sgm, case.params)
    assert sr.same_bits(d_tree, depth)
    holders = sgm == mc[..., None]
    tied = valid_pixels(sc.last(st, "cost")) & (holders.sum(axis=2) == 2) & (mc != 0)
    return tied, holders, depth, mi, d_first, mi_first


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("k", sc.TIE_ODD + sc.TIE_EVEN)
def test_adjacent_ties_reach_the_tree(W, H, k):
    """at least half of all pixels tie between depths k and k + 1 with a non-zero minimum and are accepted; for odd k the tree
    takes k + 1 where a first minimum takes k, for even k both take k.  (The depth itself cannot differ here: the parabola
    through min, min puts its vertex at k + 1/2 from either side -- the split ties below are where it differs.)"""
    tied, holders, depth, mi, d_first, mi_first = tie_figures(sc.ties(W, H, k))
    assert tied.mean() >= 0.5
    assert (holders[tied][:, [k, k + 1]]).all()
    assert (depth[tied] != 1000).all()
    assert (mi_first[tied] == k).all()
    assert (mi[tied] == (k + 1 if k % 2 else k)).all()
    assert (depth[tied] == f32(1.0) / (f32(k + 0.5) * f32(sc.DS64))).all()


@pytest.mark.parametrize("W,H", SIZES)
def test_the_tie_of_depths_0_and_1_is_rejected_by_the_tree(W, H):
    """the tree keeps index 0 (filterCostKernel rejects it); a rule that took the other minimum would accept every such pixel"""
    case = sc.ties(W, H, sc.TIE_EDGE)
    tied, holders, depth, mi, _, _ = tie_figures(case)
    assert tied.mean() >= 0.5 and holders[tied][:, [0, 1]].all()
    assert (mi[tied] == 0).all() and (depth[tied] == 1000).all()
    last_min = lambda c: (c.min(axis=-1), sr.DEP_CNT - 1 - np.argmin(c[..., ::-1], axis=-1))
    assert (sc.wta_with(last_min, sc.last(run(case), "sgm"), case.params)[0][tied] != 1000).all()


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("m", sc.SPLIT_UPPER + sc.SPLIT_LOWER)
def test_split_ties_decide_the_depth(W, H, m):
    """at least half of all pixels tie between depths m - 4 and m + 4 and are accepted; for the SPLIT_UPPER centres the tree
    takes m + 4 and its depth differs from a first minimum's (m - 4) at every one of them"""
    tied, holders, depth, mi, d_first, mi_first = tie_figures(sc.split_ties(W, H, m))
    assert tied.mean() >= 0.5
    assert holders[tied][:, [m - 4, m + 4]].all()
    assert (depth[tied] != 1000).all()
    assert (mi_first[tied] == m - 4).all()
    if m in sc.SPLIT_UPPER:
        assert (mi[tied] == m + 4).all() and (depth[tied] != d_first[tied]).all()
    else:
        assert (mi[tied] == m - 4).all() and (depth[tied] == d_first[tied]).all()


def test_tie_depths_invert_exactly():
    for k in sc.TIE_ODD + sc.TIE_EVEN + (sc.TIE_EDGE,):
        sc.tie_depth(k)
    with pytest.raises(AssertionError):
        sc.tie_depth(30)                       # (not every k does)
    assert {1, 63, 125} <= set(sc.TIE_ODD) and len(sc.TIE_ODD) >= 3 and len(sc.TIE_EVEN) >= 2
    assert all(k % 2 for k in sc.TIE_ODD) and not any(k % 2 for k in sc.TIE_EVEN)


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_var_scale_splits_the_interior_minima(W, H):
    case = sc.variance(W, H)
    st = run(case)
    _, mc, mi, _ = sc.wta_with(sr.tree_argmin, sc.last(st, "sgm"), dict(var_scale=1.0))
    interior = (mc != 0) & (mi != 0) & (mi != sr.DEP_CNT - 1)          # what var_scale = 1 accepts
    accepted = (sc.last(st, "depth") != 1000)[interior].mean()
    assert interior.sum() >= 200
    assert 0.05 <= accepted <= 0.95, accepted


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def test_sgm_parameter_sets_leave_the_defaults():
    assert len(sc.SGM_SETS) >= 2
    for p in sc.SGM_SETS:
        for name in ("pi1", "pi2", "tau_so", "sparse_ratio", "dep_sample"):
            assert f32(p[name]) != f32(sr.DEFAULTS[name]), name
        assert p["sgm_q1"] not in (0.0, 1.0) and p["sgm_q2"] not in (0.0, 1.0)
    assert any(p["sgm_q1"] < 0 or p["sgm_q2"] < 0 for p in sc.SGM_SETS)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("which", range(len(sc.SGM_SETS)))
def test_smooth_reference_takes_both_sides_of_tau_and_the_parameters_matter(W, H, which):
    """>= 50 % of the horizontal and of the vertical steps are below tau_so and >= 10 % at or above it; the SGM volume differs
    from the one the default pi1, pi2, tau_so, sgm_q1, sgm_q2 give ON THE SAME cost (same dep_sample and sparse_ratio) at
    >= 50 % of the entries of valid pixels"""
    p = sc.SGM_SETS[which]
    case = sc.smooth(W, H, p)
    tau = f32(p["tau_so"])
    for d in (np.abs(case.ref[:, 1:] - case.ref[:, :-1]), np.abs(case.ref[1:] - case.ref[:-1])):
        assert (d < tau).mean() >= 0.5 and (d >= tau).mean() >= 0.1
    st = run(case)
    base = run(sc.smooth(W, H, dict(p, **sc.SGM_NEUTRAL)))
    assert sr.same_bits(sc.last(st, "cost"), sc.last(base, "cost"))
    valid = valid_pixels(sc.last(st, "cost"))
    assert valid.mean() >= 0.4
    assert (sc.last(st, "sgm")[valid] != sc.last(base, "sgm")[valid]).mean() >= 0.5
    assert (sc.last(st, "depth") != 1000).mean() >= 0.2


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES + [(24, 16)])
def test_degenerate_poses_reach_every_denominator_class(W, H):
    """pose 0 (t = 0, w = x + y ...): 128 interior entries stay valid although a tap has 0 / 0 in both coordinates, about 90 % of
    the entries are valid, and on a cleared cost the corner pixel is rejected by w < 0 alone and w == 0 meets a non-zero
    numerator.  Pose 1 (t3 = -2): w changes sign with the depth index at every pixel; entries are rejected by w < 0 alone and by
    x / 0 inside the image."""
    R, t = sc.DEGENERATE_POSES[0]
    first, cleared = sc.tap_report(R, t, W, H, sc.DS64), sc.tap_report(R, t, W, H, sc.DS64, border=True)
    assert first["nan_valid"] >= 1 and first["valid"] >= 0.85 * first["entries"]
    assert cleared["w_only"] >= 1 and cleared["w_zero"] >= 1
    R, t = sc.DEGENERATE_POSES[1]
    assert t[2] != 0
    rep = sc.tap_report(R, t, W, H, sc.DS64)
    assert rep["w_only"] >= 1 and rep["w_zero"] >= 1 and rep["valid"] >= 1 and rep["w_negative"] > rep["valid"]
    # the restatement's cost agrees with the report: as many entries >= 0 after the first update as the report calls valid
    for pose, r in ((0, first), (1, rep)):
        case = sc.degenerate(W, H, pose)
        assert int((sc.run_case(sr.VectorisedStereo, case, upto=2)[0][1] >= 0).sum()) == r["valid"]


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_prior_edge_values_go_the_way_fuse_states(W, H):
    case = sc.prior_edges(W, H)
    st = run(case)
    before, after = st[1][1], st[2][1]           # the cost after the second update, and after the prior is fused into it
    assert (before[1:-1, 1:case.half - 1] == 0).all() and (before[:, case.half + 1:] > 0).any()
    changed = ~(before == after)
    ds = f32(sc.DS64)
    for name in sc.PRIOR_CLASSES:
        m = case.where[name]
        v = sc.PRIOR_VALUES[name]
        assert m.sum() >= 2 and (np.isnan(case.sd[m]).all() if name == "nan" else (case.sd[m] == v).all()), name
        zero_px, pos_px = m & (before == 0).all(axis=2), m & (before > 0).all(axis=2)
        assert zero_px.any() and pos_px.any(), name                     # on an all-zero cost and on an all-positive one
        assert not changed[zero_px].any(), name                          # `cost > 0`: an exact 0 never takes the prior
        if name in ("zero", "minus_zero", "nan", "negative"):            # `!(nDepth > 0)`
            assert not changed[m].any(), name
            continue
        cur = ds * np.arange(sr.DEP_CNT, dtype=np.float32)
        with np.errstate(all="ignore"):
            inv = (1.0 / np.float64(v)).astype(np.float32)
            add = (np.where(cur < inv, inv - cur, -inv + cur) / ds)[None, :] * f32(15.0) * case.dist[pos_px][:, None]
        assert sr.same_bits(after[pos_px], before[pos_px] + add), name
    assert np.finfo(np.float32).tiny > sc.PRIOR_VALUES["denormal"] > 0
    assert np.isinf(after[case.where["denormal"]]).any()                # 1 / denormal = +inf, added to every positive cost
    assert (1.0 / np.float64(sc.PRIOR_VALUES["largest"])).astype(np.float32) < np.finfo(np.float32).tiny   # a denormal inverse
    assert changed[case.where["inf"]].any()                             # 1 / inf = 0: the prior is the depth index itself
    sgm = sc.last(st, "sgm")
    nan_px = np.isnan(sgm).any(axis=2)
    assert nan_px.any() and (np.isnan(sgm).all(axis=2) == nan_px).all()  # NaN only ever as a whole pixel
    assert (sc.last(st, "depth") != 1000).mean() >= 0.05


# ---- (f) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_count12_reaches_twelve_measurements(W, H):
    case = sc.count12(W, H)
    ops = [op[0] for op in case.steps]
    assert ops.count("update") == 12 and ops.index("clear") == 8 and ops[-1] == "output"
    st = run(case)
    assert len(st) == 15
    # count 8 on a zeroed cost: (0 * 7 + tmp / 9) / 8 leaves the border unmarked, and the running mean still moves at count 12
    assert (st[7][1][0] >= 0).any() and not (st[6][1][0] >= 0).any()
    assert not sr.same_bits(st[10][1], st[11][1])
    assert (sc.last(st, "depth") != 1000).mean() >= 0.2


# ---- scalar against vectorised, (a) - (f) --------------------------------------------------------------------------------------------
def assert_same_states(a, b):
    assert [n for n, _ in a] == [n for n, _ in b]
    for k, ((name, x), (_, y)) in enumerate(zip(a, b)):
        assert sr.same_bits(x, y), "state %d (%s) differs" % (k, name)


def test_scalar_and_vectorised_agree_on_the_ties():
    """one scalar update serves every k: the tie cases share their images, so only the prior, the SGM and the WTA are redone"""
    W, H = 12, 8
    cases = [sc.ties(W, H, k) for k in sc.TIE_ODD + sc.TIE_EVEN + (sc.TIE_EDGE,)]
    s = sr.ScalarStereo(W, H, **cases[0].params)
    s.set_reference(*cases[0].steps[0][1:])
    s.update(*cases[0].steps[1][1:])
    cost = s.cost.copy()
    for case in cases:
        assert case.params == cases[0].params and all(np.array_equal(a, b) for a, b in zip(case.steps[1][1:], cases[0].steps[1][1:]))
        want = run(case)
        s.cost[:] = cost
        s.output(*case.steps[2][1:])
        assert_same_states([("cost", cost), ("cost", s.cost), ("sgm", s.sgm), ("depth", s.depth)], want)


SMALL = [sc.split_ties(22, 5, 64), sc.split_ties(22, 5, 24), sc.variance(11, 7), sc.smooth(11, 7, sc.SGM_SETS[0]), sc.smooth(11, 7, sc.SGM_SETS[1]),
         sc.smooth(11, 7, sc.SGM_SETS[2]), sc.degenerate(9, 6, 0), sc.degenerate(9, 6, 1), sc.prior_edges(12, 8), sc.count12(8, 5)]


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_scalar_and_vectorised_agree_on_the_cases(case):
    assert_same_states(sc.run_case(sr.ScalarStereo, case), run(case))


# ---- (g) -------------------------------------------------------------------------------------------------------------------------
def masks(W, H, seed=41):
    rng = np.random.default_rng(seed)
    return (rng.random((H, W)) < 0.1).astype(np.uint8), (rng.random((H, W)) < 0.1).astype(np.uint8)


GEOMETRY = [(37, 29, 74, 58), (40, 30, 47, 36), (64, 48, 32, 24)]


@pytest.mark.parametrize("W,H,real_w,real_h", GEOMETRY)
def test_both_rasterisers_agree_on_every_point_set_without_warning(W, H, real_w, real_h):
    mx, my = masks(W, H)
    sets = sc.point_sets(mx, my, W, H, real_w, real_h)
    assert [len(d) for _, d, _ in sets][:6] == list(sc.COUNTS)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for name, d, p in sets:
            a = pr.sparse_maps(d, p, mx, my, W, H, real_w, real_h)
            b = pr.sparse_maps_vectorised(d, p, mx, my, W, H, real_w, real_h)
            assert sr.same_bits(a[0], b[0]) and sr.same_bits(a[1], b[1]), name
            if len(d):
                assert (a[1] > 0).any(), name


@pytest.mark.parametrize("W,H,real_w,real_h", GEOMETRY)
def test_pile_is_decided_by_a_point_of_the_second_chunk(W, H, real_w, real_h):
    mx, my = masks(W, H)
    d, p, (cx, cy) = sc.pile(sc.quiet_pixel(mx, my), W, H, real_w, real_h)
    assert len(d) >= 300 and len(set(d.tolist())) == len(d)
    sd, _ = pr.sparse_maps_vectorised(d, p, mx, my, W, H, real_w, real_h)
    assert sd[cy, cx] == f32(d[-1])                                                  # the last point: index >= 256
    first = pr.sparse_maps_vectorised(d[:sc.CHUNK], p[:sc.CHUNK], mx, my, W, H, real_w, real_h)[0]
    assert first[cy, cx] == f32(d[sc.CHUNK - 1])                                     # every point overwrites: the chunk's last
    # the chunks in the other order end on the first chunk's last point
    order = np.concatenate([np.arange(sc.CHUNK, len(d)), np.arange(sc.CHUNK)])
    assert pr.sparse_maps_vectorised(d[order], p[order], mx, my, W, H, real_w, real_h)[0][cy, cx] == f32(d[sc.CHUNK - 1])


def test_points_that_fit_no_int_write_nothing():
    """the library's rule (kernels_stereo_prep.h): NaN, +-inf, |.| >= 2^30 before or after the scale -> no write, no error, no
    warning; the maps equal those of the same set without these points"""
    W, H, real_w, real_h = 40, 30, 47, 36
    mx, my = masks(W, H)
    d, p, unfit = sc.unfit_mix(W, H, real_w, real_h)
    assert unfit.sum() >= 2 * len(sc.UNFIT)
    for v in sc.UNFIT:
        assert any((np.isnan(v) and np.isnan(q).any()) or (q == v).any() for q in p[unfit])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for f in (pr.sparse_maps, pr.sparse_maps_vectorised):
            a = f(d, p, mx, my, W, H, real_w, real_h)
            b = f(d[~unfit], p[~unfit], mx, my, W, H, real_w, real_h)
            assert sr.same_bits(a[0], b[0]) and sr.same_bits(a[1], b[1])
            assert (a[0] > 0).sum() > 100
            # a position below 2^30 whose quotient by a scale < 1 passes it: nothing either
            c = f([1.0, 2.0], [(2.0 ** 30 - 8.0, 5.0), (5.0, 2.0 ** 30 - 8.0)], mx, my, 64, 48, 32, 24)
            assert (c[0] == -1).all() and (c[1] == 0).all()


def test_odd_point_depths_are_stored_as_they_are():
    W, H, real_w, real_h = 40, 30, 47, 36
    mx, my = masks(W, H)
    d, p = sc.odd_depths(W, H, real_w, real_h)
    sd, dist = pr.sparse_maps_vectorised(d, p, mx, my, W, H, real_w, real_h)
    written = dist > 0
    assert np.isnan(sd[written]).any() and np.isposinf(sd[written]).any() and np.isneginf(sd[written]).any()
    assert (sd[written] == 0).any() and (sd[written] == -3.0).any() and (sd[written] > 0).any()
