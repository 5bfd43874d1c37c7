"""GPU tests of the inverse-depth filter (kernels_filter.h, host_filter.h, chisel.DepthFilter, chisel.DepthEstimator) on the cases
of tests/filter_cases.py: ragged sizes, edge readings and covariances, every read-out, host and device forms, back-to-back
updates, refusals and the binding's checks.  Tolerances and their margin: tests/filter_cases.py, tests/test_filter_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import filter_cases as fc

pytestmark = pytest.mark.gpu
SIZE_IDS = ["%dx%d" % s for s in fc.SIZES]
CONSTRUCTOR = (15.0, 15.0, 0.5, 100.0)


def _states(c, ulps=0):
    return fc.oracle_states(c.H, c.W, c.n_updates, ulps)


def _update(gf, c, k, conv=lambda a: a):
    arr, cov, rcp = c.updates[k]
    gf.Update(conv(arr), cov if np.isscalar(cov) else conv(cov), reciprocal=rcp)


def _state(gf):
    return tuple(gf.read(w) for w in range(4))


def _flat(state, i):
    return tuple(v.reshape(-1)[i] for v in state)


def _same(x, y):
    return fc.bits(x) == fc.bits(y)


# ---- a. sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", fc.SIZES, ids=SIZE_IDS)
def test_every_size_against_the_oracle_after_every_update(hip_lib, size):
    from cvids_amd.chisel import DepthFilter
    c = fc.case(*size)
    want = _states(c)
    gf = DepthFilter(c.H, c.W)
    for got, value in zip(_state(gf), CONSTRUCTOR):
        assert got.shape == size and _same(got, np.full(size, value))                   # constructor values, exactly
    for k in range(c.n_updates):
        _update(gf, c, k)
        fc.close_state(_state(gf), want[k + 1], want[k], c.reading(k), "%s update %d" % (c.name, k))


# ---- b. exact classes -------------------------------------------------------------------------------------------------------------
def test_exp_of_minus_zero_is_one_on_the_device(hip_lib):
    """the "exact" first update (reading 0.5 from the constructor state) on all four maps, bit for bit against the oracle: exp(-0.0)
    is 1 and everything else is IEEE arithmetic.  If this one fails while the tolerance test above passes, the device library's
    exp(-0.0) is not 1."""
    from cvids_amd.chisel import DepthFilter
    for size in fc.SIZES:
        c = fc.case(*size)
        exact = [i for _, i in c.marks["exact"]]
        assert exact, c.name
        gf = DepthFilter(c.H, c.W)
        _update(gf, c, 0)
        got, want = _state(gf), _states(c)[1]
        for g, w, name in zip(got, want, "a b mu cov".split()):
            assert _same(g.reshape(-1)[exact], w.reshape(-1)[exact]), (c.name, name)


@pytest.mark.parametrize("size", fc.SIZES, ids=SIZE_IDS)
def test_outliers_skips_and_underflow_bit_for_bit(hip_lib, size):
    """every named class where it sits, on the device's own state before and after the update: an outlier is exactly b + 1 with a,
    mu and cov untouched, a skipped pixel is untouched, a kept one is neither; c1 == 0 ("underflow") leaves only IEEE arithmetic,
    so the device's result is the scalar restatement of the device's own state before, bit for bit -- and the oracle's wherever the
    two states were bit-equal before.  The reciprocal edge values land in the classes of the oracle fed with 1.0 / depth."""
    from cvids_amd.chisel import DepthFilter
    c = fc.case(*size)
    oracle = _states(c)
    gf = DepthFilter(c.H, c.W)
    before = _state(gf)
    seen = {"outlier": 0, "skipped": 0, "kept": 0, "underflow": 0}
    for k in range(c.n_updates):
        _update(gf, c, k)
        after = _state(gf)
        x, cov = c.reading(k).reshape(-1), c.cov_map(k).reshape(-1)
        for name, places in c.marks.items():
            for kk, i in places:
                if kk != k or name == "exact":
                    continue
                b4, now = _flat(before, i), _flat(after, i)
                o4, onow = _flat(oracle[k], i), _flat(oracle[k + 1], i)
                where = (c.name, name, k, i)
                if _same(onow, (o4[0], o4[1] + 1, o4[2], o4[3])) and (x[i] < 0.01 or x[i] > 100):          # the oracle: an outlier
                    assert name in fc.OUTLIERS + fc.RCP_OUTLIERS, where
                    assert now[1] == b4[1] + 1 and _same((now[0], now[2], now[3]), (b4[0], b4[2], b4[3])), where
                    seen["outlier"] += 1
                elif _same(onow, o4):                                                                       # the oracle: skipped
                    assert _same(now, b4), where
                    seen["skipped"] += 1
                elif name == "underflow":
                    assert _same(now, fc.scalar_update(*b4, x[i], cov[i])), where
                    assert now[2] == b4[2], where
                    if _same(b4, o4):
                        assert _same(now, onow), where
                    seen["underflow"] += 1
                else:
                    assert name in fc.KEPT + fc.RCP_KEPT, where
                    assert not _same(now, b4) and not _same(now, (b4[0], b4[1] + 1, b4[2], b4[3])), where
                    seen["kept"] += 1
        if k in c.scalars and c.scalars[k] not in fc.SCALAR_KEPT:       # -1, NaN, +inf for the whole image
            out = (x < 0.01) | (x > 100)
            assert _same(after[1].reshape(-1)[out], before[1].reshape(-1)[out] + 1)
            assert _same(after[1].reshape(-1)[~out], before[1].reshape(-1)[~out])
            assert _same(after[0], before[0]) and _same(after[2], before[2]) and _same(after[3], before[3])
        before = after
    if c.n >= 255:
        assert min(seen.values()) >= 4, seen


# ---- c. read-outs 4, 5, 6 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(7, 37), (1, 257)], ids=["7x37", "1x257"])
def test_readouts_after_every_update(hip_lib, size):
    from cvids_amd.chisel import DepthFilter
    c = fc.case(*size)
    oracle = _states(c)
    gf = DepthFilter(c.H, c.W)
    below = 0
    for k in range(c.n_updates):
        _update(gf, c, k)
        a, b, mu, _ = _state(gf)
        ratio, inv, depth = gf.read(gf.RATIO), gf.read(gf.INV_DEPTH_MASKED), gf.read(gf.DEPTH)
        # numpy on the device's own maps: bit for bit, no pixel left out
        with np.errstate(all="ignore"):
            assert _same(ratio, a / (a + b)), k
            want_inv = np.where(a / (a + b) < 0.5, 0.00001, mu)
            assert _same(inv, want_inv), k
            assert _same(depth, 1.0 / want_inv), k
        # the oracle, leaving out only what sits within rounding of 0.5
        oa, ob, omu, _ = oracle[k + 1]
        o_ratio = fc.ratio_of(oa, ob)
        decided = np.abs(o_ratio - 0.5) > 1e-9
        assert (~decided).sum() <= 0.01 * c.n, (k, int((~decided).sum()))
        fc.close(ratio, o_ratio, "update %d ratio" % k)
        o_inv = fc.masked_inv_depth(oa, ob, omu)
        fc.close(inv[decided], o_inv[decided], "update %d masked inverse depth" % k)
        fc.close(depth[decided], (1.0 / o_inv)[decided], "update %d depth" % k)
        below += int((o_inv == 0.00001).sum())
    assert below > 0          # the 1e-5 branch was reached


def test_readout_tie_on_the_device(hip_lib):
    """a / (a + b) == 0.5 is not below 0.5: a fresh filter reads its mu and 1 / mu; one outlier update later it reads 1e-5"""
    from cvids_amd.chisel import DepthFilter
    for size in ((1, 257), (7, 37)):
        gf = DepthFilter(*size)
        assert _same(gf.read(gf.RATIO), np.full(size, 0.5))
        assert _same(gf.read(gf.INV_DEPTH_MASKED), np.full(size, 0.5)) and _same(gf.read(gf.DEPTH), np.full(size, 2.0))
        gf.Update(np.full(size, 300.0), 4.05e-3)
        assert _same(gf.read(gf.B), np.full(size, 16.0)) and _same(gf.read(gf.RATIO), np.full(size, 15.0 / 31.0))
        assert _same(gf.read(gf.INV_DEPTH_MASKED), np.full(size, 0.00001)) and _same(gf.read(gf.DEPTH), np.full(size, 1.0 / 0.00001))


# ---- d. forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(7, 37), (1, 257), (1, 1)], ids=["7x37", "1x257", "1x1"])
def test_numpy_cpu_torch_and_cuda_forms_are_byte_identical(hip_lib, size):
    import torch
    from cvids_amd.chisel import DepthFilter
    c = fc.case(*size)
    forms = {"numpy": lambda a: np.array(a), "torch cpu": lambda a: torch.from_numpy(np.array(a)),
             "torch cuda": lambda a: torch.from_numpy(np.array(a)).cuda()}
    filters = {name: DepthFilter(c.H, c.W) for name in forms}
    for k in range(c.n_updates):
        for name, conv in forms.items():
            _update(filters[name], c, k, conv)
        reads = {name: [f.read(w) for w in range(7)] for name, f in filters.items()}
        for name in ("torch cpu", "torch cuda"):
            for w in range(7):
                assert _same(reads[name][w], reads["numpy"][w]), (name, k, w)
    # read(out = a device tensor): a slice in the middle of a larger tensor of sentinels
    gf, pad, sentinel = filters["numpy"], 300, -7.25
    for w in range(7):
        big = torch.full((c.n + 2 * pad,), sentinel, dtype=torch.float64, device="cuda")
        out = big[pad:pad + c.n].view(c.H, c.W)
        assert gf.read(w, out=out) is out
        host = big.cpu().numpy()
        assert (host[:pad] == sentinel).all() and (host[pad + c.n:] == sentinel).all(), w
        assert _same(host[pad:pad + c.n], gf.read(w)), w


# ---- e. no read in between --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("with_map", [False, True], ids=["scalar", "map"])
def test_eight_updates_back_to_back_from_arrays_overwritten_at_once(hip_lib, with_map, pinned):
    """the host form has consumed its arrays when Update returns: each is filled with NaN right after its call, and the one read at
    the end gives what the oracle gives on the original arrays.  Pageable numpy arrays, and page-locked CPU tensors, from which
    hipMemcpyAsync is a DMA that is still running when it returns."""
    import torch
    from cvids_amd.chisel import DepthFilter
    from oracle.depth_filter import DepthFilter as Oracle
    H, W = 480, 640
    rng = np.random.default_rng(31 + with_map + 2 * pinned)
    truth = rng.uniform(0.3, 1.2, (H, W))
    gf, of = DepthFilter(H, W), Oracle(H, W)
    before = mu_last = None
    for k in range(8):
        mu = truth + rng.normal(0.0, 0.02, (H, W))
        mu[rng.random((H, W)) < 0.03] = 300.0
        cov = rng.uniform(1e-3, 1e-2, (H, W)) if with_map else 4.05e-3
        before, mu_last = of.mu.copy(), mu.copy()
        of.update(mu, cov)
        give = (lambda a: torch.from_numpy(a.copy()).pin_memory()) if pinned else (lambda a: a.copy())
        given_mu, given_cov = give(mu), (give(cov) if with_map else cov)
        assert given_mu.dtype in (np.float64, torch.float64)                         # handed over as it is, not as a copy
        assert given_mu.is_pinned() if pinned else given_mu.flags.c_contiguous
        gf.Update(given_mu, given_cov)
        (given_mu.fill_ if pinned else given_mu.fill)(np.nan)
        if with_map:
            (given_cov.fill_ if pinned else given_cov.fill)(np.nan)
    fc.close_state(_state(gf), (of.a, of.b, of.mu, of.cov), (None, None, before, None), mu_last, "after eight updates")
    assert (of.a > 15.0).mean() > 0.9


# ---- f. long run ------------------------------------------------------------------------------------------------------------------
def test_sixty_updates(hip_lib):
    from cvids_amd.chisel import DepthFilter
    c = fc.case(*fc.LONG_SIZE, fc.LONG_UPDATES)
    want = _states(c)
    gf = DepthFilter(c.H, c.W)
    for k in range(c.n_updates):
        _update(gf, c, k)
        if k % 10 == 9 or k == c.n_updates - 1:
            fc.close_state(_state(gf), want[k + 1], want[k], c.reading(k), "update %d" % k)


# ---- g. refusals of the C entry points --------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(hip_lib):
    from cvids_amd.chisel import DepthFilter
    INVALID = 1                                                           # CHISEL_HIP_ERR_INVALID
    L = hip_lib
    h = C.c_void_p()
    assert L.chisel_hip_depth_filter_create(0, 8, -1, C.byref(h)) == INVALID and not h
    assert L.chisel_hip_depth_filter_create(8, -1, -1, C.byref(h)) == INVALID and not h
    assert L.chisel_hip_depth_filter_create(8, 8, -1, None) == INVALID
    assert L.chisel_hip_depth_filter_create(16385, 16384, -1, C.byref(h)) == INVALID and not h       # one row over 2^28 pixels
    assert L.chisel_hip_depth_filter_destroy(None) == 0
    c = fc.case(7, 37)
    gf = DepthFilter(c.H, c.W)
    for k in range(3):
        _update(gf, c, k)
    before = _state(gf)
    dst = np.full((c.H, c.W), -7.25)
    mu = np.full((c.H, c.W), 0.7)
    dev = C.c_int(-7)
    refused = (lambda: L.chisel_hip_depth_filter_read(gf.h, -1, dst.ctypes.data, 0),
               lambda: L.chisel_hip_depth_filter_read(gf.h, 7, dst.ctypes.data, 0),
               lambda: L.chisel_hip_depth_filter_read(gf.h, 2, None, 0),
               lambda: L.chisel_hip_depth_filter_read(gf.h, 2, None, 1),
               lambda: L.chisel_hip_depth_filter_read(None, 2, dst.ctypes.data, 0),
               lambda: L.chisel_hip_depth_filter_update(gf.h, None, None, 4.05e-3, 0, 0),
               lambda: L.chisel_hip_depth_filter_update(gf.h, None, mu.ctypes.data, 0.0, 0, 0),
               lambda: L.chisel_hip_depth_filter_update(gf.h, None, None, 4.05e-3, 1, 1),
               lambda: L.chisel_hip_depth_filter_update(None, mu.ctypes.data, None, 4.05e-3, 0, 0),
               lambda: L.chisel_hip_depth_filter_device(None, C.byref(dev)),
               lambda: L.chisel_hip_depth_filter_device(gf.h, None))
    for call in refused:          # one at a time: the state is looked at after each refusal
        assert call() == INVALID
        assert dev.value == -7
        assert (dst == -7.25).all()
        for got, want in zip(_state(gf), before):
            assert _same(got, want)
    assert L.chisel_hip_depth_filter_device(gf.h, C.byref(dev)) == 0 and dev.value == gf.device_id >= 0


# ---- h. the binding's checks ------------------------------------------------------------------------------------------------------
def test_binding_refuses_what_it_cannot_hand_over(hip_lib):
    import torch
    from cvids_amd.chisel import DepthFilter
    H, W = 7, 37
    c = fc.case(H, W)
    gf = DepthFilter(H, W)
    for k in range(3):
        _update(gf, c, k)
    before = _state(gf)
    ok64 = torch.full((H, W), 0.7, dtype=torch.float64, device="cuda")
    host = np.full((H, W), 0.7)
    bad_updates = [
        (torch.full((H, W), 0.7, dtype=torch.float32, device="cuda"), 4.05e-3),        # would be read as doubles past its end
        (torch.full((H, W), 0.7, dtype=torch.float16, device="cuda"), 4.05e-3),
        (torch.full((H, W + 1), 0.7, dtype=torch.float64, device="cuda"), 4.05e-3),
        (torch.full((H * W,), 0.7, dtype=torch.float64, device="cuda"), 4.05e-3),
        (ok64, torch.full((H, W), 4e-3, dtype=torch.float32, device="cuda")),
        (ok64, torch.full((W, H), 4e-3, dtype=torch.float64, device="cuda")),
        (ok64, np.full((H, W), 4e-3)),                                                  # device mu, host covariance
        (host, torch.full((H, W), 4e-3, dtype=torch.float64, device="cuda")),           # host mu, device covariance
        (torch.full((H, W), 0.7, dtype=torch.float64), torch.full((H, W), 4e-3, dtype=torch.float64, device="cuda")),
        (np.full((H, W + 1), 0.7), 4.05e-3),
        (host, np.full((H + 1, W), 4e-3)),
        ([[0.7] * W] * H, 4.05e-3),
    ]
    if torch.cuda.device_count() > 1:
        other = "cuda:%d" % ((gf.device_id + 1) % torch.cuda.device_count())
        bad_updates.append((torch.full((H, W), 0.7, dtype=torch.float64, device=other), 4.05e-3))
        bad_updates.append((ok64, torch.full((H, W), 4e-3, dtype=torch.float64, device=other)))
    for mu, cov in bad_updates:
        with pytest.raises((TypeError, ValueError)):
            gf.Update(mu, cov)
        with pytest.raises((TypeError, ValueError)):
            gf.Update(mu, cov, reciprocal=True)
    bad_outs = [torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W + 1), dtype=torch.float64, device="cuda"),
                torch.empty((H * W,), dtype=torch.float64, device="cuda"), torch.empty((H, W), dtype=torch.float64),
                np.empty((H, W)), torch.empty((H, 2 * W), dtype=torch.float64, device="cuda")[:, ::2]]
    if torch.cuda.device_count() > 1:
        bad_outs.append(torch.empty((H, W), dtype=torch.float64, device=other))
    for out in bad_outs:
        with pytest.raises((TypeError, ValueError)):
            gf.read(gf.INV_DEPTH, out=out)
    for got, want in zip(_state(gf), before):
        assert _same(got, want)
    # what is still accepted: a float32 numpy array (converted), a float32 CPU tensor, a non-contiguous CUDA tensor of doubles
    mu32 = c.updates[3][0].astype(np.float32)
    twin = DepthFilter(H, W)
    for k in range(3):
        _update(twin, c, k)
    third = DepthFilter(H, W)
    for k in range(3):
        _update(third, c, k)
    fourth = DepthFilter(H, W)
    for k in range(3):
        _update(fourth, c, k)
    gf.Update(mu32, 4.05e-3)
    twin.Update(mu32.astype(np.float64), 4.05e-3)
    third.Update(torch.from_numpy(mu32), 4.05e-3)
    wide = torch.zeros((H, 2 * W), dtype=torch.float64, device="cuda")
    wide[:, ::2] = torch.from_numpy(mu32.astype(np.float64)).cuda()
    fourth.Update(wide[:, ::2], 4.05e-3)
    for w in range(4):
        assert _same(gf.read(w), twin.read(w)) and _same(third.read(w), twin.read(w)) and _same(fourth.read(w), twin.read(w)), w
    assert not _same(gf.read(gf.A), before[0])


# ---- i. DepthEstimator ------------------------------------------------------------------------------------------------------------
def test_depth_estimator_drives_the_filter_with_the_float_constant(hip_lib):
    """cov_all is the FLOAT product (3 * DEP_SAMPLE) * (3 * DEP_SAMPLE) widened (depth_estimator.cpp:293), and one FuseNewFrame
    leaves the filter where a DepthFilter updated by hand with the mapper's map, that constant and reciprocal = True is"""
    import torch
    from cvids_amd import chisel as ch
    rw, rh, W, H = 80, 60, 64, 48
    K = (60.0, 60.0, 40.0, 30.0)
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:rh, 0:rw + 8]
    scene = np.clip(128 + 50 * np.sin(0.9 * xx + 0.3 * yy) + 40 * np.sin(0.37 * xx - 0.8 * yy) + rng.normal(0, 6, xx.shape), 0, 255).astype(np.uint8)
    ref, match = np.ascontiguousarray(scene[:, 4:4 + rw]), np.ascontiguousarray(scene[:, 1:1 + rw])
    pose0, pose1 = (np.eye(3), np.zeros(3)), (np.eye(3), np.array([0.1, 0.0, 0.0]))
    for dep_sample in (None, 0.0213):
        params = ch.stereo_default_params()
        if dep_sample is not None:
            params.dep_sample = dep_sample
        ds = np.float32(params.dep_sample)
        est = ch.DepthEstimator(torch.from_numpy(ref).cuda(), pose0, *K, 0.0, 0.0, 0.0, 0.0, width=W, height=H, params=params)
        f32 = (np.float32(3) * ds) * (np.float32(3) * ds)
        assert type(f32) is np.float32 and est.cov_all == float(f32)
        assert est.cov_all != (3 * float(ds)) * (3 * float(ds))                        # not the double product
        est.FuseNewFrame(torch.from_numpy(match).cuda(), pose1)
        depth = est._depth.cpu().numpy()                                               # what OutputImage wrote
        assert depth.shape == (rh, rw)
        hand = ch.DepthFilter(rh, rw)
        hand.Update(est._depth.clone(), est.cov_all, reciprocal=True)
        for w in range(7):
            assert _same(est.read(w), hand.read(w)), w
        with np.errstate(all="ignore"):
            x = 1.0 / depth
        out = (x < 0.01) | (x > 100)
        assert out.any() and (~out & ~np.isnan(x)).any()                               # the map holds outliers and kept readings
        assert _same(hand.read(hand.B)[out], np.full(int(out.sum()), 16.0))
        assert (hand.read(hand.A)[~out & ~np.isnan(x)] != 15.0).all()
