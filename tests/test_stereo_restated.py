"""The CPU restatement of the stereo matcher (tests/stereo_restated.py) checked against itself and by hand, and the library's
stereo entry points on a machine without the GPU.  No GPU needed."""
import numpy as np
import pytest

import stereo_restated as sr

f32 = np.float32


def scene(W, H, seed):
    """a random textured pair, a P2 weight map in the reference's range (0.8 + ..., sgm_stereo_mapper.cpp:81) and a sparse
    prior with a few pixels set (the reference's map is -1 elsewhere, :229)"""
    rng = np.random.default_rng(seed)
    ref = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    match = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    p2w = (0.8 + rng.uniform(0.0, 1.5, (H, W))).astype(np.float32)
    sd = np.full((H, W), -1.0, np.float32)
    dist = np.zeros((H, W), np.float32)
    idx = rng.choice(H * W, H * W // 8, replace=False)
    sd.flat[idx] = rng.uniform(0.4, 6.0, idx.size).astype(np.float32)
    dist.flat[idx] = rng.uniform(0.0, 1.0, idx.size).astype(np.float32)
    return ref, match, p2w, sd, dist


def random_pose(W, H, seed, shift=0.1):
    """R = K2 R_m^T R_r K1^-1, t = K2 R_m^T (t_r - t_m) for a random small motion (the reference's construction)"""
    from cvids_amd.chisel import stereo_homography
    rng = np.random.default_rng(seed)
    fx = 460.95 * W / 640.0
    K = np.array([[fx, 0, W / 2.0], [0, fx, H / 2.0], [0, 0, 1.0]])
    a = rng.normal(0.0, 0.05, 3)
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rm = np.eye(3) + ax + ax @ ax / 2.0
    u, _, vt = np.linalg.svd(Rm)
    Rm = u @ vt
    return stereo_homography(K, K, np.eye(3), np.zeros(3), Rm, rng.normal(0.0, shift, 3))


def run_sequence(cls, W, H, seed):
    """set_reference, 3 updates, output, clear, 2 updates (counts 4 and 5 on a zeroed cost), output with a sparse prior,
    set_reference again and one update: every state the sequence passes through"""
    ref, match, p2w, sd, dist = scene(W, H, seed)
    rng = np.random.default_rng(seed + 1)
    s = cls(W, H)
    states = []
    s.set_reference(ref, p2w)
    for k in range(3):
        s.update(np.roll(match, k, axis=1) + f32(k), *random_pose(W, H, seed * 10 + k))
        states.append(("cost", s.cost.copy()))
    s.output()
    states += [("sgm", s.sgm.copy()), ("depth", s.depth.copy()), ("cost", s.cost.copy())]
    s.clear()
    for k in range(2):
        s.update(match * f32(0.9) + rng.uniform(0, 3, match.shape).astype(np.float32), *random_pose(W, H, seed * 10 + 5 + k))
        states.append(("cost", s.cost.copy()))
    s.output(sd, dist)
    states += [("cost", s.cost.copy()), ("sgm", s.sgm.copy()), ("depth", s.depth.copy())]
    s.set_reference(match, p2w)
    s.update(ref, *random_pose(W, H, seed * 10 + 9))
    states.append(("cost", s.cost.copy()))
    return states


def test_scalar_and_vectorised_restatements_agree_bit_for_bit():
    W, H = 24, 16
    a = run_sequence(sr.ScalarStereo, W, H, 3)
    b = run_sequence(sr.VectorisedStereo, W, H, 3)
    assert [n for n, _ in a] == [n for n, _ in b]
    for k, ((name, x), (_, y)) in enumerate(zip(a, b)):
        assert sr.same_bits(x, y), "state %d (%s) differs" % (k, name)
    # the sequence reaches every rule: -1 entries (border, out-of-image taps), valid costs, the prior, accepted and rejected depths
    cost1 = a[0][1]
    assert (cost1 == -1).any() and (cost1 > 0).any()
    assert (cost1[1:-1, 1:-1] == -1).any(axis=2).any()            # an interior pixel with a tap out of the image
    depths = np.stack([x for n, x in a if n == "depth"])
    assert (depths == 1000).any() and (depths != 1000).any()


def test_cleared_cost_divides_by_the_running_count():
    """ClearRawCost keeps m_nMeasurementCount (sgm_stereo_mapper.cpp:202-216): after a clear, update k divides a fresh cost by k
    and leaves the border unmarked"""
    W, H = 40, 30
    ref, match, p2w, _, _ = scene(W, H, 5)
    R, t = np.eye(3, dtype=np.float32), np.array([0.0, 3.0, 0.0], np.float32)   # a vertical shift: row 0 finds match rows
    a, b = sr.VectorisedStereo(W, H), sr.VectorisedStereo(W, H)
    a.set_reference(ref, p2w)
    b.set_reference(ref, p2w)
    a.update(match, R, t)
    a.clear()
    a.update(match, R, t)       # count 2 on a zeroed cost: (0 * 1 + tmp / 9) / 2
    b.update(match, R, t)       # count 1
    assert a.count == 2
    inner = b.cost[1:-1, 1:-1]
    ok = inner >= 0
    assert ok.mean() > 0.5
    assert np.array_equal(a.cost[1:-1, 1:-1][ok], (f32(0) * f32(1) + inner[ok]) / f32(2))
    assert (b.cost[0] == -1).all() and (a.cost[0] > 0).any()


def test_tie_break_is_the_trees():
    """filterCostKernel keeps its own entry unless the partner is strictly smaller: a 1-vs-2 tie gives 2, a 0-vs-64 tie 0,
    and in general the smallest bit-reversed 7-bit index wins"""
    c = np.full(128, 5.0, np.float32)
    c[[1, 2]] = 1.0
    assert sr.tree_argmin(c)[1] == 2
    c = np.full(128, 5.0, np.float32)
    c[[0, 64]] = 1.0
    assert sr.tree_argmin(c)[1] == 0
    rev = lambda i: int(format(i, "07b")[::-1], 2)
    rng = np.random.default_rng(0)
    for _ in range(200):
        c = rng.integers(0, 4, 128).astype(np.float32)
        ties = np.flatnonzero(c == c.min())
        assert sr.tree_argmin(c)[1] == min(ties, key=rev)


def test_constants():
    assert sr.DEP_SAMPLE == f32(0.019722115)
    assert sr.DEP_SAMPLE.dtype == np.float32


def test_sparse_prior_inverse_depth_is_a_double_division():
    """FuseSparseInfoKernel: float nInvDepth = 1.0 / nDepth divides in double and narrows (calc_cost.cu:697).  A double quotient
    rounded to float is the correctly rounded float quotient (53 >= 2 * 24 + 2 bits), so the float division gives the same
    value; the restatement still takes the reference's path"""
    rng = np.random.default_rng(1)
    d = rng.uniform(0.3, 8.0, 20000).astype(np.float32)
    assert np.array_equal((1.0 / d.astype(np.float64)).astype(np.float32), f32(1.0) / d)
    W, H = 4, 3
    s = sr.VectorisedStereo(W, H)
    s.cost[:] = 1.0
    s.cost[0, 0, 7] = 0.0                          # only entries > 0 take the prior
    sd = np.full((H, W), 1.7, np.float32)
    sd[2, 3] = -1.0                                # and only pixels with a depth
    dist = np.full((H, W), 0.25, np.float32)
    s._fuse(sd, dist)
    for d in (7, 40, 100):
        inv = (1.0 / np.float64(f32(1.7))).astype(np.float32)
        cur = sr.DEP_SAMPLE * f32(d)
        diff = (inv - cur if cur < inv else -inv + cur) / sr.DEP_SAMPLE
        assert s.cost[1, 2, d] == f32(1.0) + diff * f32(15.0) * f32(0.25)
    assert s.cost[0, 0, 7] == 0.0 and (s.cost[2, 3] == 1.0).all()


def test_stereo_homography_matches_the_reference_formula():
    from cvids_amd.chisel import stereo_homography
    K = np.array([[460.95, 0, 320.0], [0, 460.95, 240.0], [0, 0, 1]])
    R, t = stereo_homography(K, K, np.eye(3), np.zeros(3), np.eye(3), np.array([0.11, 0.0, 0.0]))
    assert R.dtype == np.float32 and t.dtype == np.float32
    assert np.allclose(R, np.eye(3), atol=1e-6)
    assert t[0] == f32(-0.11 * 460.95) and t[1] == 0 and t[2] == 0


def test_stereo_create_fails_loudly_without_gpu(hip_lib):
    """No CPU fallback: without a gfx950 device chisel_hip_stereo_create fails with CHISEL_HIP_ERR_HIP"""
    import ctypes as C

    from cvids_amd import capi
    if hip_lib.chisel_hip_device_count() > 0:
        pytest.skip("a gfx950 device is present")
    h = C.c_void_p()
    assert hip_lib.chisel_hip_stereo_create(64, 48, None, 0, C.byref(h)) == 2
    from cvids_amd.chisel import StereoMapper
    with pytest.raises(capi.ChiselHipError):
        StereoMapper(64, 48)


def test_stereo_default_params(hip_lib):
    """chisel_hip_stereo_default_params: host arithmetic, no GPU"""
    from cvids_amd.chisel import stereo_default_params
    p = stereo_default_params()
    assert (p.pi1, p.pi2, p.tau_so, p.sgm_q1, p.sgm_q2, p.var_scale, p.sparse_ratio) == (16, 64, 8, 1, 1, 1, 15)
    assert f32(p.dep_sample) == sr.DEP_SAMPLE
