"""The definition of chisel_hip_align_terms / _solve / _depth (DESIGN.md "Aligning a frame to the map"), checked on the CPU through its
numpy restatement (tests/align_restated.py): the gradient against the oracle's GetSDFAndGradient, the summation tree against
hand-made vectors, the product's host solver against the restated one bit for bit, and that the definition converges on the scenes the
GPU tests use.  tests/test_gpu_align.py then holds the kernels to this restatement bit for bit."""
import ctypes
import functools
import math

import numpy as np
import pytest

from cvids_amd import synth
from tests import align_restated as ar
from tests import query_restated as qr
from tests import render_restated as rr

W, H = ar.W, ar.H
NEAR, FAR = ar.NEAR, ar.FAR
KINDS = {"constant": 0, "inverse": 1, "quadratic": 2}
INTR = synth.intrinsics(W, H)


def oracle_map(oracle_mod, frames, N, res, trunc):
    om = oracle_mod.OracleMap(N, res, False)
    om.set_integrator(KINDS[trunc[0]], trunc[1], 1.0, True, 0.05)
    for depth, pose in frames:
        om.integrate_depth(depth, pose, INTR, NEAR, FAR)
    return om


@functools.lru_cache(maxsize=None)
def _corner(case):
    import oracle
    N, res, trunc = ar.CORNER_MAPS[case]
    om = oracle_map(oracle, ar.corner_frames(), N, res, trunc)
    return om, rr.VoxelIndex(om.fields(), N, res)


@pytest.fixture
def corner(oracle_mod):
    return _corner


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("case", range(len(ar.CORNER_MAPS)))
def test_gradient_against_the_oracle(corner, case):
    """grad_sample agrees with the oracle's ChunkManager::GetSDFAndGradient in found flag, distance bits and gradient bits, at every
    13th hit point of the corner view and at a copy of them jittered by N(0, 2 voxels); both answers occur"""
    om, index = corner(case)
    res = ar.CORNER_MAPS[case][1]
    hits = rr.hit_points(ar.corner_pose(ar.CORNER_VIEW), INTR, ar.corner_frame())[::13]
    hits = hits[np.isfinite(hits).all(1)]
    rng = np.random.default_rng(synth.SEED)
    pts = np.concatenate([hits, (hits + rng.normal(0.0, 2.0 * res, hits.shape)).astype(np.float32)])
    found, d0, g = ar.grad_sample(index, pts)
    mismatches = 0
    for i, p in enumerate(pts):
        ok, dist, grad = om.get_sdf_and_gradient(p)
        same = ok == bool(found[i])
        if ok and same:
            same = np.float64(d0[i]).tobytes() == np.float64(dist).tobytes() and g[i].tobytes() == grad.tobytes()
        mismatches += not same
    print("map %d: %d points, found %.3f, %d mismatches" % (case, len(pts), float(found.mean()), mismatches))
    assert mismatches == 0
    assert found.any() and not found.all()


def test_summation_tree():
    """pairwise against vectors whose sum depends on the order, at lengths 1, 255, 256, 257 and 65 537"""
    big = 2.0 ** 53  # doubles are 2 apart from here on: big + 1 -> big and big + 3 -> big + 4 (ties to even), big + 2 is exact
    assert ar.pairwise([3.5]) == 3.5
    assert bits(ar.pairwise([-0.0]))[()] == 0  # (-0.0 + +0.0: the padding is +0.0)
    x = np.zeros(256)
    x[0], x[1], x[2] = big, 1.0, 1.0
    assert ar.pairwise(x) == big        # (big + 1) + (1 + 0): the ones are lost one by one; 1 + 1 first would give big + 2
    x = np.zeros(256)
    x[0], x[2], x[3] = big, 1.0, 1.0
    assert ar.pairwise(x) == big + 2.0  # (big + 0) + (1 + 1); left to right would give big
    # 255 values, the last slot is padding: level 1 is big + 1 -> big, 126 times 1 + 1, and 1 + 0; from there on every sum is exact
    # up to the last one, (big + 126) + 127 = big + 253 -> big + 252.  The exact sum is big + 254.
    x = np.ones(255)
    x[0] = big
    assert ar.pairwise(x) == big + 252.0
    # 257 values, a second group of one: group 0 is (big + 0) + (1 + 1) = big + 2, group 1 is 1, and big + 3 -> big + 4
    x = np.zeros(257)
    x[0], x[2], x[3], x[256] = big, 1.0, 1.0, 1.0
    assert ar.pairwise(x) == big + 4.0
    # 65 537 values: 257 groups, then 2 groups, then 1 -- against the same tree written as plain loops
    rng = np.random.default_rng(synth.SEED)
    x = rng.normal(0.0, 1.0, 65537) * 10.0 ** rng.integers(-8, 8, 65537)

    def by_hand(v):
        v = list(v)
        while True:
            v += [0.0] * ((-len(v)) % 256)
            groups = []
            for g in range(0, len(v), 256):
                lvl = v[g:g + 256]
                for _ in range(8):
                    lvl = [lvl[2 * j] + lvl[2 * j + 1] for j in range(len(lvl) // 2)]
                groups.append(lvl[0])
            v = groups
            if len(v) == 1:
                return v[0]

    got = ar.pairwise(x)
    assert got == by_hand(x.tolist())
    assert got != sum(x.tolist())  # (left to right: an order-dependent vector)
    for n in (1, 255, 256, 257):
        assert ar.pairwise(x[:n]) == by_hand(x[:n].tolist()), n


def test_solver_against_the_restatement(hip_lib, corner):
    """chisel_hip_align_solve (host code of the product, no GPU) bit for bit against ar.solve on the restated terms of the corner
    scene, damping 0 and 1e-3; all-zero terms with damping 0 are degenerate; the struct sizes"""
    from cvids_amd import capi, chisel
    assert ctypes.sizeof(capi.AlignParams) == 40 and ctypes.sizeof(capi.AlignResult) == 664
    for name in ("chisel_hip_align_terms", "chisel_hip_align_solve", "chisel_hip_align_depth"):
        assert hasattr(hip_lib, name) and name in capi.EXPORTS
    depth = ar.corner_frame()
    true_pose = ar.corner_pose(ar.CORNER_VIEW)
    for case in range(len(ar.CORNER_MAPS)):
        _, index = corner(case)
        for pose in (true_pose, ar.start_pose(true_pose, ar.CORNER_STARTS[0])):
            T = ar.terms(index, depth, pose, INTR, NEAR, FAR)
            assert T[28] > 0.5 * T[29] > 0
            for damping in (0.0, 1e-3):
                want = ar.solve(T, damping)
                got = chisel.align_solve(T, damping)
                assert want is not None and np.array_equal(bits(got), bits(want)), (case, damping, got, want)
                assert np.abs(got).max() > 0
    with pytest.raises(capi.ChiselHipError) as e:
        chisel.align_solve(np.zeros(32), 0.0)
    assert e.value.code == 5
    assert ar.solve(np.zeros(32), 0.0) is None
    dp = ctypes.POINTER(ctypes.c_double)
    xi = np.zeros(6)
    assert hip_lib.chisel_hip_align_solve(None, 0.0, xi.ctypes.data_as(dp)) == 1
    assert hip_lib.chisel_hip_align_solve(np.zeros(32).ctypes.data_as(dp), 0.0, None) == 1


@pytest.mark.parametrize("case", range(len(ar.CORNER_MAPS)))
def test_the_definition_converges(corner, case):
    """10 iterations, damping 1e-3, max_residual 0 and 0.1, from the three starts: translation and rotation error each end at most
    half of where they started, and at least 0.75 of the valid pixels are used in the first iteration"""
    _, index = corner(case)
    depth, true_pose = ar.corner_frame(), ar.corner_pose(ar.CORNER_VIEW)
    for offset in ar.CORNER_STARTS:
        for max_residual in (0.0, 0.1):
            run = ar.align(index, depth, ar.start_pose(true_pose, offset), INTR, NEAR, FAR, max_iterations=10, max_residual=max_residual, damping=1e-3)
            assert run["status"] in (ar.ITERATION_LIMIT, ar.CONVERGED)
            ar.check_corner_run(run["poses"], run["terms_first"], true_pose, "map %d start %s max_residual %g" % (case, offset, max_residual))


def test_the_wall_pins_absolute_damping(oracle_mod):
    """a plane leaves the translation inside it and the rotation about its normal unobserved.  Damping 1e-3 per used pixel leaves them
    alone: the error along z ends below 1 mm, the rotation error below 0.05 degrees, and the total translation error does not grow
    (without damping, or with damping relative to the diagonal, Cholesky does not fail on the noise and the pose slides along the wall)"""
    N, res, trunc, n_frames, view = ar.WALL_MAP
    om = oracle_map(oracle_mod, list(synth.stream("wall", n_frames, W, H)), N, res, trunc)
    index = rr.VoxelIndex(om.fields(), N, res)
    true_pose = synth.trajectory_pose(view)
    depth = synth.render_depth("wall", true_pose, INTR, W, H)
    start = ar.start_pose(true_pose, ar.WALL_START)
    run = ar.align(index, depth, start, INTR, NEAR, FAR, max_iterations=10, damping=1e-3)
    t0, r0 = ar.pose_errors(start, true_pose)
    t1, r1 = ar.pose_errors(run["pose"], true_pose)
    dz = abs(run["pose"][2, 3] - float(true_pose[2, 3]))
    print("wall: translation %.2f -> %.2f mm (z %.3f mm), rotation %.3f -> %.3f deg, status %d" % (1e3 * t0, 1e3 * t1, 1e3 * dz, r0, r1, run["status"]))
    assert dz < 1e-3
    assert r1 < 0.05
    assert t1 <= t0
