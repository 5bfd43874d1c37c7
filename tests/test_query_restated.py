"""The definition of chisel_hip_cast_rays (DESIGN.md "Querying points and rays"), checked on the CPU through its numpy restatement
(tests/query_restated.py): a view's rays give chisel_hip_render_view's depth bit for bit, the views that must stay without a hit,
rays over a map whose answers can be written down, and the layout of the two new ABI entries.  tests/test_gpu_query.py then holds
the kernels to this restatement bit for bit."""
import ctypes

import numpy as np
import pytest

from cvids_amd import synth
from tests import query_restated as qr
from tests import render_restated as rr

W, H = 160, 120
NEAR, FAR = 0.05, 5.0
KINDS = {"constant": 0, "inverse": 1, "quadratic": 2}

# scene, chunk edge, resolution, (truncator kind, parameter), frames integrated, pose whose view is cast
MAPS = [
    ("sphere_room", 16, 0.02, ("inverse", 2.0), 8, 4),
    ("box_room", 8, 0.03, ("constant", 0.1), 6, 3),
    ("box_room", 32, 0.02, ("inverse", 2.0), 7, 4),
]


def oracle_index(oracle_mod, scene, N, res, trunc, n_frames):
    om = oracle_mod.OracleMap(N, res, False)
    om.set_integrator(KINDS[trunc[0]], trunc[1], 1.0, True, 0.05)
    intr = synth.intrinsics(W, H)
    for depth, pose in synth.stream(scene, n_frames, W, H):
        om.integrate_depth(depth, pose, intr, NEAR, FAR)
    return rr.VoxelIndex(om.fields(), N, res)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN masks differ at %d places" % (what, int((gn != wn).sum()))
    assert np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]), what


@pytest.mark.parametrize("scene,N,res,trunc,n_frames,pose_k", MAPS)
def test_pinhole_rays_equal_render_depth(oracle_mod, scene, N, res, trunc, n_frames, pose_k):
    """t_hit of a view's rays (t_near = near, t_far = far on every ray) is render_restated.render_depth's image, every pixel, from the
    map's own pose and from pose 20, which looks past what was observed; a hit is exactly a finite depth"""
    index = oracle_index(oracle_mod, scene, N, res, trunc, n_frames)
    intr = synth.intrinsics(W, H)
    for k in (pose_k, 20):
        pose = synth.trajectory_pose(k)
        t_hit, status = qr.cast_rays(index, qr.view_rays(pose, intr, W, H, NEAR, FAR))
        same_bits(t_hit.reshape(H, W), rr.render_depth(index, pose, intr, W, H, NEAR, FAR), "pose %d" % k)
        assert np.array_equal(status == 1, np.isfinite(t_hit))
        share = [float((status == v).mean()) for v in range(3)]
        print("%s N=%d pose %d: status 0 / 1 / 2 shares %.4f / %.4f / %.4f" % (scene, N, k, *share))
        if k == pose_k:
            assert share[1] >= 0.99
        else:
            assert share[1] > 0.3 and share[0] > 0.05  # partly outside what the frames observed


def test_views_without_a_hit(oracle_mod):
    scene, N, res, trunc, n_frames, _ = MAPS[0]
    index = oracle_index(oracle_mod, scene, N, res, trunc, n_frames)
    intr = synth.intrinsics(W, H)
    want = {"outside": 0, "unobserved_half": 0, "behind_wall": 2}
    for name, (pose, far) in rr.no_hit_views().items():
        t_hit, status = qr.cast_rays(index, qr.view_rays(pose, intr, W, H, NEAR, far))
        assert np.isnan(t_hit).all(), name
        assert (status == want[name]).all(), (name, np.bincount(status, minlength=3))


def test_hand_made_plane():
    """N = 16, 2 cm voxels, the surface at z0 = 0.2 (the face between voxel layers 9 and 10).  A ray from (0.16, 0.16, -0.05) along +z
    with t_near = 0 and a step of one voxel samples world z = -0.05 + 0.02 k: sample 12 (z = 0.19) lies in layer 9 (s = +0.01),
    sample 13 (z = 0.21) in layer 10 (s = -0.01).  By the formula, in float32:
        t_hit = (0 + 12 step) + step (s_12 / (s_12 - s_13)),   about 0.24 + 0.01 = 0.25"""
    N, res = 16, 0.02
    index = rr.VoxelIndex(qr.plane_chunk(N, res, 0.2, +1.0), N, res)
    step = index.res
    s12, s13 = index.sdf[0, 9 * N * N], index.sdf[0, 10 * N * N]
    assert s12 > 0 > s13
    o = np.array([0.16, 0.16, -0.05], np.float32)
    expect = (np.float32(0.0) + np.float32(12) * step) + step * (s12 / (s12 - s13))
    assert abs(float(expect) - 0.25) < 1e-6
    nan = np.float32(np.nan)
    rays = np.stack([
        qr.pack(o, [[0, 0, 1]], 0.0, 0.5)[0],    # 0: the hit
        qr.pack(o, [[0, 0, 1]], 0.0, 0.2)[0],    # 1: t_far in front of the plane (the last sample is k = 10, z = 0.15)
        qr.pack(o, [[0, 0, 1]], 0.5, 0.0)[0],    # 2: t_far < t_near
        qr.pack(o, [[0, 0, 1]], nan, 0.5)[0],    # 3: a NaN bound
        qr.pack(o, [[0, 0, 1]], 0.0, nan)[0],    # 4: the other one
        qr.pack(o, [[0, 0, 2]], 0.0, 0.5)[0],    # 5: the direction doubled
        qr.pack([0.16, 0.16, 0.31], [[0, 0, -1]], 0.0, 0.5)[0],  # 6: from behind the plane: the first observed sample is <= 0
        qr.pack([nan, 0.16, -0.05], [[0, 0, 1]], 0.0, 0.5)[0],   # 7: a NaN origin
    ])
    assert qr.sample_counts(rays, step).tolist() == [26, 11, 0, 0, 0, 26, 26, 0]
    t_hit, status = qr.cast_rays(index, rays)
    assert status.tolist() == [1, 0, 0, 0, 0, 1, 2, 0]
    assert t_hit[0].tobytes() == np.float32(expect).tobytes()
    # the doubled direction samples z = -0.05 + 0.04 k: sample 6 (z = 0.19, s_12's layer) and sample 7 (z = 0.23, layer 11, s = -0.03):
    s11 = index.sdf[0, 11 * N * N]
    expect2 = (np.float32(0.0) + np.float32(6) * step) + step * (s12 / (s12 - s11))
    assert t_hit[5].tobytes() == np.float32(expect2).tobytes()
    assert abs(float(expect2) - 0.125) < 1e-6  # 0.12 + 0.02 * (0.01 / 0.04): half of 0.25
    assert np.isnan(t_hit[[1, 2, 3, 4, 6, 7]]).all()
    # per-ray independence: any order, any neighbours
    perm = np.array([5, 0, 7, 3, 6, 1, 4, 2])
    t2, s2 = qr.cast_rays(index, rays[perm])
    same_bits(t2, t_hit[perm], "permuted")
    assert np.array_equal(s2, status[perm])


def test_point_read_out_on_the_plane():
    """weight where the voxel exists, observed or not; NaN outside the chunk and for non-finite positions"""
    N, res = 16, 0.02
    fields = qr.plane_chunk(N, res, 0.2, +1.0)
    fields[(0, 0, 0)][1][5] = 0.0  # voxel (5, 0, 0): unobserved
    index = rr.VoxelIndex(fields, N, res)
    pos = np.array([[0.01, 0.01, 0.01], [0.11, 0.01, 0.01], [-0.01, 0.01, 0.01], [np.nan, 0.01, 0.01], [0.01, np.inf, 0.01]], np.float32)
    found, sdf, weight = qr.query_points(index, pos)
    assert found.tolist() == [True, False, False, False, False]
    assert sdf[0] == index.sdf[0, 0] and np.isnan(sdf[1:]).all()
    assert weight[0] == 1.0 and weight[1] == 0.0 and np.isnan(weight[2:]).all()


def test_abi_layout_of_the_query_entries(hip_lib):
    from cvids_amd import capi
    assert ctypes.sizeof(capi.Ray) == 32
    for name in ("chisel_hip_query_points", "chisel_hip_cast_rays"):
        assert hasattr(hip_lib, name), name
        assert name in capi.EXPORTS
