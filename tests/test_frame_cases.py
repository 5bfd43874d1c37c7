"""The frame cases of tests/frame_cases.py reach what they claim -- on the oracle alone (no GPU): a parity test over them says something
about a bound of the cull kernels only if the frames put voxels next to that bound.  The floors are the smallest figures measured over the
cases of each test (DESIGN.md "What the frame tests cover" has the table), some rounded down a little."""
import numpy as np
import pytest

from tests import frame_cases as fc

W, H = 64, 48


@pytest.fixture(scope="module")
def reach(oracle_mod):
    """(camera, pose, image) -> Reach of that one frame on an empty map of 8^3 voxels of 5 cm, computed once"""
    cache = {}

    def get(cam, pose, image, N=8, res=0.05, size=(W, H)):
        key = (cam, pose, image, N, res, size)
        if key not in cache:
            om = oracle_mod.OracleMap(N, res, False)
            om.set_integrator(oracle_mod.TRUNC_INVERSE, 2.0, 1.0, True, 0.05)
            intr = fc.camera(cam, *size)
            cache[key] = fc.integrate_and_reach(om, fc.depth_image(image, *size), fc.pose(pose), intr, size[0], size[1], far=intr[5])[0]
        return cache[key]

    return get


def test_poses_are_rigid_and_cameras_as_specified():
    for name in fc.POSE_NAMES:
        T = fc.pose(name).astype(np.float64)
        assert T.dtype == np.float64 and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-6) and np.linalg.det(T[:3, :3]) > 0.999
        assert np.allclose(T[:3, 3], fc.POSES[name][1], atol=2e-4) and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.allclose(fc.pose("down")[:3, :3], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], atol=1e-7)   # Rx(90)
    assert np.array_equal(fc.pose("axis")[:3, :3], np.eye(3, dtype=np.float32))
    assert fc.camera("aniso", 640, 480)[:4] == (300.0, 700.0, 192.0, 384.0)
    assert fc.camera("cx_out", 64, 48)[2] < 0 and fc.camera("cx_out", 64, 48)[3] > 48
    assert fc.camera("wide", 64, 48)[5] == 1.5 and all(fc.camera(c, 64, 48)[4] == 0.05 for c in fc.CAMERA_NAMES)


def test_images_are_as_specified():
    for (w, h) in fc.SIZES:
        for name in fc.IMAGE_NAMES:
            d = fc.depth_image(name, w, h)
            assert d.shape == (h, w) and d.dtype == np.float32 and d.flags.c_contiguous
    steps = fc.depth_image("steps", 260, 196)
    for s in (4, 8, 16, 32, 64):  # every pyramid texel of 8 x 8 pixels and up holds both values, and 27 in 35 of the 4 x 4 ones
        t = steps[:196 // s * s, :260 // s * s].reshape(196 // s, s, 260 // s, s)
        both = (t.min((1, 3)) < 1.0) & (t.max((1, 3)) > 2.0)
        assert both.all() if s >= 8 else both.mean() > 0.7, (s, both.mean())
    sp = fc.depth_image("sparse", 64, 48)
    assert np.isfinite(sp).sum() in range(12, 17) and np.isfinite(sp[[0, 0, -1, -1], [0, -1, 0, -1]]).all()
    bd = fc.depth_image("border", 64, 48)
    assert np.isnan(bd[1:-1, 1:-1]).all() and np.isfinite(bd).sum() == 2 * 64 + 2 * 46
    cl = fc.depth_image("close", 64, 48)
    assert cl.min() >= 0.06 and cl.max() <= 0.36
    assert fc.CARVE_DEPTHS == [1.2, 1.2, 1.2, 2.4, 2.4, 1.2, 2.4, 1.2, 2.4, 1.2, 2.4]
    names = [n for n, _, _ in fc.unrelated_views(64, 48)]
    assert len(set(names)) == 17 and all(a.split("-")[0] != b.split("-")[0] for a, b in zip(names, names[1:]))
    assert len(fc.all_frames(64, 48)) == 36


@pytest.mark.parametrize("pose", ["tilt", "far30"])
@pytest.mark.parametrize("cam", ["centred", "aniso", "cx_out"])
def test_reach_of_the_hostile_images(reach, cam, pose):
    r = reach(cam, pose, "steps")
    assert r.border >= 500 and r.straddle_img >= 60, r.as_dict()     # smallest measured: 506, 62
    r = reach(cam, pose, "sparse")
    assert r.few >= 10, r.as_dict()                                   # 18
    r = reach(cam, pose, "border")
    assert r.updated >= 300 and r.border == r.updated and r.off_border == 0, r.as_dict()  # 393
    r = reach(cam, pose, "close")
    assert r.near >= 15 and r.straddle_z >= 2, r.as_dict()            # 19, 2


def test_carve_sequence_carves(oracle_mod):
    om = oracle_mod.OracleMap(8, 0.05, False)
    om.set_integrator(oracle_mod.TRUNC_INVERSE, 2.0, 1.0, True, 0.0)
    intr = fc.camera("centred", W, H)
    carved = []
    for d, p in fc.carve_frames(W, H):
        om.integrate_depth(d, p, intr[:4], intr[4], intr[5])
        carved.append(om.counters()["carved"])
    assert sum(carved) > 10000, carved                                # 14 552
    # every far wall that follows a near one carves what that one left (the second far wall of the pair finds nothing left)
    assert [c > 0 for c in carved] == [d == 2.4 and fc.CARVE_DEPTHS[i - 1] == 1.2 for i, d in enumerate(fc.CARVE_DEPTHS)], carved


@pytest.mark.parametrize("pose,floor", [("tilt", 6), ("far30", 4)])
def test_close_surface_gives_pixel_boxes_wider_than_the_coarsest_level(reach, pose, floor):
    """261 x 197, 16^3 voxels of 4 cm, camera `aniso` (what test_sizes of the GPU tests runs): updated chunks whose corners span more
    than 192 pixels or reach behind the camera -- the whole-image fallback of pyramid_minmax.  Measured: 6 and 4."""
    r = reach("aniso", pose, "close", N=16, res=0.04, size=(261, 197))
    assert r.wide_box >= floor and r.straddle_z >= 1, r.as_dict()


@pytest.mark.parametrize("pose", ["tilt", "far30"])
@pytest.mark.parametrize("image", ["wall", "steps", "ramp"])
def test_tele_camera_updates_something(reach, pose, image):
    assert reach("tele", pose, image).updated >= 1


def test_deep_carve_sequence_carves(oracle_mod):
    om = oracle_mod.OracleMap(8, 0.05, False)
    om.set_integrator(oracle_mod.TRUNC_INVERSE, 2.0, 1.0, True, fc.DEEP_CARVING_DIST)
    intr = fc.camera("centred", W, H)
    carved = []
    for d, p in fc.deep_carve_frames(W, H):
        om.integrate_depth(d, p, intr[:4], intr[4], intr[5])
        carved.append(om.counters()["carved"])
    assert carved[0] == carved[2] == 0 and carved[1] >= 80 and carved[3] >= 80, carved   # 88 each


@pytest.mark.parametrize("cam", ["wide", "cx_out"])
@pytest.mark.parametrize("image", fc.EDGE_IMAGE_NAMES)
def test_close_surface_at_the_image_edge_reaches_chunks_behind_the_camera(reach, cam, image):
    """updated chunks with a corner behind the camera plane or within a quarter voxel of it (`axis`: the plane is a chunk boundary, so none of
    their voxels is behind it; `down`: some are).  Measured: 5-708 updated voxels, 2-19 such chunks."""
    r = reach(cam, "axis", image)
    assert r.updated >= 5 and r.wide_box >= 2, r.as_dict()
    r = reach(cam, "down", image)
    assert r.updated >= 5 and r.wide_box >= 2 and r.straddle_z >= 1, r.as_dict()
