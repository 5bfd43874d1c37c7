"""chisel_hip_align_terms, chisel_hip_align_solve and chisel_hip_align_depth on the GPU against their definition (DESIGN.md "Aligning a
frame to the map").

The 32 doubles of chisel_hip_align_terms are compared BIT FOR BIT (as uint64) with the numpy restatement (tests/align_restated.py) run
over the map as GetChunkIDs / GetChunk read it back: the kernel's summation tree must be the tree of the definition at every image
size.  A stated share only keeps a comparison from passing on an empty case; the cases that are empty by construction are checked for
exact zeros.  The loop is held to the conditions the CPU test holds the restated loop to (beyond the first iteration the two agree
only up to libm's last ulp of sin and cos, which can reach the float32 pose).  Each map is built once and only read."""
import ctypes as C
import functools

import numpy as np
import pytest

from cvids_amd import synth
from tests import align_restated as ar
from tests import render_restated as rr
from tests import test_gpu_render as tgr
from tests.common import compare_fields

pytestmark = pytest.mark.gpu
W, H = ar.W, ar.H
NEAR, FAR = ar.NEAR, ar.FAR

# name -> how the map is built and which frame is aligned to it
CASES = ["corner-16", "corner-8", "sphere_room-16", "box_room-8-colour"]


def intr_of(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def corner_map(case):
    from cvids_amd import chisel as ch
    N, res, trunc = ar.CORNER_MAPS[case]
    gm = ch.Chisel((N, N, N), res, False, max_chunks=8192)
    integ, cam = tgr.integrator(trunc, True), tgr.camera()
    for depth, pose in ar.corner_frames():
        gm.IntegrateDepthScan(integ, depth, pose, cam)
    return gm


@functools.lru_cache(maxsize=None)
def built(name):
    """-> (map, its VoxelIndex, scene, the true pose of the frame that is aligned)"""
    if name.startswith("corner"):
        gm = corner_map(CASES.index(name))
        scene, pose = "box_room", ar.corner_pose(ar.CORNER_VIEW)
    else:
        scene, N, res, trunc, n_frames, carving, color, pose_k = tgr.MAPS[0] if name == "sphere_room-16" else tgr.MAPS[2]
        gm = tgr.gpu_map(scene, N, res, trunc, n_frames, carving, color)
        pose = synth.trajectory_pose(pose_k)
    return gm, tgr.index_of(gm), scene, pose


def frame(scene, pose, w=W, h=H, **kw):
    return synth.render_depth(scene, pose, synth.intrinsics(w, h), w, h, **kw)


def centre_camera(w, h):
    """w x h pixels around the optical axis, at the focal length of the 160-pixel camera or longer: the small images look at what
    the maps' frames observed (synth.intrinsics(1, 1) looks 31 degrees off the axis, past it)"""
    from cvids_amd.chisel import PinholeCamera
    f = 525.0 * max(w, W) / 640.0
    return PinholeCamera(f, f, (w - 1) / 2.0, (h - 1) / 2.0, w, h, NEAR, FAR)


def check_terms(gm, index, depth, pose, cam, max_residual, what, empty=False):
    got = gm.AlignTerms(depth, pose, cam, max_residual=max_residual)
    want = ar.terms(index, depth, pose, intr_of(cam), cam.near_plane, cam.far_plane, max_residual)
    assert got.shape == (32,) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits(want)), "%s: terms differ at %s\n got %s\nwant %s" % (what, np.flatnonzero(bits(got) != bits(want)).tolist(), got, want)
    assert bits(got)[30] == 0 and bits(got)[31] == 0
    if empty:
        assert (bits(got)[:29] == 0).all() and got[29] > 0, (what, got)
    else:
        assert got[28] > 0.5 * got[29] > 0, "%s: %g of %g valid pixels used" % (what, got[28], got[29])
    return got


# ---- terms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_terms_bit_for_bit(name):
    """image sizes where the tree can go wrong -- 1 pixel, one full group, a second group of one, a ragged last block, two levels --
    and at 160 x 120: the true pose and a perturbed one, max_residual 0 and 0.1, a frame with 20 % NaN, a far plane that cuts half
    of the image off"""
    gm, index, scene, pose = built(name)
    for w, h in ((1, 1), (16, 16), (257, 1), (77, 53)):
        cam = centre_camera(w, h)
        got = check_terms(gm, index, synth.render_depth(scene, pose, intr_of(cam), w, h), pose, cam, 0.0, "%d x %d" % (w, h))
        assert got[29] == w * h
    depth, cam = frame(scene, pose), tgr.camera()
    moved = ar.start_pose(pose, ar.CORNER_STARTS[0])
    dropped = {}
    for p, what in ((pose, "true pose"), (moved, "perturbed pose"), (ar.start_pose(pose, ar.CORNER_STARTS[2]), "third start")):
        plain = check_terms(gm, index, depth, p, cam, 0.0, what)
        cut = check_terms(gm, index, depth, p, cam, 0.1, what + ", max_residual 0.1")
        assert cut[28] <= plain[28] and cut[29] == plain[29] == W * H
        dropped[what] = int(plain[28] - cut[28])
    print("%s: pixels max_residual 0.1 drops: %s" % (name, dropped))
    if name.startswith("corner"):
        assert dropped["third start"] > 1000  # (3 to 4 cm from the walls of a map truncated at 6 to 10 cm)
    holes = frame(scene, pose, nan_fraction=0.2)
    got = check_terms(gm, index, holes, moved, cam, 0.0, "20 % NaN")
    assert 0.7 * W * H < got[29] < 0.9 * W * H
    far = float(np.nanmedian(depth))
    got = check_terms(gm, index, depth, moved, tgr.camera(far=far), 0.0, "far plane at the median depth")
    assert 0.3 * W * H < got[29] < 0.7 * W * H


def test_terms_bit_for_bit_640x480():
    """307 200 pixels: three levels, 1200 -> 5 -> 1"""
    gm, index, scene, pose = built("corner-16")
    check_terms(gm, index, frame(scene, pose, 640, 480), ar.start_pose(pose, ar.CORNER_STARTS[1]), tgr.camera(640, 480), 0.0, "640 x 480")


def test_terms_of_the_empty_cases_are_exact_zeros():
    """an empty map, and the views of rr.no_hit_views() (the frame's points lie where nothing was observed): every sum is +0.0, the
    valid pixels are still counted"""
    from cvids_amd import chisel as ch
    gm, index, scene, pose = built("sphere_room-16")
    depth, cam = frame(scene, pose), tgr.camera()
    for name, (view, _) in rr.no_hit_views().items():
        check_terms(gm, index, depth, view, cam, 0.0, name, empty=True)
    fresh = ch.Chisel((16, 16, 16), 0.02, False, max_chunks=1024)
    check_terms(fresh, tgr.index_of(fresh), depth, pose, cam, 0.0, "empty map", empty=True)
    check_terms(fresh, tgr.index_of(fresh), frame(scene, pose, 77, 53), pose, tgr.camera(77, 53), 0.1, "empty map, 77 x 53", empty=True)


@pytest.mark.parametrize("name", ["corner-16", "box_room-8-colour"])
def test_terms_against_query_points(name):
    """with max_residual 0: terms[28] is the number of valid pixels whose QueryPoints(gradient=True) found-bit 1 is set at
    rr.hit_points of the frame, and terms[0], [6], [11] are `pairwise` of the squared gradient components QueryPoints returns"""
    gm, _, scene, pose = built(name)
    depth, cam = frame(scene, pose, nan_fraction=0.05), tgr.camera()
    moved = ar.start_pose(pose, ar.CORNER_STARTS[2])
    got = gm.AlignTerms(depth, moved, cam)
    z = depth.reshape(-1)
    valid = np.isfinite(z) & (np.float32(NEAR) <= z) & (z <= np.float32(FAR))
    pts = rr.hit_points(np.asarray(moved, np.float32), intr_of(cam), depth)
    q = gm.QueryPoints(np.where(valid[:, None], pts, np.float32(0)), gradient=True)
    used = valid & ((q["found"] & 2) != 0)
    assert got[29] == valid.sum() and got[28] == used.sum() and 0.5 * valid.sum() < used.sum() < valid.sum() < W * H
    g = q["gradient"].astype(np.float64)
    for axis, t in enumerate((0, 6, 11)):
        want = ar.pairwise(np.where(used, g[:, axis] * g[:, axis], 0.0))
        assert bits(got[t]) == bits(want), (axis, got[t], want)


def test_host_and_device_forms_are_equal_and_only_read_the_map():
    import torch
    gm, _, scene, pose = built("corner-8")
    cam = tgr.camera()
    depth = frame(scene, pose, nan_fraction=0.02)
    moved = ar.start_pose(pose, ar.CORNER_STARTS[1])
    before = gm.fields()
    counters = gm.counters()
    host = gm.AlignTerms(depth, moved, cam, max_residual=0.1)
    assert np.array_equal(bits(host), bits(gm.AlignTerms(depth, moved, cam, max_residual=0.1)))  # two calls
    dev = torch.device("cuda:0")
    d_depth = torch.from_numpy(depth).to(dev)
    out = torch.full((32,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert gm.AlignTerms(d_depth, moved, cam, max_residual=0.1, out=out) is out  # device frame, device terms
    gm.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(host))
    assert np.array_equal(bits(gm.AlignTerms(d_depth, moved, cam, max_residual=0.1)), bits(host))  # device frame, host terms
    out.fill_(7.0)
    torch.cuda.synchronize()
    gm.AlignTerms(depth, moved, cam, max_residual=0.1, out=out)  # host frame, device terms
    gm.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(host))
    run = gm.AlignDepth(d_depth, moved, cam, max_iterations=3, max_residual=0.1)
    again = gm.AlignDepth(depth, moved, cam, max_iterations=3, max_residual=0.1)
    for key in ("pose", "xi_last", "terms_first", "terms_last"):
        assert np.array_equal(bits(run[key]), bits(again[key])), key
    assert np.array_equal(bits(run["terms_first"]), bits(host)) and run["iterations"] == 3
    assert gm.counters() == counters
    compare_fields(before, gm.fields(), gm.V, False)


# ---- the loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner-16", "corner-8"])
def test_one_iteration(name):
    """AlignDepth(max_iterations=1): terms_first is AlignTerms, xi_last is align_solve(terms_first, damping) bit for bit, and the pose
    is ar.apply's within 1e-12 (the two differ only in libm's last ulp of sin and cos)"""
    from cvids_amd import capi, chisel
    gm, index, scene, pose = built(name)
    depth, cam = frame(scene, pose), tgr.camera()
    for offset in ar.CORNER_STARTS:
        start = ar.start_pose(pose, offset)
        for damping in (0.0, 1e-3):
            run = gm.AlignDepth(depth, start, cam, max_iterations=1, damping=damping)
            assert run["status"] == capi.ALIGN_ITERATION_LIMIT and run["iterations"] == 1
            T = gm.AlignTerms(depth, start, cam)
            assert np.array_equal(bits(run["terms_first"]), bits(T)) and np.array_equal(bits(run["terms_last"]), bits(T))
            xi = chisel.align_solve(T, damping)
            assert np.array_equal(bits(run["xi_last"]), bits(xi))
            assert np.array_equal(bits(xi), bits(ar.solve(T, damping)))
            want = ar.apply(xi, np.asarray(start, np.float32).astype(np.float64))
            assert np.abs(run["pose"] - want).max() <= 1e-12, np.abs(run["pose"] - want).max()


@pytest.mark.parametrize("name", ["corner-16", "corner-8"])
def test_the_loop_converges(name):
    """the corner cases of tests/test_align_restated.py under the same conditions: 10 iterations, damping 1e-3, max_residual 0 and
    0.1, three starts; errors at most halved, at least 0.75 of the valid pixels used in the first iteration"""
    from cvids_amd import capi
    gm, _, scene, pose = built(name)
    depth, cam = frame(scene, pose), tgr.camera()
    for offset in ar.CORNER_STARTS:
        start = ar.start_pose(pose, offset)
        for max_residual in (0.0, 0.1):
            run = gm.AlignDepth(depth, start, cam, max_iterations=10, max_residual=max_residual, damping=1e-3)
            assert run["status"] in (capi.ALIGN_ITERATION_LIMIT, capi.ALIGN_CONVERGED)
            assert run["iterations"] == 10 or run["status"] == capi.ALIGN_CONVERGED
            ar.check_corner_run([np.asarray(start, np.float32), run["pose"]], run["terms_first"], pose, "%s start %s max_residual %g" % (name, offset, max_residual))


# ---- outcomes and errors ---------------------------------------------------------------------------------------------------------
def test_outcomes():
    from cvids_amd import capi
    from cvids_amd import chisel as ch
    gm, _, scene, pose = built("corner-8")
    depth, cam = frame(scene, pose), tgr.camera()
    guess = ar.start_pose(pose, ar.CORNER_STARTS[0])
    guess_f = np.asarray(guess, np.float32).astype(np.float64)
    fresh = ch.Chisel((16, 16, 16), 0.02, False, max_chunks=1024)
    run = fresh.AlignDepth(depth, guess, cam)
    assert run["status"] == capi.ALIGN_TOO_FEW_PIXELS and run["iterations"] == 0 and not run["xi_last"].any()
    assert np.array_equal(run["pose"], guess_f)  # an empty map: the pose is the guess
    assert run["terms_first"][28] == 0 and run["terms_first"][29] > 0
    run = gm.AlignDepth(np.full((H, W), np.nan, np.float32), guess, cam)
    assert run["status"] == capi.ALIGN_TOO_FEW_PIXELS and np.array_equal(run["pose"], guess_f) and run["terms_first"][29] == 0
    run = gm.AlignDepth(depth, guess, cam, min_pixels=W * H + 1)
    assert run["status"] == capi.ALIGN_TOO_FEW_PIXELS and np.array_equal(run["pose"], guess_f) and run["terms_first"][28] > 0
    # a plane: with damping 0 the equations are singular up to rounding; whatever the outcome, it is an outcome
    N, res, trunc, n_frames, view = ar.WALL_MAP
    wall = tgr.gpu_map("wall", N, res, trunc, n_frames)
    true_pose = synth.trajectory_pose(view)
    run = wall.AlignDepth(frame("wall", true_pose), ar.start_pose(true_pose, ar.WALL_START), cam, damping=0.0)
    assert run["status"] in (capi.ALIGN_CONVERGED, capi.ALIGN_ITERATION_LIMIT, capi.ALIGN_DEGENERATE)
    print("wall, damping 0: status %s after %d updates" % (capi.ALIGN_STATUS[run["status"]], run["iterations"]))
    # ... and with the absolute damping the wall behaves as the CPU test says
    start = ar.start_pose(true_pose, ar.WALL_START)
    run = wall.AlignDepth(frame("wall", true_pose), start, cam, damping=1e-3)
    t0, _ = ar.pose_errors(start, true_pose)
    t1, r1 = ar.pose_errors(run["pose"], true_pose)
    assert abs(run["pose"][2, 3] - float(true_pose[2, 3])) < 1e-3 and r1 < 0.05 and t1 <= t0


def test_errors_in_their_order():
    from cvids_amd import capi
    from cvids_amd import chisel as ch
    L = capi.load_library()
    gm, _, scene, pose = built("corner-8")
    depth, cam = frame(scene, pose), tgr.camera()
    terms = np.zeros(32, np.float64)
    params = capi.AlignParams(10, 100, 0.0, 0.0, 1e-3, 1e-5, 1e-5)
    result = capi.AlignResult()

    def code(rc, want, word=None):
        assert rc == want, (rc, L.chisel_hip_last_error().decode())
        if word:
            assert word in L.chisel_hip_last_error().decode(), L.chisel_hip_last_error().decode()

    def both(h, f, want, word=None, params=params):
        fp = C.byref(f) if f is not None else None
        code(L.chisel_hip_align_terms(h, fp, 0.0, terms.ctypes.data, 0), want, word)
        code(L.chisel_hip_align_depth(h, fp, C.byref(params), C.byref(result)), want, word)

    good, keep = ch.depth_frame(depth, pose, cam)
    group = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, devices=[0, 0])
    shard = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, n_shards=2, shard_rank=0)
    both(group.h, None, 5, "group")   # UNSUPPORTED comes before the look at the other arguments
    both(shard.h, None, 5, "shard")
    both(group.h, good, 5, "group")
    both(shard.h, good, 5, "shard")
    both(None, good, 1, "null map")
    both(gm.h, None, 1, "null frame")
    no_image, _ = ch.depth_frame(depth, pose, cam)
    no_image.depth = None
    both(gm.h, no_image, 1, "null frame")
    for w, h in ((0, H), (W, 0), (-1, H)):
        bad, _ = ch.depth_frame(depth, pose, cam)
        bad.width, bad.height = w, h
        both(gm.h, bad, 1, "size")
    code(L.chisel_hip_align_terms(gm.h, C.byref(good), 0.0, None, 0), 1, "null terms")
    code(L.chisel_hip_align_terms(gm.h, C.byref(good), 0.0, None, 1), 1, "null terms")
    code(L.chisel_hip_align_depth(gm.h, C.byref(good), None, C.byref(result)), 1, "null params")
    code(L.chisel_hip_align_depth(gm.h, C.byref(good), C.byref(params), None), 1, "null params")
    for n in (0, -3):
        code(L.chisel_hip_align_depth(gm.h, C.byref(good), C.byref(capi.AlignParams(n, 100, 0.0, 0.0, 1e-3, 1e-5, 1e-5)), C.byref(result)), 1, "max_iterations")
    with pytest.raises(capi.ChiselHipError) as e:
        group.AlignTerms(depth, pose, cam)
    assert e.value.code == 5
    with pytest.raises(capi.ChiselHipError) as e:
        shard.AlignDepth(depth, pose, cam)
    assert e.value.code == 5
    # ... and the map still answers
    assert gm.AlignTerms(depth, pose, cam)[28] > 0 and gm.AlignDepth(depth, pose, cam, max_iterations=1)["iterations"] == 1
