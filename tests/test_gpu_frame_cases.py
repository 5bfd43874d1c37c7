"""GPU parity of the depth-frame path on the frames of tests/frame_cases.py: general poses, cameras with fx != fy and an off-centre or
outside principal point, depth images with steps inside every pyramid texel, isolated valid pixels, valid pixels on the border only, and a
surface a few voxels from the camera.  What is under test is the front half of a launch set (kernels_cull.h: depth_pyramid_kernel,
cull_kernel, brick_kernel) -- every bound there is conservative with a hand-chosen margin, and one that is too tight fails silently -- and
the fast paths of the integration kernel it selects.  Everything is bit-exact against the oracle, as in test_gpu_parity.py;
tests/test_frame_cases.py shows on the oracle alone that the frames reach the edges they are meant to."""
import numpy as np
import pytest

from cvids_amd import synth
from tests import frame_cases as fc
from tests.common import compare_fields
from tests.test_gpu_parity import _mk, _run, _run_batched

pytestmark = pytest.mark.gpu
COUNTERS = ("sdf", "col", "col_sat", "probe", "carved", "updated_chunks")


def _run_in_sixes(om, gm, integ, frames, cam, color_img=None):
    """the counters after every frame, the fields and meshes_to_update after every sixth and at the end"""
    for lo in range(0, len(frames), 6):
        _run(om, gm, integ, frames[lo:lo + 6], cam, color_img=color_img, check_each=False)


# ---- a. every pose x every image, frame by frame -------------------------------------------------------------------------------------------
def _pose_cases():
    """(camera, N, res, poses): every camera at 8^3 / 5 cm and 16^3 / 4 cm, `centred` and `aniso` also at 32^3 / 2 cm; all six poses with all six
    images each.  Where the oracle needs more than a few seconds for the 36 frames (the wide camera, 32^3 voxels) the poses are split over
    several tests, each on a map of its own."""
    out = []
    for camera in fc.CAMERA_NAMES:
        for N, res in ((8, 0.05), (16, 0.04), (32, 0.02)):
            if N == 32 and camera not in ("centred", "aniso"):
                continue
            per = 2 if N == 32 else 3 if camera == "wide" else 6
            for lo in range(0, 6, per):
                out.append(pytest.param(camera, N, res, fc.POSE_NAMES[lo:lo + per], id="%s-%d-%s" % (camera, N, "+".join(fc.POSE_NAMES[lo:lo + per]))))
    return out


@pytest.mark.parametrize("camera,N,res,poses", _pose_cases())
def test_poses_and_images(oracle_mod, camera, N, res, poses):
    om, gm, integ = _mk(oracle_mod, N, res, False, max_chunks=16384 if N == 8 else 8192 if N == 16 else 2048)
    cam = fc.pinhole(camera, 64, 48)
    frames = [(d, p) for _, d, p in fc.all_frames(64, 48, poses=poses)]
    _run_in_sixes(om, gm, integ, frames, cam)
    assert gm.NumChunks() > 10


# ---- b. image sizes ----------------------------------------------------------------------------------------------------------------------
# (3 x 67 with fy = 700 * 3 / 640 = 3.3 is a fisheye of 170 degrees: out to 3 m the reference enumerates 68 000 chunks of 16^3 voxels per frame,
# 37 s of oracle for the twelve frames.  Its far plane is 1 m: 2 600 chunks per frame.)
@pytest.mark.parametrize("W,H,N,res,far", [(w, h, 16, 0.04, 1.0 if (w, h) == (3, 67) else None) for w, h in fc.SIZES] + [(200, 136, 32, 0.02, 1.5)])
def test_sizes(oracle_mod, W, H, N, res, far):
    """narrower than one 4-pixel block, one pixel, taller than a tile, 5 x 4 ragged tiles with an odd width (the scalar pyramid path, no
    WI_TILE, the whole-image fallback) and the same with the vector path"""
    om, gm, integ = _mk(oracle_mod, N, res, False, max_chunks=8192 if N == 16 else 2048)
    cam = fc.pinhole("aniso", W, H, far=far)
    frames = [(d, p) for _, d, p in fc.all_frames(W, H, poses=("tilt", "far30"))]
    _run_in_sixes(om, gm, integ, frames, cam)
    assert gm.NumChunks() > 10


# ---- c. truncators, weights, colour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [2.0, 1.0])
@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("trunc", [("constant", 0.12), ("quadratic", 1.5), ("inverse", 0.7)])
def test_truncators_colour(oracle_mod, trunc, color, weight):
    """(the short weight reciprocal, WI_FASTWU, needs colour and weight 1)"""
    om, gm, integ = _mk(oracle_mod, 8, 0.05, color, trunc=trunc, weight=weight, max_chunks=8192)
    cam = fc.pinhole("aniso", 64, 48)
    frames = [(d, p) for _, d, p in fc.all_frames(64, 48, poses=("tilt", "neg"), images=("steps", "close", "sparse"))]
    _run(om, gm, integ, frames, cam, color_img=synth.render_color(64, 48, 3) if color else None, check_each=False)
    assert gm.NumChunks() > 50


# ---- d. a chunk created by one frame of a launch set and only carved by the next ------------------------------------------------------------------
@pytest.mark.parametrize("batch", [11, 4, 2, 1])
@pytest.mark.parametrize("color", [False, True])
def test_carving_inside_one_launch_set(oracle_mod, batch, color):
    """near wall x 3, far wall x 2, then near / far alternating, carving distance 0, from a tilted pose: inside a launch set frame k creates
    chunks that frame k + 1 can only carve (brick_kernel's `resident` from the earlier frames' in-band masks; the cull kernel's drop of
    frames that could only carve a chunk that is not resident)"""
    om, gm, integ = _mk(oracle_mod, 8, 0.05, color, carving=True, carving_dist=0.0, max_chunks=8192)
    cam = fc.pinhole("centred", 64, 48)
    frames = fc.carve_frames(64, 48)
    color_img = synth.render_color(64, 48, 3) if color else None
    if batch == 1:
        _run(om, gm, integ, frames, cam, color_img=color_img)
    else:
        _run_batched(om, gm, integ, frames, cam, color_img, batch)


@pytest.mark.parametrize("batch", [4, 2, 1])
def test_carving_distance_beyond_the_band(oracle_mod, batch):
    """carving distance 1 m, more than the band's half width: a chunk in front of both surfaces of `steps` is carved by its far pixels only --
    the carve tests of cull_post and brick_kernel must take the largest depth under the box (with the usual few centimetres every chunk that
    the far pixels can carve the near ones can carve too, or lies in the band of one of them)"""
    om, gm, integ = _mk(oracle_mod, 8, 0.05, False, carving=True, carving_dist=fc.DEEP_CARVING_DIST, max_chunks=8192)
    cam = fc.pinhole("centred", 64, 48)
    frames = fc.deep_carve_frames(64, 48)
    if batch == 1:
        _run(om, gm, integ, frames, cam)
    else:
        _run_batched(om, gm, integ, frames, cam, None, batch)


# ---- a chunk that straddles the camera plane, valid depth at the far side of the image only ------------------------------------------------------
@pytest.mark.parametrize("W,H", [(64, 48), (200, 136)])
@pytest.mark.parametrize("camera", ["wide", "cx_out"])
def test_close_surface_at_the_image_edge(oracle_mod, camera, W, H):
    """the voxels of such a chunk that lie nearest to the camera plane project beyond the box of its corners in front (and the corners behind
    project mirrored): cull_post must give it the whole image (`any_behind`)"""
    om, gm, integ = _mk(oracle_mod, 8, 0.05, False, max_chunks=8192)
    cam = fc.pinhole(camera, W, H)
    frames = [(d, p) for _, d, p in fc.all_frames(W, H, images=fc.EDGE_IMAGE_NAMES)]
    _run_in_sixes(om, gm, integ, frames, cam)
    assert gm.NumChunks() > 10


# ---- e / f. launch sets of unrelated views ----------------------------------------------------------------------------------------------------------
_reference = {}


def _unrelated(oracle_mod, N, res):
    """the 17 unrelated views through the oracle, once per chunk size: (frames, camera, final fields, counter totals, meshes_to_update)"""
    if N not in _reference:
        om = oracle_mod.OracleMap(N, res, False)
        om.set_integrator(oracle_mod.TRUNC_INVERSE, 2.0, 1.0, True, 0.05)
        cam = fc.pinhole("aniso", 64, 48)
        frames = [(d, p) for _, d, p in fc.unrelated_views(64, 48)]
        tot = dict.fromkeys(COUNTERS, 0)
        for d, p in frames:
            om.integrate_depth(d, p, (cam.fx, cam.fy, cam.cx, cam.cy), cam.near_plane, cam.far_plane)
            oc = om.counters()
            for k in tot:
                tot[k] += oc[k]
        _reference[N] = (frames, cam, om.fields(), tot, sorted(map(tuple, om.meshes_to_update().tolist())), om.V)
    return _reference[N]


def _against_reference(gm, ref):
    _, _, fields, tot, dirty, V = ref
    gc = gm.counters(reset=True)
    for k in tot:
        assert tot[k] == gc[k], "counter %s: oracle %d gpu %d" % (k, tot[k], gc[k])
    assert len(fields) == gm.NumChunks()
    compare_fields(fields, gm.fields(), V, False)
    assert dirty == sorted(map(tuple, gm.GetMeshesToUpdate().tolist()))


@pytest.mark.parametrize("force", [None, "CHISEL_HIP_FORCE_PIPELINE", "CHISEL_HIP_FORCE_UNCERTAIN"])
@pytest.mark.parametrize("batches", [(16, 1), (8, 9), (5, 5, 5, 2)])
def test_batch_of_unrelated_views(oracle_mod, batches, force, monkeypatch):
    """launch sets whose frames look from unrelated poses (the id range of a set is many times any frame's own, most (chunk, frame) pairs die
    in the range test, the frames of one brick mask have nothing in common), queued without a wait in between"""
    if force:
        monkeypatch.setenv(force, "1")
    _, gm, integ = _mk(oracle_mod, 8, 0.05, False, max_chunks=16384)
    if force:
        monkeypatch.delenv(force, raising=False)
    ref = _unrelated(oracle_mod, 8, 0.05)
    frames, cam = ref[0], ref[1]
    lo = 0
    for n in batches:
        gm.IntegrateBatch(integ, [(d, p, cam) for d, p in frames[lo:lo + n]])
        lo += n
    assert lo == len(frames)
    _against_reference(gm, ref)


@pytest.mark.parametrize("mode", ["vpl2", "vpl4", "persistent", "cull1", "cull4", "cull16"])
def test_schedules_on_hostile_frames(oracle_mod, mode, monkeypatch):
    """the forced granularities and workgroup shapes of test_gpu_parity.py::test_integration_schedules on the unrelated views, 16^3 voxels"""
    if mode in ("cull1", "cull4", "cull16"):
        monkeypatch.setenv("CHISEL_HIP_CULL_WAVES", mode[4:])
    elif mode in ("vpl2", "vpl4"):
        monkeypatch.setenv("CHISEL_HIP_VPL", mode[3:])
    else:
        monkeypatch.setenv("CHISEL_HIP_PERSISTENT", "1")
    _, gm, integ = _mk(oracle_mod, 16, 0.04, False, max_chunks=8192)
    ref = _unrelated(oracle_mod, 16, 0.04)
    frames, cam = ref[0], ref[1]
    lo = 0
    for n in (1, 4, 8, 2, 2):
        gm.IntegrateBatch(integ, [(d, p, cam) for d, p in frames[lo:lo + n]])
        lo += n
    assert lo == len(frames)
    _against_reference(gm, ref)


# ---- g. shards at chunk ids near (2500, -5000, 1250) and below zero ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards", [2, 3, 8])
def test_shards_far_from_the_origin(oracle_mod, n_shards):
    """floor_div and the residue classes of CullSpace at large and at negative ids: the union of the ranks' chunks is the oracle's map.  (The
    frames of one pose make one launch set: a set spanning both poses would have to judge 1.6e10 chunk ids and is refused.)"""
    from cvids_amd import chisel as ch
    om = oracle_mod.OracleMap(8, 0.05, False)
    om.set_integrator(oracle_mod.TRUNC_INVERSE, 2.0, 1.0, True, 0.05)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    shards = [ch.Chisel((8, 8, 8), 0.05, False, max_chunks=8192, n_shards=n_shards, shard_rank=r) for r in range(n_shards)]
    cam = fc.pinhole("aniso", 64, 48)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    tot = dict(sdf=0, probe=0, carved=0)
    for pose in ("far1k", "neg"):
        frames = [(d, p) for _, d, p in fc.all_frames(64, 48, poses=(pose,))]
        for lo in (0, 4):
            part = frames[lo:lo + 4]
            for d, p in part:
                om.integrate_depth(d, p, intr, cam.near_plane, cam.far_plane)
                oc = om.counters()
                for k in tot:
                    tot[k] += oc[k]
            for s_ in shards:
                s_.IntegrateBatch(integ, [(d, p, cam) for d, p in part])
    union = {}
    got = dict.fromkeys(tot, 0)
    for r, s_ in enumerate(shards):
        f = s_.fields()
        assert not (set(f) & set(union)), "shards overlap"
        for cid in f:
            assert ch.chunk_owner(cid, n_shards, 2) == r
        union.update(f)
        c = s_.counters()
        for k in got:
            got[k] += c[k]
    compare_fields(om.fields(), union, om.V, False, what="%d shards" % n_shards)
    assert len(union) == om.num_chunks() and got == tot
    ids = np.array(sorted(union))
    assert ids[:, 0].max() > 2400 and ids[:, 1].min() < -4900 and (ids < 0).all(1).any()
    assert min(len(s_.fields()) for s_ in shards) > 0
