"""chisel_hip_query_points and chisel_hip_cast_rays on the GPU against their definition (DESIGN.md "Querying points and rays").

Every comparison is BIT FOR BIT over every element with equal NaN masks (same_bits of tests/common.py; integer outputs with
array_equal): against the numpy restatement (tests/query_restated.py) run over the map as GetChunkIDs / GetChunk read it back,
against the single-point entries, chisel_hip_shade_vertices and chisel_hip_render_view.  A stated share only keeps a comparison from
passing on an empty case.  The maps are built once and only read, but where a test changes them."""
import functools

import numpy as np
import pytest

from cvids_amd import synth
from tests import query_restated as qr
from tests import render_restated as rr
from tests import test_gpu_render as tgr
from tests.common import compare_fields, same_bits

pytestmark = pytest.mark.gpu
W, H = tgr.W, tgr.H
NEAR, FAR = tgr.NEAR, tgr.FAR

# scene, chunk edge, resolution, truncator, frames, carving, colour voxels, pose of "the map's own view"
MAPS = [tgr.MAPS[0], tgr.MAPS[2], tgr.MAPS[3], tgr.MAPS[1]]
IDS = ["%s-%d" % (m[0], m[1]) + ("-colour" if m[6] else "") for m in MAPS]


def intr_of(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


@functools.lru_cache(maxsize=None)
def built(case):
    """the map of MAPS[case] (only ever read), its VoxelIndex, and the point sets: name -> (n, 3) float32 with the 64 hand-placed
    positions at the end"""
    scene, N, res, trunc, n_frames, carving, color, pose_k = MAPS[case]
    gm = tgr.gpu_map(scene, N, res, trunc, n_frames, carving, color)
    index = tgr.index_of(gm)
    cam, pose = tgr.camera(), synth.trajectory_pose(pose_k)
    depth = gm.RenderView(pose, cam)["depth"]
    hits = rr.hit_points(pose, intr_of(cam), depth)
    rng = np.random.default_rng(synth.SEED)
    anchor = hits[(H // 2) * W + W // 2]
    assert np.isfinite(anchor).all()
    hand = qr.hand_points(anchor, N, res)
    sets = {"jitter": np.concatenate([qr.jitter_points(hits, res, rng), hand]),
            "box": np.concatenate([qr.box_points(gm.GetChunkIDs(), N, res, rng), hand])}
    return gm, index, sets


@functools.lru_cache(maxsize=None)
def answers(case, name):
    """QueryPoints with every output the map has, once per (map, set)"""
    gm, _, sets = built(case)
    return gm.QueryPoints(sets[name], sdf=True, weight=True, gradient=True, colors=gm.use_color)


def equal_outputs(got, want, what, keys=None):
    for key in keys or want:
        if want[key] is None:
            assert got[key] is None, key
        elif want[key].dtype == np.uint8:
            assert np.array_equal(got[key], want[key]), "%s: %s differs at %d places" % (what, key, int((got[key] != want[key]).sum()))
        else:
            same_bits(got[key], want[key], "%s: %s" % (what, key))


# ---- points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(MAPS)), ids=IDS)
def test_points_against_the_restatement(case):
    """found bit 0, sdf and weight of 20 064 positions of each kind against VoxelIndex.sample over gm.fields(); then n = 1, 63, 65 and
    257 (the tails of a wave and of a block) against the same answers"""
    gm, index, sets = built(case)
    for name, pts in sets.items():
        assert len(pts) == 20064
        got = answers(case, name)
        found, sdf, weight = qr.query_points(index, pts)
        assert np.array_equal((got["found"] & 1).astype(bool), found), "%s: found differs at %d places" % (name, int(((got["found"] & 1) != found).sum()))
        same_bits(got["sdf"], sdf, name + ": sdf")
        same_bits(got["weight"], weight, name + ": weight")
        share = float(found[:qr.N_POINTS].mean())
        print("%s %s: found %.4f, voxel exists %.4f, gradient found %.4f" % (IDS[case], name, share, float(np.isfinite(weight).mean()),
                                                                              float((got["found"][:qr.N_POINTS] >> 1).mean())))
        if name == "jitter":
            assert 0.9 < share < 1
        else:
            assert 0.05 < share < 0.5
        assert np.isfinite(weight).sum() > found.sum() or name == "jitter"  # (box: voxels that exist and are unobserved)
        order = np.random.default_rng(synth.SEED + 1).permutation(len(pts))
        for n in (1, 63, 65, 257):
            pick = order[:n]
            part = gm.QueryPoints(pts[pick], sdf=True, weight=True, gradient=True, colors=gm.use_color)
            equal_outputs(part, {k: (v[pick] if v is not None else None) for k, v in got.items()}, "%s n = %d" % (name, n))


@pytest.mark.parametrize("case", range(len(MAPS)), ids=IDS)
def test_points_against_the_single_point_entries(case):
    """gradient and bit 1 against chisel_hip_get_sdf_and_gradient, sdf and bit 0 against chisel_hip_get_sdf, point by point at the 64
    hand-placed positions and 300 of each set.  The three positions with a non-finite component are held to the definition instead
    (found 0, NaN everywhere: the batched kernel does not look at the map for them, whatever the single-point kernel makes of a NaN).
    The distance GetSDFAndGradient returns beside the gradient is not compared with `sdf`: it is read at the centre
    floorf(p / res) * res + res / 2, which at a voxel's face can lie in the neighbour of the voxel GetSDF(p) reads."""
    gm, _, sets = built(case)
    seen = set()
    for name, pts in sets.items():
        got = answers(case, name)
        rows = list(range(300)) + (list(range(qr.N_POINTS, qr.N_POINTS + 64)) if name == "jitter" else [])
        for i in rows:
            p = pts[i]
            f, s, g = int(got["found"][i]), got["sdf"][i], got["gradient"][i]
            if not np.isfinite(p).all():
                assert f == 0 and np.isnan(s) and np.isnan(g).all() and np.isnan(got["weight"][i]), (i, p)
                seen.add("non-finite")
                continue
            found, dist = gm.GetSDF(p)
            assert found == bool(f & 1), (i, p)
            if found:
                assert np.float64(s).tobytes() == np.float64(dist).tobytes(), (i, p, s, dist)
            else:
                assert np.isnan(s), (i, p)
            found_g, dist_g, grad = gm.GetSDFAndGradient(p)
            assert found_g == bool(f & 2), (i, p)
            seen.add("gradient found" if found_g else "gradient not found")
            if found_g:
                assert g.tobytes() == grad.tobytes(), (i, p, g, grad)
            else:
                assert np.isnan(g).all(), (i, p)
    assert seen == {"non-finite", "gradient found", "gradient not found"}


@pytest.mark.parametrize("case", [i for i, m in enumerate(MAPS) if m[6]], ids=[IDS[i] for i, m in enumerate(MAPS) if m[6]])
def test_colours_equal_shade_vertices(case):
    """all 2 x 20 064 positions against chisel_hip_shade_vertices (stage 2), its (0, 0, 0) answers included; NaN for the non-finite ones"""
    gm, _, sets = built(case)
    for name, pts in sets.items():
        got = answers(case, name)["colors"]
        fin = np.isfinite(pts).all(1)
        assert (~fin).sum() == 3 and np.isnan(got[~fin]).all()
        _, want = tgr.shade(gm, pts[fin], np.zeros((int(fin.sum()), 3), np.float32))
        same_bits(got[fin], want, name + ": colours")
        zero = (want == 0).all(1)
        assert np.isfinite(got[fin]).all() and 0 < zero.sum() and (~zero).sum() > 100, (name, int(zero.sum()))


def test_output_subsets_and_refusals():
    from cvids_amd import capi
    from cvids_amd import chisel as ch
    L = capi.load_library()
    case = [i for i, m in enumerate(MAPS) if m[6]][0]
    gm, _, sets = built(case)
    pts = sets["jitter"][-2000:]
    full = gm.QueryPoints(pts, sdf=True, weight=True, gradient=True, colors=True)
    ptr = lambda a: a.ctypes.data if a is not None else None
    fields = [("found", np.uint8, ()), ("sdf", np.float32, ()), ("weight", np.float32, ()), ("gradient", np.float32, (3,)), ("colors", np.float32, (3,))]
    for alone, dtype, tail in fields:  # every output alone
        a = np.zeros((len(pts),) + tail, dtype)
        args = [ptr(a) if name == alone else None for name, _, _ in fields]
        assert L.chisel_hip_query_points(gm.h, ptr(pts), len(pts), *args, 0) == 0, alone
        if alone == "found":  # bit 1 is evaluated only with the gradient
            assert np.array_equal(a, full["found"] & 1)
        else:
            equal_outputs({alone: a}, full, "alone", [alone])
    f = np.zeros(len(pts), np.uint8)
    g = np.zeros((len(pts), 3), np.float32)
    assert L.chisel_hip_query_points(gm.h, ptr(pts), len(pts), ptr(f), None, None, ptr(g), None, 0) == 0
    assert np.array_equal(f, full["found"]) and (f & 2).any() and not (f & 2).all()
    equal_outputs(gm.QueryPoints(pts), {"found": full["found"] & 1, "sdf": full["sdf"], "weight": None, "gradient": None, "colors": None}, "defaults")

    def refused(code, fn, *args, **kw):
        with pytest.raises(capi.ChiselHipError) as e:
            fn(*args, **kw)
        assert e.value.code == code, e.value
        msg = L.chisel_hip_last_error().decode()
        assert msg and msg in str(e.value)
        return msg

    def raw(fn, *args):
        capi.check(fn(*args))

    one = np.zeros((1, 3), np.float32)
    out1 = np.zeros(1, np.float32)
    ray = qr.pack([0, 0, 0], [[0, 0, 1]], 0.0, 1.0)
    plain, _, _ = built(0)
    qp, cr = L.chisel_hip_query_points, L.chisel_hip_cast_rays
    assert "output" in refused(1, raw, qp, gm.h, ptr(one), 1, None, None, None, None, None, 0)            # all five NULL
    assert "negative" in refused(1, raw, qp, gm.h, ptr(one), -1, None, ptr(out1), None, None, None, 0)   # n < 0
    assert "positions" in refused(1, raw, qp, gm.h, None, 1, None, ptr(out1), None, None, None, 0)       # null positions
    assert "colour" in refused(1, plain.QueryPoints, one, colors=True)                                   # no colour voxels
    assert qp(gm.h, None, 0, None, ptr(out1), None, None, None, 0) == 0                                  # n == 0: OK, nothing launched
    assert qp(gm.h, None, 0, None, ptr(out1), None, None, None, 1) == 0
    assert qp(gm.h, None, 0, None, None, None, None, None, 0) == 0                                       # ... whatever else is passed
    assert "negative" in refused(1, raw, cr, gm.h, ptr(ray), -1, 0.0, ptr(out1), None, None, None, 0)
    assert "rays" in refused(1, raw, cr, gm.h, None, 1, 0.0, ptr(out1), None, None, None, 0)
    assert "t_hit" in refused(1, raw, cr, gm.h, ptr(ray), 1, 0.0, None, None, None, None, 0)
    assert "NaN" in refused(1, raw, cr, gm.h, ptr(ray), 1, float("nan"), ptr(out1), None, None, None, 0)
    assert "colour" in refused(1, plain.CastRays, ray[:, 0:3], ray[:, 3:6], 0.0, 1.0, colors=True)
    assert cr(gm.h, None, 0, 0.0, ptr(out1), None, None, None, 0) == 0
    assert plain.QueryPoints(one)["found"].shape == (1,) and plain.CastRays(ray[:, 0:3], ray[:, 3:6], 0.0, 1.0)["t_hit"].shape == (1,)  # ... and still answers
    group = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, devices=[0, 0])
    assert "group" in refused(5, group.QueryPoints, one)
    assert "group" in refused(5, group.CastRays, ray[:, 0:3], ray[:, 3:6], 0.0, 1.0)
    shard = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, n_shards=2, shard_rank=0)
    assert "shard" in refused(5, shard.QueryPoints, one)
    assert "shard" in refused(5, shard.CastRays, ray[:, 0:3], ray[:, 3:6], 0.0, 1.0)


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def cast(gm, rays, step=0.0, **kw):
    return gm.CastRays(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7], step=step, **kw)


def check_rays(gm, index, rays, step, what):
    got = cast(gm, rays, step)
    t_hit, status = qr.cast_rays(index, rays, step)
    same_bits(got["t_hit"], t_hit, what + ": t_hit")
    assert np.array_equal(got["status"], status), "%s: status differs at %d places" % (what, int((got["status"] != status).sum()))
    return got


@pytest.mark.parametrize("case", range(len(MAPS)), ids=IDS)
def test_rays_against_render_view(case):
    """CastRays on a view's rays is RenderView's depth, normals and colours: the map's own pose and pose 20, steps of one voxel and of
    half a voxel, 160 x 120 and 77 x 53.  The same rays with unit directions, t from 0 to 6, against the restatement, in every one of
    these cases."""
    gm, index, _ = built(case)
    res, color, pose_k = MAPS[case][2], MAPS[case][6], MAPS[case][7]
    for k in (pose_k, 20):
        pose = synth.trajectory_pose(k)
        for step in (0.0, res / 2):
            for w, h in ((W, H), (77, 53)):
                cam = tgr.camera(w, h)
                what = "pose %d step %g %d x %d" % (k, step, w, h)
                view = gm.RenderView(pose, cam, step=step, normals=True, colors=color)
                got = cast(gm, qr.view_rays(pose, intr_of(cam), w, h, NEAR, FAR), step, normals=True, colors=color)
                same_bits(got["t_hit"].reshape(h, w), view["depth"], what + ": depth")
                same_bits(got["normals"].reshape(h, w, 3), view["normals"], what + ": normals")
                if color:
                    same_bits(got["colors"].reshape(h, w, 3), view["colors"], what + ": colours")
                assert np.array_equal(got["status"] == 1, np.isfinite(got["t_hit"]))
                hit = float((got["status"] == 1).mean())
                assert (hit > 0.9) if k == pose_k else (0.3 < hit < 1.0), (what, hit)
                unit = check_rays(gm, index, qr.unit_rays(pose, intr_of(cam), w, h), step, what + ", unit directions")
                assert (unit["status"] == 1).mean() > 0.3


def test_order_and_mix():
    """a random permutation of a view's rays, the same rays each given twice, and a set that interleaves lane by lane pose-4 rays,
    rays of the "outside" view and rays with t_far < t_near: exactly the permuted, duplicated, interleaved outputs of the separate
    calls; then the first n = 1, 63, 65 and 4099 rays of the mix.  Neither a chunk kept by a lane nor the order in which a wave
    takes its rays may show."""
    gm, _, _ = built(0)
    cam = tgr.camera()
    keys = ("t_hit", "status", "normals")
    a = qr.view_rays(synth.trajectory_pose(4), intr_of(cam), W, H, NEAR, FAR)
    b = qr.view_rays(rr.no_hit_views()["outside"][0], intr_of(cam), W, H, NEAR, 5.0)
    c = a.copy()
    c[:, 6], c[:, 7] = 2.0, 1.0
    ra, rb, rc = (cast(gm, r, normals=True) for r in (a, b, c))
    assert (ra["status"] == 1).mean() > 0.99 and (rb["status"] == 0).all() and (rc["status"] == 0).all()
    perm = np.random.default_rng(synth.SEED).permutation(len(a))
    equal_outputs(cast(gm, a[perm], normals=True), {k: ra[k][perm] for k in keys}, "permuted")
    twice = np.repeat(np.arange(len(a)), 2)
    equal_outputs(cast(gm, a[twice], normals=True), {k: ra[k][twice] for k in keys}, "each ray twice")
    mix = qr.interleave(a, b, c)
    want = {k: np.stack([ra[k], rb[k], rc[k]], axis=1).reshape((-1,) + ra[k].shape[1:]) for k in keys}
    equal_outputs(cast(gm, mix, normals=True), want, "interleaved")
    for n in (1, 63, 65, 4099):  # (the three kinds side by side in every wave, and the tails of a wave and of a block)
        equal_outputs(cast(gm, mix[:n], normals=True), {k: want[k][:n] for k in keys}, "n = %d" % n)
    assert (want["status"][:4099] == 1).sum() > 1000


def test_per_ray_bounds():
    """t_far drawn per ray between 0.2 and 6 m (unit directions, t_near = 0): t_hit and status against the restatement"""
    gm, index, _ = built(0)
    cam = tgr.camera(77, 53)
    rays = qr.unit_rays(synth.trajectory_pose(4), intr_of(cam), 77, 53)
    rays[:, 7] = np.random.default_rng(synth.SEED).uniform(0.2, 6.0, len(rays)).astype(np.float32)
    got = check_rays(gm, index, rays, 0.0, "per-ray t_far")
    share = [float((got["status"] == v).mean()) for v in range(3)]
    print("per-ray bounds: status 0 / 1 / 2 shares %.3f / %.3f / %.3f" % tuple(share))
    assert share[0] > 0.1 and share[1] > 0.1


def test_after_garbage_collect_and_reset():
    """every third chunk removed, then Reset, then three frames: points and rays against the restatement over the map as read back;
    an empty map answers found 0 and status 0 everywhere"""
    scene, N, res, trunc, n_frames = MAPS[0][:5]
    gm = tgr.gpu_map(scene, N, res, trunc, n_frames)
    _, _, sets = built(0)
    pts = sets["jitter"][-4064:]
    cam = tgr.camera(77, 53)
    rays = qr.unit_rays(synth.trajectory_pose(4), intr_of(cam), 77, 53)

    def check(what):
        index = tgr.index_of(gm)
        got = gm.QueryPoints(pts, sdf=True, weight=True)
        found, sdf, weight = qr.query_points(index, pts)
        assert np.array_equal(got["found"].astype(bool), found), what
        same_bits(got["sdf"], sdf, what + ": sdf")
        same_bits(got["weight"], weight, what + ": weight")
        return float(found.mean()), check_rays(gm, index, rays, 0.0, what)

    ids = gm.GetChunkIDs()
    ids = ids[np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0]))]
    gm.GarbageCollect(ids[::3])
    assert gm.NumChunks() == len(ids) - len(ids[::3])
    share, got = check("after GarbageCollect")
    assert 0.3 < share < 0.9 and 0.05 < (got["status"] == 1).mean() < 0.99
    gm.Reset()
    empty = gm.QueryPoints(pts, sdf=True, weight=True, gradient=True)
    assert not empty["found"].any() and all(np.isnan(empty[k]).all() for k in ("sdf", "weight", "gradient"))
    empty = cast(gm, rays, normals=True)
    assert not empty["status"].any() and np.isnan(empty["t_hit"]).all() and np.isnan(empty["normals"]).all()
    integ = tgr.integrator(trunc)
    for depth, p in synth.stream(scene, 3, W, H, start=2):
        gm.IntegrateDepthScan(integ, depth, p, tgr.camera())
    share, got = check("after Reset")
    assert share > 0.9 and (got["status"] == 1).mean() > 0.9


def device_outputs(n, color, dev):
    import torch
    pts = {"found": torch.zeros(n, dtype=torch.uint8, device=dev), "sdf": torch.zeros(n, dtype=torch.float32, device=dev),
           "weight": torch.zeros(n, dtype=torch.float32, device=dev), "gradient": torch.zeros((n, 3), dtype=torch.float32, device=dev)}
    if color:
        pts["colors"] = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    return pts


def ray_outputs(n, color, dev):
    import torch
    out = {"t_hit": torch.zeros(n, dtype=torch.float32, device=dev), "status": torch.zeros(n, dtype=torch.uint8, device=dev),
           "normals": torch.zeros((n, 3), dtype=torch.float32, device=dev)}
    if color:
        out["colors"] = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    return out


def test_queries_only_read_the_map():
    """two maps fed the same frames, one of them queried in between (points with all outputs, rays with shading, into device
    tensors): voxels, counters, meshesToUpdate and the meshes of a later UpdateMeshes are identical"""
    import torch
    args = ("sphere_room", 16, 0.03, ("inverse", 2.0), 6, True, True)
    a, b = tgr.gpu_map(*args), tgr.gpu_map(*args)
    dev = torch.device("cuda:0")
    cam = tgr.camera()
    rng = np.random.default_rng(synth.SEED)
    pts = torch.from_numpy(qr.box_points(a.GetChunkIDs(), 16, 0.03, rng, 5000)).to(dev)
    rays = torch.from_numpy(np.concatenate([qr.view_rays(synth.trajectory_pose(k), intr_of(cam), W, H, NEAR, FAR) for k in (4, 20)])).to(dev)
    p_out, r_out = device_outputs(len(pts), True, dev), ray_outputs(len(rays), True, dev)
    torch.cuda.synchronize()
    for step in (0.0, 0.01):
        a.QueryPoints(pts, out=p_out)
        a.CastRays(rays, None, None, None, step=step, out=r_out)
    a.synchronize()
    assert p_out["found"].any() and (r_out["status"] == 1).any()
    assert a.counters() == b.counters()
    assert sorted(map(tuple, a.GetMeshesToUpdate().tolist())) == sorted(map(tuple, b.GetMeshesToUpdate().tolist()))
    assert a.NumChunks() == b.NumChunks()
    compare_fields(b.fields(), a.fields(), a.V, True)
    a.UpdateMeshes()
    b.UpdateMeshes()
    a.QueryPoints(pts, out=p_out)
    ma, mb = tgr.mesh_state(a), tgr.mesh_state(b)
    assert set(ma) == set(mb) and len(ma) > 10
    for cid in ma:
        for key in ("vertices", "normals", "colors", "grids"):
            assert ma[cid][key].tobytes() == mb[cid][key].tobytes(), (cid, key)
    assert a.GetMeshesToUpdate().tolist() == b.GetMeshesToUpdate().tolist()


def test_queries_between_two_launch_sets_of_a_pipelined_stream():
    """device frames, nothing waited for: IntegrateBatch, QueryPoints and CastRays into device tensors, IntegrateBatch.  The answers
    are those of the map after the first batch, and the final map is the one of the same stream without the queries."""
    import torch
    from cvids_amd import chisel as ch
    N, res, trunc = 16, 0.03, ("inverse", 2.0)
    cam, integ = tgr.camera(), tgr.integrator(trunc)
    frames = list(synth.stream("sphere_room", 8, W, H))
    dev = torch.device("cuda:0")
    d_dev = [torch.from_numpy(d).to(dev) for d, _ in frames]
    rays_h = qr.view_rays(synth.trajectory_pose(4), intr_of(cam), W, H, NEAR, FAR)
    pts_h = qr.hit_points_of(rays_h, synth.render_depth("sphere_room", synth.trajectory_pose(4), synth.intrinsics(W, H), W, H).reshape(-1))
    pts, rays = torch.from_numpy(pts_h).to(dev), torch.from_numpy(rays_h).to(dev)
    p_out, r_out = device_outputs(len(pts), False, dev), ray_outputs(len(rays), False, dev)
    torch.cuda.synchronize()
    a, b, c = (ch.Chisel((N, N, N), res, False, max_chunks=8192) for _ in range(3))
    a.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    a.QueryPoints(pts, out=p_out)
    a.CastRays(rays, None, None, None, out=r_out)
    a.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4, 8)])
    b.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    b.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4, 8)])
    c.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    a.synchronize()
    mid_p = {k: v.cpu().numpy() for k, v in p_out.items()}
    mid_r = {k: v.cpu().numpy() for k, v in r_out.items()}
    equal_outputs(mid_p, c.QueryPoints(pts_h, sdf=True, weight=True, gradient=True), "points between the launch sets", list(mid_p))
    equal_outputs(mid_r, cast(c, rays_h, normals=True), "rays between the launch sets", list(mid_r))
    index = tgr.index_of(c)
    found, sdf, _ = qr.query_points(index, pts_h)
    assert np.array_equal((mid_p["found"] & 1).astype(bool), found) and found.mean() > 0.9
    same_bits(mid_p["sdf"], sdf, "... against the restatement")
    same_bits(mid_r["t_hit"].reshape(H, W), rr.render_depth(index, synth.trajectory_pose(4), intr_of(cam), W, H, NEAR, FAR), "... against the restatement")
    assert (mid_r["status"] == 1).mean() > 0.9
    after = a.QueryPoints(pts_h)  # (eight frames: other distances than after four)
    assert (after["sdf"].view(np.uint32) != mid_p["sdf"].view(np.uint32)).any()
    assert a.NumChunks() == b.NumChunks()
    compare_fields(b.fields(), a.fields(), a.V, False)
    assert a.counters() == b.counters()


def test_host_and_device_forms_are_equal():
    import torch
    case = [i for i, m in enumerate(MAPS) if m[6]][0]
    gm, _, sets = built(case)
    dev = torch.device("cuda:0")
    pts_h = sets["box"][-4099:]
    cam = tgr.camera(77, 53)
    rays_h = qr.view_rays(synth.trajectory_pose(20), intr_of(cam), 77, 53, NEAR, FAR)
    pts, rays = torch.from_numpy(pts_h).to(dev), torch.from_numpy(rays_h).to(dev)
    p_out, r_out = device_outputs(len(pts), True, dev), ray_outputs(len(rays), True, dev)
    torch.cuda.synchronize()
    assert gm.QueryPoints(pts, out=p_out) is p_out
    assert gm.CastRays(rays, None, None, None, out=r_out) is r_out
    gm.synchronize()
    host_p = gm.QueryPoints(pts_h, sdf=True, weight=True, gradient=True, colors=True)
    host_r = cast(gm, rays_h, normals=True, colors=True)
    equal_outputs({k: v.cpu().numpy() for k, v in p_out.items()}, host_p, "points", list(p_out))
    equal_outputs({k: v.cpu().numpy() for k, v in r_out.items()}, host_r, "rays", list(r_out))
    assert 0 < (host_r["status"] == 1).mean() < 1
    # origins, directions and bounds as separate device tensors: packed on torch's stream, the map ordered behind it
    only = {"t_hit": torch.zeros(len(rays), dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    gm.CastRays(rays[:, 0:3], rays[:, 3:6], NEAR, FAR, out=only)
    gm.synchronize()
    same_bits(only["t_hit"].cpu().numpy(), host_r["t_hit"], "t_hit alone, packed on the device")
    # one output alone into a device tensor
    alone = {"gradient": torch.zeros((len(pts), 3), dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    gm.QueryPoints(pts, out=alone)
    gm.synchronize()
    same_bits(alone["gradient"].cpu().numpy(), host_p["gradient"], "gradient alone")


def test_device_inputs_behind_an_event():
    """positions and rays produced on another stream, their completion handed over with chisel_hip_wait_event: the next query waits
    for the event on the device (and uses it up), and answers what the host form answers"""
    import torch
    gm, _, sets = built(0)
    dev = torch.device("cuda:0")
    pts_h = sets["jitter"][-4099:]
    fin = np.isfinite(pts_h).all(1)
    cam = tgr.camera(77, 53)
    rays_h = qr.view_rays(synth.trajectory_pose(4), intr_of(cam), 77, 53, NEAR, FAR)
    p_out, r_out = device_outputs(len(pts_h), False, dev), ray_outputs(len(rays_h), False, dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for what in ("points", "rays"):
        with torch.cuda.stream(side):
            busy = torch.ones((2048, 2048), device=dev)
            for _ in range(20):  # (keeps the side stream busy ahead of the copy, so that a query that did not wait would read zeros)
                busy = busy @ busy * 0.0 + 1.0
            src = torch.from_numpy(pts_h if what == "points" else rays_h).pin_memory()
            data = torch.zeros(src.shape, dtype=torch.float32, device=dev)
            data.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        gm.wait_event(ev.cuda_event)
        if what == "points":
            gm.QueryPoints(data, out=p_out)
        else:
            gm.CastRays(data, None, None, None, out=r_out)
        gm.synchronize()
        side.synchronize()
    host_p = gm.QueryPoints(pts_h, sdf=True, weight=True, gradient=True)
    host_r = cast(gm, rays_h, normals=True)
    equal_outputs({k: v.cpu().numpy() for k, v in p_out.items()}, host_p, "points behind an event", list(p_out))
    equal_outputs({k: v.cpu().numpy() for k, v in r_out.items()}, host_r, "rays behind an event", list(r_out))
    assert (host_p["found"][fin] & 1).mean() > 0.9 and (host_r["status"] == 1).mean() > 0.9
