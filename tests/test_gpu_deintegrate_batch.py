"""chisel_hip_deintegrate_batch on the GPU (DESIGN.md 3.10 "Many frames in one call") against its restatement -- the fold of the single
frame's restatement over the frames (tests/deintegrate_batch_cases.py) --, bit for bit through GetChunk: every distance and weight, the
colours untouched, the six stats, the emptied ids, the dirty set, the counters; against the library's own single-frame entry; the order
of the frames, the boundaries of the launch sets, hand-built weights, mixed inputs, ordering on the stream, ids and collection,
ReintegrateDepthScans, every refusal, and who frees the scratch."""
import ctypes as C

import numpy as np
import pytest

from tests import deintegrate_batch_cases as bc
from tests import deintegrate_gpu as gd
from tests import deintegrate_restated as dr
from tests import frame_cases as fc
from tests import merge_restated as mr
from tests.common import compare_meshes, fields_of, free_bytes, upload

pytestmark = pytest.mark.gpu
W, H = dr.W, dr.H


def camera_of(frame, cam):
    """the PinholeCamera of a frame (depth, pose, (fx, fy, cx, cy)): its own intrinsics and image size, the sequence's planes"""
    from cvids_amd.chisel import PinholeCamera
    fx, fy, cx, cy = frame[2][:4]
    return PinholeCamera(fx, fy, cx, cy, frame[0].shape[-1], frame[0].shape[-2], cam[4], cam[5])


def scans(frames, cam, images=None):
    """-> the list DeintegrateDepthScans takes; images: what stands in for the frames' own (device tensors)"""
    return [((images[i] if images is not None else f[0]), f[1], camera_of(f, cam)) for i, f in enumerate(frames)]


def take_out_batch(gm, frames, rules, cam, N, images=None, **kw):
    """the frames de-integrated in one call on the GPU and folded out of the fields the map holds now in the restatement; everything
    of the contract compared -> (restated field, restated stats, restated detail, what the call returned)"""
    before, listed = fields_of(gm, N), gd.dirty(gm)
    counters = gm.counters()
    want, wstats, detail = bc.restated_batch(before, frames, rules, N, dr.GRIDS[N])
    got = gm.DeintegrateDepthScans(gd.integrator(rules), scans(frames, cam, images), color_rules=rules.color_rules, **kw)
    print(wstats, bc.batch_reach(detail) if frames else {})
    assert {k: got[k] for k in dr.STAT_NAMES} == wstats, (got, wstats)
    ids = list(map(tuple, got["emptied_ids"].tolist()))
    assert sorted(ids) == detail["emptied"] and len(set(ids)) == len(ids)
    after = fields_of(gm, N)
    if kw.get("collect"):
        want = {cid: v for cid, v in want.items() if cid not in set(detail["emptied"])}
    mr.assert_fields_bit_equal(want, after, True, "after the batch")  # (sdf, weight, and rgbw as it was)
    assert gm.counters() == counters  # CHISEL_HIP_CNT_* count forward executions
    if not kw.get("collect"):
        assert gd.dirty(gm) == listed | (gd.neighbourhoods(detail["touched"]) if detail["touched"] else set())
    return want, wstats, detail, got


def filled(seq, N, trunc, color_rules, carving=True, n=20):
    """a map with the first n of the sequence's 20 frames in it -> (map, frames, camera, rules)"""
    frames, cam = bc.frames20(seq)
    rules = dr.rules_of(trunc, color_rules, carving)
    gm = gd.new_map(N, color_rules)
    gd.integrate(gm, rules, frames[:n], cam)
    return gm, frames, cam, rules


# ---- a. the cases: 17 frames, a full launch set and a set of one ---------------------------------------------------------------------------
@pytest.mark.parametrize("seq,N,trunc,color_rules", bc.CASES, ids=lambda v: str(v))
def test_cases_against_the_restated_fold(seq, N, trunc, color_rules):
    gm, frames, cam, rules = filled(seq, N, trunc, color_rules)
    _, wstats, detail, _ = take_out_batch(gm, frames[bc.OUT], rules, cam, N)
    assert wstats["chunks_tested"] == 17 * gm.NumChunks() and wstats["chunks_touched"] > 17 and wstats["chunks_emptied"] > 0
    assert wstats["voxels_updated"] > 1000 and wstats["voxels_cleared"] > 100 and wstats["voxels_skipped"] > 0
    gm.close()


def test_chunks_of_32_cubed():
    """the same construction where a lane owns 32 quads of a chunk, not one or four"""
    gm, frames, cam, rules = filled("tilt", 32, "constant", False)
    _, wstats, _, _ = take_out_batch(gm, frames[bc.OUT], rules, cam, 32)
    assert wstats["chunks_touched"] > 17 and wstats["chunks_emptied"] > 0 and wstats["voxels_updated"] > 1000 and wstats["voxels_cleared"] > 100 and wstats["voxels_skipped"] > 0
    gm.close()


# ---- b. against the library itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,N,trunc,color_rules", [bc.CASES[1], bc.CASES[2]], ids=lambda v: str(v))
def test_batch_is_the_single_calls_in_order(seq, N, trunc, color_rules):
    a, frames, cam, rules = filled(seq, N, trunc, color_rules)
    b, _, _, _ = filled(seq, N, trunc, color_rules)
    integ = gd.integrator(rules)
    total, ids = dict.fromkeys(dr.STAT_NAMES, 0), []
    for f in frames[bc.OUT]:
        got = a.DeintegrateDepthScan(integ, f[0], f[1], camera_of(f, cam), color_rules=color_rules)
        for k in dr.STAT_NAMES:
            total[k] += got[k]
        ids += list(map(tuple, got["emptied_ids"].tolist()))
    got = b.DeintegrateDepthScans(integ, scans(frames[bc.OUT], cam), color_rules=color_rules)
    print(total)
    assert {k: got[k] for k in dr.STAT_NAMES} == total and total["chunks_emptied"] > 0
    assert len(ids) == len(set(ids)) and sorted(map(tuple, got["emptied_ids"].tolist())) == sorted(ids)
    mr.assert_fields_bit_equal(fields_of(a, N), fields_of(b, N), True, "17 single calls against one batch")
    assert gd.dirty(a) == gd.dirty(b) and a.counters() == b.counters()
    a.close()
    b.close()


def test_single_and_batch_calls_interleaved_without_a_wait():
    """both entries share one set of scratch in the map: a single call, a batch and a single call queued with stats=False on device
    images (nothing waited for), then the same three kinds with stats and ids; every count, the fields and the dirty set against the
    restated fold of the same frames in the same order"""
    import torch
    gm, frames, cam, rules = filled(*bc.CASES[2])
    N, integ = 8, gd.integrator(rules)
    out = frames[bc.OUT]
    images = [torch.from_numpy(np.ascontiguousarray(f[0])).to("cuda:0") for f in out]
    torch.cuda.synchronize()
    field, listed, touched = fields_of(gm, N), gd.dirty(gm), set()
    for lo, hi in ((0, 1), (1, 6), (6, 7)):  # queued: nothing returned, nothing waited for
        part = scans(out[lo:hi], cam, images[lo:hi])
        if hi - lo == 1:
            assert gm.DeintegrateDepthScan(integ, *part[0], color_rules=rules.color_rules, stats=False) is None
        else:
            assert gm.DeintegrateDepthScans(integ, part, color_rules=rules.color_rules, stats=False) is None
    field, _, detail = bc.restated_batch(field, out[:7], rules, N, dr.GRIDS[N])
    touched |= detail["touched"]
    emptied = 0
    for lo, hi in ((7, 8), (8, 16), (16, 17)):  # behind them, on the same scratch: stats and ids
        part = scans(out[lo:hi], cam, images[lo:hi])
        if hi - lo == 1:
            got = gm.DeintegrateDepthScan(integ, *part[0], color_rules=rules.color_rules)
        else:
            got = gm.DeintegrateDepthScans(integ, part, color_rules=rules.color_rules)
        field, wstats, detail = bc.restated_batch(field, out[lo:hi], rules, N, dr.GRIDS[N])
        print((lo, hi), wstats)
        assert {k: got[k] for k in dr.STAT_NAMES} == wstats, (got, wstats)
        assert sorted(map(tuple, got["emptied_ids"].tolist())) == detail["emptied"]
        touched |= detail["touched"]
        emptied += wstats["chunks_emptied"]
    assert emptied > 0 and len(touched) > 17
    mr.assert_fields_bit_equal(field, fields_of(gm, N), True, "single, batch, single, twice")
    assert gd.dirty(gm) == listed | gd.neighbourhoods(touched)
    gm.close()


# ---- c. the order of the frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [(2, 3), (3, 2)], ids=lambda v: str(v))
def test_frames_apply_in_call_order(order):
    gm, frames, cam, rules = filled(*bc.CASES[2])
    take_out_batch(gm, [frames[i] for i in order], rules, cam, 8)
    gm.close()


# ---- d. the boundaries of the launch sets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 20])
def test_set_boundaries(n):
    gm, frames, cam, rules = filled("tilt", 8, "quadratic", True)
    _, _, _, got = take_out_batch(gm, frames[:n], rules, cam, 8)
    if n == 1:  # ... and the single-frame entry on a twin map
        twin, _, _, _ = filled("tilt", 8, "quadratic", True)
        one = twin.DeintegrateDepthScan(gd.integrator(rules), frames[0][0], frames[0][1], camera_of(frames[0], cam), color_rules=True)
        assert {k: one[k] for k in dr.STAT_NAMES} == {k: got[k] for k in dr.STAT_NAMES}
        assert sorted(map(tuple, one["emptied_ids"].tolist())) == sorted(map(tuple, got["emptied_ids"].tolist()))
        mr.assert_fields_bit_equal(fields_of(twin, 8), fields_of(gm, 8), True, "a batch of one against the single entry")
        assert gd.dirty(twin) == gd.dirty(gm)
        twin.close()
    gm.close()


# ---- e. hand-built weights: every branch, in the middle of a batch -----------------------------------------------------------------------
@pytest.mark.parametrize("seq,N,trunc,color_rules", [("neg_aniso", 8, "inverse", True), ("hostile", 16, "quadratic", False)], ids=lambda v: str(v))
def test_hand_built_weights_in_the_middle(oracle_mod, seq, N, trunc, color_rules):
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules)
    field = dr.hand_built(dr.oracle_map(oracle_mod, N, dr.GRIDS[N], rules, frames[:3], cam).fields(), frames[1], rules, N, dr.GRIDS[N])
    gm = gd.new_map(N, color_rules)
    upload(gm, field)
    _, _, detail, _ = take_out_batch(gm, [frames[0], frames[1], frames[2]], rules, cam, N)
    r = dr.reach(detail["per_frame"][1])  # what the hand-built frame meets behind the first one
    for k in ("updated", "cleared_zero", "cleared_residue", "cleared_negative", "skipped"):
        assert r[k] > 0, (k, r)
    gm.close()


# ---- f. mixed inputs in one call --------------------------------------------------------------------------------------------------------
def test_mixed_memory_spaces_and_image_sizes():
    import torch
    frames, cam = bc.frames20("tilt")
    small_cam = fc.camera("aniso", 40, 30)
    small = [(fc.depth_image(name, 40, 30, seed=i), frames[i][1], small_cam[:4]) for i, name in enumerate(("wall", "ramp", "steps"))]
    rules = dr.rules_of("inverse", False, carving=True)
    gm = gd.new_map(8, False)
    integ = gd.integrator(rules)
    mixed = [frames[0], small[0], frames[1], frames[2], small[1], frames[3], small[2], frames[4]]
    for f in mixed:
        gm.IntegrateDepthScan(integ, f[0], f[1], camera_of(f, cam))
    images = [torch.from_numpy(np.ascontiguousarray(f[0])).to("cuda:0") if i % 3 != 1 else f[0] for i, f in enumerate(mixed)]  # device, host, device, ...
    torch.cuda.synchronize()
    _, wstats, _, _ = take_out_batch(gm, mixed, rules, cam, 8, images=images)
    assert wstats["voxels_updated"] > 1000
    for f in mixed[:3]:
        gm.IntegrateDepthScan(integ, f[0], f[1], camera_of(f, cam))
    all_device = [torch.from_numpy(np.ascontiguousarray(f[0])).to("cuda:0") for f in mixed[:3]]
    torch.cuda.synchronize()
    take_out_batch(gm, mixed[:3], rules, cam, 8, images=all_device)
    gm.close()


# ---- g. nothing to do, and ordering on the stream ------------------------------------------------------------------------------------------
def test_a_batch_that_sees_nothing_and_an_empty_one():
    gm, frames, cam, rules = filled("tilt", 8, "constant", False, n=4)
    away = []
    for d, pose, intr in frames[:3]:
        p = np.array(pose, np.float32)
        p[:3, :3] = p[:3, :3] @ np.diag([1.0, -1.0, -1.0]).astype(np.float32)  # half a turn about the camera's x axis
        away.append((d, p, intr))
    _, wstats, _, _ = take_out_batch(gm, away, rules, cam, 8)
    assert wstats == dict(dict.fromkeys(dr.STAT_NAMES, 0), chunks_tested=3 * gm.NumChunks()) and gm.NumChunks() > 50
    _, wstats, _, got = take_out_batch(gm, [], rules, cam, 8)
    assert wstats == dict.fromkeys(dr.STAT_NAMES, 0) and len(got["emptied_ids"]) == 0
    assert gm.DeintegrateDepthScans(gd.integrator(rules), [], stats=False) is None
    gm.close()


def test_queued_without_a_wait():
    """a batch in, the batch de-integration behind it (stats=False, device images: nothing waited for), a frame behind that; against
    the same with a wait after every call, whose de-integration is held to the restatement"""
    import torch
    frames, cam = bc.frames20("tilt")
    rules = dr.rules_of("inverse", carving=True)
    integ = gd.integrator(rules)
    out = frames[1:19]  # two launch sets
    results = {}
    for mode in ("host-waits", "host", "device"):
        gm = gd.new_map(8, False)
        images = [torch.from_numpy(f[0]).to("cuda:0") for f in out] if mode == "device" else None
        torch.cuda.synchronize()
        gm.IntegrateBatch(integ, scans(frames, cam))
        if mode == "host-waits":
            take_out_batch(gm, out, rules, cam, 8)
        else:
            assert gm.DeintegrateDepthScans(integ, scans(out, cam, images), stats=False) is None
        gm.IntegrateDepthScan(integ, frames[3][0], frames[3][1], camera_of(frames[3], cam))
        gm.synchronize()
        results[mode] = fields_of(gm, 8)
        gm.close()
    assert len(results["host"]) > 50
    mr.assert_fields_bit_equal(results["host-waits"], results["device"], False, "queued without a wait")
    mr.assert_fields_bit_equal(results["host-waits"], results["host"], False, "host images")


# ---- h. ids and collection -----------------------------------------------------------------------------------------------------------------
def test_fewer_ids_than_emptied_chunks():
    from cvids_amd import capi, chisel as ch
    gm, frames, cam, rules = filled(*bc.CASES[2])
    out = frames[bc.OUT]
    _, wstats, detail = bc.restated_batch(fields_of(gm, 8), out, rules, 8, dr.GRIDS[8])
    assert wstats["chunks_emptied"] > 3
    fa, keep = (ch.DepthFrame * len(out))(), []
    for i, f in enumerate(out):
        fa[i], k = ch.depth_frame(f[0], f[1], camera_of(f, cam))
        keep.append(k)
    st = capi.DeintegrateStats()
    ids = np.full((4, 3), 77777, np.int32)
    gm._use(gd.integrator(rules))
    capi.check(gm.L.chisel_hip_deintegrate_batch(gm.h, len(out), fa, 1, C.byref(st), ids.ctypes.data_as(C.POINTER(C.c_int)), 2))
    assert {k: int(getattr(st, k)) for k in dr.STAT_NAMES} == wstats  # the count is the truth ...
    assert (ids[2:] == 77777).all() and len({tuple(r) for r in ids[:2].tolist()} & set(detail["emptied"])) == 2  # ... and max_ids ids are written
    gm.close()


def test_emptied_chunks_are_collected():
    gm, frames, cam, rules = filled(*bc.CASES[2])
    want, wstats, detail, _ = take_out_batch(gm, frames[bc.OUT], rules, cam, 8, collect=True)
    assert wstats["chunks_emptied"] > 3
    assert sorted(map(tuple, gm.GetChunkIDs().tolist())) == sorted(want) and not set(want) & set(detail["emptied"])
    gm.close()


# ---- i. the corrected stretch of trajectory ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color_rules", [False, True])
def test_reintegrate_scans(oracle_mod, color_rules):
    """ReintegrateDepthScans is DeintegrateDepthScans + IntegrateBatch, bit for bit; what it leaves is the oracle's map of the frames as
    they are within the bound the CPU test measured; and the map is good for meshing and for a further frame"""
    N, trunc = 8, "constant"
    frames, wrong, cam = bc.reintegration_frames()
    rules = dr.rules_of(trunc, color_rules)
    integ, camera = gd.integrator(rules), gd.pinhole(cam)
    colour = dr.color_image() if color_rules else None
    a, b = gd.new_map(N, color_rules), gd.new_map(N, color_rules)
    for gm in (a, b):
        gd.integrate(gm, rules, wrong, cam)
    old = [(wrong[i][0], wrong[i][1], camera) for i in bc.REINTEGRATED]
    new_poses = [frames[i][1] for i in bc.REINTEGRATED]
    out = a.ReintegrateDepthScans(integ, old, new_poses, colors=[colour] * len(old) if color_rules else None)
    b.DeintegrateDepthScans(integ, old, color_rules=color_rules)
    again = [(frames[i][0], frames[i][1], camera) for i in bc.REINTEGRATED]
    b.IntegrateBatch(integ, again, [(colour, p, camera) for _, p, _ in again] if color_rules else None)
    assert out["voxels_updated"] > 0
    mr.assert_fields_bit_equal(fields_of(b, N), fields_of(a, N), True, "ReintegrateDepthScans")
    b.close()
    right = dr.oracle_map(oracle_mod, N, dr.GRIDS[N], rules, frames, cam).fields()
    worst, same_w = dr.max_sdf_difference({c: (s, w, None) for c, (s, w, _) in a.fields().items()}, right)
    print("against the oracle: max |d sdf| %.9e, weights bit-equal: %s; bound %.9e" % (worst, same_w, bc.REINTEGRATION_BOUND[color_rules]))
    assert worst <= bc.REINTEGRATION_BOUND[color_rules]
    # the mesh over what the map lists, and a further frame, against the oracle started from the downloaded fields
    om = oracle_mod.OracleMap(N, dr.GRIDS[N], color_rules)
    om.set_integrator(rules.kind, float(rules.param), float(rules.weight), rules.carving, float(rules.carving_dist))
    for cid, (s, w, c) in a.fields().items():
        om.put_chunk(cid, s, w, c)
    om.recompute_meshes(sorted(gd.dirty(a)))
    a.UpdateMeshes(force=True)
    n, nv = compare_meshes(om, a, color_rules)
    assert n >= 10 and nv > 1000 and len(gd.dirty(a)) == 0
    d, p, intr = frames[0][0], dr.perturbed(frames[0][1], 0.01, 0.5), frames[0][2]
    gd.integrate(a, rules, [(d, p, intr)], cam)
    if color_rules:
        om.integrate_depth_color(d, p, intr, dr.color_image(), near=cam[4], far=cam[5])
    else:
        om.integrate_depth(d, p, intr, near=cam[4], far=cam[5])
    mr.assert_fields_bit_equal({c: (s, w, x if x is not None else np.zeros((N ** 3, 4), np.uint8)) for c, (s, w, x) in om.fields().items()},
                               fields_of(a, N), True, "a frame after the re-integration")
    a.close()


# ---- j. refusals and lifetime --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_alone():
    from cvids_amd import capi, chisel as ch
    frames, cam = dr.sequence("tilt")
    rules = dr.rules_of("constant")
    gm = gd.new_map(8, False)
    gd.integrate(gm, rules, frames[:2], cam)
    state = lambda: (fields_of(gm, 8), gm.counters(), gm.NumChunks(), sorted(gd.dirty(gm)))
    start = state()
    n = 18  # two launch sets

    def refused(code, handle=gm, stats=True, ids=True, max_ids=4, count=n, null_frames=False, at=None, **change):
        fa = (ch.DepthFrame * n)()
        keep = []
        for i in range(n):
            fa[i], k = ch.depth_frame(frames[i % 4][0], frames[i % 4][1], gd.pinhole(cam))
            keep.append(k)
        for k, v in change.items():
            if k == "pose":
                fa[at].pose[v[0]] = v[1]
            else:
                setattr(fa[at], k, v)
        st, buf = capi.DeintegrateStats(), np.zeros((4, 3), np.int32)
        rc = gm.L.chisel_hip_deintegrate_batch(handle.h if handle is not None else None, count, None if null_frames else fa, 0,
                                               C.byref(st) if stats else None, buf.ctypes.data_as(C.POINTER(C.c_int)) if ids else None, max_ids)
        assert capi.STATUS[rc] == code, (capi.STATUS[rc], code, change)
        message = gm.L.chisel_hip_last_error()
        assert b"chisel_hip_deintegrate_batch" in message
        if at is not None:
            assert b"frame %d:" % at in message, message  # the message names the frame
        now = state()
        mr.assert_fields_bit_equal(start[0], now[0], False, "after a refusal")
        assert now[1:] == start[1:]

    refused("ERR_INVALID", handle=None)
    refused("ERR_INVALID", null_frames=True)
    refused("ERR_INVALID", count=-1)
    for at in (0, 9, 17):  # first, in the middle, last: behind frames that are fine
        refused("ERR_INVALID", at=at, depth=None)
        refused("ERR_INVALID", at=at, width=0)
        refused("ERR_INVALID", at=at, height=-3)
        refused("ERR_INVALID", at=at, width=1 << 16, height=1 << 15)  # 2^31 pixels
        for bad in (np.nan, np.inf):
            refused("ERR_INVALID", at=at, pose=(11, bad))
            refused("ERR_INVALID", at=at, fx=bad)
            refused("ERR_INVALID", at=at, cy=bad)
    refused("ERR_INVALID", max_ids=-1)
    refused("ERR_INVALID", stats=False)  # ids without stats
    group = gd.new_map(8, False, devices=[0, 0])
    shard = gd.new_map(8, False, n_shards=2, shard_rank=0)
    refused("ERR_UNSUPPORTED", handle=group)
    refused("ERR_UNSUPPORTED", handle=shard)
    # ... and the call goes through afterwards: the refusals left nothing behind
    take_out_batch(gm, [frames[1], frames[0]], rules, cam, 8)
    for m in (gm, group, shard):
        m.close()


def test_cycles_return_their_memory():
    """a map created, filled, de-integrated in batches and destroyed four times; the free device memory after the first cycle against
    that after the fourth, within half the footprint of the voxel pool.  And a second call allocates nothing."""
    N, max_chunks = 16, 1024
    footprint = max_chunks * N ** 3 * (4 + 4)
    frames, cam = bc.frames20("tilt")
    rules = dr.rules_of("constant")
    second = []

    def cycle():
        gm = gd.new_map(N, False, max_chunks=max_chunks, device_id=0)
        gd.integrate(gm, rules, frames[:8], cam)
        integ = gd.integrator(rules)
        assert gm.DeintegrateDepthScans(integ, scans(frames[4:8], cam))["voxels_updated"] > 0
        a = free_bytes()
        assert gm.DeintegrateDepthScans(integ, scans(frames[1:4], cam))["voxels_cleared"] > 0
        assert gm.DeintegrateDepthScans(integ, scans(frames[:1], cam), stats=False) is None
        second.append(a - free_bytes())
        gm.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; drift %d; taken by later calls: %s" % (readings, footprint, drift, second))
    assert abs(drift) < footprint // 2, (readings, footprint)
    assert all(v <= 0 for v in second), second
