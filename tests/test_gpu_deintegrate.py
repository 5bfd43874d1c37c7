"""chisel_hip_deintegrate_depth on the GPU against its restatement (tests/deintegrate_restated.py), bit for bit through
GetChunk: every distance and weight, the colours untouched, the six stats, the emptied ids; then what a map must still be good for
afterwards -- collecting the emptied chunks, meshing, integrating a frame --, the ordering on the map's stream, every refusal, and who
frees the scratch."""
import ctypes as C

import numpy as np
import pytest

from tests import deintegrate_restated as dr
from tests import merge_restated as mr
from tests.common import compare_meshes as _compare_meshes
from tests.common import fields_of, free_bytes, upload
from tests.deintegrate_gpu import dirty, integrate, integrator, new_map, pinhole, take_out

pytestmark = pytest.mark.gpu


# ---- a. integrated maps ---------------------------------------------------------------------------------------------------------------------
def _cases():
    """every chunk size with every truncator and both rule sets; the sequence, the carving setting and which frame leaves (first,
    middle, last) rotate"""
    out, i = [], 0
    seqs = list(dr.SEQUENCES)
    for N in (8, 16, 32):
        for trunc in dr.TRUNCATORS:
            for color_rules in (False, True):
                out.append((seqs[i % len(seqs)], N, trunc, color_rules, bool((i // 2) % 2), ("first", "middle", "last")[i % 3]))
                i += 1
    return out


@pytest.mark.parametrize("seq,N,trunc,color_rules,carving,which", _cases(), ids=lambda v: str(v))
def test_integrated_maps(seq, N, trunc, color_rules, carving, which):
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules, carving)
    gm = new_map(N, color_rules)
    integrate(gm, rules, frames, cam)
    j = {"first": 0, "middle": len(frames) // 2, "last": len(frames) - 1}[which]
    _, wstats, _, _ = take_out(gm, frames[j], rules, cam, N)
    assert wstats["chunks_touched"] > 10 and wstats["voxels_updated"] + wstats["voxels_cleared"] > 100  # (`sparse` has 16 valid pixels)
    gm.close()


# ---- b. hand-built fields: every branch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,N,trunc,color_rules", [("tilt", 8, "constant", False), ("neg_aniso", 8, "inverse", True),
                                                     ("hostile", 16, "quadratic", False), ("cx_out", 32, "inverse", True)], ids=lambda v: str(v))
def test_hand_built_fields(oracle_mod, seq, N, trunc, color_rules):
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules)
    field = dr.hand_built(dr.oracle_map(oracle_mod, N, dr.GRIDS[N], rules, frames[:2], cam).fields(), frames[1], rules, N, dr.GRIDS[N])
    gm = new_map(N, color_rules)
    upload(gm, field)
    _, _, detail, _ = take_out(gm, frames[1], rules, cam, N)
    r = dr.reach(detail)
    for k in ("updated", "cleared_zero", "cleared_residue", "cleared_negative", "skipped"):
        assert r[k] > 0, (k, r)
    gm.close()


def test_a_frame_that_sees_nothing():
    """the camera turned away from everything the map holds: all zero but chunks_tested, the dirty list as it was"""
    frames, cam = dr.sequence("tilt")
    rules = dr.rules_of("constant")
    gm = new_map(8, False)
    integrate(gm, rules, frames, cam)
    depth, pose, intr = frames[0]
    away = np.array(pose, np.float32)
    away[:3, :3] = away[:3, :3] @ np.diag([1.0, -1.0, -1.0]).astype(np.float32)  # half a turn about the camera's x axis
    _, wstats, _, _ = take_out(gm, (depth, away, intr), rules, cam, 8)
    assert wstats == dict(dict.fromkeys(dr.STAT_NAMES, 0), chunks_tested=gm.NumChunks()) and gm.NumChunks() > 50
    gm.close()


# ---- c. the emptied chunks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["collect", "ids"])
def test_emptied_chunks_can_be_collected(how):
    frames, cam = dr.sequence("neg_aniso")
    rules = dr.rules_of("inverse")
    gm = new_map(8, False)
    integrate(gm, rules, frames, cam)
    want, wstats, detail, got = take_out(gm, frames[-1], rules, cam, 8, collect=(how == "collect"))
    if how == "ids":
        gm.GarbageCollect(got["emptied_ids"])
        want = {cid: v for cid, v in want.items() if cid not in set(detail["emptied"])}
    assert wstats["chunks_emptied"] > 3
    left = sorted(map(tuple, gm.GetChunkIDs().tolist()))
    assert left == sorted(want) == dr.holds_weight(want)  # exactly the chunks that still hold weight
    gm.close()


def test_fewer_ids_than_emptied_chunks():
    from cvids_amd import capi, chisel as ch
    frames, cam = dr.sequence("neg_aniso")
    rules = dr.rules_of("inverse")
    gm = new_map(8, False)
    integrate(gm, rules, frames, cam)
    _, wstats, detail = dr.restated_deintegrate(fields_of(gm, 8), frames[-1], rules, 8, dr.GRIDS[8])
    assert wstats["chunks_emptied"] > 3
    f, keep = ch.depth_frame(frames[-1][0], frames[-1][1], pinhole(cam))
    st = capi.DeintegrateStats()
    ids = np.full((4, 3), 77777, np.int32)
    capi.check(gm.L.chisel_hip_deintegrate_depth(gm.h, C.byref(f), 0, C.byref(st), ids.ctypes.data_as(C.POINTER(C.c_int)), 2))
    assert st.chunks_emptied == wstats["chunks_emptied"]  # the count is the truth ...
    assert (ids[2:] == 77777).all() and len({tuple(r) for r in ids[:2].tolist()} & set(detail["emptied"])) == 2  # ... and max_ids ids are written
    gm.close()


# ---- d. meshes and a follow-on frame -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,N,color_rules", [("tilt", 8, True), ("neg_aniso", 16, False)])
def test_mesh_after_deintegration(oracle_mod, seq, N, color_rules):
    """UpdateMeshes before and after against the oracle's recompute on the downloaded fields, over the ids the map lists"""
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of("constant", color_rules)
    gm = new_map(N, color_rules)
    integrate(gm, rules, frames, cam)
    om = oracle_mod.OracleMap(N, dr.GRIDS[N], color_rules)
    for stage in ("before", "after"):
        if stage == "after":
            _, wstats, detail, _ = take_out(gm, frames[1], rules, cam, N)
            assert wstats["chunks_emptied"] > 0 and wstats["chunks_touched"] > wstats["chunks_emptied"]
        for cid, (s, w, c) in gm.fields().items():
            om.put_chunk(cid, s, w, c)
        om.recompute_meshes(sorted(dirty(gm)))
        gm.UpdateMeshes(force=True)
        n, nv = _compare_meshes(om, gm, color_rules)
        print("%s: %d meshes, %d vertices" % (stage, n, nv))
        assert n >= 10 and nv > 1000 and len(dirty(gm)) == 0
    gm.close()


@pytest.mark.parametrize("color_rules", [False, True])
def test_frame_into_the_map_afterwards(oracle_mod, color_rules):
    """a frame integrated afterwards gives the oracle's fields when the oracle starts from the downloaded fields: the bookkeeping
    (residency, the dirty list, the sign summaries the culling reads) survives"""
    frames, cam = dr.sequence("tilt")
    rules = dr.rules_of("inverse", color_rules, carving=True)
    gm = new_map(8, color_rules)
    integrate(gm, rules, frames[:3], cam)
    take_out(gm, frames[1], rules, cam, 8)
    om = oracle_mod.OracleMap(8, dr.GRIDS[8], color_rules)
    om.set_integrator(rules.kind, float(rules.param), float(rules.weight), rules.carving, float(rules.carving_dist))
    for cid, (s, w, c) in gm.fields().items():
        om.put_chunk(cid, s, w, c)
    gm.counters(reset=True)
    integrate(gm, rules, frames[3:], cam)
    d, p, intr = frames[3]
    if color_rules:
        om.integrate_depth_color(d, p, intr, dr.color_image(), near=cam[4], far=cam[5])
    else:
        om.integrate_depth(d, p, intr, near=cam[4], far=cam[5])
    oc, gc = om.counters(), gm.counters()
    for k in ("sdf", "col", "col_sat", "probe", "carved", "updated_chunks"):
        assert oc[k] == gc[k], (k, oc[k], gc[k])
    assert oc["sdf"] > 1000 and om.num_chunks() == gm.NumChunks()
    mr.assert_fields_bit_equal({c: (s, w, x if x is not None else np.zeros((512, 4), np.uint8)) for c, (s, w, x) in om.fields().items()},
                               fields_of(gm, 8), True, "frame after the de-integration")
    gm.close()


# ---- e. ordering ---------------------------------------------------------------------------------------------------------------------------
def test_queued_without_a_wait():
    """a batch, the de-integration behind it (stats=False), a frame behind that.  `device`: the depth image is a device tensor, so the
    call waits for nothing -- this is the leg that shows the ordering on the map's stream; `host`: a host array, which the call has
    copied before it returns (it waits for its own copy), so it shows that both kinds of image give the same fields; `host-waits`:
    the reference, a wait after every call"""
    import torch
    frames, cam = dr.sequence("tilt")
    rules = dr.rules_of("inverse", carving=True)
    integ, camera = integrator(rules), pinhole(cam)
    results = {}
    for mode in ("host-waits", "host", "device"):
        gm = new_map(16, False)
        d, p, _ = frames[1]
        image = torch.from_numpy(d).to("cuda:0") if mode == "device" else d
        torch.cuda.synchronize()
        gm.IntegrateBatch(integ, [(d, p, camera) for d, p, _ in frames[:3]])
        if mode == "host-waits":
            gm.synchronize()
        assert gm.DeintegrateDepthScan(integ, image, p, camera, stats=False) is None
        if mode == "host-waits":
            gm.synchronize()
        gm.IntegrateDepthScan(integ, frames[3][0], frames[3][1], camera)
        gm.synchronize()
        results[mode] = fields_of(gm, 16)
        gm.close()
    assert len(results["host"]) > 50
    mr.assert_fields_bit_equal(results["host-waits"], results["device"], False, "queued without a wait")
    mr.assert_fields_bit_equal(results["host-waits"], results["host"], False, "host image")


@pytest.mark.parametrize("color_rules", [False, True])
def test_reintegrate_is_the_composition(color_rules):
    frames, cam = dr.sequence("tilt")
    rules = dr.rules_of("constant", color_rules)
    integ, camera = integrator(rules), pinhole(cam)
    d, p, _ = frames[1]
    colour = dr.color_image() if color_rules else None
    a, b = new_map(8, color_rules), new_map(8, color_rules)
    for gm in (a, b):
        integrate(gm, rules, [frames[0], (d, dr.perturbed(p), None), frames[2]], cam)
    out = a.ReintegrateDepthScan(integ, d, dr.perturbed(p), p, camera, color_image=colour)
    b.DeintegrateDepthScan(integ, d, dr.perturbed(p), camera, color_rules=color_rules)
    integrate(b, rules, [frames[1]], cam)
    assert out["voxels_updated"] > 0
    mr.assert_fields_bit_equal(fields_of(b, 8), fields_of(a, 8), True, "ReintegrateDepthScan")
    a.close()
    b.close()


# ---- f. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_alone():
    from cvids_amd import capi, chisel as ch
    frames, cam = dr.sequence("tilt")
    rules = dr.rules_of("constant")
    gm = new_map(8, False)
    integrate(gm, rules, frames[:2], cam)
    state = lambda: (fields_of(gm, 8), gm.counters(), gm.NumChunks(), sorted(dirty(gm)))
    start = state()
    depth, pose, _ = frames[1]

    def refused(code, handle=gm, stats=True, ids=True, max_ids=4, null_frame=False, **change):
        f, keep = ch.depth_frame(depth, pose, pinhole(cam))
        for k, v in change.items():
            if k == "pose":
                f.pose[v[0]] = v[1]
            else:
                setattr(f, k, v)
        st, buf = capi.DeintegrateStats(), np.zeros((4, 3), np.int32)
        rc = gm.L.chisel_hip_deintegrate_depth(handle.h if handle is not None else None, None if null_frame else C.byref(f), 0,
                                               C.byref(st) if stats else None, buf.ctypes.data_as(C.POINTER(C.c_int)) if ids else None, max_ids)
        assert capi.STATUS[rc] == code, (capi.STATUS[rc], code, change)
        assert b"chisel_hip_deintegrate_depth" in gm.L.chisel_hip_last_error()
        now = state()
        mr.assert_fields_bit_equal(start[0], now[0], False, "after a refusal")
        assert now[1:] == start[1:]

    refused("ERR_INVALID", handle=None)
    refused("ERR_INVALID", null_frame=True)
    refused("ERR_INVALID", depth=None)
    refused("ERR_INVALID", width=0)
    refused("ERR_INVALID", height=-3)
    refused("ERR_INVALID", width=1 << 16, height=1 << 15)  # 2^31 pixels
    for bad in (np.nan, np.inf, -np.inf):
        refused("ERR_INVALID", pose=(0, bad))
        refused("ERR_INVALID", pose=(11, bad))
        for k in ("fx", "fy", "cx", "cy"):
            refused("ERR_INVALID", **{k: bad})
    refused("ERR_INVALID", max_ids=-1)
    refused("ERR_INVALID", stats=False)  # ids without stats
    group = new_map(8, False, devices=[0, 0])
    shard = new_map(8, False, n_shards=2, shard_rank=0)
    refused("ERR_UNSUPPORTED", handle=group)
    refused("ERR_UNSUPPORTED", handle=shard)
    # ... and the call goes through afterwards: the refusals left nothing behind
    take_out(gm, frames[1], rules, cam, 8)
    for m in (gm, group, shard):
        m.close()


# ---- g. lifetime ---------------------------------------------------------------------------------------------------------------------------
def test_cycles_return_their_memory():
    """tests/test_gpu_merge.py's pattern: a map created, filled, de-integrated and destroyed four times; the free device memory after the
    first cycle against that after the fourth, within half the footprint of the voxel pool.  And a second call allocates nothing."""
    N, max_chunks = 16, 1024
    footprint = max_chunks * N ** 3 * (4 + 4)
    frames, cam = dr.sequence("tilt")
    rules = dr.rules_of("constant")
    second = []

    def cycle():
        gm = new_map(N, False, max_chunks=max_chunks, device_id=0)
        integrate(gm, rules, frames[:3], cam)
        integ, camera = integrator(rules), pinhole(cam)
        assert gm.DeintegrateDepthScan(integ, frames[1][0], frames[1][1], camera)["voxels_cleared"] > 0
        a = free_bytes()
        assert gm.DeintegrateDepthScan(integ, frames[2][0], frames[2][1], camera)["voxels_cleared"] > 0
        second.append(a - free_bytes())
        gm.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; drift %d; taken by a second call: %s" % (readings, footprint, drift, second))
    assert abs(drift) < footprint // 2, (readings, footprint)
    assert all(v <= 0 for v in second), second
