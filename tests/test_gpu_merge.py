"""chisel_hip_merge_map on the GPU against its restatement (tests/merge_restated.py), bit for bit through AddChunk /
GetChunk: chunk-id sets, every voxel array, the four stats, the counters; then what a merged map must still be good for -- meshing,
integrating a frame -- the ordering against the source's stream, every refusal, and who frees the scratch."""
import ctypes as C

import numpy as np
import pytest

from cvids_amd import synth
from tests import merge_restated as mr
from tests import voxel_fields as vf
from tests.common import compare_fields, fields_of, free_bytes, small_camera, upload
from tests.common import compare_meshes as _compare_meshes

pytestmark = pytest.mark.gpu
MAX_CHUNKS = 512
_id = lambda c: "%d-%s-%s" % c


def new_map(N, res, color=True, max_chunks=MAX_CHUNKS, **kw):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), res, color, max_chunks=max_chunks, **kw)


def no_colour(field):
    return {cid: (s, w, np.zeros_like(c)) for cid, (s, w, c) in field.items()}


def run_case(N, name, kind, dst_color=True, src_color=True, **dst_kw):
    """-> (dst map, src map, restated field, restated stats): both maps uploaded, merged once, everything of the contract compared"""
    src_f, dst_f, pose, res = mr.case(N, name, kind)
    want, wstats, _ = mr.merged(N, name, kind, dst_color, src_color)
    src, dst = new_map(N, res, src_color), new_map(N, res, dst_color, **dst_kw)
    upload(src, src_f)
    upload(dst, dst_f)
    before = dst.counters()
    src_before, epoch_before = src.counters(), topology_epoch(dst)
    stats = dst.MergeMap(src, pose)
    print((N, name, kind), stats)
    assert stats == {k: wstats[k] for k in stats}, (stats, wstats)
    mr.assert_fields_bit_equal(want if dst_color else no_colour(want), fields_of(dst, N), True, "dst %s %s" % (name, kind))
    mr.assert_fields_bit_equal(src_f if src_color else no_colour(src_f), fields_of(src, N), True, "src")
    assert dst.NumChunks() == len(want)
    after = dst.counters()
    delta = {k: after[k] - before[k] for k in after}
    expect = dict.fromkeys(after, 0)
    expect.update(sdf=wstats["voxels_updated"], col=wstats["col"], new_chunks=wstats["dst_chunks_created"], updated_chunks=wstats["dst_chunks_updated"])
    assert delta == expect, (delta, expect)
    assert src.counters() == src_before
    assert (topology_epoch(dst) != epoch_before) or wstats["dst_chunks_created"] == 0
    return dst, src, want, wstats


def topology_epoch(gm):
    out = C.c_uint64(0)
    from cvids_amd.capi import check
    check(gm.L.chisel_hip_topology_epoch(gm.h, C.byref(out)))
    return out.value


# ---- a. the cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mr.case_names(), ids=_id)
def test_cases(case):
    dst, src, _, _ = run_case(*case)
    dst.close()
    src.close()


def test_growing_pool():
    """a pool that starts with 16 chunks of 32^3 and has to take 27 candidates: it grows before the first chunk is created"""
    dst, src, want, _ = run_case(32, "rpy_neg", "empty", max_chunks=-1)
    info = dst.pool_info()
    assert info["growable"] and info["grown"] >= 1 and info["committed"] >= len(want)
    dst.close()
    src.close()


# ---- b. colour ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_color,src_color", [(True, True), (False, True), (True, False)])
def test_colour(dst_color, src_color):
    """colour in both maps, only in the source, only in the destination: in the last two the destination's rgbw is what it was"""
    dst, src, want, wstats = run_case(8, "rpy_neg", "dense", dst_color, src_color)
    if dst_color and not src_color:
        dst_f = mr.case(8, "rpy_neg", "dense")[1]
        for cid, (_, _, c) in fields_of(dst, 8).items():
            assert mr.same_bits(c, dst_f[cid][2] if cid in dst_f else np.zeros((8 ** 3, 4), np.uint8))
    assert (wstats["col"] > 0) == (dst_color and src_color)
    dst.close()
    src.close()


# ---- c. mesh ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,name", [(8, "rpy_neg"), (16, "rpy_neg"), (8, "shift_voxels")])
def test_mesh_after_merge(oracle_mod, N, name):
    """UpdateMeshes on the merged map against the oracle's recompute on the restated field, over the 27-neighbourhoods of the updated chunks"""
    src_f, dst_f, pose, res = mr.case(N, name, "dense")
    dst, src, want, _ = run_case(N, name, "dense")
    detail = mr.merged(N, name, "dense")[2]
    updated = [cid for cid, d in detail.items() if d["updates"] > 0]
    todo = sorted({(x + dx, y + dy, z + dz) for x, y, z in updated for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)})
    listed = set(map(tuple, dst.GetMeshesToUpdate().tolist()))
    assert set(updated) <= listed and listed == set(todo), (len(listed), len(todo))
    om = oracle_mod.OracleMap(N, res, True)
    for cid, (s, w, c) in want.items():
        om.put_chunk(cid, s, w, c)
    om.recompute_meshes(todo)
    dst.UpdateMeshes(force=True)
    n, nv = _compare_meshes(om, dst, True)
    print("%d updated chunks, %d meshes, %d vertices" % (len(updated), n, nv))
    assert n >= 1 and nv > 0  # (a chunk without a mesh is in neither list: _compare_meshes has compared the id sets)
    assert len(dst.GetMeshesToUpdate()) == 0
    dst.close()
    src.close()


# ---- d. follow-on use ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "empty"])
def test_frame_into_the_merged_map(oracle_mod, kind):
    """a depth frame integrated into the merged map gives the oracle's result for that frame on the restated field: the pool invariant
    (free slots hold default voxels, also those of chunks created and removed again) and the bookkeeping survive a merge"""
    from cvids_amd import chisel as ch
    N, name = 8, "rpy_neg"
    src_f, dst_f, pose, res = mr.case(N, name, kind)
    dst, src, want, _ = run_case(N, name, kind)
    om = oracle_mod.OracleMap(N, res, True)
    for cid, (s, w, c) in want.items():
        om.put_chunk(cid, s, w, c)
    om.set_integrator(0, 0.12, 1.0, True, 0.05)
    integ = ch.ProjectionIntegrator(ch.ConstantTruncator(0.12), ch.ConstantWeighter(1.0), 0.05, True)
    cam = small_camera(64, 48)
    centre = np.mean(np.array(sorted(want), np.float64), axis=0) * (N * res) + 0.5 * N * res
    cam_pose = np.eye(4, dtype=np.float32)
    cam_pose[:3, 3] = centre - np.array([0.0, 0.0, 0.7])
    yy, xx = np.mgrid[0:48, 0:64]
    depth = (0.7 + 0.1 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.float32)
    color_img = synth.render_color(64, 48, 3)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    dst.counters(reset=True)
    om.integrate_depth_color(depth, cam_pose, intr, color_img, near=cam.near_plane, far=cam.far_plane)
    dst.IntegrateDepthScanColor(integ, depth, cam_pose, cam, color_img, cam_pose, cam)
    oc, gc = om.counters(), dst.counters()
    for k in ("sdf", "col", "col_sat", "probe", "carved", "updated_chunks"):
        assert oc[k] == gc[k], (k, oc[k], gc[k])
    assert oc["sdf"] > 1000
    assert om.num_chunks() == dst.NumChunks()
    compare_fields(om.fields(), dst.fields(), N ** 3, True, what="frame after merge")
    mr.assert_fields_bit_equal(om.fields(), fields_of(dst, N), True, "frame after merge")
    dst.close()
    src.close()


# ---- e. ordering --------------------------------------------------------------------------------------------------------------------------
def test_merge_follows_integration_without_a_wait():
    """two frames are integrated into the source, the merge follows at once, and the source takes a third frame at once after it: the
    same bits as with a synchronise of both maps between all calls"""
    from cvids_amd import chisel as ch
    N, res, W, H = 16, 0.04, 160, 120
    cam = small_camera(W, H)
    frames = list(synth.stream("sphere_room", 3, W, H))
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    pose = mr.poses(res)["rpy_neg"]
    results = []
    for waits in (False, True):
        src, dst = new_map(N, res, False, 4096), new_map(N, res, False, 8192)
        dst.IntegrateDepthScan(integ, frames[2][0], frames[2][1], cam)
        for depth, p in frames[:2]:
            src.IntegrateDepthScan(integ, depth, p, cam)
            if waits:
                src.synchronize()
        if waits:
            dst.synchronize()
        dst.MergeMap(src, pose, stats=False)
        if waits:
            dst.synchronize()
            src.synchronize()
        src.IntegrateDepthScan(integ, frames[2][0], frames[2][1], cam)
        dst.synchronize()
        src.synchronize()
        results.append((fields_of(dst, N), fields_of(src, N)))
        dst.close()
        src.close()
    (d0, s0), (d1, s1) = results
    assert len(d0) > 50 and len(s0) > 50
    mr.assert_fields_bit_equal(d1, d0, False, "dst")
    mr.assert_fields_bit_equal(s1, s0, False, "src")


# ---- f. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_maps_alone():
    from cvids_amd import capi
    N, name = 8, "rpy_neg"
    src_f, dst_f, pose, res = mr.case(N, name, "dense")
    src, dst = new_map(N, res), new_map(N, res, max_chunks=len(dst_f))  # (a fixed pool that holds the destination's own chunks and no more)
    upload(src, src_f)
    upload(dst, dst_f)
    state = lambda: (fields_of(dst, N), fields_of(src, N), dst.counters(), src.counters(), dst.NumChunks(), src.NumChunks(),
                     sorted(map(tuple, dst.GetMeshesToUpdate().tolist())))
    start = state()

    def refused(code, d, s, p):
        p12 = (C.c_float * 12)(*np.asarray(p, np.float32)[:3, :4].reshape(12).tolist())
        st = capi.MergeStats()
        rc = dst.L.chisel_hip_merge_map(d.h if d is not None else None, s.h if s is not None else None, p12, C.byref(st))
        assert capi.STATUS[rc] == code, (capi.STATUS[rc], code)
        now = state()
        mr.assert_fields_bit_equal(start[0], now[0], True, "dst after a refusal")
        mr.assert_fields_bit_equal(start[1], now[1], True, "src after a refusal")
        assert now[2:] == start[2:]

    refused("ERR_INVALID", None, src, pose)
    refused("ERR_INVALID", dst, None, pose)
    refused("ERR_INVALID", dst, dst, pose)
    other_n, other_res = new_map(16, res), new_map(N, float(np.nextafter(np.float32(res), np.float32(1))))
    refused("ERR_INVALID", dst, other_n, pose)
    refused("ERR_INVALID", other_n, src, pose)
    refused("ERR_INVALID", dst, other_res, pose)
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (2, 3)):
            p = pose.copy()
            p[at] = bad
            refused("ERR_INVALID", dst, src, p)
    stretched = pose.copy()
    stretched[:, :3] *= np.float32(1.001)  # R^T R - I = 2e-3
    refused("ERR_INVALID", dst, src, stretched)
    sheared = pose.copy()
    sheared[0, 1] += np.float32(3e-4)
    refused("ERR_INVALID", dst, src, sheared)
    group = new_map(N, res, devices=[0, 0])
    shard = new_map(N, res, n_shards=2, shard_rank=0)
    refused("ERR_UNSUPPORTED", dst, group, pose)
    refused("ERR_UNSUPPORTED", group, src, pose)
    refused("ERR_UNSUPPORTED", dst, shard, pose)
    refused("ERR_UNSUPPORTED", shard, src, pose)
    if capi.load_library().chisel_hip_device_count() >= 2:  # (maps on different devices need two of them)
        elsewhere = new_map(N, res, device_id=1)
        refused("ERR_INVALID", dst, elsewhere, pose)
        elsewhere.close()
    refused("ERR_POOL_FULL", dst, src, pose)  # the merge would create chunks and the pool has no slot left: decided before the first one
    # ... and the same maps merge once the pool has room: the refusals left nothing behind
    roomy = new_map(N, res)
    upload(roomy, dst_f)
    want, wstats, _ = mr.merged(N, name, "dense")
    stats = roomy.MergeMap(src, pose)
    assert stats == {k: wstats[k] for k in stats}
    mr.assert_fields_bit_equal(want, fields_of(roomy, N), True, "after the refusals")
    for m in (src, dst, other_n, other_res, group, shard, roomy):
        m.close()


# ---- g. lifetime --------------------------------------------------------------------------------------------------------------------------
def test_merge_cycles_return_their_memory():
    """tests/test_gpu_lifetime.py's pattern: two maps created, merged and destroyed four times; the free device memory after the first
    cycle against that after the fourth, within half the footprint of one map's voxel pool.  And a second merge into the same
    destination allocates nothing."""
    N, res, max_chunks = 16, mr.RES[16], 1024
    footprint = max_chunks * N ** 3 * (4 + 4 + 4)  # sdf, weight and colour of one fixed pool: 50 MB
    src_f, dst_f, pose, _ = mr.case(N, "rpy_neg", "dense")
    second = []

    def cycle():
        src, dst = new_map(N, res, True, max_chunks, device_id=0), new_map(N, res, True, max_chunks, device_id=0)
        upload(src, src_f)
        upload(dst, dst_f)
        assert dst.MergeMap(src, pose)["voxels_updated"] > 0
        a = free_bytes()
        assert dst.MergeMap(src, pose)["voxels_updated"] > 0
        second.append(a - free_bytes())
        src.close()
        dst.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; drift %d; taken by a second merge: %s" % (readings, footprint, drift, second))
    assert abs(drift) < footprint // 2, (readings, footprint)
    assert all(v <= 0 for v in second), second
