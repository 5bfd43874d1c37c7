"""chisel_hip_distance_field on the GPU against its definition (DESIGN.md 3.11 "Distance field").

The answer is a set of integers, so every comparison is array_equal over every element (same_bits for the float distances): against the
numpy restatement (tests/distance_restated.py: `separable`, and `brute` where the edge values are concerned) run over the map as it
was uploaded or as GetChunkIDs / GetChunk read it back, against chisel_hip_query_points at the voxel centres, and of the device against
itself for windows placed differently.  A stated share only keeps a comparison from passing on an empty case.  The maps are built once
and only read, but where a test changes them."""
import functools
import os
import subprocess

import numpy as np
import pytest

from cvids_amd import synth
from tests import distance_restated as dr
from tests import hash_cases as hc
from tests import test_gpu_render as tgr
from tests import voxel_fields as vf
from tests.common import compare_fields, free_bytes, same_bits, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.0625
BASE = (-2, -1, -3)
B = 3
W, H = tgr.W, tgr.H


def new_map(N, res=RES, color=False, max_chunks=256, **kw):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), res, color, max_chunks=max_chunks, **kw)


@functools.lru_cache(maxsize=None)
def sparse_field(N):
    return dr.sparse(N, B, 7, RES, base=BASE)


@functools.lru_cache(maxsize=None)
def sparse_map(N):
    """the hand-built sparse map of chunk edge N (only ever read)"""
    gm = new_map(N)
    upload(gm, sparse_field(N))
    assert gm.NumChunks() == B ** 3 - 2
    return gm


@functools.lru_cache(maxsize=None)
def sparse_states(N, R, offset):
    origin, dims = dr.block_window(N, B, BASE)
    st = dr.states(sparse_field(N), N, origin, dims, R, offset)
    st.setflags(write=False)
    return st


def check_window(gm, fields, N, origin, dims, R, flag, offset, ref=dr.separable, st=None, what=""):
    """state, dist2 and distance of one call against the restatement over `fields` -> the call's answer"""
    got = gm.DistanceField(origin, dims, R, flag, offset, distance=True)
    if st is None:
        st = dr.states(fields, N, origin, dims, R, offset)
    want = ref(st, R, flag)
    what = "%s N %d origin %s dims %s R %d flag %d offset %r" % (what, N, origin, dims, R, flag, offset)
    shape = (dims[2], dims[1], dims[0])
    assert got["state"].shape == shape and got["state"].dtype == np.uint8 and got["dist2"].shape == shape and got["dist2"].dtype == np.int32
    assert np.array_equal(got["state"], dr.window_of(st, R)), "%s: state differs at %d places" % (what, int((got["state"] != dr.window_of(st, R)).sum()))
    assert np.array_equal(got["dist2"], want), "%s: dist2 differs at %d of %d places" % (what, int((got["dist2"] != want).sum()), want.size)
    same_bits(got["distance"], dr.distance(want, gm.voxel_resolution), what + ": distance")
    return got


# ---- 1. hand-built sparse maps, R 1 to 13 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 13])
@pytest.mark.parametrize("N", [8, 16, 32])
def test_sparse_maps_against_the_restatement(N, R):
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B, BASE)
    for offset in (0.0, RES / 2, -RES / 2):
        for flag in (False, True):
            got = check_window(gm, None, N, origin, dims, R, flag, offset, st=sparse_states(N, R, offset))
            if not flag and offset == 0.0:  # reach, on the device's own output
                r = dr.check_reach(got["state"], got["dist2"], R)
                print("N %d R %d: %s" % (N, R, {k: (len(v) if k == "values" else round(v, 4)) for k, v in r.items()}))
            if flag:
                assert np.array_equal(got["dist2"] == 0, got["state"] != 1)


# ---- 2. the largest radius -----------------------------------------------------------------------------------------------------------
def test_radius_64():
    N, R = 8, 64
    origin, dims = dr.block_window(N, B, BASE)
    got = check_window(sparse_map(N), sparse_field(N), N, origin, dims, R, False, 0.0)
    vals = np.unique(got["dist2"])
    print("R = 64: %d distinct values, largest %d, without an obstacle %d" % (len(vals), int(vals.max()), int((got["dist2"] < 0).sum())))
    assert len(vals) > 200 and vals.max() > 13 * 13


# ---- 3. edge values ------------------------------------------------------------------------------------------------------------------
def test_edge_values_against_the_definition():
    """+-0.0, denormals and the weights around GetSDF's 1e-12 (voxel_fields.thresholds), surface offsets 0 and -0.0, against `brute`"""
    N, R, base = 8, 2, (-1, -1, -1)
    field = vf.thresholds(N, 2, 11, RES, base=base)
    gm = new_map(N)
    upload(gm, field)
    origin, dims = dr.block_window(N, 2, base, (3, 3, 3), (3, 3, 3))
    sdf, wgt, resident = dr.voxel_box(field, N, origin, dims)
    observed = resident & (wgt.astype(np.float64) > 1e-12)
    for offset in (0.0, -0.0):
        for flag in (False, True):
            got = check_window(gm, field, N, origin, dims, R, flag, offset, ref=dr.brute)
        state = got["state"]
        neg_zero = observed & (sdf == 0) & np.signbit(sdf)
        neg_denormal = observed & (sdf < 0) & (np.abs(sdf) < np.finfo(np.float32).tiny)
        assert neg_zero.sum() > 50 and (state[neg_zero] == 1).all()          # -0.0 < 0 is false
        assert neg_denormal.sum() > 50 and (state[neg_denormal] == 2).all()  # a negative denormal is occupied
        edge, edge_next = resident & (wgt == vf.W_EDGE), resident & (wgt == vf.W_EDGE_NEXT)
        assert edge.sum() > 10 and (state[edge] == 0).all() and edge_next.sum() > 10 and (state[edge_next] != 0).all()
    gm.close()


# ---- 4. window shapes and placements -------------------------------------------------------------------------------------------------
def test_window_shapes_and_placements():
    """seven shapes (the tails of a wave, of a bit word and of a tile along each axis) at three origins -- inside a chunk, on a chunk
    face, 2 R outside the block --: each equals the same cells of one large window, which equals the restatement"""
    N, R = 8, 5
    gm, field = sparse_map(N), sparse_field(N)
    lo, hi = np.array(BASE) * N, (np.array(BASE) + B) * N
    shapes = [(1, 1, 1), (63, 1, 1), (64, 2, 1), (65, 3, 2), (257, 2, 2), (2, 65, 3), (3, 2, 65)]
    places = [lo + (3, 2, 5), lo + (N, N, 2 * N), hi + 2 * R]
    big_origin = tuple(int(v) for v in lo - 12)
    big_dims = tuple(int(v) for v in hi + 2 * R + (257, 65, 65) - (lo - 12))
    for flag in (False, True):
        big = check_window(gm, field, N, big_origin, big_dims, R, flag, 0.0, what="large")
        for dims in shapes:
            for place in places:
                origin = tuple(int(v) for v in place)
                got = gm.DistanceField(origin, dims, R, flag, 0.0, distance=True)
                o = [origin[a] - big_origin[a] for a in range(3)]
                cells = (slice(o[2], o[2] + dims[2]), slice(o[1], o[1] + dims[1]), slice(o[0], o[0] + dims[0]))
                for key in ("state", "dist2"):
                    assert np.array_equal(got[key], big[key][cells]), (flag, dims, origin, key)
                same_bits(got["distance"], np.ascontiguousarray(big["distance"][cells]), "%s at %s" % (dims, origin))
        assert (big["dist2"] > 0).any() and (flag or (big["dist2"] < 0).any())


# ---- 5. against an existing entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 16])
def test_state_equals_query_points_at_the_voxel_centres(N):
    """found bit 0 and sdf < offset of chisel_hip_query_points at ((float)g + 0.5f) * res: with res = 1 / 16 the centres are exact"""
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B, BASE)
    q = gm.QueryPoints(dr.centres(origin, dims, RES))
    found = (q["found"] & 1).astype(bool)
    for offset in (0.0, RES / 2):
        with np.errstate(invalid="ignore"):
            want = np.where(found, np.where(q["sdf"] < np.float32(offset), 2, 1), 0).astype(np.uint8).reshape(dims[2], dims[1], dims[0])
        got = gm.DistanceField(origin, dims, 1, False, offset, dist2=False)
        assert got["dist2"] is None and got["distance"] is None
        assert np.array_equal(got["state"], want), int((got["state"] != want).sum())
        assert all((want == k).mean() >= 0.0005 for k in range(3))


# ---- 6. an integrated map --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 2], ids=["sphere_room-16", "box_room-8-colour"])
def test_an_integrated_map(case):
    """A 48 x 40 x 24 window, R = 8, against the restatement over gm.fields(); again after GarbageCollect of a third of the chunks, and
    after Reset.  The window is centred on the surface point the central pixel of frame 0 sees: a box of that size centred on the camera
    itself lies in free space that holds no chunk in either scene (every voxel unknown, no obstacle), which says nothing."""
    scene, N, res, trunc, n_frames, carving, color, _ = tgr.MAPS[case]
    gm = tgr.gpu_map(scene, N, res, trunc, n_frames, carving, color)
    depth0, pose0 = next(iter(synth.stream(scene, 1, W, H)))
    fx, fy, cx, cy = synth.intrinsics(W, H)
    z = float(depth0[H // 2, W // 2])
    p0 = np.asarray(pose0, np.float64)
    hit = p0[:3, :3] @ np.array([(W // 2 + 0.5 - cx) / fx * z, (H // 2 + 0.5 - cy) / fy * z, z]) + p0[:3, 3]
    dims, R = (48, 40, 24), 8
    origin = tuple(int(np.floor(hit[a] / res)) - dims[a] // 2 for a in range(3))
    for flag in (False, True):
        got = check_window(gm, gm.fields(), N, origin, dims, R, flag, 0.0, what=scene)
    first = gm.DistanceField(origin, dims, R)
    assert (first["state"] == 2).any() and (first["dist2"] > 0).any()
    ids = gm.GetChunkIDs()
    ids = ids[np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0]))]
    gm.GarbageCollect(ids[::3])
    fields = gm.fields()
    assert len(fields) == len(ids) - len(ids[::3])
    for flag in (False, True):
        got = check_window(gm, fields, N, origin, dims, R, flag, 0.0, what=scene + " after GarbageCollect")
    assert (got["state"] != first["state"]).any() and (got["state"] == 2).any()
    gm.Reset()
    empty = gm.DistanceField(origin, dims, R, False, 0.0, distance=True)
    assert not empty["state"].any() and (empty["dist2"] == -1).all() and np.isposinf(empty["distance"]).all()
    empty = gm.DistanceField(origin, dims, R, True, 0.0, distance=True)
    assert not empty["state"].any() and (empty["dist2"] == 0).all() and (empty["distance"] == 0).all()
    gm.close()


# ---- 7. one crowded table ------------------------------------------------------------------------------------------------------------
def test_on_a_table_without_an_empty_bucket():
    """one far id per bucket uploaded and collected (tests/hash_cases.py: saturation_rounds): every bucket a tombstone, so that the
    look-up of an absent chunk inside the box of created ids is ended by the loop's bound alone; then the sparse map into it"""
    N, R = 8, 5
    gm = new_map(N, max_chunks=512)
    cap = gm.hash_table()["capacity"]
    for ids in hc.saturation_rounds(cap, 400):
        for k, cid in enumerate(ids):
            s, w, _ = hc.blocker_voxels(k, N ** 3)
            gm.AddChunk(cid, s, w)
        gm.GarbageCollect(ids)
    upload(gm, sparse_field(N))
    t = gm.hash_table()
    assert hc.n_empty(t) == 0 and gm.NumChunks() == B ** 3 - 2
    hc.check_invariants(t, "saturated")
    origin, dims = dr.block_window(N, B, BASE)
    for flag in (False, True):
        check_window(gm, None, N, origin, dims, R, flag, 0.0, st=sparse_states(N, R, 0.0), what="crowded")
    gm.close()


# ---- 8. plumbing -----------------------------------------------------------------------------------------------------------------------
def device_outputs(dims, dev, names=("state", "dist2", "distance")):
    import torch
    shape = (dims[2], dims[1], dims[0])
    kinds = {"state": torch.uint8, "dist2": torch.int32, "distance": torch.float32}
    return {k: torch.full(shape, 77, dtype=kinds[k], device=dev) for k in names}


def equal_answers(got, want, what):
    for key in got:
        if key == "distance":
            same_bits(got[key], want[key], what + ": distance")
        else:
            assert np.array_equal(got[key], want[key]), "%s: %s differs at %d places" % (what, key, int((got[key] != want[key]).sum()))


def test_host_and_device_outputs_are_equal():
    import torch
    N, R = 16, 5
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B, BASE)
    dev = torch.device("cuda:0")
    out = device_outputs(dims, dev)
    torch.cuda.synchronize()
    assert gm.DistanceField(origin, dims, R, False, RES / 2, out=out) is out
    gm.synchronize()
    host = gm.DistanceField(origin, dims, R, False, RES / 2, distance=True)
    equal_answers({k: v.cpu().numpy() for k, v in out.items()}, host, "device outputs")
    for name in ("state", "dist2", "distance"):  # each output alone, on the device and on the host
        alone = device_outputs(dims, dev, (name,))
        torch.cuda.synchronize()
        gm.DistanceField(origin, dims, R, False, RES / 2, out=alone)
        gm.synchronize()
        equal_answers({name: alone[name].cpu().numpy()}, host, name + " alone on the device")
        only = gm.DistanceField(origin, dims, R, False, RES / 2, **{k: k == name for k in ("state", "dist2", "distance")})
        assert [k for k, v in only.items() if v is not None] == [name]
        equal_answers({name: only[name]}, host, name + " alone on the host")
    assert (host["dist2"] > 0).any() and (host["dist2"] < 0).any()


def test_the_call_only_reads_the_map():
    """two maps fed the same frames, one of them asked for distance fields in between (host and device outputs): voxels, counters,
    meshesToUpdate and the meshes of a later UpdateMeshes are identical"""
    import torch
    args = ("sphere_room", 16, 0.03, ("inverse", 2.0), 6, True, True)
    a, b = tgr.gpu_map(*args), tgr.gpu_map(*args)
    dev = torch.device("cuda:0")
    dims = (48, 40, 24)
    out = device_outputs(dims, dev)
    torch.cuda.synchronize()
    for origin in ((-24, -20, 72), (-30, -10, 66)):
        for flag in (False, True):
            a.DistanceField(origin, dims, 8, flag, 0.0, distance=True)
            a.DistanceField(origin, dims, 8, flag, 0.01, out=out)
    a.synchronize()
    assert (out["state"] == 2).any()
    assert a.counters() == b.counters()
    assert sorted(map(tuple, a.GetMeshesToUpdate().tolist())) == sorted(map(tuple, b.GetMeshesToUpdate().tolist()))
    assert a.NumChunks() == b.NumChunks()
    compare_fields(b.fields(), a.fields(), a.V, True)
    a.UpdateMeshes()
    b.UpdateMeshes()
    a.DistanceField((-24, -20, 72), dims, 8)
    ma, mb = tgr.mesh_state(a), tgr.mesh_state(b)
    assert set(ma) == set(mb) and len(ma) > 10
    for cid in ma:
        for key in ("vertices", "normals", "colors", "grids"):
            assert ma[cid][key].tobytes() == mb[cid][key].tobytes(), (cid, key)
    assert a.GetMeshesToUpdate().tolist() == b.GetMeshesToUpdate().tolist()
    a.close()
    b.close()


def test_between_two_launch_sets_of_a_pipelined_stream():
    """device frames, nothing waited for: IntegrateBatch, DistanceField into device tensors, IntegrateBatch.  The answer is that of
    the map after the first batch, and the final map is the one of the same stream without the call."""
    import torch
    N, res, trunc = 16, 0.03, ("inverse", 2.0)
    cam, integ = tgr.camera(), tgr.integrator(trunc)
    frames = list(synth.stream("sphere_room", 8, W, H))
    dev = torch.device("cuda:0")
    d_dev = [torch.from_numpy(d).to(dev) for d, _ in frames]
    origin, dims, R = (-24, -20, 72), (48, 40, 24), 8
    out = device_outputs(dims, dev)
    torch.cuda.synchronize()
    a, b, c = (new_map(N, res, max_chunks=8192) for _ in range(3))
    a.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    a.DistanceField(origin, dims, R, out=out)
    a.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4, 8)])
    b.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    b.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4, 8)])
    c.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    a.synchronize()
    mid = {k: v.cpu().numpy() for k, v in out.items()}
    equal_answers(mid, c.DistanceField(origin, dims, R, distance=True), "between the launch sets")
    st = dr.states(c.fields(), N, origin, dims, R, 0.0)
    assert np.array_equal(mid["dist2"], dr.separable(st, R)) and (mid["state"] == 2).any()
    after = a.DistanceField(origin, dims, R)  # (eight frames: other voxels observed than after four)
    assert (after["state"] != mid["state"]).any()
    assert a.NumChunks() == b.NumChunks()
    compare_fields(b.fields(), a.fields(), a.V, False)
    assert a.counters() == b.counters()
    for m in (a, b, c):
        m.close()


def test_scratch_is_kept_grown_and_freed_with_the_map():
    """a second call of the same size allocates nothing, a larger window grows the scratch, a smaller one fits what is there, and the
    memory is back when the map is gone (cycles, as tests/test_gpu_lifetime.py measures a footprint)"""
    import torch
    N, R = 8, 8
    dev = torch.device("cuda:0")
    small, large = (40, 40, 40), (256, 200, 120)
    footprint = (large[0] + 2 * R) * (large[1] + 2 * R) * (large[2] + 2 * R) * 4  # roughly: two 16-bit arrays over the widened window
    o_small, o_large = device_outputs(small, dev), device_outputs(large, dev)
    second, grown, fits = [], [], []

    def cycle():
        gm = new_map(N)
        upload(gm, sparse_field(N))
        gm.DistanceField((-20, -12, -28), small, R, out=o_small)
        a = free_bytes()
        gm.DistanceField((-21, -13, -27), small, R, True, out=o_small)
        second.append(a - free_bytes())
        gm.DistanceField((-40, -30, -50), large, R, out=o_large)
        b = free_bytes()
        grown.append(a - b)
        gm.DistanceField((-20, -12, -28), small, R, out=o_small)
        gm.DistanceField((-40, -30, -50), large, R, out=o_large)
        fits.append(b - free_bytes())
        gm.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; drift %d; second call %s; grown by %s; later calls %s" % (readings, footprint, drift, second, grown, fits))
    assert abs(drift) < footprint // 2, (readings, footprint)
    assert all(v <= 0 for v in second) and all(v <= 0 for v in fits), (second, fits)
    assert all(v >= footprint // 2 for v in grown), (grown, footprint)


def test_refusals():
    """every refusal with its code; nothing is touched, and the map answers afterwards"""
    import ctypes as C
    from cvids_amd import capi
    N = 8
    gm = sparse_map(N)
    L = capi.load_library()
    origin, dims = dr.block_window(N, B, BASE)
    before = gm.DistanceField(origin, dims, 5, distance=True)
    state = np.full(8, 77, np.uint8)
    d2 = np.full(8, 77, np.int32)

    def refused(code, word, origin=(0, 0, 0), dims=(2, 2, 2), R=1, offset=0.0, window=True, outputs=True):
        w = capi.DistanceWindow((C.c_int * 3)(*origin), (C.c_int * 3)(*dims), R, 0, offset)
        rc = L.chisel_hip_distance_field(gm.h, C.byref(w) if window else None, state.ctypes.data if outputs else None, d2.ctypes.data if outputs else None, None, 0)
        msg = L.chisel_hip_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert (state == 77).all() and (d2 == 77).all()

    refused(1, "null window", window=False)
    refused(1, "output", outputs=False)
    for a in range(3):
        for bad in (0, -1):
            refused(1, "dimension", dims=tuple(bad if k == a else 2 for k in range(3)))
    for bad in (0, -3, 65, 1 << 20):
        refused(1, "radius", R=bad)
    refused(1, "NaN", offset=float("nan"))
    lim = 1 << 30
    for a in range(3):
        refused(1, "2^30", origin=tuple(lim - 1 if k == a else 0 for k in range(3)))
        refused(1, "2^30", origin=tuple(-lim if k == a else 0 for k in range(3)))
    refused(5, "more than 2^30 voxels", origin=(-500, -500, -500), dims=(1008, 1008, 1009), R=8)
    refused(5, "more than 2^30 voxels", dims=(lim - 200, 1, 1), R=64)
    with pytest.raises(capi.ChiselHipError) as e:  # ... and through the Python method
        gm.DistanceField(origin, dims, 65)
    assert e.value.code == 1 and "radius" in str(e.value)
    with pytest.raises(capi.ChiselHipError) as e:
        gm.DistanceField(origin, (0, 4, 4), 5)
    assert e.value.code == 1
    with pytest.raises(capi.ChiselHipError) as e:
        gm.DistanceField(origin, (1 << 11, 1 << 11, 1 << 11), 5)
    assert e.value.code == 5
    equal_answers(gm.DistanceField(origin, dims, 5, distance=True), before, "after the refusals")
    # the far corner of the accepted coordinates: no chunk id there is one the look-up accepts, every voxel is unknown
    far = gm.DistanceField((lim - 9, lim - 9, -lim + 3), (6, 6, 6), 3, distance=True)
    assert not far["state"].any() and (far["dist2"] == -1).all()
    far = gm.DistanceField((lim - 9, lim - 9, -lim + 3), (6, 6, 6), 3, True)
    assert (far["dist2"] == 0).all()
    from cvids_amd import chisel as ch
    group = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, devices=[0, 0])
    with pytest.raises(capi.ChiselHipError) as e:
        group.DistanceField((0, 0, 0), (4, 4, 4), 2)
    assert e.value.code == 5 and "group" in str(e.value)
    shard = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, n_shards=2, shard_rank=0)
    with pytest.raises(capi.ChiselHipError) as e:
        shard.DistanceField((0, 0, 0), (4, 4, 4), 2)
    assert e.value.code == 5 and "shard" in str(e.value)
    group.close()
    shard.close()


def test_distance_window_of_a_metric_box():
    gm = sparse_map(8)
    origin, dims = gm.DistanceWindow((-1.0, -0.5, -1.5), (0.5, 1.0, 0.0))
    assert origin == (-16, -8, -24) and dims == (24, 24, 24)  # centres (g + 0.5) / 16 in [lo, hi]
    origin, dims = gm.DistanceWindow((0.03125, 0.0, 0.04), (0.03125, 0.0625, 0.05))
    assert origin == (0, 0, 1) and dims == (1, 1, 0)  # a centre on the box's face is inside; no centre: an empty axis
    got = gm.DistanceField(*gm.DistanceWindow((-1.0, -0.5, -1.5), (0.5, 1.0, 0.0)), 3)
    assert got["state"].shape == (24, 24, 24)


def test_the_facade_program_answers_what_python_answers():
    """cvids_amd/open_chisel/tests/facade_distance.cpp: chisel::Chisel::DistanceField on three frames of a wall; its checksums are
    those of the Python host path on the same frames"""
    from cvids_amd import chisel as ch
    tdir = os.path.join(ROOT, "cvids_amd", "open_chisel", "tests")
    subprocess.check_call(["make", "-C", tdir, "distance"])
    run = subprocess.run([os.path.join(tdir, "facade_distance")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "facade_distance ok" in run.stdout, run.stdout + run.stderr
    Wf, Hf, N, res = 64, 48, 8, 0.05
    gm = new_map(N, res)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    cam = ch.PinholeCamera(52.5, 52.5, 31.5, 23.5, Wf, Hf, 0.05, 5.0)
    pose = np.eye(4, dtype=np.float32)
    for k in range(3):
        gm.IntegrateDepthScan(integ, np.full((Hf, Wf), np.float32(1.5) + np.float32(0.1) * np.float32(k), np.float32), pose, cam)
    got = gm.DistanceField((-12, -10, 22), (24, 20, 18), 6, False, 0.0, distance=True)

    def fnv1a(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
            h = ((h ^ byte) * 1099511628211) & ((1 << 64) - 1)
        return h

    line = [l for l in run.stdout.splitlines() if l.startswith("checksum")][0].split()
    assert line[1::2] == ["state", "dist2", "distance"]
    assert [int(v, 16) for v in line[2::2]] == [fnv1a(got[k]) for k in ("state", "dist2", "distance")], run.stdout
    assert (got["state"] == 2).any() and (got["state"] == 1).any() and (got["state"] == 0).any()
    gm.close()
