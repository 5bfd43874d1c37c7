"""chisel_hip_coarse_mesh on the GPU: a marching-cubes mesh over every s-th voxel of the selected chunks.

The reference of every comparison is the restatement (tests/coarse_mesh_restated.py: direct indexing of the uploaded fields and the
oracle's MeshCube), which tests/test_coarse_mesh_restated.py pins to the oracle's own GenerateMesh at stride 1; for the shading
chisel_hip_shade_vertices on the call's own vertices; for an integrated scene the oracle's meshes.  Everything is compared bit for bit.
What the fields reach (all 256 configurations, cubes skipped for an absent neighbour and for a weight, corners in 2, 4 and 8 chunks)
is asserted on these very fields by the CPU test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cvids_amd import capi
from tests import coarse_mesh_restated as cr
from tests import hash_cases as hc
from tests import voxel_fields as vf
from tests.common import fields_of, free_bytes, make_frames, small_camera, upload
from tests.test_coarse_mesh_restated import B, RES, SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = (-1000, 900, -37)  # a negative, far base
CASES = [(8, 1), (8, 2), (8, 4), (8, 8), (16, 1), (16, 2), (16, 4), (16, 16), (32, 2), (32, 8), (32, 32), (32, 1)]


def new_map(N, color=True, max_chunks=64, **kw):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), RES[N], color, max_chunks=max_chunks, **kw)


class Built:
    """the fields of this module, their maps and their restatements, each made once and only read afterwards"""

    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        self.fields, self.maps, self.restated = {}, {}, {}

    def field(self, family, N, base=(0, 0, 0)):
        key = (family, N, tuple(base))
        if key not in self.fields:
            self.fields[key] = getattr(vf, family)(N, B, SEED, res=RES[N], base=base)
        return self.fields[key]

    def map(self, family, N, base=(0, 0, 0)):
        key = (family, N, tuple(base))
        if key not in self.maps:
            gm = new_map(N)
            upload(gm, self.field(family, N, base))
            self.maps[key] = gm
        return self.maps[key]

    def want(self, family, N, s, base=(0, 0, 0), selection=None):
        key = (family, N, s, tuple(base), None if selection is None else tuple(map(tuple, selection)))
        if key not in self.restated:
            self.restated[key] = cr.coarse_mesh(self.oracle_mod, self.field(family, N, base), N, RES[N], s, selection)
        return self.restated[key]

    def release(self):
        for gm in self.maps.values():
            gm.close()
        self.maps.clear()


@pytest.fixture(scope="module")
def built(oracle_mod):
    b = Built(oracle_mod)
    yield b
    b.release()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_mesh(got, want, what, normals=True):
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    assert np.array_equal(got["ids"], want["ids"]), what
    assert np.array_equal(got["table"], want["table"]), what
    keys = ("vertices", "normals") if normals else ("vertices",)
    for key in keys:
        g = got[key].cpu().numpy()[:len(want[key])] if hasattr(got[key], "is_cuda") else got[key]
        assert g.shape == want[key].shape, (what, key, g.shape, want[key].shape)
        assert np.array_equal(bits(g), bits(want[key])), "%s: %d of %d %s floats differ in their bits" % (
            what, int((bits(g) != bits(want[key])).sum()), g.size, key)


def refused(call, code, word=None):
    with pytest.raises(capi.ChiselHipError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    return str(e.value)


# ---- bit for bit against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [(0, 0, 0), FAR], ids=("origin", "far"))
@pytest.mark.parametrize("N,s", CASES)
@pytest.mark.parametrize("family", ["dense", "thresholds"])
def test_bit_for_bit_against_the_restatement(built, family, N, s, base):
    """vertices, face normals, table, ids and totals; at N = 32, s = 1 one chunk with its seven + neighbours (a list of one id), every
    other case the whole block; s = N is one cube per chunk, its corners in eight chunks"""
    gm = built.map(family, N, base)
    selection = [tuple(int(v) for v in base)] if (N, s) == (32, 1) else None
    want = built.want(family, N, s, base, selection)
    got = gm.CoarseMesh(s, ids=selection, colors=False, stages=0)
    assert_mesh(got, want, "%s N %d s %d base %s" % (family, N, s, base))
    if family == "dense":
        assert want["totals"]["vertices"] > 0 and want["totals"]["cubes_meshed"] == ((B * N // s - 1) ** 3 if selection is None else N ** 3)
    if s == N:
        assert want["totals"]["cubes_meshed"] <= 1


# ---- a selection beyond one batch of the scan and beyond the grid ---------------------------------------------------------------------------
BIG = 13  # 13^3 = 2197 chunks of 8^3 voxels: 8 x 256 + 149 for the scan's carry, 149 more than the grid of 2048 workgroups


@pytest.fixture(scope="module")
def big():
    """-> (field, its sorted ids, the map): made once, only read"""
    N = 8
    field = vf.dense(N, BIG, SEED, res=RES[N])
    ids = sorted(field)
    gm = new_map(N, max_chunks=4096)
    gm.ScatterChunks(ids, *(np.stack([field[c][k] for c in ids]) for k in range(3)))
    yield field, ids, gm
    gm.close()


@pytest.mark.parametrize("s", [4, 8])
def test_every_chunk_of_a_large_map(big, oracle_mod, s):
    """the scan carries its sum over eight full batches of chunks, and every chunk kernel strides over its grid; at s = 8 the empty
    chunks among the others are skipped inside the emit kernel's strided loop"""
    field, ids, gm = big
    want = cr.coarse_mesh(oracle_mod, field, 8, RES[8], s)
    assert want["totals"]["chunks"] == BIG ** 3 == 2197 > 8 * 256 and want["totals"]["chunks"] > 2048
    assert (want["totals"]["chunks_nonempty"] == 2197) if s == 4 else (0 < want["totals"]["chunks_nonempty"] < 2197)
    assert_mesh(gm.CoarseMesh(s, colors=False, stages=0), want, "13^3 chunks, s %d" % s)
    assert gm.CoarseMeshSize(s) == want["totals"]


def test_a_long_scrambled_list_with_repetitions(big, oracle_mod):
    field, ids, gm = big
    s = 4
    pick = [ids[i] for i in np.random.default_rng(SEED).integers(0, len(ids), 2100)]
    assert len(set(pick)) < len(pick) and pick != sorted(pick)
    assert_mesh(gm.CoarseMesh(s, ids=pick, colors=False, stages=0), cr.coarse_mesh(oracle_mod, field, 8, RES[8], s, pick), "a list of 2100")
    # a non-resident id in the last batch of the scan
    pick[2099] = (BIG + 7, BIG + 7, BIG + 7)
    with pytest.raises(KeyError) as e:
        gm.CoarseMesh(s, ids=pick, colors=False, stages=0)
    assert "id 2099 " in str(e.value)
    with pytest.raises(KeyError) as e:
        gm.CoarseMeshSize(s, ids=pick)
    assert "id 2099 " in str(e.value)


# ---- shading ----------------------------------------------------------------------------------------------------------------------------
def shade(gm, vertices, face_normals, stages):
    """chisel_hip_shade_vertices on the call's own vertices and face normals; colours start as zeros"""
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    v = np.ascontiguousarray(vertices, np.float32)
    n = np.ascontiguousarray(face_normals, np.float32).copy()
    c = np.zeros_like(v)
    capi.check(gm.L.chisel_hip_shade_vertices(gm.h, fp(v), len(v), fp(n), fp(c), stages))
    return n, c


@pytest.mark.parametrize("N,s", [(8, 1), (16, 2), (32, 4)])
def test_shading_is_shade_vertices(built, N, s):
    gm = built.map("thresholds", N)
    plain = gm.CoarseMesh(s, colors=False, stages=0)
    assert len(plain["vertices"]) > 100
    changed = 0
    for stages in (1, 2, 3):
        got = gm.CoarseMesh(s, normals=True, colors=True, stages=stages)
        n, c = shade(gm, plain["vertices"], plain["normals"], stages)
        assert np.array_equal(bits(got["vertices"]), bits(plain["vertices"]))
        assert np.array_equal(bits(got["normals"]), bits(n)), stages
        assert np.array_equal(bits(got["colors"]), bits(c)), stages
        if stages & 1:
            changed += int((bits(n) != bits(plain["normals"])).any(1).sum())
        if stages & 2:
            assert (c != 0).any()
        else:
            assert not got["colors"].any()
    assert changed > 0  # (a gradient look-up succeeded somewhere: the stage is not a no-op)


def test_a_map_without_colour_refuses_colours():
    N = 8
    gm = new_map(N, color=False)
    upload(gm, vf.dense(N, B, SEED, res=RES[N]))
    refused(lambda: gm.CoarseMesh(2, colors=True, stages=0), 1, "without colour")
    refused(lambda: gm.CoarseMesh(2, colors=False, stages=2), 1, "without colour")
    assert gm.CoarseMesh(2, colors=False, stages=1)["totals"]["vertices"] > 0
    gm.close()


# ---- stride 1 against the oracle ----------------------------------------------------------------------------------------------------------
def test_stride_1_is_the_oracles_mesh_of_an_integrated_scene(oracle_mod):
    from tests.test_gpu_parity import _mk
    N, res = 8, 0.05
    om, gm, integ = _mk(oracle_mod, N, res, False)
    cam = small_camera(96, 72)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    for d, p in make_frames("sphere_room", 3, 96, 72):
        om.integrate_depth(d, p, intr, cam.near_plane, cam.far_plane)
        gm.IntegrateDepthScan(integ, d, p, cam)
    om.update_meshes(force=True)
    got = gm.CoarseMesh(1, stages=0)
    meshed = {tuple(c): om.get_mesh(tuple(c)) for c in om.mesh_ids().tolist()}
    total = 0
    for (first, count), cid in zip(got["table"].tolist(), map(tuple, got["ids"].tolist())):
        ref = meshed.get(cid)
        want = ref["vertices"] if ref is not None else np.zeros((0, 3), np.float32)
        assert count == len(want), cid
        assert cr.triangles_as_bits(got["vertices"][first:first + count]) == cr.triangles_as_bits(want), cid
        total += count
    assert total == got["totals"]["vertices"] == sum(len(m["vertices"]) for m in meshed.values()) > 1000
    assert set(meshed) <= set(map(tuple, got["ids"].tolist()))
    gm.close()


# ---- selections ---------------------------------------------------------------------------------------------------------------------------
def test_selections(built, oracle_mod):
    N, s = 8, 2
    field = dict(built.field("thresholds", N))
    hollow = (5, 5, 5)  # a chunk whose mesh is empty: nothing observed
    field[hollow] = (np.zeros(N ** 3, np.float32), np.zeros(N ** 3, np.float32), np.zeros((N ** 3, 4), np.uint8))
    gm = new_map(N)
    upload(gm, field)
    mesh = lambda sel: cr.coarse_mesh(oracle_mod, field, N, RES[N], s, sel)
    # all, in list_chunks' order
    got = gm.CoarseMesh(s, colors=False, stages=0)
    assert got["ids"].tolist() == gm.GetChunkIDs().tolist() == [list(c) for c in sorted(field)]
    assert_mesh(got, mesh(None), "all")
    row = got["table"][got["ids"].tolist().index(list(hollow))]
    assert row[1] == 0 and row[0] == got["totals"]["vertices"]  # (the last chunk: its first is the total)
    assert gm.CoarseMeshSize(s) == got["totals"]
    # a box
    box = ((0, 0, 0), (1, 0, 1))
    got = gm.CoarseMesh(s, box=box, colors=False, stages=0)
    assert len(got["ids"]) == 4
    assert_mesh(got, mesh(cr.selection_all(field, box)), "box")
    assert gm.CoarseMeshSize(s, box=((7, 7, 7), (9, 9, 9))) == {"chunks": 0, "chunks_nonempty": 0, "cubes_meshed": 0, "vertices": 0}
    # a list in the caller's order, with a duplicate and the hollow chunk
    pick = [(1, 1, 0), (0, 0, 0), hollow, (1, 1, 0), (0, 1, 1)]
    got = gm.CoarseMesh(s, ids=pick, colors=False, stages=0)
    assert_mesh(got, mesh(pick), "list")
    assert got["table"][2].tolist() == [got["table"][3][0], 0]
    assert gm.CoarseMeshSize(s, ids=pick) == got["totals"]
    # a listed id that is not resident
    with pytest.raises(KeyError) as e:
        gm.CoarseMesh(s, ids=[(0, 0, 0), (1, 1, 1), (3, 3, 3), (9, 9, 9)], colors=False, stages=0)
    assert "id 2 " in str(e.value)
    with pytest.raises(KeyError):
        gm.CoarseMeshSize(s, ids=[(9, 9, 9)])
    gm.close()


def test_an_empty_map():
    gm = new_map(8)
    zero = {"chunks": 0, "chunks_nonempty": 0, "cubes_meshed": 0, "vertices": 0}
    assert gm.CoarseMeshSize(2) == zero
    got = gm.CoarseMesh(2, stages=0)
    assert got["totals"] == zero and got["vertices"].shape == (0, 3) and got["table"].shape == (0, 2) and got["ids"].shape == (0, 3)
    gm.close()


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------
def raw_call(gm, req, cap, v, n, c, on_device=0, table=None, ids=None):
    """-> (status, totals)"""
    t = capi.CoarseTotals(-1, -1, -1, -1)
    ptr = lambda a: (a if isinstance(a, int) else a.ctypes.data) if a is not None else None
    rc = gm.L.chisel_hip_coarse_mesh(gm.h, C.byref(req) if req is not None else None, cap, ptr(v), ptr(n), ptr(c), on_device,
                                     table.ctypes.data_as(C.POINTER(C.c_int64)) if table is not None else None,
                                     ids.ctypes.data_as(C.POINTER(C.c_int)) if ids is not None else None, C.byref(t))
    return rc, {name: int(getattr(t, name)) for name, _ in capi.CoarseTotals._fields_}


def test_capacity(built):
    import torch
    N, s = 16, 2
    gm = built.map("dense", N)
    want = built.want("dense", N, s)
    V, n = want["totals"]["vertices"], want["totals"]["chunks"]
    req = capi.CoarseRequest()
    req.stride, req.stages = s, 0
    rc, size = raw_call(gm, req, 0, None, None, None)
    assert rc == 0 and size == want["totals"]
    # one short: refused, totals filled, nothing written
    v, nn = np.full((V, 3), -7.25, np.float32), np.full((V, 3), -7.25, np.float32)
    table, ids = np.full((n, 2), -9, np.int64), np.full((n, 3), -9, np.int32)
    rc, totals = raw_call(gm, req, V - 1, v, nn, None, table=table, ids=ids)
    assert rc == 1 and "capacity" in gm.L.chisel_hip_last_error().decode() and totals == size
    assert (v == -7.25).all() and (nn == -7.25).all() and (table == -9).all() and (ids == -9).all()
    # exact
    rc, totals = raw_call(gm, req, V, v, nn, None, table=table, ids=ids)
    assert rc == 0 and totals == size
    assert_mesh({"vertices": v, "normals": nn, "table": table, "ids": ids, "totals": totals}, want, "exact capacity")
    # device tensors between sentinels: nothing outside [0, 3 V)
    pad = 6
    dev = torch.device("cuda:0")
    flat = [torch.full((pad + 3 * V + 3 * 5 + pad,), -7.25, dtype=torch.float32, device=dev) for _ in range(2)]
    out = {"vertices": flat[0][pad:pad + 3 * (V + 5)].view(V + 5, 3), "normals": flat[1][pad:pad + 3 * (V + 5)].view(V + 5, 3)}
    got = gm.CoarseMesh(s, out=out, stages=0)
    gm.synchronize()
    assert_mesh(got, want, "device tensors")
    for t in flat:
        h = t.cpu().numpy()
        assert (h[:pad] == -7.25).all() and (h[pad + 3 * V:] == -7.25).all(), "a sentinel was overwritten"
    short = {"vertices": torch.zeros((V - 1, 3), dtype=torch.float32, device=dev)}
    refused(lambda: gm.CoarseMesh(s, out=short, stages=0), 1, "capacity")
    assert not short["vertices"].any()


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_device_outputs_behind_an_integration_and_the_map_is_only_read(oracle_mod):
    import torch
    from tests.test_gpu_parity import _mk
    N, res, s = 16, 0.04, 2
    _, gm, integ = _mk(oracle_mod, N, res, True, max_chunks=1024)
    cam = small_camera(96, 72)
    from cvids_amd import synth
    cimg = synth.render_color(96, 72, 3)
    frames = make_frames("sphere_room", 3, 96, 72)
    for d, p in frames[:2]:
        gm.IntegrateDepthScanColor(integ, d, p, cam, cimg, p, cam)
    rows = 400000
    dev = torch.device("cuda:0")
    out = {k: torch.full((rows, 3), -7.25, dtype=torch.float32, device=dev) for k in ("vertices", "normals", "colors")}
    d, p = frames[2]
    gm.IntegrateDepthScanColor(integ, d, p, cam, cimg, p, cam)  # queued just before; no synchronise by the caller
    got = gm.CoarseMesh(s, out=out)
    gm.synchronize()
    V = got["totals"]["vertices"]
    assert 1000 < V < rows
    before, to_update, counters = fields_of(gm, N), gm.GetMeshesToUpdate().tolist(), gm.counters()
    host = gm.CoarseMesh(s)
    again = gm.CoarseMesh(s)
    assert host["totals"] == got["totals"] == again["totals"]
    assert np.array_equal(host["table"], got["table"]) and np.array_equal(host["ids"], got["ids"])
    for key in ("vertices", "normals", "colors"):
        g = out[key].cpu().numpy()
        assert np.array_equal(bits(g[:V]), bits(host[key])), key
        assert (g[V:] == -7.25).all(), key
        assert np.array_equal(bits(again[key]), bits(host[key])), key  # two calls in a row: identical bits
    # the map is only read
    after = fields_of(gm, N)
    assert sorted(before) == sorted(after)
    for cid in before:
        for a, b in zip(before[cid], after[cid]):
            assert a.tobytes() == b.tobytes(), cid
    assert gm.GetMeshesToUpdate().tolist() == to_update and len(to_update) > 0
    assert gm.counters() == counters
    gm.close()


def test_cycles_return_their_memory(built):
    N, s = 32, 2
    field = built.field("dense", N)
    footprint = 64 * N ** 3 * 12  # the pool of the map: 25 MB

    def cycle():
        gm = new_map(N)
        upload(gm, field)
        assert gm.CoarseMesh(s)["totals"]["vertices"] > 0
        assert gm.CoarseMesh(1, ids=[(0, 0, 0)], stages=0)["totals"]["vertices"] > 0
        gm.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    print("free after each cycle: %s" % readings)
    assert abs(readings[0] - readings[-1]) < footprint // 2, readings


def test_refusals(built):
    from cvids_amd import chisel as ch
    N, s = 8, 2
    gm = built.map("dense", N)
    V = built.want("dense", N, s)["totals"]["vertices"]
    v = np.full((V, 3), -7.25, np.float32)
    req = capi.CoarseRequest()
    req.stride = s
    err = lambda: gm.L.chisel_hip_last_error().decode()
    assert raw_call(gm, req, V, v, None, None)[0] == 0
    v[:] = -7.25

    class Null:
        L, h = gm.L, None
    assert raw_call(Null, req, V, v, None, None)[0] == 1 and "null" in err()
    assert raw_call(gm, None, V, v, None, None)[0] == 1 and "null" in err()
    for stride in (0, -1, 3, N + 1, 2 * N):
        bad = capi.CoarseRequest()
        bad.stride = stride
        assert raw_call(gm, bad, V, v, None, None)[0] == 1 and "stride" in err(), stride
        assert raw_call(gm, bad, 0, None, None, None)[0] == 1 and "stride" in err(), stride
    bad = capi.CoarseRequest()
    bad.stride, bad.stages = s, 4
    assert raw_call(gm, bad, V, v, None, None)[0] == 1 and "stages" in err()
    assert raw_call(gm, req, V, None, None, None)[0] == 1 and "no output" in err()
    assert raw_call(gm, req, V, None, v, None)[0] == 1 and "without vertices" in err()
    assert raw_call(gm, req, -1, v, None, None)[0] == 1 and "negative" in err()
    assert gm.L.chisel_hip_coarse_mesh(gm.h, C.byref(req), 0, None, None, None, 0, None, None, None) == 1 and "totals" in err()
    # whatever chisel_hip_gather_chunks refuses of a selection
    refused(lambda: gm.CoarseMesh(s, ids=[(0, 0, 0)], box=((0, 0, 0), (1, 1, 1))), 1, "box together")
    refused(lambda: gm.CoarseMesh(s, box=((0, 2, 0), (1, 1, 1))), 1, "lo > hi")
    assert "id 1 " in refused(lambda: gm.CoarseMesh(s, ids=[(0, 0, 0), (0, hc.ID_MAX + 1, 0)]), 1, "range")
    bad = capi.CoarseRequest()
    bad.stride, bad.chunks.n_ids = s, 3
    assert raw_call(gm, bad, V, v, None, None)[0] == 1 and "without an id list" in err()
    bad.chunks.n_ids = -1
    assert raw_call(gm, bad, V, v, None, None)[0] == 1 and "negative" in err()
    assert (v == -7.25).all()
    # a group, and one shard of several
    grp = shard = None
    try:
        grp = ch.Chisel((N, N, N), RES[N], True, max_chunks=64, devices=[0, 0])
        assert raw_call(grp, req, V, v, None, None)[0] == 5 and "group" in err()
        shard = new_map(N, n_shards=2, shard_rank=0)
        assert raw_call(shard, req, V, v, None, None)[0] == 5 and "one shard of several" in err()
        assert raw_call(shard, req, 0, None, None, None)[0] == 5
    finally:
        for m in (grp, shard):
            if m is not None:
                m.close()
    assert (v == -7.25).all()


# ---- the facade -------------------------------------------------------------------------------------------------------------------------
def weighted_sum(a):
    """facade_coarse.cpp's checksum: sum of (index + 1) x word over the array's 32-bit words, modulo 2^64"""
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((w * np.arange(1, len(w) + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_the_facade_program_meshes_what_python_meshes(tmp_path):
    """cvids_amd/open_chisel/tests/facade_coarse.cpp: ChunkManager::GenerateCoarseMesh at strides 1, 2, 4, 8 -- vertex counts and a
    checksum per array against Python's coarse mesh of the same three frames -- and the file of Chisel::SaveCoarseMeshToPLY against
    SaveCoarseMeshPLY's"""
    from cvids_amd import chisel as ch
    tdir = os.path.join(ROOT, "cvids_amd", "open_chisel", "tests")
    exe = os.path.join(tdir, "facade_coarse")
    subprocess.check_call(["make", "-C", tdir, "coarse"])  # (make decides whether the binary is current)
    ply = str(tmp_path / "facade.ply")
    run_ = subprocess.run([exe, ply], capture_output=True, text=True, timeout=300)
    assert run_.returncode == 0 and "facade_coarse ok" in run_.stdout, run_.stdout + run_.stderr
    lines = dict(l.split(" ", 1) for l in run_.stdout.splitlines() if " " in l)
    W, H, N = 64, 48, 8
    gm = ch.Chisel((N, N, N), 0.05, True)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    cam = ch.PinholeCamera(52.5, 52.5, 31.5, 23.5, W, H, 0.05, 5.0)
    v, u = np.mgrid[0:H, 0:W]
    color = np.stack([(7 * u + 13 * v + 50 * c) & 255 for c in range(3)], -1).astype(np.uint8)
    pose = np.eye(4, dtype=np.float32)
    for k in range(3):
        depth = (1.5 + 0.25 * k + 0.0078125 * u - 0.00390625 * v).astype(np.float32)  # (every term exact in binary)
        gm.IntegrateDepthScanColor(integ, depth, pose, cam, color, pose, cam)
    for stride in (1, 2, 4, 8):
        got = gm.CoarseMesh(stride)
        n, sv, sn, sc = lines["stride%d" % stride].split()
        assert int(n) == len(got["vertices"]) and (stride > 2 or int(n) > 0), stride
        for name, want in (("vertices", sv), ("normals", sn), ("colors", sc)):
            assert int(want, 16) == weighted_sum(got[name]), (stride, name)
    mine = str(tmp_path / "python.ply")
    assert gm.SaveCoarseMeshPLY(mine, 2)
    assert open(mine, "rb").read() == open(ply, "rb").read() and os.path.getsize(mine) > 1000
    gm.close()


# ---- the crowded hash table ---------------------------------------------------------------------------------------------------------------
def test_on_a_crowded_hash_table(built):
    """the block's chunks pushed off their home buckets by blockers that went in first, every second blocker collected afterwards --
    tombstones on the probe paths --, and blockers left on the homes of the absent + neighbours: the slot look-ups of a list and the
    neighbour look-ups of both kernels walk long probes and pass tombstones.  The reach is asserted on the device's own read-out."""
    N, s = 8, 2
    field = built.field("thresholds", N)
    gm = new_map(N, max_chunks=512)
    cap = gm.hash_table()["capacity"]
    assert cap == 1024
    block = sorted(field)
    looked_up = sorted({(x + dx, y + dy, z + dz) for x, y, z in block for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)})
    blockers, seen = [], set()
    for cid in looked_up:
        home = hc.home_of(cid, cap)
        for h in range(home, home + 3):  # (three buckets from the home on: the probe walks them)
            if h % cap not in seen:
                seen.add(h % cap)
                blockers += hc.far_ids(h % cap, 2, cap)
    for k, cid in enumerate(blockers):
        sdf, w, c = hc.blocker_voxels(k, N ** 3, True)
        gm.AddChunk(cid, sdf, w, c)
    upload(gm, field)
    gm.GarbageCollect(blockers[::2])
    t = gm.hash_table()
    r = hc.reach(t, block)
    print("reach of the block's ids: %s; %d tombstones, %d blockers" % (r, hc.n_tombstones(t), len(blockers)))
    assert r["off_home"] == len(block) and r["tomb"] == len(block) and hc.n_tombstones(t) == len(blockers[::2])
    assert_mesh(gm.CoarseMesh(s, ids=block, colors=False, stages=0), built.want("thresholds", N, s), "crowded, a list")
    everything = gm.CoarseMesh(s, colors=False, stages=0)
    mine = [i for i, c in enumerate(map(tuple, everything["ids"].tolist())) if c in field]
    assert len(mine) == len(block) and len(everything["ids"]) == len(block) + len(blockers) - len(blockers[::2])
    assert np.array_equal(everything["table"][mine][:, 1], built.want("thresholds", N, s)["table"][:, 1])
    gm.close()
