"""chisel_hip_mesh_components and chisel_hip_filter_mesh on the GPU: the connected components of an indexed mesh and the mesh without
its small ones.

The reference of every comparison is the restatement (tests/mesh_components_restated.py: a dictionary of parents, sorted roots, boolean
masks), which tests/test_mesh_components_restated.py pins to scipy's connected components.  Labels, table, maps, renumbered ids, totals
and the copied float rows are compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cvids_amd import capi
from tests import mesh_components_restated as mc
from tests.common import free_bytes, make_frames, small_camera, upload
from tests.test_coarse_mesh_restated import RES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.hand_cases()
KNOBS = ((1, False), (3, False), (2, True), (1, True))
ROWS = ("vertices", "normals", "colors")


def new_map(N=8, color=True, max_chunks=64, **kw):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), RES[N], color, max_chunks=max_chunks, **kw)


@pytest.fixture(scope="module")
def gm():
    """the map that lends its device, its stream and its scratch to the calls on arrays made by hand"""
    m = new_map()
    yield m
    m.close()


@pytest.fixture(scope="module")
def wanted():
    """the restatement of every hand-made case, made once and only read: name -> (components, {knobs: filtered}, float rows)"""
    out = {}
    for name, V, idx in CASES:
        rows = mc.float_rows(V, 17)
        out[name] = (mc.components(V, idx), {k: mc.filter_mesh(V, idx, k[0], k[1], rows) for k in KNOBS}, rows)
    return out


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


def assert_components(got, want, what, V, T):
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    for key, rows in (("vertex_component", V), ("triangle_component", T)):
        if key not in got:  # (an output that was not asked for)
            continue
        g = host(got[key])[:rows]
        assert g.dtype == np.int32 and np.array_equal(g, want[key]), "%s: %s differ in %d places" % (what, key, int((g != want[key]).sum()))
    assert got["table"].dtype == np.int64 and np.array_equal(got["table"], want["table"]), what


def assert_filtered(got, want, what, V, T):
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    live = {"indices": want["totals"]["kept_triangles"], "vertex_map": V, "triangle_map": T}
    for key in ("indices", "vertex_map", "triangle_map") + ROWS:
        if want.get(key) is None or key not in got:  # (an output that was not asked for)
            continue
        g = np.ascontiguousarray(host(got[key])[:live.get(key, want["totals"]["kept_vertices"])])
        assert g.shape == want[key].shape and g.dtype == want[key].dtype, (what, key, g.shape, want[key].shape, g.dtype)
        assert g.tobytes() == want[key].tobytes(), "%s: %s differ" % (what, key)  # (bytes: the float rows hold NaNs)


def mesh_of(V, idx, rows):
    return {"vertices": rows["vertices"], "indices": idx, "normals": rows["normals"], "colors": rows["colors"], "totals": {"vertices": V, "triangles": len(idx)}}


# ---- index arrays made by hand --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V,idx", CASES, ids=[c[0] for c in CASES])
def test_hand_made_arrays_through_host_arrays(gm, wanted, name, V, idx):
    comp, filtered, rows = wanted[name]
    assert_components(gm.MeshComponents(idx, n_vertices=V), comp, name, V, len(idx))
    for knobs in KNOBS:
        assert_filtered(gm.FilterMesh(mesh_of(V, idx, rows), *knobs), filtered[knobs], "%s %s" % (name, knobs), V, len(idx))


PAD = 7


def between_sentinels(torch, rows, width, dtype, fill, spare=0):
    """-> (the flat tensor, its view of rows + spare rows behind PAD sentinels)"""
    n = (rows + spare) * max(width, 1)
    flat = torch.full((PAD + n + PAD,), fill, dtype=dtype, device="cuda:0")
    view = flat[PAD:PAD + n]
    return flat, (view.view(rows + spare, width) if width else view)


def assert_sentinels(flat, live, fill, what):
    h = flat.cpu().numpy()
    assert (h[:PAD] == fill).all() and (h[PAD + live:] == fill).all(), "a sentinel of %s was overwritten" % what


@pytest.mark.parametrize("name,V,idx", CASES, ids=[c[0] for c in CASES])
def test_hand_made_arrays_through_device_tensors_between_sentinels(gm, wanted, name, V, idx):
    import torch
    comp, filtered, rows = wanted[name]
    T = len(idx)
    d_idx = torch.from_numpy(idx).to("cuda:0")
    flat_v, out_v = between_sentinels(torch, V, 0, torch.int32, -9)
    flat_t, out_t = between_sentinels(torch, T, 0, torch.int32, -9)
    got = gm.MeshComponents(d_idx, n_vertices=V, out={"vertex_component": out_v, "triangle_component": out_t})
    gm.synchronize()
    assert_components(got, comp, name, V, T)
    assert_sentinels(flat_v, V, -9, "vertex_component")
    assert_sentinels(flat_t, T, -9, "triangle_component")
    mesh = {k: (torch.from_numpy(np.ascontiguousarray(rows[k])).to("cuda:0") if k in rows else d_idx) for k in ROWS + ("indices",)}
    mesh["totals"] = {"vertices": V, "triangles": T}
    for knobs in KNOBS[1:3]:
        want = filtered[knobs]
        spare = 3  # (room behind the live rows: it stays as it was)
        flats, out = {}, {}
        for key in ROWS:
            flats[key], out[key] = between_sentinels(torch, V, 3, torch.float32, -7.25, spare)
        flats["indices"], out["indices"] = between_sentinels(torch, T, 3, torch.int32, -9, spare)
        flats["vertex_map"], out["vertex_map"] = between_sentinels(torch, V, 0, torch.int32, -9)
        flats["triangle_map"], out["triangle_map"] = between_sentinels(torch, T, 0, torch.int32, -9)
        got = gm.FilterMesh(mesh, *knobs, out=out)
        gm.synchronize()
        assert_filtered(got, want, "%s %s, device" % (name, knobs), V, T)
        live = {"indices": 3 * want["totals"]["kept_triangles"], "vertex_map": V, "triangle_map": T}
        for key, flat in flats.items():
            assert_sentinels(flat, live.get(key, 3 * want["totals"]["kept_vertices"]), -9 if flat.dtype == torch.int32 else -7.25, key)
    # narrowed tensors of the call's own
    got = gm.FilterMesh(mesh, *KNOBS[0])
    gm.synchronize()
    assert_filtered(got, filtered[KNOBS[0]], "%s, tensors of its own" % name, V, T)
    assert got["vertices"].shape[0] == filtered[KNOBS[0]]["totals"]["kept_vertices"] and got["indices"].shape[0] == filtered[KNOBS[0]]["totals"]["kept_triangles"]


def test_garbage_gives_an_answer_not_a_fault(gm):
    """a device array of arbitrary words: almost every triangle is invalid, the few valid ones are joined, nothing else is touched"""
    import torch
    V, T = 1000, 5000
    rng = np.random.default_rng(23)
    idx = rng.integers(-2 ** 31, 2 ** 31, (T, 3), dtype=np.int64).astype(np.int32)
    idx[::97] = rng.integers(0, V, (len(idx[::97]), 3))
    want = mc.components(V, idx)
    assert 40 < T - want["totals"]["invalid_triangles"] < 100
    assert_components(gm.MeshComponents(torch.from_numpy(idx).to("cuda:0"), n_vertices=V), want, "garbage", V, T)
    rows = mc.float_rows(V, 2)
    assert_filtered(gm.FilterMesh(mesh_of(V, idx, rows), 1), mc.filter_mesh(V, idx, 1, False, rows), "garbage, filtered", V, T)
    # no vertex at all: every triangle is invalid
    none = gm.MeshComponents(idx, n_vertices=0)
    assert none["totals"] == dict(dict.fromkeys(mc.TOTALS, 0), triangles=T, invalid_triangles=T) and (none["triangle_component"] == -1).all()
    empty = gm.MeshComponents(np.zeros((0, 3), np.int32))
    assert empty["totals"] == dict.fromkeys(mc.TOTALS, 0) and empty["table"].shape == (0, 3)
    assert gm.FilterMesh({"vertices": np.zeros((0, 3), np.float32), "indices": np.zeros((0, 3), np.int32)})["totals"] == dict.fromkeys(mc.TOTALS, 0)


def test_back_to_back_calls_of_different_sizes(wanted):
    """on a fresh map: the scratch is made by a small call, grown by a large one, reused by a small one and by the large one again"""
    m = new_map()
    by_name = {c[0]: c for c in CASES}
    for name in ("a strip", "many tiles", "a fan", "a path, shuffled", "many tiles", "one triangle"):
        _, V, idx = by_name[name]
        comp, filtered, rows = wanted[name]
        assert_components(m.MeshComponents(idx, n_vertices=V), comp, name, V, len(idx))
        assert_filtered(m.FilterMesh(mesh_of(V, idx, rows), *KNOBS[1]), filtered[KNOBS[1]], name, V, len(idx))
    m.close()


# ---- the blobs: an indexed mesh of the device's own -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_maps():
    maps = {}
    for N in (8, 16):
        m = new_map(N, max_chunks=128)
        upload(m, mc.blobs(N, mc.BLOCK[N], mc.SPHERES, RES[N]))
        maps[N] = m
    yield maps
    for m in maps.values():
        m.close()


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("N", [8, 16])
def test_the_blobs_of_a_map(blob_maps, N, s):
    m = blob_maps[N]
    half = [c for c in sorted(m.GetChunkIDs().tolist()) if c[0] < mc.BLOCK[N] // 2]  # (the chunks at the cut are extras: owners that are not selected)
    for ids in (None, half):
        mesh = m.IndexedMesh(s, ids=ids, normals=True, colors=True)
        V, T = mesh["totals"]["vertices"], mesh["totals"]["triangles"]
        what = "blobs N %d s %d %s" % (N, s, "all" if ids is None else "a list")
        want = mc.components(V, mesh["indices"])
        assert_components(m.MeshComponents(mesh["indices"], n_vertices=V), want, what, V, T)
        counts = sorted(want["table"][:, 2].tolist())
        if ids is None:
            assert len(counts) == len(mc.SPHERES) and len(set(counts)) == len(counts) and counts[0] >= 8
            for c in range(len(counts)):
                assert mc.closed(mesh["indices"][want["triangle_component"] == c]), (what, c)
        else:
            assert mesh["totals"]["owners"] > mesh["totals"]["chunks"] and 2 <= len([c for c in counts if c]) and T > 100
        rows = {k: mesh[k] for k in ROWS}
        for knobs in ((1, False), (max(counts[-2], 1), False), (counts[-1] + 1, False), (1, True)):
            assert_filtered(m.FilterMesh(mesh, *knobs), mc.filter_mesh(V, mesh["indices"], knobs[0], knobs[1], rows), "%s %s" % (what, knobs), V, T)


def test_indexed_mesh_into_filter_mesh_without_a_host_copy(blob_maps):
    """IndexedMesh(out=...) and FilterMesh(out=...) back to back, nothing synchronised between them: the filter is queued behind the
    mesh on the map's stream; the tensors have more rows than the mesh, whose size is the totals entry"""
    import torch
    N, s = 8, 1
    m = blob_maps[N]
    spare = 100
    size = m.IndexedMeshSize(s)
    V, T = size["vertices"], size["triangles"]
    dev = torch.device("cuda:0")
    mesh_out = {k: torch.full((V + spare, 3), -7.25, dtype=torch.float32, device=dev) for k in ROWS}
    mesh_out["indices"] = torch.full((T + spare, 3), -9, dtype=torch.int32, device=dev)
    for knobs in ((50, False), (1, True)):
        out = {k: torch.full((V + spare, 3), -7.25, dtype=torch.float32, device=dev) for k in ROWS}
        out["indices"] = torch.full((T + spare, 3), -9, dtype=torch.int32, device=dev)
        out["vertex_map"] = torch.full((V + spare,), -9, dtype=torch.int32, device=dev)
        out["triangle_map"] = torch.full((T + spare,), -9, dtype=torch.int32, device=dev)
        mesh = m.IndexedMesh(s, out=mesh_out)
        got = m.FilterMesh(mesh, *knobs, out=out)
        m.synchronize()
        assert mesh["totals"]["vertices"] == V and mesh["totals"]["triangles"] == T
        down = {k: mesh_out[k].cpu().numpy()[:T if k == "indices" else V] for k in mesh_out}
        want = mc.filter_mesh(V, down["indices"], knobs[0], knobs[1], {k: down[k] for k in ROWS})
        assert 0 < want["totals"]["kept_components"] < len(mc.SPHERES)
        assert_filtered(got, want, "device to device %s" % (knobs,), V, T)
        assert (down["normals"] != 0).any() and (down["colors"] != 0).any()
        kv, kt = want["totals"]["kept_vertices"], want["totals"]["kept_triangles"]
        for k in ROWS:
            assert (out[k][kv:] == -7.25).all(), k
        assert (out["indices"][kt:] == -9).all() and (out["vertex_map"][V:] == -9).all() and (out["triangle_map"][T:] == -9).all()


def test_queued_behind_an_integration(oracle_mod):
    """frames are integrated, the mesh is taken and filtered, and nobody synchronises until the end: every step reads what the step
    before it left on the map's stream"""
    import torch
    from cvids_amd import synth
    from tests.test_gpu_parity import _mk
    N, res, s = 8, 0.05, 2
    _, m, integ = _mk(oracle_mod, N, res, True, max_chunks=1024)
    cam = small_camera(96, 72)
    cimg = synth.render_color(96, 72, 3)
    dev = torch.device("cuda:0")
    cap = 200000
    mesh_out = {k: torch.zeros((cap, 3), dtype=torch.float32, device=dev) for k in ROWS}
    mesh_out["indices"] = torch.zeros((cap, 3), dtype=torch.int32, device=dev)
    out = {"vertices": torch.zeros((cap, 3), dtype=torch.float32, device=dev), "indices": torch.zeros((cap, 3), dtype=torch.int32, device=dev),
           "vertex_map": torch.zeros(cap, dtype=torch.int32, device=dev)}
    labels = {"vertex_component": torch.zeros(cap, dtype=torch.int32, device=dev)}
    for d, p in make_frames("sphere_room", 3, 96, 72):
        m.IntegrateDepthScanColor(integ, d, p, cam, cimg, p, cam)
    mesh = m.IndexedMesh(s, out=mesh_out)
    V, T = mesh["totals"]["vertices"], mesh["totals"]["triangles"]
    got = m.FilterMesh(mesh, 64, out=out)
    comp = m.MeshComponents(mesh_out["indices"][:T], n_vertices=V, out=labels)
    m.synchronize()
    assert 100 < V < cap and V < T < cap
    down = mesh_out["indices"].cpu().numpy()[:T]
    want = mc.filter_mesh(V, down, 64, False, {"vertices": mesh_out["vertices"].cpu().numpy()[:V]})
    print("integrated scene: V %d T %d, %d components, the largest %d triangles, %d kept of %d triangles at 64" % (
        V, T, want["totals"]["components"], want["totals"]["largest_triangles"], want["totals"]["kept_triangles"], T))
    assert_filtered(got, want, "behind an integration", V, T)
    assert_components(comp, mc.components(V, down), "behind an integration", V, T)
    m.close()


# ---- the size query, capacities, refusals ---------------------------------------------------------------------------------------------------
def ptr(a):
    return (a if isinstance(a, int) else a.ctypes.data) if a is not None else None


def raw_components(m, V, T, idx, vc, tc, cap, table, on_device=0, totals=True):
    t = capi.ComponentsTotals(*([-1] * 8))
    rc = m.L.chisel_hip_mesh_components(m.h, V, T, ptr(idx), on_device, ptr(vc), ptr(tc), cap, table.ctypes.data_as(C.POINTER(C.c_int64)) if table is not None else None,
                                        C.byref(t) if totals else None)
    return rc, {name: int(getattr(t, name)) for name, _ in capi.ComponentsTotals._fields_}


def raw_filter(m, V, T, idx, v, n, c, min_triangles, largest_only, cap_v, cap_t, ov, ox, on, oc, vm, tm, on_device=0, totals=True):
    t = capi.ComponentsTotals(*([-1] * 8))
    rc = m.L.chisel_hip_filter_mesh(m.h, V, T, ptr(idx), ptr(v), ptr(n), ptr(c), min_triangles, largest_only, cap_v, cap_t, ptr(ov), ptr(ox), ptr(on), ptr(oc),
                                    ptr(vm), ptr(tm), on_device, C.byref(t) if totals else None)
    return rc, {name: int(getattr(t, name)) for name, _ in capi.ComponentsTotals._fields_}


class Arrays:
    """the arguments of both entries for one hand-made case, the outputs filled with sentinels"""

    def __init__(self, name, wanted):
        _, self.V, self.idx = next(c for c in CASES if c[0] == name)
        self.comp, self.filtered, self.rows = wanted[name]
        self.T = len(self.idx)
        self.v, self.n, self.c = (np.ascontiguousarray(self.rows[k]) for k in ROWS)
        self.ov, self.on, self.oc = (np.full((self.V, 3), -7.25, np.float32) for _ in range(3))
        self.ox = np.full((self.T, 3), -9, np.int32)
        self.vm, self.tm, self.vc, self.tc = (np.full(n, -9, np.int32) for n in (self.V, self.T, self.V, self.T))
        self.table = np.full((self.V, 3), -9, np.int64)

    def untouched(self):
        return all((a == -7.25).all() for a in (self.ov, self.on, self.oc)) and all((a == -9).all() for a in (self.ox, self.vm, self.tm, self.vc, self.tc, self.table))


def test_size_queries_and_capacities(gm, wanted):
    a = Arrays("equal largest components", wanted)
    V, T, C_ = a.V, a.T, a.comp["totals"]["components"]
    err = lambda: gm.L.chisel_hip_last_error().decode()
    # the components' size query: no output named
    rc, totals = raw_components(gm, V, T, a.idx, None, None, 0, None)
    assert rc == 0 and totals == a.comp["totals"] and a.untouched()
    rc, totals = raw_components(gm, V, T, a.idx, None, None, 0, a.table)  # (a table without a capacity is none)
    assert rc == 0 and totals == a.comp["totals"] and a.untouched()
    # a short table: refused, totals filled, nothing written
    rc, totals = raw_components(gm, V, T, a.idx, a.vc, a.tc, C_ - 1, a.table)
    assert rc == 1 and "table capacity" in err() and totals == a.comp["totals"] and a.untouched()
    rc, totals = raw_components(gm, V, T, a.idx, a.vc, a.tc, C_, a.table)
    assert rc == 0 and totals == a.comp["totals"] and np.array_equal(a.table[:C_], a.comp["table"]) and (a.table[C_:] == -9).all()
    assert np.array_equal(a.vc, a.comp["vertex_component"]) and np.array_equal(a.tc, a.comp["triangle_component"])
    a = Arrays("equal largest components", wanted)
    # the filter's size query fills all eight totals and writes nothing, whatever pointers it is given
    knobs = (4, False)  # (three of the four components with triangles)
    want = mc.filter_mesh(V, a.idx, knobs[0], knobs[1], a.rows)
    kv, kt = want["totals"]["kept_vertices"], want["totals"]["kept_triangles"]
    assert 0 < kv < V and 0 < kt < T
    rc, totals = raw_filter(gm, V, T, a.idx, a.v, a.n, a.c, knobs[0], int(knobs[1]), 0, 0, a.ov, a.ox, a.on, a.oc, a.vm, a.tm)
    assert rc == 0 and totals == want["totals"] and a.untouched()
    # one short in either count: refused, totals filled, nothing written
    for cap_v, cap_t, word in ((kv - 1, kt, "vertex capacity"), (kv, kt - 1, "triangle capacity"), (0, kt, "vertex capacity"), (kv, 0, "triangle capacity")):
        rc, totals = raw_filter(gm, V, T, a.idx, a.v, a.n, a.c, knobs[0], int(knobs[1]), cap_v, cap_t, a.ov, a.ox, a.on, a.oc, a.vm, a.tm)
        assert rc == 1 and word in err() and totals == want["totals"] and a.untouched(), (cap_v, cap_t)
    # exact: the rows behind the kept ones stay as they were
    rc, totals = raw_filter(gm, V, T, a.idx, a.v, a.n, a.c, knobs[0], int(knobs[1]), kv, kt, a.ov, a.ox, a.on, a.oc, a.vm, a.tm)
    assert rc == 0
    assert_filtered({"vertices": a.ov, "normals": a.on, "colors": a.oc, "indices": a.ox, "vertex_map": a.vm, "triangle_map": a.tm, "totals": totals}, want, "exact", V, T)
    assert all((o[kv:] == -7.25).all() for o in (a.ov, a.on, a.oc)) and (a.ox[kt:] == -9).all()
    # the maps alone, under any capacity but the query's
    a = Arrays("equal largest components", wanted)
    rc, totals = raw_filter(gm, V, T, a.idx, None, None, None, knobs[0], int(knobs[1]), 1, 1, None, None, None, None, a.vm, a.tm)
    assert rc == 0 and totals == want["totals"] and np.array_equal(a.vm, want["vertex_map"]) and np.array_equal(a.tm, want["triangle_map"])


def test_refusals_leave_the_outputs_untouched(gm, wanted):
    from cvids_amd import chisel as ch
    a = Arrays("a strip", wanted)
    V, T = a.V, a.T
    err = lambda: gm.L.chisel_hip_last_error().decode()
    big = 2 ** 31

    class Null:
        L, h = gm.L, None
    comp = lambda m=gm, V=V, T=T, idx=a.idx, vc=a.vc, tc=a.tc, cap=V, table=a.table, totals=True: raw_components(m, V, T, idx, vc, tc, cap, table, 0, totals)[0]
    assert comp(m=Null) == 1 and "null map" in err()
    assert comp(V=-1) == 1 and "negative" in err()
    assert comp(T=-1) == 1 and "negative" in err()
    assert comp(V=big) == 5 and "vertices" in err()
    assert comp(T=(big - 1) // 3 + 1) == 5 and "index entries" in err()
    assert comp(idx=None) == 1 and "null indices" in err()
    assert comp(cap=-1) == 1 and "negative capacity" in err()
    assert comp(table=None) == 1 and "without a table" in err()
    assert comp(vc=None, tc=None, cap=0, table=None, totals=False) == 1 and "size query without totals" in err()
    good = dict(m=gm, V=V, T=T, idx=a.idx, v=a.v, n=a.n, c=a.c, min_triangles=1, largest_only=0, cap_v=V, cap_t=T, ov=a.ov, ox=a.ox, on=a.on, oc=a.oc, vm=a.vm,
                tm=a.tm, on_device=0, totals=True)
    filt = lambda **kw: raw_filter(**dict(good, **kw))[0]
    assert filt(m=Null) == 1 and "null map" in err()
    assert filt(V=-1) == 1 and filt(T=-1) == 1 and "negative" in err()
    assert filt(V=big) == 5 and filt(T=(big - 1) // 3 + 1) == 5 and "index entries" in err()
    assert filt(idx=None) == 1 and "null indices" in err()
    assert filt(min_triangles=0) == 1 and "min_triangles" in err()
    assert filt(largest_only=2) == 1 and filt(largest_only=-1) == 1 and "largest_only" in err()
    assert filt(cap_v=-1) == 1 and filt(cap_t=-1) == 1 and "negative capacity" in err()
    assert filt(cap_v=0, cap_t=0, totals=False) == 1 and "size query without totals" in err()
    assert filt(v=None) == 1 and "vertices out without vertices in" in err()
    assert filt(n=None) == 1 and "normals out without normals in" in err()
    assert filt(c=None) == 1 and "colors out without colors in" in err()
    assert filt(on=None) == 1 and "normals in without normals out" in err()
    assert filt(oc=None) == 1 and "colors in without colors out" in err()
    assert filt(ov=None) == 1 and "indices out without vertices out" in err()
    assert filt(ov=None, ox=None) == 1 and "without vertices out" in err()
    grp = None
    try:
        grp = ch.Chisel((8, 8, 8), RES[8], True, max_chunks=64, devices=[0, 0])
        assert comp(m=grp) == 5 and "group" in err()
        assert filt(m=grp) == 5 and "group" in err()
    finally:
        if grp is not None:
            grp.close()
    assert a.untouched()
    assert filt() == 0 and comp() == 0 and not a.untouched()


def test_cycles_return_their_memory(wanted):
    _, V, idx = next(c for c in CASES if c[0] == "many tiles")
    rows = wanted["many tiles"][2]
    footprint = 64 * 8 ** 3 * 12 + 8 * 4 * V  # the pool of the map and the scratch of one call: 2.5 MB; three cycles lie between the readings

    def cycle():
        m = new_map()
        assert m.MeshComponents(idx, n_vertices=V)["totals"]["components"] > 1000
        assert m.FilterMesh(mesh_of(V, idx, rows), 2)["totals"]["kept_vertices"] > 1000
        m.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    print("free after each cycle: %s" % readings)
    assert abs(readings[0] - readings[-1]) < footprint, readings


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_the_clean_ply_is_the_restated_results(blob_maps, tmp_path, binary):
    N, s = 8, 2
    m = blob_maps[N]
    mesh = m.IndexedMesh(s, normals=False, colors=True)
    counts = sorted(mc.components(len(mesh["vertices"]), mesh["indices"])["table"][:, 2].tolist())
    threshold = counts[2]
    want = mc.filter_mesh(len(mesh["vertices"]), mesh["indices"], threshold, False, {"vertices": mesh["vertices"], "colors": mesh["colors"]})
    assert want["totals"]["kept_components"] == 3
    mine, theirs = str(tmp_path / "clean.ply"), str(tmp_path / "restated.ply")
    assert m.SaveCleanMeshPLY(mine, s, threshold, binary=binary)
    assert m._write_indexed_ply(theirs, want, binary)
    assert open(mine, "rb").read() == open(theirs, "rb").read() and os.path.getsize(mine) > 1000
    head = open(mine, "rb").read().split(b"end_header")[0].decode()
    assert "element vertex %d" % want["totals"]["kept_vertices"] in head and "element face %d" % want["totals"]["kept_triangles"] in head
    # the unfiltered file is what it was
    plain = str(tmp_path / "plain.ply")
    assert m.SaveIndexedMeshPLY(plain, s, binary=binary) and m._write_indexed_ply(theirs, mesh, binary)
    assert open(plain, "rb").read() == open(theirs, "rb").read()
    assert not m.SaveCleanMeshPLY(str(tmp_path / "no_such_directory" / "x.ply"), s, threshold)


# ---- the facade -------------------------------------------------------------------------------------------------------------------------
def weighted_sum(a):
    """facade_components.cpp's checksum: sum of (index + 1) x word over the array's 32-bit words, modulo 2^64"""
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((w * np.arange(1, len(w) + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_the_facade_program_filters_what_python_filters(tmp_path):
    """cvids_amd/open_chisel/tests/facade_components.cpp: ChunkManager::FilterMesh on the indexed mesh of three frames -- counts and a
    checksum per array against Python's -- and the file of Chisel::SaveCleanMeshToPLY against SaveCleanMeshPLY's text form"""
    from cvids_amd import chisel as ch
    tdir = os.path.join(ROOT, "cvids_amd", "open_chisel", "tests")
    exe = os.path.join(tdir, "facade_components")
    subprocess.check_call(["make", "-C", tdir, "components"])  # (make decides whether the binary is current)
    ply = str(tmp_path / "facade.ply")
    run_ = subprocess.run([exe, ply], capture_output=True, text=True, timeout=300)
    assert run_.returncode == 0 and "facade_components ok" in run_.stdout, run_.stdout + run_.stderr
    lines = dict(l.split(" ", 1) for l in run_.stdout.splitlines() if " " in l)
    W, H, N = 64, 48, 8
    m = ch.Chisel((N, N, N), 0.05, True)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    cam = ch.PinholeCamera(52.5, 52.5, 31.5, 23.5, W, H, 0.05, 5.0)
    v, u = np.mgrid[0:H, 0:W]
    color = np.stack([(7 * u + 13 * v + 50 * c) & 255 for c in range(3)], -1).astype(np.uint8)
    pose = np.eye(4, dtype=np.float32)
    for k in range(3):
        depth = (1.5 + 0.25 * k + 0.0078125 * u - 0.00390625 * v).astype(np.float32)  # (every term exact in binary)
        m.IntegrateDepthScanColor(integ, depth, pose, cam, color, pose, cam)
    for stride, min_triangles, largest in ((1, 1, 0), (1, 64, 0), (2, 16, 0), (2, 1, 1)):
        got = m.FilterMesh(m.IndexedMesh(stride), min_triangles, bool(largest))
        words = lines["stride%d_min%d_largest%d" % (stride, min_triangles, largest)].split()
        t = got["totals"]
        assert [int(w) for w in words[:5]] == [t["components"], t["largest_triangles"], t["kept_components"], t["kept_vertices"], t["kept_triangles"]], (stride, min_triangles)
        assert t["kept_vertices"] > 0
        for name, want in zip(("vertices", "normals", "colors", "indices"), words[5:]):
            assert int(want, 16) == weighted_sum(got[name]), (stride, min_triangles, name)
    mine = str(tmp_path / "python.ply")
    assert m.SaveCleanMeshPLY(mine, 2, 16, binary=False)
    assert open(mine, "rb").read() == open(ply, "rb").read() and os.path.getsize(mine) > 1000
    m.close()
