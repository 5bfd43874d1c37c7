"""chisel_hip_indexed_mesh on the GPU: the coarse mesh's triangles over one vertex per crossed lattice edge.

The reference of every comparison is the restatement (tests/indexed_mesh_restated.py: every cube, dictionaries keyed by (owner, lattice
point, axis)), which tests/test_indexed_mesh_restated.py pins to the coarse restatement; for the shading chisel_hip_shade_vertices on
the call's own vertices.  Vertices, indices, both tables, owner ids and totals are compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cvids_amd import capi
from tests import hash_cases as hc
from tests import indexed_mesh_restated as ir
from tests import voxel_fields as vf
from tests.common import fields_of, free_bytes, make_frames, same_bits, small_camera, upload
from tests.test_coarse_mesh_restated import B, RES, SEED
from tests.test_indexed_mesh_restated import MEASURED_ULPS, SPHERE, ulps_apart

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = (-1000, 900, -37)  # a negative, far base
# N = 32, s = 1: M = 32, a row mask uses all 32 bits and the last bit's popcount-below; N = 32, s = 32: M = 1
CASES = [(8, 1), (8, 2), (8, 4), (8, 8), (16, 1), (16, 4), (32, 1), (32, 32)]
KEYS = ("vertices", "indices", "table", "owner_table", "owner_ids")


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
            if family == "sphere":
                self.fields[key] = ir.sphere(N, SPHERE["B"], SPHERE["radius"], SPHERE["centre"], RES[N], base)
            else:
                self.fields[key] = getattr(vf, family)(N, B, SEED, res=RES[N], base=base)
        return self.fields[key]

    def map(self, family, N, base=(0, 0, 0)):
        key = (family, N, tuple(base))
        if key not in self.maps:
            gm = new_map(N, max_chunks=128 if family == "sphere" else 64)
            upload(gm, self.field(family, N, base))
            self.maps[key] = gm
        return self.maps[key]

    def want(self, family, N, s, base=(0, 0, 0), selection=None, box=None):
        key = (family, N, s, tuple(base), None if selection is None else tuple(map(tuple, selection)), box)
        if key not in self.restated:
            self.restated[key] = ir.indexed_mesh(self.oracle_mod, self.field(family, N, base), N, RES[N], s, selection, box)
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


def host(a, rows):
    return a.cpu().numpy()[:rows] if hasattr(a, "is_cuda") else a


def assert_mesh(got, want, what):
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    for key in KEYS:
        g = host(got[key], len(want[key]))
        assert g.shape == want[key].shape and g.dtype == want[key].dtype, (what, key, g.shape, want[key].shape, g.dtype)
        if key == "vertices":
            same_bits(np.ascontiguousarray(g), want[key], "%s: vertices" % what)
        else:
            assert np.array_equal(g, want[key]), "%s: %s differ in %d places" % (what, key, int((g != want[key]).sum()))


def refused(call, code, word=None):
    with pytest.raises(capi.ChiselHipError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    return str(e.value)


def manifold(indices, V):
    """-> (edges, the set of use counts of the undirected edges); every id below V, every vertex referenced, no vertex twice in a triangle"""
    idx = np.asarray(indices)
    assert idx.min() >= 0 and idx.max() < V and len(np.unique(idx)) == V
    assert (idx[:, 0] != idx[:, 1]).all() and (idx[:, 1] != idx[:, 2]).all() and (idx[:, 0] != idx[:, 2]).all()
    uses = ir.edge_uses(idx)
    return len(uses), set(uses.values())


# ---- bit for bit against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,s", CASES)
@pytest.mark.parametrize("family", ["dense", "thresholds"])
def test_bit_for_bit_against_the_restatement(built, family, N, s):
    """at N = 32, s = 1 one chunk with its seven + neighbours as extras (a list of one id), every other case the whole block, whose + side
    is absent; s = N is one cube per chunk, its twelve edges in up to seven owners"""
    gm = built.map(family, N)
    selection = [(0, 0, 0)] if (N, s) == (32, 1) else None
    want = built.want(family, N, s, selection=selection)
    got = gm.IndexedMesh(s, ids=selection, normals=False, colors=False)
    assert_mesh(got, want, "%s N %d s %d" % (family, N, s))
    assert gm.IndexedMeshSize(s, ids=selection) == want["totals"]
    if family == "dense":
        assert want["totals"]["triangles"] > 0 and want["totals"]["cubes_meshed"] == ((B * N // s - 1) ** 3 if selection is None else N ** 3)
        counts = manifold(got["indices"], want["totals"]["vertices"])[1]
        assert N != 8 or counts <= {1, 2}
    if selection is not None:
        assert want["totals"]["owners"] == 8 and int((want["owner_table"][1:, 1] > 0).sum()) >= 3 and want["owner_table"][7, 1] == 0  # (the diagonal neighbour owns no edge of the cubes)
    if (N, s) == (32, 1) and family == "dense":  # half of the chunk's 3 x 32^3 edges are crossed: rows with many bits, the last among them
        assert want["owner_table"][0, 1] > 32 * 32 * 32


# ---- a selection beyond one batch of the scans and beyond the grid -------------------------------------------------------------------------
BIG = 13  # 13^3 = 2197 chunks of 8^3 voxels: 8 x 256 + 149 for the scans' carry, 149 more than the grid of 2048 workgroups


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
    """both scans carry their sums over eight full batches, and every chunk and owner kernel strides over its grid"""
    field, ids, gm = big
    want = ir.indexed_mesh(oracle_mod, field, 8, RES[8], s)
    assert want["totals"]["owners"] == want["totals"]["chunks"] == BIG ** 3 == 2197 > 2048
    assert_mesh(gm.IndexedMesh(s, normals=False, colors=False), want, "13^3 chunks, s %d" % s)
    assert gm.IndexedMeshSize(s) == want["totals"]


def test_a_long_scrambled_list(big, oracle_mod):
    field, ids, gm = big
    s = 4
    pick = [ids[i] for i in np.random.default_rng(SEED).permutation(len(ids))[:300]]
    assert len(set(pick)) == 300 and pick != sorted(pick)
    want = ir.indexed_mesh(oracle_mod, field, 8, RES[8], s, selection=pick)
    # the extras carry the owners' scan into further batches, and some of them own vertices
    assert want["totals"]["chunks"] == 300 and want["totals"]["owners"] > 3 * 256 and int((want["owner_table"][300:, 1] > 0).sum()) > 0
    assert_mesh(gm.IndexedMesh(s, ids=pick, normals=False, colors=False), want, "a list of 300")
    # a non-resident id in the last batch of the chunks' scan
    pick[299] = (BIG + 7, BIG + 7, BIG + 7)
    with pytest.raises(KeyError) as e:
        gm.IndexedMesh(s, ids=pick, normals=False, colors=False)
    assert "id 299 " in str(e.value)


@pytest.mark.parametrize("family,N,s", [("dense", 8, 1), ("thresholds", 8, 2), ("dense", 16, 4)])
def test_far_from_the_origin(built, family, N, s):
    assert_mesh(built.map(family, N, FAR).IndexedMesh(s, normals=False, colors=False), built.want(family, N, s, FAR), "far %s N %d s %d" % (family, N, s))


def test_nan_distances(built, oracle_mod):
    """a NaN distance is legal input: it reads as "not below zero", and an edge from it to a negative end has a NaN vertex"""
    N, s = 8, 1
    field = {cid: (sdf.copy(), w, c) for cid, (sdf, w, c) in built.field("dense", N).items()}
    rng = np.random.default_rng(11)
    for cid in field:
        field[cid][0][rng.choice(N ** 3, 9, replace=False)] = np.nan
    gm = new_map(N)
    upload(gm, field)
    want = ir.indexed_mesh(oracle_mod, field, N, RES[N], s)
    got = gm.IndexedMesh(s, normals=False, colors=False)
    assert np.isnan(want["vertices"]).any()
    assert_mesh(got, want, "NaN")
    gm.close()


# ---- the sphere: a closed 2-manifold on the device's own output -------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 4])
def test_the_sphere_is_closed(built, s):
    N = 8
    gm = built.map("sphere", N)
    got = gm.IndexedMesh(s, normals=False, colors=False)
    assert_mesh(got, built.want("sphere", N, s), "sphere s %d" % s)
    V, T = got["totals"]["vertices"], got["totals"]["triangles"]
    edges, counts = manifold(got["indices"], V)
    assert counts == {2} and V - edges + T == 2 and 2 * V == T + 4 and T > 100


def test_plus_side_absent(built, oracle_mod):
    """the sphere without its chunks at x = 2 and x = 3: the cubes on that face yield nothing, the surface is open there, and the owners on
    the + side are gone"""
    N, s = 8, 2
    field = {cid: v for cid, v in built.field("sphere", N).items() if cid[0] < 2}
    gm = new_map(N)
    upload(gm, field)
    want = ir.indexed_mesh(oracle_mod, field, N, RES[N], s)
    got = gm.IndexedMesh(s, normals=False, colors=False)
    assert_mesh(got, want, "+ side absent")
    assert manifold(got["indices"], got["totals"]["vertices"])[1] == {1, 2}
    # a list whose + neighbours are partly absent: the absent candidates are no owners
    pick = [(1, 1, 1), (1, 2, 2)]
    want = ir.indexed_mesh(oracle_mod, field, N, RES[N], s, selection=pick)
    got = gm.IndexedMesh(s, ids=pick, normals=False, colors=False)
    assert_mesh(got, want, "+ side absent, a list")
    assert 2 < want["totals"]["owners"] < 2 + 14 and all(c[0] < 2 for c in got["owner_ids"].tolist())
    gm.close()


# ---- selections ---------------------------------------------------------------------------------------------------------------------------
def test_selections(built):
    N, s = 8, 2
    gm = built.map("sphere", N)
    field = built.field("sphere", N)
    # all, in list_chunks' order: no extras
    got = gm.IndexedMesh(s, normals=False, colors=False)
    assert got["owner_ids"].tolist() == gm.GetChunkIDs().tolist() == [list(c) for c in sorted(field)]
    assert got["totals"]["owners"] == got["totals"]["chunks"] == 64
    # a box that cuts the sphere: the extras own vertices
    box = ((1, 1, 1), (2, 1, 2))
    want = built.want("sphere", N, s, box=box)
    got = gm.IndexedMesh(s, box=box, normals=False, colors=False)
    assert_mesh(got, want, "box")
    assert want["totals"]["chunks"] == 4 and want["totals"]["owners"] > 4 and int((want["owner_table"][4:, 1] > 0).sum()) > 0
    assert gm.IndexedMeshSize(s, box=box) == want["totals"]
    zero = {"chunks": 0, "owners": 0, "cubes_meshed": 0, "vertices": 0, "triangles": 0}
    assert gm.IndexedMeshSize(s, box=((7, 7, 7), (9, 9, 9))) == zero
    # a list in a scrambled order: positions are the whole map's
    pick = [(2, 1, 1), (0, 3, 2), (1, 1, 1), (2, 2, 2), (1, 2, 1), (3, 3, 3)]
    want = built.want("sphere", N, s, selection=pick)
    got = gm.IndexedMesh(s, ids=pick, normals=False, colors=False)
    assert_mesh(got, want, "list")
    whole = built.want("sphere", N, s)
    order = [tuple(c) for c in whole["owner_ids"].tolist()]
    for row, cid in zip(got["table"].tolist(), pick):
        first, count = whole["table"][order.index(cid)].tolist()
        assert row[1] == count
        mine = got["vertices"][got["indices"][row[0]:row[0] + row[1]].reshape(-1)]
        assert mine.tobytes() == whole["vertices"][whole["indices"][first:first + count].reshape(-1)].tobytes(), cid
    # a listed id that is not resident; a duplicate
    with pytest.raises(KeyError) as e:
        gm.IndexedMesh(s, ids=[(0, 0, 0), (1, 1, 1), (9, 9, 9), (3, 3, 3)], normals=False, colors=False)
    assert "id 2 " in str(e.value)
    with pytest.raises(KeyError):
        gm.IndexedMeshSize(s, ids=[(9, 9, 9)])
    assert "id 2 " in refused(lambda: gm.IndexedMesh(s, ids=[(1, 1, 1), (0, 0, 0), (1, 1, 1)]), 1, "repeats")
    refused(lambda: gm.IndexedMeshSize(s, ids=[(1, 1, 1), (1, 1, 1)]), 1, "repeats")


def test_an_empty_map():
    gm = new_map(8)
    zero = {"chunks": 0, "owners": 0, "cubes_meshed": 0, "vertices": 0, "triangles": 0}
    assert gm.IndexedMeshSize(2) == zero
    got = gm.IndexedMesh(2)
    assert got["totals"] == zero and got["vertices"].shape == (0, 3) and got["indices"].shape == (0, 3) and got["table"].shape == (0, 2)
    gm.close()


# ---- shading ----------------------------------------------------------------------------------------------------------------------------
def shade(gm, vertices, stages):
    """chisel_hip_shade_vertices on the call's own vertices with zero normals; colours start as zeros"""
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    v = np.ascontiguousarray(vertices, np.float32)
    n, c = np.zeros_like(v), np.zeros_like(v)
    capi.check(gm.L.chisel_hip_shade_vertices(gm.h, fp(v), len(v), fp(n), fp(c), stages))
    return n, c


@pytest.mark.parametrize("family,N,s", [("thresholds", 8, 1), ("thresholds", 16, 2), ("sphere", 8, 2)])
def test_shading_is_shade_vertices(built, family, N, s):
    gm = built.map(family, N)
    plain = gm.IndexedMesh(s, normals=False, colors=False)
    assert len(plain["vertices"]) > 100
    got = gm.IndexedMesh(s, normals=True, colors=True)
    n, c = shade(gm, plain["vertices"], 3)
    assert np.array_equal(bits(got["vertices"]), bits(plain["vertices"])) and np.array_equal(got["indices"], plain["indices"])
    assert np.array_equal(bits(got["normals"]), bits(n)) and np.array_equal(bits(got["colors"]), bits(c))
    assert (n != 0).any() and (c != 0).any()
    only = gm.IndexedMesh(s, normals=True, colors=False)
    assert np.array_equal(bits(only["normals"]), bits(n)) and only["colors"] is None
    if family == "thresholds":
        assert (n == 0).all(1).any()  # (a look-up failed somewhere: the zeros stay)


def test_a_map_without_colour_refuses_colours():
    N = 8
    gm = new_map(N, color=False)
    upload(gm, vf.dense(N, B, SEED, res=RES[N]))
    refused(lambda: gm.IndexedMesh(2, colors=True), 1, "without colour")
    got = gm.IndexedMesh(2)
    assert got["totals"]["vertices"] > 0 and got["colors"] is None and got["normals"].shape == got["vertices"].shape
    gm.close()


# ---- capacities, device outputs -----------------------------------------------------------------------------------------------------------
def raw_call(gm, req, cap_v, cap_t, v, x, n, c, on_device=0, table=None, owner_table=None, owner_ids=None, totals=True):
    """-> (status, totals)"""
    t = capi.IndexedTotals(-1, -1, -1, -1, -1)
    ptr = lambda a: (a if isinstance(a, int) else a.ctypes.data) if a is not None else None
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
    rc = gm.L.chisel_hip_indexed_mesh(gm.h, C.byref(req) if req is not None else None, cap_v, cap_t, ptr(v), ptr(x), ptr(n), ptr(c), on_device,
                                      i64(table), i64(owner_table), owner_ids.ctypes.data_as(C.POINTER(C.c_int)) if owner_ids is not None else None,
                                      C.byref(t) if totals else None)
    return rc, {name: int(getattr(t, name)) for name, _ in capi.IndexedTotals._fields_}


def test_capacity_and_device_tensors(built):
    import torch
    N, s = 16, 4
    gm = built.map("dense", N)
    want = built.want("dense", N, s)
    V, T, n = want["totals"]["vertices"], want["totals"]["triangles"], want["totals"]["chunks"]
    req = capi.CoarseRequest()
    req.stride, req.stages = s, 0
    v, x = np.full((V, 3), -7.25, np.float32), np.full((T, 3), -9, np.int32)
    table, owner_table, owner_ids = np.full((n, 2), -9, np.int64), np.full((n, 2), -9, np.int64), np.full((n, 3), -9, np.int32)
    untouched = lambda: (v == -7.25).all() and (x == -9).all()
    # the size query fills totals and tables and writes nothing else, whatever pointers it is given
    rc, size = raw_call(gm, req, 0, 0, v, x, None, None, table=table, owner_table=owner_table, owner_ids=owner_ids)
    assert rc == 0 and size == want["totals"] and untouched()
    assert np.array_equal(table, want["table"]) and np.array_equal(owner_table, want["owner_table"]) and np.array_equal(owner_ids, want["owner_ids"])
    # one short in either count: refused, totals filled, nothing written
    for cap_v, cap_t, word in ((V - 1, T, "vertex capacity"), (V, T - 1, "triangle capacity"), (0, T, "vertex capacity"), (V, 0, "triangle capacity")):
        table[:], owner_table[:], owner_ids[:] = -9, -9, -9
        rc, totals = raw_call(gm, req, cap_v, cap_t, v, x, None, None, table=table, owner_table=owner_table, owner_ids=owner_ids)
        assert rc == 1 and word in gm.L.chisel_hip_last_error().decode() and totals == size, (cap_v, cap_t)
        assert untouched() and (table == -9).all() and (owner_table == -9).all() and (owner_ids == -9).all()
    # exact
    rc, totals = raw_call(gm, req, V, T, v, x, None, None, table=table, owner_table=owner_table, owner_ids=owner_ids)
    assert rc == 0
    assert_mesh({"vertices": v, "indices": x, "table": table, "owner_table": owner_table, "owner_ids": owner_ids, "totals": totals}, want, "exact capacity")
    # device tensors between sentinels: nothing outside the live rows; host arrays equal device arrays
    pad, spare = 6, 5
    dev = torch.device("cuda:0")
    host_mesh = gm.IndexedMesh(s)
    flat = {k: torch.full((pad + 3 * (V + spare) + pad,), -7.25, dtype=torch.float32, device=dev) for k in ("vertices", "normals", "colors")}
    flat["indices"] = torch.full((pad + 3 * (T + spare) + pad,), -9, dtype=torch.int32, device=dev)
    rows = {k: (T if k == "indices" else V) for k in flat}
    out = {k: t[pad:pad + 3 * (rows[k] + spare)].view(rows[k] + spare, 3) for k, t in flat.items()}
    got = gm.IndexedMesh(s, out=out)
    gm.synchronize()
    assert_mesh(got, want, "device tensors")
    for k, t in flat.items():
        h, fill = t.cpu().numpy(), (-9 if k == "indices" else -7.25)
        assert (h[:pad] == fill).all() and (h[pad + 3 * rows[k]:] == fill).all(), "a sentinel of %s was overwritten" % k
        live = h[pad:pad + 3 * rows[k]].reshape(-1, 3)
        assert live.tobytes() == np.ascontiguousarray(host_mesh[k]).tobytes(), k
    short = {"vertices": torch.zeros((V - 1, 3), dtype=torch.float32, device=dev), "indices": torch.zeros((T, 3), dtype=torch.int32, device=dev)}
    refused(lambda: gm.IndexedMesh(s, out=short), 1, "capacity")
    assert not short["vertices"].any() and not short["indices"].any()


def test_refusals(built):
    from cvids_amd import chisel as ch
    N, s = 8, 2
    gm = built.map("dense", N)
    tot = built.want("dense", N, s)["totals"]
    V, T = tot["vertices"], tot["triangles"]
    v, nn, x = np.full((V, 3), -7.25, np.float32), np.full((V, 3), -7.25, np.float32), np.full((T, 3), -9, np.int32)
    req = capi.CoarseRequest()
    req.stride, req.stages = s, 1
    err = lambda: gm.L.chisel_hip_last_error().decode()
    assert raw_call(gm, req, V, T, v, x, nn, None)[0] == 0
    v[:], nn[:], x[:] = -7.25, -7.25, -9

    class Null:
        L, h = gm.L, None
    assert raw_call(Null, req, V, T, v, x, None, None)[0] == 1 and "null" in err()
    assert raw_call(gm, None, V, T, v, x, None, None)[0] == 1 and "null" in err()
    for stride in (0, -1, 3, N + 1, 2 * N):
        bad = capi.CoarseRequest()
        bad.stride = stride
        assert raw_call(gm, bad, V, T, v, x, None, None)[0] == 1 and "stride" in err(), stride
        assert raw_call(gm, bad, 0, 0, None, None, None, None)[0] == 1 and "stride" in err(), stride
    bad = capi.CoarseRequest()
    bad.stride, bad.stages = s, 4
    assert raw_call(gm, bad, V, T, v, x, None, None)[0] == 1 and "stages" in err()
    bad.stages = 2
    assert raw_call(gm, bad, V, T, v, x, nn, None)[0] == 1 and "normals without stage bit 0" in err()
    assert raw_call(gm, req, V, T, None, None, None, None)[0] == 1 and "no output" in err()
    assert raw_call(gm, req, V, T, None, x, None, None)[0] == 1 and "indices without vertices" in err()
    assert raw_call(gm, req, V, T, None, None, nn, None)[0] == 1 and "without vertices" in err()
    assert raw_call(gm, req, -1, T, v, x, None, None)[0] == 1 and "negative" in err()
    assert raw_call(gm, req, V, -1, v, x, None, None)[0] == 1 and "negative" in err()
    assert raw_call(gm, req, 0, 0, None, None, None, None, totals=False)[0] == 1 and "totals" in err()
    # whatever chisel_hip_gather_chunks refuses of a selection
    refused(lambda: gm.IndexedMesh(s, ids=[(0, 0, 0)], box=((0, 0, 0), (1, 1, 1))), 1, "box together")
    refused(lambda: gm.IndexedMesh(s, box=((0, 2, 0), (1, 1, 1))), 1, "lo > hi")
    assert "id 1 " in refused(lambda: gm.IndexedMesh(s, ids=[(0, 0, 0), (0, hc.ID_MAX + 1, 0)]), 1, "range")
    bad = capi.CoarseRequest()
    bad.stride, bad.chunks.n_ids = s, 3
    assert raw_call(gm, bad, V, T, v, x, None, None)[0] == 1 and "without an id list" in err()
    assert (v == -7.25).all() and (nn == -7.25).all() and (x == -9).all()
    # a group, and one shard of several
    grp = shard = None
    try:
        grp = ch.Chisel((N, N, N), RES[N], True, max_chunks=64, devices=[0, 0])
        assert raw_call(grp, req, V, T, v, x, None, None)[0] == 5 and "group" in err()
        shard = new_map(N, n_shards=2, shard_rank=0)
        assert raw_call(shard, req, V, T, v, x, None, None)[0] == 5 and "one shard of several" in err()
        assert raw_call(shard, req, 0, 0, None, None, None, None)[0] == 5
    finally:
        for m in (grp, shard):
            if m is not None:
                m.close()
    assert (v == -7.25).all() and (x == -9).all()


# ---- an integrated scene; the map is only read -------------------------------------------------------------------------------------------
def test_an_integrated_scene_and_the_map_is_only_read(oracle_mod):
    import torch
    from cvids_amd import synth
    from tests.test_gpu_parity import _mk
    N, res, s = 8, 0.05, 2
    _, gm, integ = _mk(oracle_mod, N, res, True, max_chunks=1024)
    cam = small_camera(96, 72)
    cimg = synth.render_color(96, 72, 3)
    frames = make_frames("sphere_room", 3, 96, 72)
    for d, p in frames[:2]:
        gm.IntegrateDepthScanColor(integ, d, p, cam, cimg, p, cam)
    dev = torch.device("cuda:0")
    rows = 200000
    out = {k: torch.full((rows, 3), -7.25, dtype=torch.float32, device=dev) for k in ("vertices", "normals", "colors")}
    out["indices"] = torch.full((rows, 3), -9, dtype=torch.int32, device=dev)
    d, p = frames[2]
    gm.IntegrateDepthScanColor(integ, d, p, cam, cimg, p, cam)  # queued just before; no synchronise by the caller
    got = gm.IndexedMesh(s, out=out)
    gm.synchronize()
    V, T = got["totals"]["vertices"], got["totals"]["triangles"]
    assert 100 < V < rows and V < T < rows
    before, to_update, counters = fields_of(gm, N), gm.GetMeshesToUpdate().tolist(), gm.counters()
    mine, again = gm.IndexedMesh(s), gm.IndexedMesh(s)
    soup = gm.CoarseMesh(s, stages=0)
    # against the restatement of the downloaded field
    want = ir.indexed_mesh(oracle_mod, before, N, res, s)
    assert_mesh(mine, want, "integrated scene")
    assert_mesh(got, want, "integrated scene, device tensors")
    for key in ("vertices", "indices", "normals", "colors"):
        g = out[key].cpu().numpy()
        live = T if key == "indices" else V
        assert g[:live].tobytes() == mine[key].tobytes() == again[key].tobytes(), key
        assert (g[live:] == (-9 if key == "indices" else -7.25)).all(), key
    # de-indexed against the coarse mesh of the same map: the same rows, positions within the bound off the degenerate edges
    flat = mine["vertices"][mine["indices"].reshape(-1)]
    assert flat.shape == soup["vertices"].shape and np.array_equal(mine["table"] * 3, soup["table"])
    keep = ~want["degenerate"][mine["indices"].reshape(-1)]
    apart = ulps_apart(flat[keep], soup["vertices"][keep], float(np.abs(soup["vertices"]).max()))
    print("integrated scene: V %d T %d, canonical against per-cube position %.3f ulp" % (V, T, apart))
    assert apart <= 2 * MEASURED_ULPS
    assert manifold(mine["indices"], V)[1] <= {1, 2}
    # the map is only read
    after = fields_of(gm, N)
    assert sorted(before) == sorted(after)
    for cid in before:
        for a, b in zip(before[cid], after[cid]):
            assert a.tobytes() == b.tobytes(), cid
    assert sorted(gm.GetMeshesToUpdate().tolist()) == sorted(to_update) and len(to_update) > 0  # (a set: its listing has no fixed order)
    assert gm.counters() == counters
    gm.close()


def test_cycles_return_their_memory(built):
    N, s = 32, 2
    field = built.field("dense", N)
    footprint = 64 * N ** 3 * 12  # the pool of the map: 25 MB

    def cycle():
        gm = new_map(N)
        upload(gm, field)
        assert gm.IndexedMesh(s)["totals"]["vertices"] > 0
        assert gm.IndexedMesh(1, ids=[(0, 0, 0)], normals=False, colors=False)["totals"]["vertices"] > 0
        gm.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    print("free after each cycle: %s" % readings)
    assert abs(readings[0] - readings[-1]) < footprint // 2, readings


# ---- the files --------------------------------------------------------------------------------------------------------------------------
def test_both_ply_files_parse_back(built, tmp_path):
    N, s = 8, 2
    gm = built.map("sphere", N)
    mesh = gm.IndexedMesh(s, normals=False, colors=True)
    V, T = len(mesh["vertices"]), len(mesh["indices"])
    rgb = (mesh["colors"] * np.float32(255.0)).astype(np.int32)
    # text
    path = str(tmp_path / "indexed.ply")
    assert gm.SaveIndexedMeshPLY(path, s, binary=False)
    lines = open(path).read().split("\n")
    end = lines.index("end_header")
    assert "element vertex %d" % V in lines[:end] and "element face %d" % T in lines[:end]
    body = lines[end + 1:]
    verts = np.array([l.split() for l in body[:V]], np.float64)
    assert np.allclose(verts[:, :3], mesh["vertices"], rtol=1e-5, atol=1e-6) and np.array_equal(verts[:, 3:6].astype(np.int32), rgb)
    faces = np.array([l.split() for l in body[V:V + T]], np.int64)
    assert (faces[:, 0] == 3).all() and np.array_equal(faces[:, 1:], mesh["indices"])
    # binary
    path = str(tmp_path / "indexed_binary.ply")
    assert gm.SaveIndexedMeshPLY(path, s)
    raw = open(path, "rb").read()
    head, rest = raw.split(b"end_header\n", 1)
    assert b"format binary_little_endian 1.0" in head and ("element vertex %d" % V).encode() in head and ("element face %d" % T).encode() in head
    assert len(rest) == 15 * V + 13 * T
    vert = np.frombuffer(rest[:15 * V], np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    face = np.frombuffer(rest[15 * V:], np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert vert["p"].tobytes() == mesh["vertices"].tobytes() and np.array_equal(vert["c"].astype(np.int32), rgb)
    assert (face["n"] == 3).all() and np.array_equal(face["i"], mesh["indices"])
    assert not gm.SaveIndexedMeshPLY(str(tmp_path / "no_such_directory" / "x.ply"), s)


# ---- the facade -------------------------------------------------------------------------------------------------------------------------
def weighted_sum(a):
    """facade_indexed.cpp's checksum: sum of (index + 1) x word over the array's 32-bit words, modulo 2^64"""
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((w * np.arange(1, len(w) + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_the_facade_program_meshes_what_python_meshes(tmp_path):
    """cvids_amd/open_chisel/tests/facade_indexed.cpp: ChunkManager::GenerateIndexedMesh at strides 1, 2, 4, 8 -- counts and a checksum
    per array against Python's indexed mesh of the same three frames -- and the file of Chisel::SaveIndexedMeshToPLY against
    SaveIndexedMeshPLY's text form"""
    from cvids_amd import chisel as ch
    tdir = os.path.join(ROOT, "cvids_amd", "open_chisel", "tests")
    exe = os.path.join(tdir, "facade_indexed")
    subprocess.check_call(["make", "-C", tdir, "indexed"])  # (make decides whether the binary is current)
    ply = str(tmp_path / "facade.ply")
    run_ = subprocess.run([exe, ply], capture_output=True, text=True, timeout=300)
    assert run_.returncode == 0 and "facade_indexed ok" in run_.stdout, run_.stdout + run_.stderr
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
        got = gm.IndexedMesh(stride)
        n, t, sv, sn, sc, sx = lines["stride%d" % stride].split()
        assert int(n) == len(got["vertices"]) and int(t) == len(got["indices"]) and (stride > 2 or int(n) > 0), stride
        for name, want in (("vertices", sv), ("normals", sn), ("colors", sc), ("indices", sx)):
            assert int(want, 16) == weighted_sum(got[name]), (stride, name)
    mine = str(tmp_path / "python.ply")
    assert gm.SaveIndexedMeshPLY(mine, 2, binary=False)
    assert open(mine, "rb").read() == open(ply, "rb").read() and os.path.getsize(mine) > 1000
    gm.close()


# ---- the crowded hash table ---------------------------------------------------------------------------------------------------------------
def test_on_a_crowded_hash_table(built):
    """the block's chunks pushed off their home buckets by blockers that went in first, every second blocker collected afterwards --
    tombstones on the probe paths --, and blockers left on the homes of the absent + neighbours: the slot look-ups of owners and extras
    and the neighbour look-ups of the kernels walk long probes and pass tombstones"""
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
    assert r["off_home"] == len(block) and r["tomb"] == len(block) and hc.n_tombstones(t) == len(blockers[::2])
    scrambled = [block[i] for i in (5, 0, 7, 2, 3, 6, 1, 4)]
    want = built.want("thresholds", N, s, selection=scrambled)
    assert_mesh(gm.IndexedMesh(s, ids=scrambled, normals=False, colors=False), want, "crowded, a list")
    half = [c for c in block if c[0] == 0]
    assert_mesh(gm.IndexedMesh(s, ids=half, normals=False, colors=False), built.want("thresholds", N, s, selection=half), "crowded, half the block")
    box = ((0, 0, 0), (1, 1, 1))
    assert_mesh(gm.IndexedMesh(s, box=box, normals=False, colors=False), built.want("thresholds", N, s, box=box), "crowded, a box")
    gm.close()
