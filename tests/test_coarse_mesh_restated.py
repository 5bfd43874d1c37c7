"""The restatement of the coarse mesh (tests/coarse_mesh_restated.py) against the oracle, on the CPU: at stride 1 it is
the oracle's own GenerateMesh up to the order of the triangles; at stride s it has the vertex counts of the oracle's mesh of the
decimated field; and the fields the GPU tests use reach what they are meant to reach -- counted on those very fields."""
import numpy as np
import pytest

from tests import coarse_mesh_restated as cr
from tests import voxel_fields as vf

SEED = 3      # (with it the dense field at (16, 2) reaches all 256 configurations: test_reach_of_the_dense_field)
RES = {8: 0.03, 16: 0.07, 32: 0.05}  # one non-dyadic resolution per chunk size
B = 2


def oracle_map_of(oracle_mod, field, N, res):
    om = oracle_mod.OracleMap(N, res, True)
    for cid, (s, w, c) in field.items():
        om.put_chunk(cid, s, w, c)
    om.recompute_meshes(sorted(field))
    return om


@pytest.mark.parametrize("family", ["dense", "thresholds"])
def test_stride_1_is_the_oracles_mesh(oracle_mod, family):
    """per chunk the same multiset of triangles, bit for bit: the reference walks the interior and then three border planes, so only
    the order differs"""
    N, res = 8, RES[8]
    field = getattr(vf, family)(N, B, SEED, res=res)
    om = oracle_map_of(oracle_mod, field, N, res)
    got = cr.coarse_mesh(oracle_mod, field, N, res, 1)
    assert got["ids"].tolist() == [list(c) for c in sorted(field)]
    total = 0
    for (first, count), cid in zip(got["table"].tolist(), map(tuple, got["ids"].tolist())):
        mesh = om.get_mesh(cid)
        assert count == len(mesh["vertices"]), cid
        assert cr.triangles_as_bits(got["vertices"][first:first + count]) == cr.triangles_as_bits(mesh["vertices"]), cid
        total += count
    assert total == got["totals"]["vertices"] == len(got["vertices"]) > 0


@pytest.mark.parametrize("N,s", [(16, 2), (32, 2), (32, 4)])
def test_decimation(oracle_mod, N, s):
    """the restatement at stride s has, chunk by chunk, the vertex counts of the oracle's mesh of the decimated field in a map of
    chunk edge N / s and resolution s res"""
    res = RES[N]
    field = vf.thresholds(N, B, SEED, res=res)
    got = cr.coarse_mesh(oracle_mod, field, N, res, s)
    small = cr.decimate(field, N, s)
    om = oracle_map_of(oracle_mod, small, N // s, float(np.float32(s) * np.float32(res)))
    counts = {tuple(cid): int(c) for cid, (_, c) in zip(got["ids"].tolist(), got["table"].tolist())}
    want = {cid: len(om.get_mesh(cid)["vertices"]) for cid in small}
    assert counts == want
    assert sum(want.values()) > 0


def test_reach_of_the_dense_field():
    """(N, s) = (16, 2), B = 2: 15^3 fully observed cubes, all 256 configurations among them, the rest skipped for an absent neighbour;
    corners in 2, 4 and 8 chunks"""
    N, s = 16, 2
    r = cr.reach(vf.dense(N, B, SEED, res=RES[N]), N, s)
    assert r["meshed"] == 3375 and r["low_weight"] == 0 and r["absent"] == 8 * 8 ** 3 - 3375
    assert len(r["configurations"]) == 256, len(r["configurations"])
    assert all(r["span"][k] > 0 for k in (1, 2, 4, 8)), r["span"]


@pytest.mark.parametrize("N,s", [(8, 1), (8, 2), (8, 4), (8, 8), (16, 1), (16, 2), (16, 4), (16, 16), (32, 2), (32, 8), (32, 32)])
@pytest.mark.parametrize("family", ["dense", "thresholds"])
def test_reach_of_every_case(family, N, s):
    """every field of the GPU tests: cubes skipped for an absent neighbour; the thresholds fields: cubes skipped for a weight; corners
    in 2, 4 and 8 chunks (at s = N every meshed cube has its corners in eight)"""
    r = cr.reach(getattr(vf, family)(N, B, SEED, res=RES[N]), N, s)
    assert r["absent"] > 0
    if family == "thresholds":
        assert r["low_weight"] > 0
    else:
        assert r["meshed"] == (B * N // s - 1) ** 3
    if s == N:
        assert r["span"][8] == r["meshed"]
    else:  # (one cube of the block has its corners in eight chunks: in a thresholds field its weights may reject it)
        assert all(r["span"][k] > 0 for k in ((2, 4, 8) if family == "dense" else (2, 4))), r["span"]


def test_tiny_crossing_edges_are_reached():
    """crossing edges under InterpolateVertex's 1e-6 on a thresholds field of the GPU tests"""
    N, s = 16, 2
    assert cr.reach(vf.thresholds(N, B, SEED, res=RES[N]), N, s)["tiny_edges"] > 0
