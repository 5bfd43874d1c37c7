"""The restatement of the mesh components (tests/mesh_components_restated.py) against scipy's connected components on
every shared case, what the cases reach, and the filter's own laws.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import indexed_mesh_restated as ir
from tests import mesh_components_restated as mc
from tests.test_coarse_mesh_restated import RES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.hand_cases()


def scipy_labels(V, idx):
    idx = mc.as_triangles(idx)
    idx = idx[mc.valid_rows(V, idx)]
    u = np.concatenate([idx[:, 0], idx[:, 0]])
    w = np.concatenate([idx[:, 1], idx[:, 2]])
    graph = sp.coo_matrix((np.ones(len(u), np.int8), (u, w)), shape=(V, V)).tocsr()
    return connected_components(graph, directed=False)


def assert_against_scipy(V, idx, what):
    got = mc.components(V, idx)
    n, labels = scipy_labels(V, idx) if V else (0, np.zeros(0, np.int32))
    assert got["totals"]["components"] == n == len(got["table"]), what
    mine = got["vertex_component"]
    # the same partition: the pairs (mine, scipy's) are a bijection
    pairs = set(zip(mine.tolist(), labels.tolist()))
    assert len(pairs) == n and len({a for a, _ in pairs}) == n and len({b for _, b in pairs}) == n, what
    # the numbering rule, on its own: a component's root is its smallest vertex, numbers ascend with the roots
    roots = got["table"][:, 0]
    assert (np.diff(roots) > 0).all(), what
    for c in range(n):
        members = np.flatnonzero(mine == c)
        assert members[0] == roots[c] and len(members) == got["table"][c, 1], (what, c)
    valid = mc.valid_rows(V, idx)
    tri = got["triangle_component"]
    assert (tri[~valid] == -1).all() and (tri[valid] == mine[mc.as_triangles(idx)[valid, 0]]).all(), what
    assert np.array_equal(got["table"][:, 2], np.bincount(tri[valid], minlength=n)), what
    assert got["totals"]["invalid_triangles"] == int((~valid).sum()) and got["table"][:, 1].sum() == V, what
    return got


@pytest.mark.parametrize("name,V,idx", CASES, ids=[c[0] for c in CASES])
def test_the_restatement_is_scipys_partition_with_the_numbering_rule(name, V, idx):
    assert_against_scipy(V, idx, name)


def test_what_the_hand_made_cases_reach():
    got = {name: mc.components(V, idx) for name, V, idx in CASES if V < 1000}
    assert got["no triangle"]["totals"]["components"] == 5 and (got["no triangle"]["table"][:, 2] == 0).all()
    assert got["a strip"]["totals"]["components"] == got["a fan"]["totals"]["components"] == got["one triangle"]["totals"]["components"] == 1
    joined = got["two strips joined by the last triangle"]
    assert joined["table"][0].tolist() == [0, 12 + 14 + 1, 23] and joined["totals"]["components"] == 1 + (40 - 27)  # (vertex 39 is the last triangle's own)
    assert got["repeated triangles"]["table"][0].tolist() == [0, 5, 9] and got["repeated triangles"]["table"][2].tolist() == [6, 4, 6]
    equal = got["equal ids"]
    assert equal["totals"]["invalid_triangles"] == 0 and [row for row in equal["table"].tolist() if row[2]] == [[1, 3, 2], [4, 2, 2], [7, 1, 1], [8, 2, 1]]
    assert (got["vertices no triangle names"]["table"][:, 2] == 0).sum() == 30 - 6 - 4
    bad = got["ids out of range"]
    assert bad["totals"]["invalid_triangles"] == 7 and bad["totals"]["triangles"] == 14 and (bad["triangle_component"] == -1).sum() == 7
    tie = got["equal largest components"]["table"]
    assert sorted(tie[:, 2].tolist())[-3:] == [5, 5, 5] and int(np.argmax(tie[:, 2])) == 0
    for V in (mc.TILE - 1, mc.TILE, mc.TILE + 1):
        for T in (mc.TILE - 1, mc.TILE, mc.TILE + 1):
            t = got["V %d T %d" % (V, T)]["table"]
            assert len(t) > 100 and (t[:, 2] == 0).sum() > 40 and (t[:, 2] > 2).sum() > 5  # alone, empty groups, crowded groups
    name, V, idx = next(c for c in CASES if c[0] == "many tiles")
    assert V // mc.TILE > mc.TILE and len(idx) // mc.TILE > mc.TILE


@pytest.mark.parametrize("name", ["a path, descending", "a path, descending, then its first triangle again", "a path, shuffled"])
def test_the_deep_path_makes_long_find_walks(name):
    """under a sequential in-order run of the device's hook rule, without any shortening of paths: listed in descending order the path
    becomes one chain, which the walk to the root afterwards (the label step) goes down whole, and a union that starts at its far end
    walks it inside the hook step; the shuffled order is measured and printed (its trees are shallow)"""
    _, V, idx = next(c for c in CASES if c[0] == name)
    in_hook, to_root, parent = mc.hook_walks(V, idx)
    print("%s: longest find walk of a union %d, longest walk to the root afterwards %d" % (name, in_hook, to_root))
    assert {v for v in range(V) if parent[v] == v} == {0}
    if name != "a path, shuffled":
        assert to_root >= mc.PATH > 64  # one chain from the last vertex down to vertex 0
    if name == "a path, descending, then its first triangle again":
        assert in_hook >= mc.PATH > 64


def test_thresholds_keep_none_some_and_all():
    _, V, idx = next(c for c in CASES if c[0] == "equal largest components")
    rows = mc.float_rows(V, 3)
    none = mc.filter_mesh(V, idx, 6, rows=rows)
    assert none["totals"]["kept_components"] == 0 and none["indices"].shape == (0, 3) and none["vertices"].shape == (0, 3) and (none["vertex_map"] == -1).all()
    some = mc.filter_mesh(V, idx, 4, rows=rows)
    assert some["totals"]["kept_components"] == 3 and some["totals"]["kept_triangles"] == 15 and some["totals"]["kept_vertices"] == 21
    every = mc.filter_mesh(V, idx, 1, rows=rows)
    assert every["totals"]["kept_components"] == 4 and every["totals"]["kept_triangles"] == 18 == len(idx)
    # the tie: the lowest number, which is not the first in the array
    one = mc.filter_mesh(V, idx, 1, True, rows=rows)
    assert one["totals"]["kept_components"] == 1 and one["totals"]["kept_triangles"] == 5 and np.flatnonzero(one["vertex_map"] >= 0).tolist() == list(range(7))
    assert one["vertices"].tobytes() == rows["vertices"][:7].tobytes()
    assert mc.filter_mesh(V, idx, 6, True)["totals"]["kept_components"] == 0


@pytest.mark.parametrize("name,V,idx", CASES, ids=[c[0] for c in CASES])
def test_filter_laws(name, V, idx):
    rows = mc.float_rows(V, 11)
    for min_triangles, largest_only in ((1, False), (3, False), (2, True)):
        once = mc.filter_mesh(V, idx, min_triangles, largest_only, rows)
        V1 = once["totals"]["kept_vertices"]
        # what is kept keeps its order and its bits
        keep_v = once["vertex_map"] >= 0
        assert np.array_equal(once["vertex_map"][keep_v], np.arange(V1))
        for key in rows:
            assert once[key].tobytes() == rows[key][keep_v].tobytes()
        keep_t = once["triangle_map"] >= 0
        assert np.array_equal(once["vertex_map"][mc.as_triangles(idx)[keep_t]], once["indices"])
        # idempotent
        twice = mc.filter_mesh(V1, once["indices"], min_triangles, largest_only, {k: once[k] for k in rows})
        assert twice["totals"]["kept_vertices"] == V1 and twice["totals"]["invalid_triangles"] == 0
        assert np.array_equal(twice["indices"], once["indices"]) and all(twice[k].tobytes() == once[k].tobytes() for k in rows)
        assert np.array_equal(twice["vertex_map"], np.arange(V1)) and np.array_equal(twice["triangle_map"], np.arange(len(once["indices"])))
        if (min_triangles, largest_only) == (1, False):  # exactly the vertices without a triangle go
            idx_ = mc.as_triangles(idx)
            named = np.zeros(V, bool)
            named[idx_[mc.valid_rows(V, idx_)].reshape(-1)] = True
            assert np.array_equal(keep_v, named) and once["totals"]["kept_triangles"] == len(idx) - once["totals"]["invalid_triangles"]


@pytest.fixture(scope="module")
def blob_meshes(oracle_mod):
    N = 8
    field = mc.blobs(N, mc.BLOCK[N], mc.SPHERES, RES[N])
    return {s: ir.indexed_mesh(oracle_mod, field, N, RES[N], s) for s in (1, 2)}


@pytest.mark.parametrize("s", [1, 2])
def test_the_blobs_are_as_many_closed_components_as_spheres(blob_meshes, s):
    mesh = blob_meshes[s]
    V, idx = mesh["totals"]["vertices"], mesh["indices"]
    got = assert_against_scipy(V, idx, "blobs s %d" % s)
    counts = got["table"][:, 2]
    print("blobs, stride %d: V %d T %d, triangles per component %s" % (s, V, len(idx), counts.tolist()))
    assert len(counts) == len(mc.SPHERES) and (counts >= 1).all() and len(set(counts.tolist())) == len(counts)
    for c in range(len(counts)):
        assert mc.closed(idx[got["triangle_component"] == c]), c
    # the sphere across the chunk corner has vertices in eight owners, the one across the face in two or more
    owner_of = np.repeat(np.arange(len(mesh["owner_table"])), mesh["owner_table"][:, 1])
    owners = [len(set(owner_of[got["vertex_component"] == c].tolist())) for c in range(len(counts))]
    assert max(owners) == 8 and sorted(owners)[-2] >= 2
    # thresholds that keep none, some and all of them
    ordered = sorted(counts.tolist())
    for min_triangles, want in ((ordered[-1] + 1, 0), (ordered[2], 3), (1, 5)):
        assert mc.filter_mesh(V, idx, min_triangles)["totals"]["kept_components"] == want
    only = mc.filter_mesh(V, idx, 1, True, {"vertices": mesh["vertices"]})
    assert only["totals"]["kept_triangles"] == ordered[-1] and mc.closed(only["indices"])


# ---- the mirrors and the header -----------------------------------------------------------------------------------------------------------
def test_components_mirrors_are_the_headers_size():
    from cvids_amd import capi
    assert ctypes.sizeof(capi.ComponentsTotals) == 64
    assert "chisel_hip_mesh_components" in capi.EXPORTS and "chisel_hip_filter_mesh" in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "chisel_hip.h")).read()
    assert re.search(r"int\s+chisel_hip_mesh_components\s*\(", header) and re.search(r"int\s+chisel_hip_filter_mesh\s*\(", header)
    fields = re.search(r"typedef struct \{ int64_t ([a-z_, ]+); \} chisel_hip_components_totals;", header).group(1).split(", ")
    assert [n for n, _ in capi.ComponentsTotals._fields_] == fields == list(mc.TOTALS)
    checks = open(os.path.join(ROOT, "cvids_amd", "csrc", "components_checks.h")).read()
    assert int(re.search(r"COMPONENTS_TILE = (\d+)", checks).group(1)) == mc.TILE
