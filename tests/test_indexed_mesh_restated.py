"""The restatement of the indexed mesh (tests/indexed_mesh_restated.py) on the CPU: the table property the definition of
USED rests on; de-indexed it is the coarse restatement row for row, positions within a measured bound; the index invariants; closed
surfaces are 2-manifolds with Euler characteristic 2; positions do not depend on the selection; extras, a far base, one cube a chunk."""
import json
import os

import numpy as np
import pytest

from tests import coarse_mesh_restated as cr
from tests import indexed_mesh_restated as ir
from tests import voxel_fields as vf
from tests.test_coarse_mesh_restated import B, RES, SEED

HERE = os.path.dirname(os.path.abspath(__file__))
N = 8
# Canonical (per-edge) against per-cube position, measured on the fields of this file: at most 1 ulp of the largest coordinate of the
# mesh on every vertex that is not on a degenerate edge (both are P + (Q - P) t with the same t up to the rounding of P and Q, which
# are built from different base voxels).  The tests assert twice the measured value.
MEASURED_ULPS = 1
SPHERE = dict(B=4, radius=9.6, centre=(15.3, 16.1, 15.7))


def sphere_field():
    return ir.sphere(N, SPHERE["B"], SPHERE["radius"], SPHERE["centre"], RES[N])


class Made:
    """fields and restatements of this module, each made once and only read afterwards"""

    def __init__(self, oracle_mod):
        self.oracle_mod, self.fields, self.meshes, self.soups = oracle_mod, {}, {}, {}

    def field(self, family, base=(0, 0, 0)):
        key = (family, tuple(base))
        if key not in self.fields:
            self.fields[key] = sphere_field() if family == "sphere" else getattr(vf, family)(N, B, SEED, res=RES[N], base=base)
        return self.fields[key]

    def indexed(self, family, s, base=(0, 0, 0), selection=None, box=None):
        key = (family, s, tuple(base), None if selection is None else tuple(selection), box)
        if key not in self.meshes:
            self.meshes[key] = ir.indexed_mesh(self.oracle_mod, self.field(family, base), N, RES[N], s, selection, box)
        return self.meshes[key]

    def coarse(self, family, s, base=(0, 0, 0)):
        key = (family, s, tuple(base))
        if key not in self.soups:
            self.soups[key] = cr.coarse_mesh(self.oracle_mod, self.field(family, base), N, RES[N], s)
        return self.soups[key]


@pytest.fixture(scope="module")
def made(oracle_mod):
    return Made(oracle_mod)


def test_a_row_names_exactly_the_edges_whose_corner_bits_differ():
    gold = json.load(open(os.path.join(HERE, "golden", "mc_triangle_table.json")))
    pairs = [tuple(p) for p in gold["edge_index_pairs"]]
    assert pairs == [tuple(p) for p in vf.EDGES]
    for index, row in enumerate(gold["triangle_table"]):
        named = {e for e in row if e != -1}
        crossed = {e for e, (a, b) in enumerate(pairs) if ((index >> a) ^ (index >> b)) & 1}
        assert named == crossed, index


def ulps_apart(a, b, scale):
    """|a - b| in ulps of `scale` (float32), the largest over the rows given"""
    if len(a) == 0:
        return 0.0
    ulp = float(np.spacing(np.float32(scale)))
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / ulp


@pytest.mark.parametrize("base", [(0, 0, 0), (400, -300, 7)], ids=("origin", "far"))
@pytest.mark.parametrize("family,s", [("dense", 1), ("dense", 2), ("thresholds", 1), ("thresholds", 2), ("thresholds", 4), ("dense", 8)])
def test_deindexed_it_is_the_coarse_restatement(made, family, s, base):
    """row for row: the same triangles per chunk, every position within twice the measured bound off the degenerate edges; s = N is one
    cube per chunk"""
    got, want = made.indexed(family, s, base), made.coarse(family, s, base)
    soup = ir.deindexed(got)
    assert soup.shape == want["vertices"].shape
    assert np.array_equal(got["table"] * 3, want["table"])
    assert got["totals"]["cubes_meshed"] == want["totals"]["cubes_meshed"] and got["totals"]["triangles"] * 3 == want["totals"]["vertices"]
    plain = ~got["degenerate"][got["indices"].reshape(-1)]
    finite = np.isfinite(want["vertices"]).all(1) & np.isfinite(soup).all(1)
    assert np.array_equal(np.isfinite(want["vertices"]).all(1), np.isfinite(soup).all(1))
    rows = plain & finite
    scale = float(np.abs(want["vertices"][rows]).max()) if rows.any() else 1.0
    apart = ulps_apart(soup[rows], want["vertices"][rows], scale)
    print("%s s %d base %s: V %d T %d, %d degenerate rows, canonical against per-cube position %.3f ulp of %.4g" % (
        family, s, base, got["totals"]["vertices"], got["totals"]["triangles"], int((~plain).sum()), apart, scale))
    assert apart <= 2 * MEASURED_ULPS
    if family == "thresholds" and s == 1:
        assert int((~plain).sum()) > 0  # (the degenerate branch is reached, and left out of the comparison)
    if s == N:
        assert got["totals"]["cubes_meshed"] <= 1
    if family == "dense" and s == 2 and base == (0, 0, 0):
        assert got["totals"]["triangles"] > 0


@pytest.mark.parametrize("family,s", [("dense", 1), ("dense", 2), ("thresholds", 1), ("thresholds", 2), ("sphere", 1), ("sphere", 2), ("sphere", 4)])
def test_index_invariants(made, family, s):
    got = made.indexed(family, s)
    V, idx = got["totals"]["vertices"], got["indices"]
    assert V == len(got["vertices"]) == int(got["owner_table"][:, 1].sum()) and len(idx) == int(got["table"][:, 1].sum()) > 0
    assert idx.min() >= 0 and idx.max() < V
    assert len(np.unique(idx)) == V  # every vertex is referenced
    assert (idx[:, 0] != idx[:, 1]).all() and (idx[:, 1] != idx[:, 2]).all() and (idx[:, 0] != idx[:, 2]).all()
    assert max(ir.edge_uses(idx).values()) <= 2
    firsts = np.concatenate([[0], np.cumsum(got["owner_table"][:, 1])[:-1]])
    assert np.array_equal(got["owner_table"][:, 0], firsts)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_the_sphere_is_a_closed_2_manifold(made, s):
    got = made.indexed("sphere", s)
    V, T = got["totals"]["vertices"], got["totals"]["triangles"]
    uses = ir.edge_uses(got["indices"])
    print("sphere s %d: V %d, E %d, T %d, %.1f bytes a triangle" % (s, V, len(uses), T, (12 * T + 12 * V) / T))
    assert set(uses.values()) == {2}
    assert V - len(uses) + T == 2 and 2 * V == T + 4 and T > 100


def test_positions_do_not_depend_on_the_selection(made):
    """one chunk in the sphere's middle: de-indexed, bit for bit the whole map's rows of that chunk; its extras own vertices and are
    ordered as defined"""
    s = 2
    whole = made.indexed("sphere", s)
    ids = [tuple(c) for c in whole["owner_ids"].tolist()]
    pick = max(range(len(ids)), key=lambda c: int(whole["table"][c][1]) if max(ids[c]) < 3 else -1)
    one = made.indexed("sphere", s, selection=(ids[pick],))
    first, count = whole["table"][pick].tolist()
    assert count > 0 and one["totals"]["triangles"] == count
    want = whole["vertices"][whole["indices"][first:first + count].reshape(-1)]
    assert ir.deindexed(one).tobytes() == want.tobytes()
    extras = [tuple(c) for c in one["owner_ids"].tolist()[1:]]
    x, y, z = ids[pick]
    assert extras == sorted((x + dx, y + dy, z + dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1) if dx + dy + dz)
    assert one["owner_ids"].tolist()[0] == list(ids[pick])
    assert int((one["owner_table"][1:, 1] > 0).sum()) > 0  # the reach: extras own vertices
    assert whole["totals"]["owners"] == whole["totals"]["chunks"]  # "all" has no extras


def test_a_box_has_its_extras_ascending(made):
    s, box = 2, ((1, 1, 1), (2, 1, 2))
    got = made.indexed("sphere", s, box=box)
    n = got["totals"]["chunks"]
    assert n == 4 and got["owner_ids"][:n].tolist() == [list(c) for c in cr.selection_all(made.field("sphere"), box)]
    extras = [tuple(c) for c in got["owner_ids"][n:].tolist()]
    assert extras == sorted(extras) and len(extras) == len(set(extras)) > 0 and not set(extras) & set(map(tuple, got["owner_ids"][:n].tolist()))
    assert got["indices"].max() == got["totals"]["vertices"] - 1
