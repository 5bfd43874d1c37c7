"""The restatement of the mesh adjacency, the vertex normals and the smoothing (tests/mesh_adjacency_restated.py) pinned
on the CPU: the rows against scipy.sparse, the flags against the edge uses, the marching-cubes valence bound from the golden table, the
normals of a sphere against the radial direction, and the smoothing's laws."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import indexed_mesh_restated as ir
from tests import mesh_adjacency_restated as ma
from tests import mesh_components_restated as mc
from tests.test_coarse_mesh_restated import RES
from tests.test_indexed_mesh_restated import SPHERE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CASES = [c for c in mc.hand_cases() if c[1] < 1000] + [("clusters", 3000, mc.clusters(3000, 3100, 5))]
BLOCKS = {8: 4, 16: 2, 32: 1}  # chunks along an edge of the 32^3 voxels of the blobs
# The largest angle between the restated vertex normal and the radial direction on the restated sphere (radius 9.6 voxels) at strides
# 1, 2, 4, in degrees, measured on the restatement by this file (test_sphere_normals_point_outwards prints them); asserted with a 25 %
# margin.  Beside them, for the README: the gradient normals the device's IndexedMesh gives the same vertices are within 2.96 / 2.90 /
# 2.81 degrees at strides 1 / 2 / 4 (mean 1.0; tools/mesh_smooth_bench.py on the device, profiles/mesh_smooth_bench.txt -- the
# restatement has no gradient normals): this field is exact, so its gradient is the sphere's normal, and the vertex normals are the facets'.
MEASURED_ANGLE = {1: 4.660, 2: 8.865, 4: 18.839}  # (means: 1.895, 3.867, 10.311)
# RMS radial deviation after 10 Taubin iterations over the one before, on the sphere with 0.3 voxels of seeded radial noise (measured
# here, printed by test_taubin_smooths_a_noisy_sphere)
MEASURED_RATIO = 0.375  # (0.30013 -> 0.11265 voxels)


def scipy_rows(V, idx):
    """-> (incidence CSR (V x T), neighbour CSR (V x V) whose data is c(v, u)), both with sorted indices"""
    idx = mc.as_triangles(idx)
    T = len(idx)
    v, t, a, b = [], [], [], []
    for k in np.flatnonzero(mc.valid_rows(V, idx)).tolist():
        ids = sorted(set(idx[k].tolist()))
        v += ids
        t += [k] * len(ids)
        for x in ids:
            for y in ids:
                if x != y:
                    a.append(x)
                    b.append(y)
    inc = sp.coo_matrix((np.ones(len(v), np.int32), (v, t)), shape=(V, max(T, 1))).tocsr()
    nbr = sp.coo_matrix((np.ones(len(a), np.int32), (a, b)), shape=(max(V, 1), max(V, 1))).tocsr()
    for m in (inc, nbr):
        m.sum_duplicates()
        m.sort_indices()
    return inc, nbr


def assert_against_scipy(V, idx, what):
    got = ma.adjacency(V, idx)
    inc, nbr = scipy_rows(V, idx)
    assert np.array_equal(got["tri_offsets"], inc.indptr[:V + 1]) and np.array_equal(got["tri_items"], inc.indices), what
    assert (inc.data == 1).all()
    assert np.array_equal(got["nbr_offsets"], nbr.indptr[:V + 1]) and np.array_equal(got["nbr_items"], nbr.indices), what
    flags = np.zeros(V, np.int32)
    for v in range(V):
        c = nbr.data[nbr.indptr[v]:nbr.indptr[v + 1]]
        flags[v] = (ma.BOUNDARY if (c == 1).any() else 0) | (ma.NONMANIFOLD if (c > 2).any() else 0) | (ma.ISOLATED if inc.indptr[v] == inc.indptr[v + 1] else 0)
    assert np.array_equal(got["flags"], flags), what
    t = got["totals"]
    assert t["incidences"] == len(inc.indices) and t["neighbors"] == len(nbr.indices) and t["max_incident"] == (np.diff(inc.indptr).max() if V else 0), what
    assert t["invalid_triangles"] == int((~mc.valid_rows(V, mc.as_triangles(idx))).sum()) and t["isolated_vertices"] == int((flags & 4 != 0).sum()), what
    return got


@pytest.mark.parametrize("name,V,idx", CASES, ids=[c[0] for c in CASES])
def test_the_rows_are_scipys(name, V, idx):
    assert_against_scipy(V, idx, name)


def test_what_the_hand_made_cases_reach():
    got = {name: ma.adjacency(V, idx) for name, V, idx in CASES}
    assert got["no triangle"]["totals"]["isolated_vertices"] == 5 and got["no triangle"]["tri_offsets"].tolist() == [0] * 6
    one = got["one triangle"]
    assert one["nbr_items"].tolist() == [1, 2, 0, 2, 0, 1] and (one["flags"] == ma.BOUNDARY).all()
    fan = got["a fan"]
    assert fan["totals"]["max_incident"] == 7 and fan["totals"]["max_neighbors"] == 8 and fan["incidence"][0] == list(range(7))
    rep = got["repeated triangles"]  # the same triangle three times: c(v, u) = 3 and more
    assert rep["totals"]["nonmanifold_vertices"] > 0 and rep["totals"]["max_incident"] > 3
    eq = got["equal ids"]  # (7, 7, 7) names nobody else: vertex 7 has a triangle and no neighbour
    assert eq["incidence"][7] == [1] and eq["neighbors"][7] == [] and eq["flags"][7] == 0 and eq["incidence"][4] == [0, 4] and eq["neighbors"][4] == [5]
    bad = got["ids out of range"]
    assert bad["totals"]["invalid_triangles"] == 7
    assert got["clusters"]["totals"]["max_incident"] <= ma.MAX_INCIDENT and got["clusters"]["totals"]["isolated_vertices"] > 700


@pytest.fixture(scope="module")
def meshes(oracle_mod):
    """the restated indexed meshes this file looks at, made once: (family, N, s, box) -> mesh"""
    made = {}
    for N in (8, 16, 32):
        field = mc.blobs(N, BLOCKS[N], mc.SPHERES, RES[N])
        for s in (1, 2):  # (at stride 4 the largest blob passes the last lattice point: its mesh is open there)
            made[("blobs", N, s, None)] = ir.indexed_mesh(oracle_mod, field, N, RES[N], s)
    field = ir.sphere(8, SPHERE["B"], SPHERE["radius"], SPHERE["centre"], RES[8])
    for s in (1, 2, 4):
        made[("sphere", 8, s, None)] = ir.indexed_mesh(oracle_mod, field, 8, RES[8], s)
    box = ((0, 0, 0), (1, 3, 3))
    made[("sphere", 8, 1, box)] = ir.indexed_mesh(oracle_mod, field, 8, RES[8], 1, box=box)
    return made


def test_the_restated_meshes_against_scipy_and_the_edge_uses(meshes):
    for key, mesh in meshes.items():
        V, idx = mesh["totals"]["vertices"], mesh["indices"]
        got = assert_against_scipy(V, idx, key)
        assert 0 < got["totals"]["max_incident"] <= 20, key  # marching cubes' bound
        # no triangle of these meshes repeats an id: c(v, u) is the number of triangles at the edge (v, u)
        uses = ir.edge_uses(idx)
        on_rim = np.zeros(V, bool)
        crowded = np.zeros(V, bool)
        for (u, w), n in uses.items():
            assert u != w
            on_rim[[u, w]] |= n == 1
            crowded[[u, w]] |= n > 2
        assert np.array_equal(got["flags"] & ma.BOUNDARY != 0, on_rim) and np.array_equal(got["flags"] & ma.NONMANIFOLD != 0, crowded), key
        family, N, s, box = key
        if box is None:
            assert got["totals"]["boundary_vertices"] == 0 and mc.closed(idx), key  # closed surfaces
        else:
            assert 10 < got["totals"]["boundary_vertices"] < V // 4, key  # the selection's open rim
        assert got["totals"]["nonmanifold_vertices"] == 0 and got["totals"]["isolated_vertices"] == 0


def test_marching_cubes_cannot_exceed_the_valence_limit():
    """an edge vertex is shared by the 4 cubes around its lattice edge, and a cube's case uses one edge in at most `most` triangles"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "mc_triangle_table.json")))
    table = next(v for k, v in gold.items() if "triangle" in k.lower() and "table" in k.lower())
    most = 0
    for row in table:
        edges = [e for e in row if e >= 0]
        assert len(edges) % 3 == 0
        triangles = [set(edges[i:i + 3]) for i in range(0, len(edges), 3)]
        for e in range(12):
            most = max(most, sum(e in t for t in triangles))
    assert most == 5 and 4 * most <= ma.MAX_INCIDENT
    checks = open(os.path.join(ROOT, "cvids_amd", "csrc", "adjacency_checks.h")).read()
    assert int(re.search(r"MESH_MAX_INCIDENT = (\d+)", checks).group(1)) == ma.MAX_INCIDENT


def sphere_centre(res):
    """(a voxel's value belongs to its centre, half a voxel behind its corner)"""
    return (np.array(SPHERE["centre"], np.float64) + 0.5) * res


def angles_to_radial(mesh, normals, res):
    centre = sphere_centre(res)
    radial = mesh["vertices"].astype(np.float64) - centre
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    n = normals.astype(np.float64)
    return np.degrees(np.arccos(np.clip((n * radial).sum(1) / np.linalg.norm(n, axis=1), -1, 1)))


@pytest.mark.parametrize("s", [1, 2, 4])
def test_sphere_normals_point_outwards(meshes, s):
    """the restated normals against the analytic radial direction: unit length, outwards (where MeshCube's face normals point), within
    the measured angle and a 25 % margin"""
    mesh = meshes[("sphere", 8, s, None)]
    V, idx = mesh["totals"]["vertices"], mesh["indices"]
    normals = ma.vertex_normals(ma.adjacency(V, idx), idx, mesh["vertices"])
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert np.abs(length - 1).max() < 1e-6
    angle = angles_to_radial(mesh, normals, RES[8])
    print("sphere, stride %d: V %d, largest angle to the radial direction %.3f degrees, mean %.3f" % (s, V, angle.max(), angle.mean()))
    assert angle.max() <= 1.25 * MEASURED_ANGLE[s]


def test_normals_of_nothing_are_zeros():
    V, idx = 6, np.array([(0, 1, 2), (3, 3, 4)], np.int32)  # vertex 5 is isolated, (3, 3, 4) has no area
    P = ma.positions(V, 1)
    n = ma.vertex_normals(ma.adjacency(V, idx), idx, P)
    assert (n[3:] == 0).all() and not np.signbit(n[3:]).any() and (np.abs(np.linalg.norm(n[:3], axis=1) - 1) < 1e-6).all()
    assert n[0].tobytes() == n[1].tobytes() == n[2].tobytes()


def test_identities_and_pins():
    for name, V, idx in CASES[:12]:
        adj = ma.adjacency(V, idx)
        P = ma.positions(V, 9)
        assert ma.smooth(adj, P, 0, 0.5, -0.53, 3).tobytes() == P.tobytes(), name
        assert ma.smooth(adj, P, 3, 0.0, 0.0, 0).tobytes() == P.tobytes(), name
        for pin in (0, 3):
            Q = ma.smooth(adj, P, 2, 0.5, -0.53, pin)
            stays = ma.pinned(adj["flags"], adj["neighbors"], pin)
            assert Q[stays].tobytes() == P[stays].tobytes(), (name, pin)
            assert ma.adjacency(V, idx, pin)["totals"]["pinned_vertices"] == int(stays.sum())
    V, idx = next((V, idx) for name, V, idx in CASES if name == "a strip")
    adj, P = ma.adjacency(V, idx), ma.positions(V, 9)
    assert (adj["flags"] == ma.BOUNDARY).all() and ma.smooth(adj, P, 5, 0.5, -0.53, ma.BOUNDARY).tobytes() == P.tobytes()
    assert (ma.smooth(adj, P, 1, 0.5, 0.0, 0) != P).any()


def test_a_flat_grid_stays_flat_and_moves_as_the_umbrella_says():
    n = 6
    P, idx = ma.flat_grid(n)
    V = len(P)
    adj = ma.adjacency(V, idx)
    inner = adj["flags"] == 0
    assert inner.sum() == (n - 1) ** 2 and (adj["flags"][~inner] == ma.BOUNDARY).all()
    assert all(len(adj["neighbors"][v]) == 6 for v in np.flatnonzero(inner))
    # the six neighbours of an inner vertex of this triangulation lie symmetrically around it: pinned rim, nothing moves
    Q = ma.smooth(adj, P, 4, 0.5, -0.53, ma.BOUNDARY)
    assert Q.tobytes() == P.tobytes()
    # lift nothing, shift one inner vertex by 1/16 along x: coordinates are small dyadic rationals, every sum is exact
    R = P.copy()
    c = 3 * (n + 1) + 3
    R[c, 0] += F(0.0625)
    Q = ma.smooth_pass(adj, R, 0.5, ma.BOUNDARY)
    assert (Q[:, 2] == F(0.5)).all()
    want = R.astype(np.float64)
    for v in np.flatnonzero(inner):
        mean = R[adj["neighbors"][v]].astype(np.float64).mean(0)
        want[v] = R[v] + 0.5 * (mean - R[v])
    # (a mean of six is not dyadic: the closed form holds to an ulp of the coordinate; the shifted vertex's own step is exact)
    assert np.abs(Q - want).max() <= np.spacing(F(1.0))
    assert Q[c, 0] == F(P[c, 0] + F(0.0625) * F(0.5)) and Q[c, 1] == P[c, 1]


def test_taubin_smooths_a_noisy_sphere(meshes):
    mesh = meshes[("sphere", 8, 1, None)]
    V, idx, res = mesh["totals"]["vertices"], mesh["indices"], RES[8]
    centre = sphere_centre(res)
    P = mesh["vertices"].astype(np.float64)
    radial = (P - centre) / np.linalg.norm(P - centre, axis=1)[:, None]
    noise = np.random.default_rng(4).standard_normal(V) * 0.3 * res
    noisy = (P + radial * noise[:, None]).astype(F)
    adj = ma.adjacency(V, idx)
    smoothed = ma.smooth(adj, noisy, 10, 0.5, -0.53, 3)
    rms = lambda Q: float(np.sqrt(((np.linalg.norm(Q.astype(np.float64) - centre, axis=1) - SPHERE["radius"] * res) ** 2).mean()))
    before, after = rms(noisy), rms(smoothed)
    print("noisy sphere: V %d, RMS radial deviation %.5f -> %.5f voxels, ratio %.3f" % (V, before / res, after / res, after / before))
    assert after < before and after / before <= 1.25 * MEASURED_RATIO
    # it does not shrink: the mean radius stays within 1 % (plain Laplacian smoothing with the same steps loses more)
    mean_r = lambda Q: float(np.linalg.norm(Q.astype(np.float64) - centre, axis=1).mean())
    assert abs(mean_r(smoothed) - mean_r(noisy)) < 0.01 * mean_r(noisy)


# ---- the mirrors and the header -----------------------------------------------------------------------------------------------------------
def test_adjacency_mirrors_are_the_headers():
    from cvids_amd import capi
    assert ctypes.sizeof(capi.AdjacencyTotals) == 96
    header = open(os.path.join(ROOT, "include", "chisel_hip.h")).read()
    for name in ("chisel_hip_mesh_adjacency", "chisel_hip_mesh_vertex_normals", "chisel_hip_smooth_mesh"):
        assert name in capi.EXPORTS and re.search(r"int\s+%s\s*\(" % name, header)
    body = re.search(r"typedef struct \{([^}]*)\} chisel_hip_adjacency_totals;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for part in body.split(";") for n in part.replace("int64_t", "").split(",") if n.strip()]
    assert [n for n, _ in capi.AdjacencyTotals._fields_] == fields == list(ma.TOTALS)
    assert int(re.search(r"#define CHISEL_HIP_MESH_MAX_INCIDENT (\d+)", header).group(1)) == capi.MESH_MAX_INCIDENT == ma.MAX_INCIDENT
    assert (capi.MESH_BOUNDARY, capi.MESH_NONMANIFOLD, capi.MESH_ISOLATED) == (ma.BOUNDARY, ma.NONMANIFOLD, ma.ISOLATED)
