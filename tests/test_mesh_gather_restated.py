"""tests/mesh_gather_restated.py on hand values (no GPU): the marker-colour rule for a normal equal to light0, opposite to it,
orthogonal to both lights, a NaN normal and a sum that exceeds 1; the concatenation's table against a naive loop."""
import numpy as np

from tests import mesh_gather_restated as R

F = np.float32


def test_marker_rule_on_hand_values():
    l0, l1 = (F(0.6), F(0.0), F(0.8)), (F(0.0), F(1.0), F(0.0))
    diffuse, ambient = F(0.5), F(0.2)
    n = np.array([[0.6, 0.0, 0.8],      # = light0: d0 = 0.36 + 0.64 (in fp32), d1 = 0
                  [-0.6, 0.0, -0.8],    # opposite: both terms clamp to 0 -> ambient alone
                  [0.8, 0.0, -0.6],     # orthogonal to both lights -> ambient alone (d0 = 0.48 - 0.48 = 0 exactly in fp32)
                  [np.nan, 0.0, 1.0],   # a NaN normal: s_k = 0 -> ambient alone
                  [0.0, 5.0, 5.0]],     # d0 = 4, d1 = 5: 2 + 2.5 + 0.2 > 1 -> 1
                 F)
    got = R.marker_rgba(n, l0, l1, diffuse, ambient)
    assert got.dtype == F and got.shape == (5, 4)
    d0 = F(F(F(0.6) * F(0.6)) + F(F(0.0) * F(0.0))) + F(F(0.8) * F(0.8))
    first = F(F(F(d0 * diffuse) + F(0.0)) + ambient)
    want = np.array([first, ambient, ambient, ambient, F(1.0)], F)
    for k in range(3):
        assert np.array_equal(got[:, k].view(np.uint32), want.view(np.uint32)), (got[:, k], want)
    assert np.array_equal(got[:, 3], np.ones(5, F))
    assert not np.isnan(got).any()
    # the light is used as given: a longer light0 gives a brighter vertex
    assert R.marker_rgba(n[:1], (F(1.2), F(0.0), F(1.6)), l1, F(0.25), ambient)[0, 0] == first


def test_gather_is_the_concatenation_with_its_table():
    rng = np.random.default_rng(5)
    sizes = [(9, 2), (0, 0), (3, 1), (0, 3), (30, 7)]
    meshes = [{"vertices": rng.random((v, 3), F), "normals": rng.random((v, 3), F), "colors": None, "grids": rng.random((g, 3), F)} for v, g in sizes]
    lights = {"light0": (0.1, 0.2, 0.3), "light1": (-0.5, 0.2, 0.2), "diffuse": 0.5, "ambient": 0.2}
    res = R.gather(meshes, lights)
    v = g = 0
    for i, (m, (nv, ng)) in enumerate(zip(meshes, sizes)):  # the naive loop
        row = res["table"][i]
        assert tuple(row) == ((v, nv, g, ng) if nv + ng else (0, 0, 0, 0))
        assert np.array_equal(res["vertices"][v:v + nv], m["vertices"]) and np.array_equal(res["normals"][v:v + nv], m["normals"])
        assert np.array_equal(res["grids"][g:g + ng], m["grids"])
        assert np.array_equal(res["rgba"][v:v + nv], R.marker_rgba(m["normals"], **lights))
        v, g = v + nv, g + ng
    assert len(res["vertices"]) == v and len(res["grids"]) == g and res["colors"] is None
    for m in meshes:
        m["colors"] = rng.random((len(m["vertices"]), 3), F)
    res = R.gather(meshes, lights)
    assert np.array_equal(res["rgba"][:, :3], res["colors"]) and (res["rgba"][:, 3] == 1).all()
    empty = R.gather([])
    assert empty["table"].shape == (0, 4) and empty["vertices"].shape == (0, 3)


def test_default_lights_are_chisel_servers():
    """lightDir (0.8, -0.2, 0.7) normalised twice in fp32, lightDir1 unnormalised, diffuse 0.5, ambient 0.2"""
    from cvids_amd.chisel import Chisel, marker_light_dir
    v = np.array([0.8, -0.2, 0.7], F)
    for _ in range(2):
        v = (v / np.sqrt(F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))).astype(F)
    assert tuple(F(x) for x in marker_light_dir()) == tuple(v)
    assert abs(float(np.linalg.norm(np.asarray(marker_light_dir(), np.float64))) - 1.0) < 1e-6
    L = Chisel.MARKER_LIGHTS
    assert L["light1"] == (-0.5, 0.2, 0.2) and L["diffuse"] == 0.5 and L["ambient"] == 0.2
