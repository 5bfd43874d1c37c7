"""The numpy restatement of chisel_hip_frontiers (tests/frontier_restated.py) against itself, on the CPU: scipy's labelling equals the
flood fill over a dictionary on the sparse maps and on every hand volume, the hand volumes give the clusters they were drawn for, the
builder of fields gives back the states it was handed, and the sparse maps reach what the GPU tests rely on -- so that no test can pass
on an empty answer."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import distance_restated as dr
from tests import frontier_restated as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.0625
BASE = (-2, -1, -3)


@functools.lru_cache(maxsize=None)
def sparse_wide(N, B):
    origin, dims = dr.block_window(N, B, BASE)
    return fr.wide_states(dr.sparse(N, B, fr.SPARSE_SEED, RES, base=BASE), N, origin, dims)


def same_answer(a, b):
    for key in ("state", "label", "voxels", "table", "all", "sizes"):
        assert np.array_equal(a[key], b[key]), key
    assert a["totals"] == b["totals"]


@pytest.mark.parametrize("N,B", fr.SPARSE_CASES)
def test_the_two_labellings_agree_on_the_sparse_maps(N, B):
    wide = sparse_wide(N, B)
    for connectivity in (6, 18, 26):
        for k, min_voxels in ((1, 1), (2, 16)):
            same_answer(fr.answer(wide, k, connectivity, min_voxels), fr.answer(wide, k, connectivity, min_voxels, labeller=fr.clusters_flood))


@pytest.mark.parametrize("N,B", fr.SPARSE_CASES)
def test_reach_of_the_sparse_maps(N, B):
    """the frontier voxels are 3 ... 20 % of the window; at connectivity 6 at least 100 clusters and 100 of one voxel; at connectivity
    26 at least 5 clusters; the largest cluster has at least 1000 voxels and crosses a tile border on every axis"""
    wide = sparse_wide(N, B)
    six, all26 = fr.answer(wide, 1, 6, 1), fr.answer(wide, 1, 26, 1)
    share = six["totals"]["frontier"] / six["state"].size
    singles = int((six["sizes"] == 1).sum())
    print("N %d B %d: frontier share %.4f, clusters %d (%d singles) at 6, %d at 26, largest %d" %
          (N, B, share, six["totals"]["clusters"], singles, all26["totals"]["clusters"], all26["totals"]["largest_voxels"]))
    assert 0.03 <= share <= 0.20
    assert six["totals"]["clusters"] >= 100 and singles >= 100
    assert all26["totals"]["clusters"] >= 5
    for a in (six, all26):
        big = a["table"][int(np.argmax(a["table"][:, 1]))]
        assert big[1] == a["totals"]["largest_voxels"] >= 1000 and fr.spans_tiles(big), big
        t = a["totals"]
        assert t["unknown"] + t["free"] + t["occupied"] == a["state"].size and min(t["unknown"], t["free"], t["occupied"]) > 0
        assert t["kept_clusters"] == t["clusters"] and t["kept_voxels"] == t["frontier"] == len(a["voxels"])
    # the knobs change the answer: more faces asked for, fewer frontier voxels; a size filter drops clusters and marks their voxels -2
    # (four unknown faces are rare on these maps -- the hand volumes reach them -- two are not)
    assert fr.answer(wide, 4, 26, 1)["totals"]["frontier"] < fr.answer(wide, 2, 26, 1)["totals"]["frontier"] < all26["totals"]["frontier"]
    assert fr.answer(wide, 2, 26, 1)["totals"]["frontier"] >= 100
    f16 = fr.answer(wide, 1, 6, 16)
    assert 0 < f16["totals"]["kept_clusters"] < six["totals"]["clusters"] and (f16["label"] == -2).sum() == six["totals"]["frontier"] - f16["totals"]["kept_voxels"] > 0
    assert np.array_equal(f16["label"] >= -2, np.ones_like(f16["label"], bool)) and np.array_equal(f16["label"] == -1, six["label"] == -1)
    assert (f16["table"][:, 1] >= 16).all() and (np.diff(f16["table"][:, 0]) > 0).all()


def test_table_rows_are_what_the_list_says():
    wide = sparse_wide(8, 3)
    a = fr.answer(wide, 1, 18, 2)
    v, t = a["voxels"].astype(np.int64), a["table"]
    nz, ny, nx = a["state"].shape
    lin = (v[:, 2] * ny + v[:, 1]) * nx + v[:, 0]
    assert (np.diff(lin) > 0).all() and np.array_equal(a["label"].ravel()[lin], v[:, 3])
    faces = fr.unknown_faces(wide).ravel()[lin]
    for k in (0, len(t) // 2, len(t) - 1):
        m = v[:, 3] == k
        assert t[k, 0] == lin[m].min() and t[k, 1] == m.sum() and t[k, 11] == faces[m].sum() and (faces[m] >= 1).all()
        assert np.array_equal(t[k, 2:5], v[m, :3].sum(0)) and np.array_equal(t[k, 5:8], v[m, :3].min(0)) and np.array_equal(t[k, 8:11], v[m, :3].max(0))
    c = fr.centres((10, -20, 30), t, RES)
    assert c.shape == (len(t), 3) and np.allclose(c[0], ((np.array([10, -20, 30]) + t[0, 2:5] / t[0, 1]) + 0.5) * RES, rtol=0, atol=1e-12)


@pytest.mark.parametrize("N", [8, 16])
def test_hand_volumes(N):
    base = (N - 3, -N - 5, 2 * N - 7)  # chunk borders inside every volume
    for name, (volume, expected) in fr.hand_volumes().items():
        for absent in (True, False):
            fields, origin, dims = fr.hand_case(name, N, base, absent=absent)
            wide = fr.wide_states(fields, N, origin, dims)
            assert np.array_equal(dr.window_of(wide, 1), volume), name  # the builder gives back what it was handed
            assert (wide[0] == 0).all() and (wide[:, :, -1] == 0).all()  # ... and unknown around it
            for n, connectivity in enumerate((26, 18, 6)):
                a = fr.answer(wide, 1, connectivity, 1)
                same_answer(a, fr.answer(wide, 1, connectivity, 1, labeller=fr.clusters_flood))
                if expected is not None:
                    assert a["totals"]["clusters"] == expected[n], (name, connectivity, a["totals"])
    # the serpentine: every corridor voxel a frontier voxel, one cluster that crosses every tile of the window
    fields, origin, dims = fr.hand_case("serpentine", N, base)
    a = fr.answer(fr.wide_states(fields, N, origin, dims), 1, 6, 1)
    assert a["totals"]["frontier"] == a["totals"]["free"] == a["totals"]["largest_voxels"] > 12 * 20 * 40  # (the rows, and the joints)
    tiles = {(x // fr.TILE[0], y // fr.TILE[1], z // fr.TILE[2]) for x, y, z, _ in a["voxels"].tolist()}
    assert len(tiles) == 3 * 3 * 3
    # the comb: one cluster whose teeth meet in the last row only
    fields, origin, dims = fr.hand_case("comb", N, base)
    wide = fr.wide_states(fields, N, origin, dims)
    assert fr.answer(wide, 1, 26, 1)["totals"]["clusters"] == 1
    cut = fr.wide_states(fields, N, origin, (dims[0], dims[1] - 1, dims[2]))  # without the last row: the teeth alone
    assert fr.answer(cut, 1, 26, 1)["totals"]["clusters"] == 20
    # the bridge outside the window: two clusters, with it one
    fields, origin, dims = fr.hand_case("bridge", N, base, window=((0, 0, 0), (8, 5, 3)))
    assert fr.answer(fr.wide_states(fields, N, origin, dims), 1, 26, 1)["totals"]["clusters"] == 2
    # exactly k unknown faces: a frontier voxel for min_unknown_faces <= k
    for k in range(7):
        fields, origin, dims = fr.hand_case("faces%d" % k, N, base)
        wide = fr.wide_states(fields, N, origin, dims)
        assert int(fr.unknown_faces(wide)[1, 1, 1]) == k
        for m in range(1, 7):
            assert fr.answer(wide, m, 26, 1)["totals"]["frontier"] == int(k >= m), (k, m)
    # the uniform windows
    for name, frontier in (("all_unknown", 0), ("all_occupied", 0), ("all_free", 70 * 10 * 9 - 68 * 8 * 7)):
        fields, origin, dims = fr.hand_case(name, N, base)
        t = fr.answer(fr.wide_states(fields, N, origin, dims), 1, 6, 1)["totals"]
        assert t["frontier"] == frontier and t["clusters"] == int(frontier > 0) and t[name[4:]] == 70 * 10 * 9, (name, t)


def test_frontier_mirrors_are_the_headers_size():
    from cvids_amd import capi
    assert ctypes.sizeof(capi.FrontierWindow) == 40 and ctypes.sizeof(capi.FrontierTotals) == 64
    assert "chisel_hip_frontiers" in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "chisel_hip.h")).read()
    assert re.search(r"int\s+chisel_hip_frontiers\s*\(", header)
    fields = re.search(r"typedef struct \{ int64_t ([a-z_, ]+); \} chisel_hip_frontier_totals;", header).group(1).split(", ")
    assert [n for n, _ in capi.FrontierTotals._fields_] == fields == list(fr.TOTALS)
    assert list(capi.FRONTIER_TABLE_COLUMNS) == list(fr.COLUMNS)
    checks = open(os.path.join(ROOT, "cvids_amd", "csrc", "frontier_checks.h")).read()
    tile = re.search(r"FRONTIER_TILE_X = (\d+), FRONTIER_TILE_Y = (\d+), FRONTIER_TILE_Z = (\d+)", checks).groups()
    assert tuple(int(v) for v in tile) == fr.TILE
    assert int(re.search(r"FRONTIER_MAX_VOXELS = 1ll << (\d+)", checks).group(1)) == 26 and capi.FRONTIER_MAX_VOXELS == fr.MAX_VOXELS == 1 << 26
