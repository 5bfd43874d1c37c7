"""chisel_hip_travel_field and chisel_hip_travel_path on the GPU against their definition (DESIGN.md 3.19 "Travel field").

The answer is a set of integers, so every comparison is array_equal over every element -- cost, step, state, the group table and the
totals except the diagnostics "rounds" and "tile_visits" -- against the restatement (tests/travel_restated.py: scipy's Dijkstra on the
explicit grid graph, which tests/test_travel_restated.py pins to a numpy relaxation and a heapq Dijkstra) run over the map as it was
uploaded or as GetChunkIDs / GetChunk read it back.  A stated reach only keeps a comparison from passing on an empty case."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from cvids_amd import synth
from tests import distance_restated as dr
from tests import frontier_restated as fr
from tests import test_gpu_render as tgr
from tests import travel_restated as tr
from tests.common import compare_fields, free_bytes, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.0625
BASE = (-2, -1, -3)
B_OF = {8: 3, 16: 2, 32: 2}
W, H = tgr.W, tgr.H
KEYS = ("cost", "step", "state")


def new_map(N, res=RES, color=False, max_chunks=256, **kw):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), res, color, max_chunks=max_chunks, **kw)


@functools.lru_cache(maxsize=None)
def sparse_field(N):
    return dr.sparse(N, B_OF[N], fr.SPARSE_SEED, RES, base=BASE)


@functools.lru_cache(maxsize=None)
def sparse_map(N):
    """the hand-built sparse map of chunk edge N (only ever read)"""
    gm = new_map(N)
    upload(gm, sparse_field(N))
    return gm


def equal_answers(got, want, what, keys=KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, "%s: %s is %s %s, not %s %s" % (
            what, key, got[key].dtype, got[key].shape, want[key].dtype, want[key].shape)
        assert np.array_equal(got[key], want[key]), "%s: %s differs at %d of %d places" % (what, key, int((got[key] != want[key]).sum()), want[key].size)
    if want["table"] is None:
        assert got["table"] is None, what
    else:
        assert got["table"].dtype == np.int64 and np.array_equal(got["table"], want["table"]), "%s: table %s, not %s" % (what, got["table"], want["table"])
    totals = {k: v for k, v in got["totals"].items() if k not in tr.DIAGNOSTICS}
    assert totals == want["totals"], "%s: totals %s, not %s" % (what, totals, want["totals"])
    assert set(got["totals"]) - set(totals) == set(tr.DIAGNOSTICS)


def check_window(gm, fields, N, origin, dims, seeds, connectivity=26, step_cost=(10, 14, 17), max_cost=1 << 30, clearance=0, unknown_is_obstacle=False,
                 offset=0.0, targets=None, n_groups=0, what="", traversable=None):
    """every output of one call against the restatement over `fields` -> (the call's answer, the restatement's)"""
    got = gm.TravelField(origin, dims, seeds, connectivity, step_cost, max_cost, clearance, unknown_is_obstacle, offset, state=True, targets=targets,
                         n_groups=n_groups)
    state, trav = traversable if traversable is not None else tr.traversable(fields, N, origin, dims, clearance, unknown_is_obstacle, offset)
    want = tr.answer(state, trav, seeds, connectivity, step_cost, max_cost, targets, n_groups)
    what = "%s N %d origin %s dims %s connectivity %d costs %s max_cost %d clearance %d/%s" % (what, N, origin, dims, connectivity, step_cost, max_cost,
                                                                                              clearance, unknown_is_obstacle)
    equal_answers(got, want, what)
    return got, want


def volume_case(gm, volume, N, base):
    """a state volume uploaded into the emptied map -> (fields, origin, dims)"""
    fields = fr.fields_from_states(volume, N, base)
    gm.Reset()
    upload(gm, fields)
    return fields, tuple(int(v) for v in base), tuple(int(v) for v in volume.shape[::-1])


# ---- 1. tile seams ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 16, 32])
def test_tile_seams(N):
    """two free voxels, (15, 15, 7) and its face, edge or corner neighbour across the tile border, the seed on either: the other is
    reached exactly when the connectivity has the move, through the flag on the face, edge or corner neighbour of the tile"""
    gm = new_map(N, max_chunks=512)
    for kind, level in (("face", 1), ("edge", 2), ("corner", 3)):
        volume, seeds = tr.seam(kind)
        other = [tuple(int(a[1]) for a in np.nonzero(volume == fr.FREE))[::-1]]
        assert seeds == [(15, 15, 7)] and other != seeds
        fields, origin, dims = volume_case(gm, volume, N, (N - 15, 3 - N, 2 * N - 7))
        for seed in (seeds, other):
            for connectivity, has in ((6, 1), (18, 2), (26, 3)):
                got, _ = check_window(gm, fields, N, origin, dims, seed, connectivity, what="seam " + kind)
                t = got["totals"]
                assert t["traversable"] == 2 and t["seeds_used"] == 1 and t["reached"] == (2 if has >= level else 1), (kind, connectivity, t)
                if has >= level:
                    assert t["tile_visits"] >= 2 and t["rounds"] >= 2 and t["largest_cost"] == (10, 14, 17)[level - 1], t
        longer = volume.copy()
        longer[7, 15, 14] = fr.FREE  # the seed inside the tile: the rim voxel (15, 15, 7) is lowered by a round, which wakes the neighbour
        fields, origin, dims = volume_case(gm, longer, N, (N - 15, 3 - N, 2 * N - 7))
        for connectivity, has in ((6, 1), (18, 2), (26, 3)):
            got, _ = check_window(gm, fields, N, origin, dims, [(14, 15, 7)], connectivity, what="seam behind a step " + kind)
            t = got["totals"]
            assert t["traversable"] == 3 and t["reached"] == (3 if has >= level else 2) and (has < level or (t["rounds"] >= 2 and t["tile_visits"] >= 2)), (kind, connectivity, t)
    gm.close()


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 16])
def test_window_shapes(N):
    """ragged tiles on every axis; seeds at (0, 0, 0), at the last voxel and on either side of the first tile's far corner"""
    rng = np.random.default_rng(11)
    gm = new_map(N, max_chunks=512)
    reached = 0
    for dims in ((70, 1, 1), (1, 1, 9), (17, 17, 9), (16, 16, 8), (40, 36, 12)):
        nx, ny, nz = dims
        volume = rng.choice(np.array([fr.UNKNOWN, fr.FREE, fr.OCCUPIED], np.uint8), size=(nz, ny, nx), p=[0.1, 0.8, 0.1])
        seeds = [s for s in ((0, 0, 0), (nx - 1, ny - 1, nz - 1), (15, 15, 7), (16, 16, 8)) if all(s[a] < dims[a] for a in range(3))]
        for s in seeds:
            volume[s[2], s[1], s[0]] = fr.FREE
        fields, origin, _ = volume_case(gm, volume, N, (3 - N, N + 5, -7))
        for connectivity in (6, 18, 26):
            for one in seeds + [seeds]:
                got, _ = check_window(gm, fields, N, origin, dims, one if isinstance(one, list) else [one], connectivity, (3, 4, 5), what="shape")
                reached += got["totals"]["reached"]
    assert reached > 50000
    gm.close()


# ---- 3. many rounds -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["serpentine", "comb"])
def test_many_rounds(name):
    """a one-voxel corridor that crosses tile borders again and again, the seed at its first voxel: the host loop runs several batches"""
    from cvids_amd import capi
    N = 8
    gm = new_map(N, max_chunks=512)
    volume, seeds = tr.cases()[name]
    fields, origin, dims = volume_case(gm, volume, N, (N - 3, -N - 5, 2 * N - 7))
    traversable = tr.traversable(fields, N, origin, dims)
    for step_cost in tr.COST_SETS:
        for connectivity in (6, 26):
            got, _ = check_window(gm, None, N, origin, dims, seeds, connectivity, step_cost, what=name, traversable=traversable)
            t = got["totals"]
            print("%s connectivity %d costs %s: rounds %d tile visits %d largest %d" % (name, connectivity, step_cost, t["rounds"], t["tile_visits"], t["largest_cost"]))
            assert t["reached"] == t["traversable"] == int((volume == fr.FREE).sum())
            if name == "serpentine":
                assert t["rounds"] > 2 * capi.TRAVEL_ROUNDS_PER_WAIT, t
    gm.close()


# ---- 4. ties, max_cost, seeds -------------------------------------------------------------------------------------------------------------
def test_ties_in_an_open_box():
    N = 16
    gm = new_map(N, max_chunks=512)
    volume, seeds = tr.cases()["open_box"]
    fields, origin, dims = volume_case(gm, volume, N, (5, -9, 3))
    for connectivity in (6, 18, 26):
        for step_cost in tr.COST_SETS:
            got, want = check_window(gm, fields, N, origin, dims, seeds, connectivity, step_cost, what="open box")
    half = got["cost"][:, :, :20].max(), got["cost"][:, :, 20:].max()
    assert got["totals"]["reached"] == volume.size and abs(int(half[0]) - int(half[1])) <= 17  # the costs meet in the middle
    step = tr.step_of(want["cost"], 26, tr.COST_SETS[-1])
    c = want["cost"].astype(np.int64)  # voxels with more than one fitting move: the smallest code wins
    fits = np.zeros(c.shape, np.int64)
    for o in tr.offsets(26):
        dst, src = tr._views(c.shape, o)
        fits[dst] += (c[src] >= 0) & (c[src] + tr.move_cost(o, tr.COST_SETS[-1]) == c[dst])
    many = int((fits > 1).sum())
    assert many > 1000 and np.array_equal(got["step"], step)
    gm.close()


def test_max_cost_cuts():
    N = 8
    gm = new_map(N, max_chunks=512)
    volume, seeds = tr.cases()["small_serpentine"]
    fields, origin, dims = volume_case(gm, volume, N, (1, 2, 3))
    traversable = tr.traversable(fields, N, origin, dims)
    full = int((volume == fr.FREE).sum())
    for max_cost, cut in ((0, True), (1, True), (9, True), (10, True), (1555, True), (1 << 30, False)):
        for connectivity in (6, 26):
            got, _ = check_window(gm, None, N, origin, dims, seeds, connectivity, max_cost=max_cost, what="max_cost", traversable=traversable)
            t = got["totals"]
            assert t["traversable"] == full and (t["reached"] < full) == cut and t["largest_cost"] <= max_cost, t
            assert t["reached"] == (1 if max_cost < 10 else t["reached"]) and (max_cost != 1555 or t["reached"] > 50)
    gm.close()


def test_seeds():
    """a seed on an occupied voxel, on an unknown one, all seeds ignored, duplicates, a thousand seeds"""
    N = 8
    gm = new_map(N, max_chunks=512)
    volume = tr.walled()
    fields, origin, dims = volume_case(gm, volume, N, (-4, 6, -5))
    occupied, unknown, free = (6, 20, 6), (2, 11, 6), (1, 1, 1)
    assert volume[6, 20, 6] == fr.OCCUPIED and volume[6, 11, 2] == fr.UNKNOWN and volume[1, 1, 1] == fr.FREE
    got, _ = check_window(gm, fields, N, origin, dims, [occupied, free, unknown], what="mixed seeds")
    assert got["totals"]["seeds_used"] == 1 and got["totals"]["seeds_ignored"] == 2 and got["totals"]["reached"] > 10000
    got, _ = check_window(gm, fields, N, origin, dims, [occupied, unknown], what="all ignored")
    t = got["totals"]
    assert t["seeds_used"] == 0 and t["reached"] == 0 and t["largest_cost"] == -1 and (got["cost"] == -1).all() and (got["step"] == 255).all() and t["rounds"] == 0
    got, _ = check_window(gm, fields, N, origin, dims, [free] * 5 + [(38, 34, 10)] * 3, 18, what="duplicates")
    assert got["totals"]["seeds_used"] == 8 and (got["step"] == 13).sum() == 2
    rng = np.random.default_rng(3)
    thousand = np.stack([rng.integers(0, dims[a], 1000) for a in range(3)], axis=1)
    got, _ = check_window(gm, fields, N, origin, dims, thousand, 26, (3, 4, 5), what="a thousand seeds")
    assert got["totals"]["seeds_used"] > 700 and got["totals"]["seeds_ignored"] > 50
    gm.close()


# ---- 5. clearance, integrated maps, the hand volumes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 16, 32])
def test_clearance_on_the_sparse_maps(N):
    """windows that overhang the block: obstacles beyond the window's rim keep free voxels from being traversable"""
    gm, fields = sparse_map(N), sparse_field(N)
    lo = np.array(BASE) * N
    origin, dims = tuple(int(v) for v in lo + (4, 5, 6)), (17, 15, 13)  # inside the block: the map goes on beyond every rim
    for clearance in (1, 2, 3):
        for flag in (False, True):
            state, trav = tr.traversable(fields, N, origin, dims, clearance, flag)
            z, y, x = (a[:4] for a in np.nonzero(trav))
            seeds = np.stack([x, y, z], axis=1) if len(x) else np.array([[0, 0, 0]])
            got, _ = check_window(gm, None, N, origin, dims, seeds, 26, clearance=clearance, unknown_is_obstacle=flag, what="clearance", traversable=(state, trav))
            # reach: a free voxel that only obstacles outside the window keep from being traversable
            st = dr.states(fields, N, origin, dims, clearance, 0.0)
            inner = st.copy()
            rim = np.ones(st.shape, bool)
            rim[clearance:-clearance, clearance:-clearance, clearance:-clearance] = False
            inner[rim] = fr.FREE
            without = (state == fr.FREE) & (dr.separable(inner, clearance, flag) == -1)
            assert (without & ~trav).any() and got["totals"]["traversable"] < got["totals"]["free"], (clearance, flag)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    got, _ = check_window(gm, fields, N, origin, dims, [(dims[0] // 2, dims[1] // 2, 3)], 18, clearance=2, what="block window")
    got0, _ = check_window(gm, fields, N, origin, dims, [(dims[0] // 2, dims[1] // 2, 3)], 18, clearance=0, what="block window")
    assert got0["totals"]["traversable"] > got["totals"]["traversable"] > 0


def test_an_integrated_map():
    """three frames of sphere_room; the window holds the camera's voxel and the surface point its central pixel sees.  The camera's
    own voxel is a seed (the frames leave it unobserved: it is ignored and counted), the first free voxel along the central ray another"""
    scene, N, res, trunc = "sphere_room", 16, 0.03, ("inverse", 2.0)
    gm = tgr.gpu_map(scene, N, res, trunc, 3, True, False)
    depth0, pose0 = next(iter(synth.stream(scene, 1, W, H)))
    fx, fy, cx, cy = synth.intrinsics(W, H)
    z = float(depth0[H // 2, W // 2])
    p0 = np.asarray(pose0, np.float64)
    hit = p0[:3, :3] @ np.array([(W // 2 + 0.5 - cx) / fx * z, (H // 2 + 0.5 - cy) / fy * z, z]) + p0[:3, 3]
    cam, hit = np.floor(p0[:3, 3] / res).astype(int), np.floor(hit / res).astype(int)
    lo, hi = np.minimum(cam, hit) - (24, 20, 6), np.maximum(cam, hit) + (24, 20, 12)
    origin, dims = tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)
    assert dims[0] * dims[1] * dims[2] < 300000
    fields = gm.fields()
    state, _ = tr.traversable(fields, N, origin, dims)
    at = cam - lo
    column = np.flatnonzero(state[:, at[1], at[0]] == fr.FREE)  # (the central ray runs along +z)
    assert len(column) > 0
    seeds = [tuple(int(v) for v in at), (int(at[0]), int(at[1]), int(column[0]))]
    for connectivity, clearance in ((26, 0), (6, 0), (18, 2)):
        got, _ = check_window(gm, fields, N, origin, dims, seeds, connectivity, clearance=clearance, what=scene)
        print("%s connectivity %d clearance %d: %s" % (scene, connectivity, clearance, got["totals"]))
    free = gm.TravelField(origin, dims, seeds, 26)["totals"]
    assert free["seeds_used"] >= 1 and free["seeds_used"] + free["seeds_ignored"] == 2 and free["reached"] > 1000 and free["occupied"] > 0, free
    gm.close()


def test_hand_volumes_of_one_state():
    N = 8
    gm = new_map(N, max_chunks=512)
    for name in ("all_unknown", "all_occupied", "all_free"):
        fields, origin, dims = fr.hand_case(name, N, (N - 3, -N - 5, 2 * N - 7))
        gm.Reset()
        upload(gm, fields)
        for connectivity in (6, 26):
            got, _ = check_window(gm, fields, N, origin, dims, [(0, 0, 0), (69, 9, 8)], connectivity, what=name)
            assert got["totals"]["reached"] == (70 * 10 * 9 if name == "all_free" else 0)
    gm.close()


# ---- 6. targets ---------------------------------------------------------------------------------------------------------------------------
def test_frontier_voxels_as_targets_without_a_host_copy():
    import torch
    N = 16
    gm, fields = sparse_map(N), sparse_field(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    dev = torch.device("cuda:0")
    size = gm.FrontiersSize(origin, dims, 1, 26, 4)
    rows = torch.full((size["kept_voxels"], 4), 77, dtype=torch.int32, device=dev)
    front = gm.Frontiers(origin, dims, 1, 26, 4, out={"voxels": rows})
    K = front["totals"]["kept_clusters"]
    state, trav = tr.traversable(fields, N, origin, dims)
    z, y, x = (a[:1] for a in np.nonzero(trav))
    seeds = [(int(x[0]), int(y[0]), int(z[0]))]
    shape = (dims[2], dims[1], dims[0])
    out = {"cost": torch.full(shape, 77, dtype=torch.int32, device=dev)}
    got = gm.TravelField(origin, dims, seeds, 26, targets=rows, n_groups=K, out=out)
    gm.synchronize()
    want = tr.answer(state, trav, seeds, 26, targets=rows.cpu().numpy(), n_groups=K)
    assert np.array_equal(got["table"], want["table"]) and np.array_equal(out["cost"].cpu().numpy(), want["cost"])
    assert {k: v for k, v in got["totals"].items() if k not in tr.DIAGNOSTICS} == want["totals"]
    assert K > 3 and (got["table"][:, 1] > 0).any() and got["totals"]["targets_reached"] > 100 and got["totals"]["targets_ignored"] == 0
    host = gm.TravelField(origin, dims, seeds, 26, targets=rows.cpu().numpy(), n_groups=K)  # the same rows from host memory
    assert np.array_equal(host["table"], got["table"]) and np.array_equal(host["cost"], want["cost"])


def test_target_rows_ignored_unreached_and_tied():
    N = 8
    gm = new_map(N, max_chunks=512)
    volume, seeds = tr.cases()["open_box"]
    volume = volume.copy()
    volume[:, :, 30] = fr.OCCUPIED  # the columns behind it are not reached from (0, 0, 0)
    fields, origin, dims = volume_case(gm, volume, N, (5, -9, 3))
    seeds = [(0, 0, 0)]
    targets = np.array([(3, 0, 0, 0), (0, 3, 0, 0), (0, 0, 3, 0), (5, 5, 5, 0),      # group 0: a tie of three for the least cost
                        (35, 3, 3, 1), (36, 4, 4, 1),                              # group 1: no reached row
                        (40, 0, 0, 2), (0, -1, 0, 2), (0, 0, 12, 2), (1, 1, 1, 2),  # three rows outside the window
                        (1, 1, 1, -1), (1, 1, 1, 4), (2, 2, 2, 3)], np.int32)      # two groups out of range
    got, want = check_window(gm, fields, N, origin, dims, seeds, 6, (1, 1, 1), targets=targets, n_groups=4, what="targets")
    t = got["totals"]
    assert t["targets_ignored"] == 5 and t["targets_reached"] == 6
    assert got["table"].tolist() == [[4, 4, 3, 3], [2, 0, -1, -1], [1, 1, 3, (1 * 36 + 1) * 40 + 1], [1, 1, 6, (2 * 36 + 2) * 40 + 2]]
    only = gm.TravelField(origin, dims, seeds, 6, (1, 1, 1), cost=False, step=False, targets=targets, n_groups=4)  # the table alone
    assert only["cost"] is None and only["step"] is None and np.array_equal(only["table"], got["table"])
    gm.close()


# ---- 7. plumbing ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def guarded(shape, dtype, dev):
    import torch
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), 77, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def sentinels_kept(whole):
    return bool((whole[:GUARD] == 77).all()) and bool((whole[-GUARD:] == 77).all())


def sparse_request(N):
    fields = sparse_field(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    state, trav = tr.traversable(fields, N, origin, dims)
    z, y, x = np.nonzero(trav)
    k = len(x) // 2
    return origin, dims, [(int(x[0]), int(y[0]), int(z[0])), (int(x[k]), int(y[k]), int(z[k]))], (state, trav)


def test_host_arrays_equal_device_tensors_and_the_call_twice():
    import torch
    N = 16
    gm = sparse_map(N)
    origin, dims, seeds, traversable = sparse_request(N)
    shape = (dims[2], dims[1], dims[0])
    dev = torch.device("cuda:0")
    host, _ = check_window(gm, None, N, origin, dims, seeds, 18, traversable=traversable, what="host arrays")
    assert host["totals"]["reached"] > 1000
    tensors = {name: guarded(shape, dtype, dev) for name, dtype in (("cost", torch.int32), ("step", torch.uint8), ("state", torch.uint8))}
    torch.cuda.synchronize()
    out = {name: t for name, (_, t) in tensors.items()}
    res = gm.TravelField(origin, dims, seeds, 18, out=out)
    gm.synchronize()
    for name in KEYS:
        assert res[name] is out[name] and np.array_equal(out[name].cpu().numpy(), host[name]) and sentinels_kept(tensors[name][0]), name
    assert {k: v for k, v in res["totals"].items() if k not in tr.DIAGNOSTICS} == {k: v for k, v in host["totals"].items() if k not in tr.DIAGNOSTICS}
    for name in KEYS:  # each output alone
        whole, t = guarded(shape, out[name].dtype, dev)
        torch.cuda.synchronize()
        gm.TravelField(origin, dims, seeds, 18, out={name: t})
        gm.synchronize()
        assert np.array_equal(t.cpu().numpy(), host[name]) and sentinels_kept(whole), name
    gm.TravelField((0, 0, 0), (20, 20, 20), [(1, 1, 1)], 6, clearance=2)  # (another window through the same scratch in between)
    again = gm.TravelField(origin, dims, seeds, 18, state=True)
    for name in KEYS:
        assert again[name].tobytes() == host[name].tobytes(), name
    # TravelPath on the device result equals the restated walk, and its summed move costs are the cost
    far = np.unravel_index(int(np.argmax(host["cost"])), host["cost"].shape)
    start = (int(far[2]), int(far[1]), int(far[0]))
    path = gm.TravelPath(out["step"], start)
    assert path.dtype == np.int32 and np.array_equal(path, tr.walk(host["step"], start)) and len(path) > 10
    assert tr.walk_cost(path, (10, 14, 17)) == int(host["cost"][far]) and host["cost"][path[-1, 2], path[-1, 1], path[-1, 0]] == 0


def test_the_call_only_reads_the_map():
    N = 8
    gm = new_map(N)
    upload(gm, sparse_field(N))
    origin, dims, seeds, _ = sparse_request(N)
    fields, table, counters = gm.fields(), gm.hash_table(), gm.counters()
    for connectivity, clearance in ((6, 0), (26, 2)):
        gm.TravelField(origin, dims, seeds, connectivity, clearance=clearance, state=True)
    compare_fields(fields, gm.fields(), gm.V, False)
    after = gm.hash_table()
    assert set(after) == set(table) and all(np.array_equal(np.asarray(after[k]), np.asarray(table[k])) for k in table)
    assert gm.counters() == counters
    gm.close()
    args = ("sphere_room", 16, 0.03, ("inverse", 2.0), 4, True, True)
    a, b = tgr.gpu_map(*args), tgr.gpu_map(*args)
    a.UpdateMeshes()
    b.UpdateMeshes()
    a.TravelField((-48, -48, 36), (96, 96, 64), [(48, 48, 10)], 26, clearance=1)
    ma, mb = tgr.mesh_state(a), tgr.mesh_state(b)
    assert set(ma) == set(mb) and len(ma) > 10
    for cid in ma:
        for key in ("vertices", "normals", "colors", "grids"):
            assert ma[cid][key].tobytes() == mb[cid][key].tobytes(), (cid, key)
    compare_fields(b.fields(), a.fields(), a.V, True)
    a.close()
    b.close()


def test_scratch_is_kept_grown_and_freed_with_the_map():
    N = 8
    small, large = (40, 40, 40), (256, 200, 120)
    footprint = large[0] * large[1] * large[2] * 4  # roughly: an int per voxel of the window
    second, grown, fits = [], [], []

    def cycle():
        gm = new_map(N)
        upload(gm, sparse_field(N))
        gm.TravelField((-20, -12, -28), small, [(20, 20, 20)], cost=False, step=False)
        a = free_bytes()
        gm.TravelField((-21, -13, -27), small, [(20, 20, 20)], 6, cost=False, step=False)
        second.append(a - free_bytes())
        gm.TravelField((-40, -30, -50), large, [(50, 40, 60)], cost=False, step=False)
        b = free_bytes()
        grown.append(a - b)
        gm.TravelField((-20, -12, -28), small, [(20, 20, 20)], cost=False, step=False)
        gm.TravelField((-40, -30, -50), large, [(50, 40, 60)], cost=False, step=False)
        fits.append(b - free_bytes())
        gm.close()

    readings = []
    for _ in range(3):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; drift %d; second call %s; grown by %s; later calls %s" % (readings, footprint, drift, second, grown, fits))
    assert abs(drift) < footprint // 2, (readings, footprint)
    assert all(v <= 0 for v in second) and all(v <= 0 for v in fits), (second, fits)
    assert all(v >= footprint // 2 for v in grown), (grown, footprint)


def travel_window(origin=(0, 0, 0), dims=(2, 2, 2), connectivity=26, step_cost=(10, 14, 17), max_cost=1 << 30, clearance=0, flag=0, offset=0.0):
    from cvids_amd import capi
    return capi.TravelWindow((C.c_int * 3)(*origin), (C.c_int * 3)(*dims), connectivity, (C.c_int * 3)(*step_cost), max_cost, clearance, flag, offset)


def raw_call(gm, w, seeds, n_seeds, targets=None, n_targets=0, n_groups=0, cost=None, step=None, state=None, table=None, totals=True):
    """chisel_hip_travel_field with host arrays, as the C ABI takes it -> (status, totals as a dict, the error text)"""
    from cvids_amd import capi
    L = capi.load_library()
    t = capi.TravelTotals(*([-7] * 12))
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = L.chisel_hip_travel_field(gm.h, C.byref(w) if w is not None else None, seeds.ctypes.data_as(C.POINTER(C.c_int32)) if seeds is not None else None, n_seeds,
                                   ptr(targets), n_targets, n_groups, ptr(cost), ptr(step), ptr(state),
                                   table.ctypes.data_as(C.POINTER(C.c_int64)) if table is not None else None, 0, C.byref(t) if totals else None)
    return rc, {n: int(getattr(t, n)) for n, _ in t._fields_}, L.chisel_hip_last_error().decode()


def test_the_size_query_writes_nothing():
    N = 8
    gm = sparse_map(N)
    origin, dims, seeds, traversable = sparse_request(N)
    want = tr.answer(*traversable, seeds, 26)
    rc, totals, _ = raw_call(gm, travel_window(origin, dims), np.asarray(seeds, np.int32), len(seeds))
    assert rc == 0 and {k: v for k, v in totals.items() if k not in tr.DIAGNOSTICS} == want["totals"] and totals["rounds"] > 0
    query = gm.TravelField(origin, dims, seeds, cost=False, step=False)
    assert query["cost"] is None and query["step"] is None and query["state"] is None and query["table"] is None and query["totals"] == totals


def test_refusals():
    """every refusal with its code, in the header's order; nothing is written, and the map answers afterwards"""
    from cvids_amd import capi
    from cvids_amd import chisel as ch
    N = 8
    gm = sparse_map(N)
    origin, dims, seeds, _ = sparse_request(N)
    before = gm.TravelField(origin, dims, seeds, state=True)
    cost, step, state = np.full(8, 77, np.int32), np.full(8, 77, np.uint8), np.full(8, 77, np.uint8)
    table, rows = np.full((2, 4), 77, np.int64), np.zeros((3, 4), np.int32)
    one = np.zeros((1, 3), np.int32)

    def refused(code, word, window=True, totals=True, seeds=one, n_seeds=1, targets=rows, n_targets=3, n_groups=2, with_table=True, **knobs):
        w = travel_window(**knobs) if window else None
        rc, t, msg = raw_call(gm, w, seeds, n_seeds, targets, n_targets, n_groups, cost, step, state, table if with_table else None, totals)
        assert rc == code and word in msg, (rc, msg)
        assert (cost == 77).all() and (step == 77).all() and (state == 77).all() and (table == 77).all() and all(v == -7 for v in t.values())

    refused(1, "null window", window=False)
    refused(1, "null seeds", seeds=None)
    refused(1, "null totals", totals=False)
    for bad in (0, -1, (1 << 20) + 1):
        refused(1, "n_seeds", n_seeds=bad)
    for a in range(3):
        for bad in (0, -1):
            refused(1, "dimension", dims=tuple(bad if k == a else 2 for k in range(3)))
        for bad in (-1, 2):
            s = np.zeros((2, 3), np.int32)
            s[1, a] = bad
            refused(1, "seed outside", seeds=s, n_seeds=2)
    for bad in (0, 4, 8, 27):
        refused(1, "connectivity", connectivity=bad)
    for k in range(3):
        for bad in (0, -3, 65536):
            refused(1, "step cost", connectivity=6, step_cost=tuple(bad if j == k else 5 for j in range(3)))
    for bad in (-1, (1 << 30) + 1):
        refused(1, "max_cost", max_cost=bad)
    for bad in (-1, 65):
        refused(1, "clearance", clearance=bad)
    refused(1, "NaN", offset=float("nan"))
    refused(1, "negative", n_targets=-1)
    refused(1, "negative", n_groups=-1)
    refused(1, "without the targets", targets=None)
    refused(1, "n_groups", n_groups=0)
    refused(1, "table without targets", n_targets=0, n_groups=0)
    lim = 1 << 30
    for a in range(3):
        refused(1, "2^30", origin=tuple(lim - 1 if k == a else 0 for k in range(3)))
        refused(1, "2^30", origin=tuple(-lim if k == a else 0 for k in range(3)))
        refused(1, "2^30", origin=tuple(lim - 11 if k == a else 0 for k in range(3)), clearance=11)
    refused(5, "more than 2^26 voxels", origin=(-500, -500, -500), dims=(512, 512, 257))
    refused(5, "more than 2^26 voxels", dims=((1 << 26) + 1, 1, 1))
    refused(5, "more than 2^30 voxels", dims=(1 << 26, 1, 1), clearance=64)
    refused(1, "2^30", origin=(lim - 3, 0, 0), dims=(4, 1 << 13, 1 << 13))  # a coordinate (invalid) in front of the size (unsupported)
    refused(1, "connectivity", dims=(1 << 10, 1 << 10, 1 << 10), connectivity=5)
    with pytest.raises(capi.ChiselHipError) as e:  # ... and through the Python method
        gm.TravelField(origin, dims, seeds, 7)
    assert e.value.code == 1 and "connectivity" in str(e.value)
    with pytest.raises(capi.ChiselHipError) as e:
        gm.TravelField(origin, (1 << 9, 1 << 9, 1 << 9), seeds, cost=False, step=False)
    assert e.value.code == 5
    after = gm.TravelField(origin, dims, seeds, state=True)
    for name in KEYS:
        assert np.array_equal(after[name], before[name])
    group = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, devices=[0, 0])
    with pytest.raises(capi.ChiselHipError) as e:
        group.TravelField((0, 0, 0), (4, 4, 4), [(0, 0, 0)])
    assert e.value.code == 5 and "group" in str(e.value)
    shard = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, n_shards=2, shard_rank=0)
    with pytest.raises(capi.ChiselHipError) as e:
        shard.TravelField((0, 0, 0), (4, 4, 4), [(0, 0, 0)])
    assert e.value.code == 5 and "shard" in str(e.value)
    group.close()
    shard.close()
    with pytest.raises(capi.ChiselHipError) as e:  # TravelPath: an unreached start
        gm.TravelPath(np.full((2, 2, 2), 255, np.uint8), (0, 0, 0))
    assert e.value.code == 1 and "not reached" in str(e.value)


def test_the_facade_program_answers_what_python_answers():
    """cvids_amd/open_chisel/tests/facade_travel.cpp: chisel::Chisel::TravelField and TravelPath on three frames of a wall; its totals
    and checksums are those of the Python host path on the same frames"""
    from cvids_amd import chisel as ch
    tdir = os.path.join(ROOT, "cvids_amd", "open_chisel", "tests")
    subprocess.check_call(["make", "-C", tdir, "travel"])
    run = subprocess.run([os.path.join(tdir, "facade_travel")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "facade_travel ok" in run.stdout, run.stdout + run.stderr
    Wf, Hf, N, res = 64, 48, 8, 0.05
    gm = new_map(N, res)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    cam = ch.PinholeCamera(52.5, 52.5, 31.5, 23.5, Wf, Hf, 0.05, 5.0)
    pose = np.eye(4, dtype=np.float32)
    for k in range(3):
        gm.IntegrateDepthScan(integ, np.full((Hf, Wf), np.float32(1.5) + np.float32(0.1) * np.float32(k), np.float32), pose, cam)
    origin, dims = (-12, -10, 2), (24, 20, 38)
    field = gm.DistanceField(origin, dims, 1)  # the seed: the first voxel of the central column that is traversable at clearance 1
    column = np.flatnonzero((field["state"][:, 10, 12] == fr.FREE) & (field["dist2"][:, 10, 12] == -1))
    assert len(column) > 0
    seeds = [(12, 10, int(column[0]))]
    assert [l for l in run.stdout.splitlines() if l.startswith("seed")][0].split() == ["seed", "12", "10", str(seeds[0][2])]
    front = gm.Frontiers(origin, dims, 1, 26, 2)
    K = front["totals"]["kept_clusters"]
    got, _ = check_window(gm, gm.fields(), N, origin, dims, seeds, 26, clearance=1, targets=front["voxels"], n_groups=K, what="facade")

    def fnv1a(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
            h = ((h ^ byte) * 1099511628211) & ((1 << 64) - 1)
        return h

    lines = run.stdout.splitlines()
    totals = [l for l in lines if l.startswith("totals")][0].split()
    assert {k: int(v) for k, v in zip(totals[1::2], totals[2::2])} == {k: v for k, v in got["totals"].items() if k not in tr.DIAGNOSTICS}, run.stdout
    line = [l for l in lines if l.startswith("checksum")][0].split()
    assert line[1::2] == ["cost", "step", "table", "path"]
    far = np.unravel_index(int(np.argmax(got["cost"])), got["cost"].shape)
    path = gm.TravelPath(got["step"], (int(far[2]), int(far[1]), int(far[0])))
    assert [int(v, 16) for v in line[2::2]] == [fnv1a(got["cost"]), fnv1a(got["step"]), fnv1a(got["table"]), fnv1a(path)], run.stdout
    assert got["totals"]["reached"] > 100 and K > 0 and len(path) > 3
    gm.close()
