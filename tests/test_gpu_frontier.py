"""chisel_hip_frontiers on the GPU against its definition (DESIGN.md 3.18 "Frontiers").

The answer is a set of integers, so every comparison is array_equal over every element: against the numpy restatement
(tests/frontier_restated.py) run over the map as it was uploaded or as GetChunkIDs / GetChunk read it back, against
chisel_hip_distance_field for the states, and of the device against itself.  A stated share only keeps a comparison from passing on an
empty case.  The maps are built once and only read, but where a test changes them."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from cvids_amd import synth
from tests import distance_restated as dr
from tests import frontier_restated as fr
from tests import hash_cases as hc
from tests import test_gpu_render as tgr
from tests.common import compare_fields, free_bytes, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.0625
BASE = (-2, -1, -3)
B_OF = {8: 3, 16: 2, 32: 2}
W, H = tgr.W, tgr.H
KEYS = ("state", "label", "voxels", "table")


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
    assert gm.NumChunks() == B_OF[N] ** 3 - 2
    return gm


@functools.lru_cache(maxsize=None)
def sparse_wide(N, offset=0.0):
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    wide = fr.wide_states(sparse_field(N), N, origin, dims, offset)
    wide.setflags(write=False)
    return wide


def equal_answers(got, want, what, keys=KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, "%s: %s is %s %s, not %s %s" % (
            what, key, got[key].dtype, got[key].shape, want[key].dtype, want[key].shape)
        assert np.array_equal(got[key], want[key]), "%s: %s differs at %d of %d places" % (what, key, int((got[key] != want[key]).sum()), want[key].size)
    assert got["totals"] == want["totals"], "%s: totals %s, not %s" % (what, got["totals"], want["totals"])


def check_window(gm, fields, N, origin, dims, k=1, connectivity=26, min_voxels=1, offset=0.0, wide=None, what=""):
    """every output of one call against the restatement over `fields` -> (the call's answer, the restatement's)"""
    got = gm.Frontiers(origin, dims, k, connectivity, min_voxels, offset, state=True)
    if wide is None:
        wide = fr.wide_states(fields, N, origin, dims, offset)
    want = fr.answer(wide, k, connectivity, min_voxels)
    what = "%s N %d origin %s dims %s faces %d connectivity %d min_voxels %d offset %r" % (what, N, origin, dims, k, connectivity, min_voxels, offset)
    equal_answers(got, want, what)
    assert got["centres"].dtype == np.float64 and np.array_equal(got["centres"], fr.centres(origin, want["table"], gm.voxel_resolution)), what + ": centres"
    return got, want


# ---- 1. hand-built sparse maps: chunk edges and parameters -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 16, 32])
def test_sparse_maps_against_the_restatement(N):
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    wide = sparse_wide(N)
    for connectivity in (6, 18, 26):
        for k in (1, 2, 4):
            for min_voxels in (1, 2, 16):
                got, _ = check_window(gm, None, N, origin, dims, k, connectivity, min_voxels, wide=wide)
                if k == 1 and min_voxels == 1:  # reach, on the device's own output
                    t = got["totals"]
                    share = t["frontier"] / got["state"].size
                    singles = int((got["table"][:, 1] == 1).sum())
                    big = got["table"][int(np.argmax(got["table"][:, 1]))]
                    print("N %d connectivity %d: share %.4f clusters %d singles %d largest %d" % (N, connectivity, share, t["clusters"], singles, t["largest_voxels"]))
                    assert 0.03 <= share <= 0.20 and t["largest_voxels"] == big[1] >= 1000 and fr.spans_tiles(big)
                    assert t["clusters"] >= (100 if connectivity == 6 else 5) and (connectivity != 6 or singles >= 100)
                if min_voxels == 16 and k == 1:
                    assert 0 < got["totals"]["kept_clusters"] < got["totals"]["clusters"] and (got["label"] == -2).any()
    for offset in (RES / 2, -RES / 2):  # other voxels occupied: other free voxels
        got, _ = check_window(gm, None, N, origin, dims, 1, 18, 2, offset, wide=sparse_wide(N, offset))
        assert got["totals"]["occupied"] != fr.answer(wide)["totals"]["occupied"]


# ---- 2. window shapes and placements ---------------------------------------------------------------------------------------------------
def test_window_shapes():
    """the tails of a word (nx = 1, 63, 64, 65, 129), flat windows (ny, nz = 1), windows smaller than a tile and no multiple of it, at
    three origins: inside a chunk, on a chunk face, overhanging the block's far corner"""
    N = 8
    gm, field = sparse_map(N), sparse_field(N)
    lo, hi = np.array(BASE) * N, (np.array(BASE) + B_OF[N]) * N
    shapes = [(1, 1, 1), (63, 1, 1), (64, 2, 1), (65, 3, 2), (129, 2, 2), (1, 40, 1), (1, 1, 30), (5, 7, 3), (16, 16, 8), (17, 17, 9), (15, 33, 7), (30, 1, 20)]
    places = [lo + (3, 2, 5), lo + (N, N, 2 * N), hi - (9, 5, 4)]
    frontier = 0
    for dims in shapes:
        for place in places:
            for connectivity in (6, 26):
                got, _ = check_window(gm, field, N, tuple(int(v) for v in place), dims, 1, connectivity, 1)
                frontier += got["totals"]["frontier"]
    assert frontier > 1000


def test_window_placements():
    """overhanging the map on every side (the sparse maps' own window does), wholly outside it, at negative indices, and far from the
    origin: chunk ids up to 2^20 - 2, the last the look-up accepts, with the window reaching past them"""
    N = 8
    gm, field = sparse_map(N), sparse_field(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE, (20, 18, 17), (19, 21, 18))
    got, _ = check_window(gm, field, N, origin, dims, 1, 18, 2, what="overhanging")
    assert got["totals"]["frontier"] > 1000
    for origin in ((500, 500, 500), (-700, 3, 9)):
        got, _ = check_window(gm, field, N, origin, (40, 20, 10), what="outside")
        assert got["totals"]["unknown"] == 8000 and got["totals"]["clusters"] == 0 and (got["label"] == -1).all() and got["voxels"].shape == (0, 4)
    got, _ = check_window(gm, field, N, (-30, -20, -40), (30, 25, 30), 2, 6, 1, what="negative indices")
    assert got["totals"]["frontier"] > 50
    far_base = (dr.ID_MAX - 1, dr.ID_MAX - 1, dr.ID_MIN)
    far_field = dr.sparse(N, 2, 5, RES, base=far_base)
    far = new_map(N)
    upload(far, far_field)
    origin, dims = dr.block_window(N, 2, far_base)
    got, _ = check_window(far, far_field, N, origin, dims, 1, 6, 1, what="far")
    assert got["totals"]["frontier"] > 300 and got["totals"]["clusters"] > 3
    lim = 1 << 30  # the far corner of the accepted coordinates: every voxel unknown
    t = far.FrontiersSize((lim - 7, lim - 7, -lim + 1), (6, 6, 6))
    assert t["unknown"] == 216 and t["frontier"] == 0
    far.close()


def test_a_window_of_more_than_256_scan_tiles():
    """dims (2048, 64, 33): 32 words a row x 2112 rows = 67 584 words in 264 scan tiles of 256 words, so the one workgroup that scans
    the tile sums goes round twice and carries its running 64-bit sum (kept clusters | kept voxels) into the second round.  A nearly
    empty map with two small patches of free voxels in unknown space: one whose frontier lies in the first rows of the window, one in
    the plane z = 32, whose first word is word 65 536, the first of tile 256 -- a lost carry numbers the second patch's clusters from
    0 again and puts their voxels at the head of the list"""
    N = 8
    origin, dims = (-1000, 5, -11), (2048, 64, 33)
    bars = np.zeros((3, 7, 12), np.uint8)
    bars[1, 1:6:2, 1:11] = fr.FREE  # three bars along x, a row of unknown voxels between them: three clusters at every connectivity
    plane = np.zeros((1, 9, 140), np.uint8)
    plane[0, 1:8:2, 1:139] = fr.FREE  # four bars of 138 voxels over three or four words of a row
    fields = fr.fields_from_states(bars, N, (origin[0] + 70, origin[1] + 2, origin[2]))
    far = fr.fields_from_states(plane, N, (origin[0] + 950, origin[1] + 50, origin[2] + 32))
    assert not set(fields) & set(far)
    fields.update(far)
    gm = new_map(N)
    upload(gm, fields)
    words = (dims[0] // 64) * dims[1] * dims[2]
    assert words == 67584 and -(-words // 256) == 264
    wide = fr.wide_states(fields, N, origin, dims)
    for connectivity, min_voxels in ((26, 1), (6, 11)):
        got, want = check_window(gm, None, N, origin, dims, 1, connectivity, min_voxels, wide=wide, what="264 scan tiles")
        t = got["totals"]
        kept = 7 if min_voxels == 1 else 4  # (a bar of the first patch has 10 voxels)
        assert t["clusters"] == 7 and t["kept_clusters"] == kept and t["kept_voxels"] == (30 if min_voxels == 1 else 0) + 4 * 138, t
        rows = got["table"]
        first_word = (rows[:, 7] * dims[1] + rows[:, 6]) * (dims[0] // 64) + rows[:, 5] // 64  # of the cluster's first voxel: min z, min y, min x
        assert (first_word >= 256 * 256).sum() == 4 and (first_word < 256 * 256).sum() == kept - 4  # behind and in front of the first round
        assert np.array_equal(got["voxels"][-4 * 138:, 2], np.full(4 * 138, 32)) and set(got["voxels"][-4 * 138:, 3].tolist()) == set(range(kept - 4, kept))
    gm.close()


# ---- 3. the hand volumes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,absent", [(8, True), (8, False), (16, True)])
def test_hand_volumes(N, absent):
    """every hand volume at a base that puts chunk and tile borders inside it, at every connectivity; the faces cases at every
    min_unknown_faces; the serpentine and the comb with a size filter too"""
    base = (N - 3, -N - 5, 2 * N - 7)
    gm = new_map(N, max_chunks=512)
    for name, (volume, expected) in fr.hand_volumes().items():
        fields, origin, dims = fr.hand_case(name, N, base, absent=absent)
        gm.Reset()
        upload(gm, fields)
        wide = fr.wide_states(fields, N, origin, dims)
        for n, connectivity in enumerate((26, 18, 6)):
            got, _ = check_window(gm, None, N, origin, dims, 1, connectivity, 1, wide=wide, what=name)
            assert expected is None or got["totals"]["clusters"] == expected[n], (name, connectivity, got["totals"])
        if name.startswith("faces"):
            for k in range(1, 7):
                got, _ = check_window(gm, None, N, origin, dims, k, 26, 1, wide=wide, what=name)
                assert got["totals"]["frontier"] == int(int(name[5:]) >= k)
        if name in ("serpentine", "comb"):
            got, _ = check_window(gm, None, N, origin, dims, 2, 6, 16, wide=wide, what=name)
            assert got["totals"]["kept_clusters"] == 1 and got["totals"]["largest_voxels"] == got["totals"]["frontier"]
            shifted = tuple(o - d for o, d in zip(origin, (5, 3, 2)))  # other tile borders through the same corridor
            check_window(gm, fields, N, shifted, tuple(d + 9 for d in dims), 1, 6, 1, what=name + " shifted")
        if name == "bridge":
            got, _ = check_window(gm, fields, N, origin, (8, 5, 3), 1, 26, 1, what="bridge outside the window")
            assert got["totals"]["clusters"] == 2
    gm.close()


# ---- 4. against an existing entry, on integrated maps ------------------------------------------------------------------------------------
def test_state_equals_distance_field():
    for N in (8, 16):
        gm = sparse_map(N)
        origin, dims = dr.block_window(N, B_OF[N], BASE)
        for offset in (0.0, RES / 2):
            field = gm.DistanceField(origin, dims, 1, False, offset, dist2=False)["state"]
            got = gm.Frontiers(origin, dims, surface_offset=offset, state=True, label=False, voxels=False)
            assert got["label"] is None and got["voxels"] is None and got["state"].dtype == np.uint8
            assert np.array_equal(got["state"], field) and all((field == s).mean() > 0.0005 for s in range(3))


@pytest.mark.parametrize("case", [0, 2], ids=["sphere_room-16", "box_room-8-colour"])
def test_an_integrated_map(case):
    """test_gpu_distance.py's window around the surface point the central pixel of frame 0 sees, against the restatement over
    gm.fields(); again after GarbageCollect of a third of the chunks, and after Reset"""
    scene, N, res, trunc, n_frames, carving, color, _ = tgr.MAPS[case]
    gm = tgr.gpu_map(scene, N, res, trunc, n_frames, carving, color)
    depth0, pose0 = next(iter(synth.stream(scene, 1, W, H)))
    fx, fy, cx, cy = synth.intrinsics(W, H)
    z = float(depth0[H // 2, W // 2])
    p0 = np.asarray(pose0, np.float64)
    hit = p0[:3, :3] @ np.array([(W // 2 + 0.5 - cx) / fx * z, (H // 2 + 0.5 - cy) / fy * z, z]) + p0[:3, 3]
    dims = (48, 40, 24)
    origin = tuple(int(np.floor(hit[a] / res)) - dims[a] // 2 for a in range(3))
    fields = gm.fields()
    for connectivity, k, min_voxels in ((26, 1, 1), (6, 2, 4), (18, 1, 16)):
        first, _ = check_window(gm, fields, N, origin, dims, k, connectivity, min_voxels, what=scene)
    assert first["totals"]["occupied"] > 0 and first["totals"]["free"] > 0
    # that window lies in the band around the surface, where occupied voxels part the free ones from the unknown; three chunks further
    # in every direction the band's chunks end, towards the camera in free voxels
    wide_dims = (96, 96, 96)
    wide_origin = tuple(int(np.floor(hit[a] / res)) - 48 for a in range(3))
    for connectivity, k, min_voxels in ((26, 1, 1), (6, 1, 4)):
        wide_first, _ = check_window(gm, fields, N, wide_origin, wide_dims, k, connectivity, min_voxels, what=scene + " wide")
    print("%s: %s" % (scene, wide_first["totals"]))
    assert wide_first["totals"]["frontier"] > 0 and wide_first["totals"]["clusters"] > 0
    ids = gm.GetChunkIDs()
    ids = ids[np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0]))]
    gm.GarbageCollect(ids[::3])
    fields = gm.fields()
    check_window(gm, fields, N, origin, dims, 1, 18, 16, what=scene + " after GarbageCollect")
    got, _ = check_window(gm, fields, N, wide_origin, wide_dims, 1, 6, 4, what=scene + " wide after GarbageCollect")
    assert (got["state"] != wide_first["state"]).any() and got["totals"]["frontier"] > 0
    gm.Reset()
    empty = gm.Frontiers(origin, dims, state=True)
    assert not empty["state"].any() and (empty["label"] == -1).all() and empty["totals"]["unknown"] == 48 * 40 * 24 and len(empty["table"]) == 0
    gm.close()


def test_on_a_table_without_an_empty_bucket():
    """one far id per bucket uploaded and collected (tests/hash_cases.py: saturation_rounds): every bucket a tombstone, so that the
    look-up of an absent chunk inside the box of created ids is ended by the loop's bound alone; then the sparse map into it"""
    N = 8
    gm = new_map(N, max_chunks=512)
    cap = gm.hash_table()["capacity"]
    for ids in hc.saturation_rounds(cap, 400):
        for k, cid in enumerate(ids):
            s, w, _ = hc.blocker_voxels(k, N ** 3)
            gm.AddChunk(cid, s, w)
        gm.GarbageCollect(ids)
    upload(gm, sparse_field(N))
    t = gm.hash_table()
    assert hc.n_empty(t) == 0 and gm.NumChunks() == B_OF[N] ** 3 - 2
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    check_window(gm, None, N, origin, dims, 1, 26, 2, wide=sparse_wide(N), what="crowded")
    gm.close()


# ---- 5. plumbing ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def guarded(shape, dtype, dev):
    """a contiguous tensor of `shape` between two runs of GUARD sentinels in one allocation -> (the whole, the tensor)"""
    import torch
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), 77, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def sentinels_kept(whole):
    return bool((whole[:GUARD] == 77).all()) and bool((whole[-GUARD:] == 77).all())


def test_host_arrays_equal_device_tensors():
    import torch
    N = 16
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    shape = (dims[2], dims[1], dims[0])
    dev = torch.device("cuda:0")
    host = gm.Frontiers(origin, dims, 1, 6, 2, state=True)  # (connectivity 6: the clusters of one voxel are dropped)
    kept = host["totals"]["kept_voxels"]
    assert kept > 1000 and (host["label"] == -2).any()
    w_state, state = guarded(shape, torch.uint8, dev)
    w_label, label = guarded(shape, torch.int32, dev)
    w_rows, rows = guarded((kept, 4), torch.int32, dev)  # exactly the live rows: the sentinels behind them are the first row not to write
    torch.cuda.synchronize()
    out = {"state": state, "label": label, "voxels": rows}
    res = gm.Frontiers(origin, dims, 1, 6, 2, out=out)
    gm.synchronize()
    assert res["state"] is state and res["label"] is label and res["voxels"] is rows
    got = {"state": state.cpu().numpy(), "label": label.cpu().numpy(), "voxels": rows.cpu().numpy(), "table": res["table"], "totals": res["totals"]}
    equal_answers(got, host, "device tensors")
    assert np.array_equal(res["centres"], host["centres"])
    assert sentinels_kept(w_state) and sentinels_kept(w_label) and sentinels_kept(w_rows)
    for name in ("state", "label", "voxels"):  # each output alone, on the device and on the host
        whole, t = guarded(tuple(out[name].shape), out[name].dtype, dev)
        torch.cuda.synchronize()
        alone = gm.Frontiers(origin, dims, 1, 6, 2, out={name: t})
        gm.synchronize()
        assert np.array_equal(t.cpu().numpy(), host[name]) and sentinels_kept(whole) and np.array_equal(alone["table"], host["table"]), name
        only = gm.Frontiers(origin, dims, 1, 6, 2, **{k: k == name for k in ("state", "label", "voxels")})
        assert [k for k in ("state", "label", "voxels") if only[k] is not None] == [name] and np.array_equal(only[name], host[name])
    roomy_whole, roomy = guarded((kept + 5, 4), torch.int32, dev)  # more rows than needed: the rest keeps its bytes
    torch.cuda.synchronize()
    gm.Frontiers(origin, dims, 1, 6, 2, out={"voxels": roomy})
    gm.synchronize()
    assert np.array_equal(roomy[:kept].cpu().numpy(), host["voxels"]) and bool((roomy[kept:] == 77).all()) and sentinels_kept(roomy_whole)


def raw_call(gm, w, state=None, label=None, cap_v=0, voxels=None, cap_c=0, table=None, totals=True):
    """chisel_hip_frontiers with host arrays, as the C ABI takes it -> (status, totals as a dict, the error text)"""
    from cvids_amd import capi
    L = capi.load_library()
    t = capi.FrontierTotals(*([-7] * 8))
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = L.chisel_hip_frontiers(gm.h, C.byref(w) if w is not None else None, ptr(state), ptr(label), cap_v, ptr(voxels), cap_c,
                                table.ctypes.data_as(C.POINTER(C.c_int64)) if table is not None else None, 0, C.byref(t) if totals else None)
    return rc, {n: int(getattr(t, n)) for n, _ in t._fields_}, L.chisel_hip_last_error().decode()


def frontier_window(origin, dims, k=1, connectivity=26, min_voxels=1, offset=0.0):
    from cvids_amd import capi
    return capi.FrontierWindow((C.c_int * 3)(*origin), (C.c_int * 3)(*dims), k, connectivity, min_voxels, offset)


def test_size_query_exact_capacities_and_one_short():
    N = 8
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    want = fr.answer(sparse_wide(N), 1, 6, 2)
    w = frontier_window(origin, dims, 1, 6, 2)
    rc, size, _ = raw_call(gm, w)
    assert rc == 0 and size == want["totals"] == gm.FrontiersSize(origin, dims, 1, 6, 2)
    K, kept, V = size["kept_clusters"], size["kept_voxels"], dims[0] * dims[1] * dims[2]
    assert K > 3 and kept > 1000

    def arrays():
        return np.full(V, 77, np.uint8), np.full(V, 77, np.int32), np.full((kept + 2, 4), 77, np.int32), np.full((K + 2, 12), 77, np.int64)

    state, label, rows, table = arrays()
    rc, totals, _ = raw_call(gm, w, state, label, kept, rows, K, table)
    assert rc == 0 and totals == size
    got = {"state": state.reshape(want["state"].shape), "label": label.reshape(want["label"].shape), "voxels": rows[:kept], "table": table[:K], "totals": totals}
    equal_answers(got, want, "exact capacities")
    assert (rows[kept:] == 77).all() and (table[K:] == 77).all()
    for cap_v, cap_c, word in ((kept - 1, K, "voxel capacity"), (kept, K - 1, "cluster capacity"), (1, 1, "voxel capacity")):
        state, label, rows, table = arrays()
        rc, totals, msg = raw_call(gm, w, state, label, cap_v, rows, cap_c, table)
        assert rc == 1 and word in msg and totals == size, (rc, msg, totals)
        assert (state == 77).all() and (label == 77).all() and (rows == 77).all() and (table == 77).all()
    state, label, rows, table = arrays()  # arrays with capacity 0 are not asked for: the size query
    rc, totals, _ = raw_call(gm, w, None, None, 0, rows, 0, table)
    assert rc == 0 and totals == size and (rows == 77).all() and (table == 77).all()
    rc, totals, _ = raw_call(gm, w, None, label, 0, None, K, table)  # the label and the table, no list
    assert rc == 0 and np.array_equal(label.reshape(want["label"].shape), want["label"]) and np.array_equal(table[:K], want["table"])


def test_the_call_twice_gives_the_same_bytes():
    N = 32
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    a = gm.Frontiers(origin, dims, 1, 26, 2, state=True)
    gm.Frontiers((0, 0, 0), (20, 20, 20), 2, 6, 1)  # (another window through the same scratch in between)
    b = gm.Frontiers(origin, dims, 1, 26, 2, state=True)
    for key in KEYS + ("centres",):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["totals"] == b["totals"] and a["totals"]["kept_voxels"] > 1000


def test_the_call_only_reads_the_map():
    """voxels, hash table and counters before and after calls with host and device outputs; and two maps fed the same frames, one of
    them asked for frontiers in between, mesh alike afterwards"""
    import torch
    N = 8
    gm = new_map(N)
    upload(gm, sparse_field(N))
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    fields, table, counters = gm.fields(), gm.hash_table(), gm.counters()
    dev = torch.device("cuda:0")
    label = torch.full((dims[2], dims[1], dims[0]), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for connectivity in (6, 26):
        gm.Frontiers(origin, dims, 1, connectivity, 2, state=True)
        gm.Frontiers(origin, dims, 2, connectivity, 1, out={"label": label})
    gm.synchronize()
    assert bool((label >= 0).any())
    compare_fields(fields, gm.fields(), gm.V, False)
    after = gm.hash_table()
    assert set(after) == set(table) and all(np.array_equal(np.asarray(after[k]), np.asarray(table[k])) for k in table)
    assert gm.counters() == counters and gm.NumChunks() == B_OF[N] ** 3 - 2
    gm.close()
    args = ("sphere_room", 16, 0.03, ("inverse", 2.0), 6, True, True)
    a, b = tgr.gpu_map(*args), tgr.gpu_map(*args)
    for origin in ((-48, -48, 36), (-30, -10, 66)):  # (the first: where test_an_integrated_map finds frontier voxels)
        a.Frontiers(origin, (48, 40, 24), 1, 26, 2)
        found = a.Frontiers(origin, (96, 96, 96), 1, 26, 2)["totals"]["frontier"]
        assert found > 0 or origin != (-48, -48, 36)
    assert a.counters() == b.counters() and a.NumChunks() == b.NumChunks()
    assert sorted(map(tuple, a.GetMeshesToUpdate().tolist())) == sorted(map(tuple, b.GetMeshesToUpdate().tolist()))
    compare_fields(b.fields(), a.fields(), a.V, True)
    a.UpdateMeshes()
    b.UpdateMeshes()
    a.Frontiers((-24, -20, 72), (48, 40, 24))
    ma, mb = tgr.mesh_state(a), tgr.mesh_state(b)
    assert set(ma) == set(mb) and len(ma) > 10
    for cid in ma:
        for key in ("vertices", "normals", "colors", "grids"):
            assert ma[cid][key].tobytes() == mb[cid][key].tobytes(), (cid, key)
    a.close()
    b.close()


def test_between_two_launch_sets_of_a_pipelined_stream():
    """device frames: IntegrateBatch, Frontiers into device tensors, IntegrateBatch.  The answer is that of the map after the first
    batch, and the final map is the one of the same stream without the call."""
    import torch
    N, res, trunc = 16, 0.03, ("inverse", 2.0)
    cam, integ = tgr.camera(), tgr.integrator(trunc)
    frames = list(synth.stream("sphere_room", 8, W, H))
    dev = torch.device("cuda:0")
    d_dev = [torch.from_numpy(d).to(dev) for d, _ in frames]
    origin, dims = (-48, -48, 36), (96, 96, 96)  # (around test_gpu_distance.py's window: out to where the band's chunks end)
    shape = (dims[2], dims[1], dims[0])
    out = {"state": torch.full(shape, 77, dtype=torch.uint8, device=dev), "label": torch.full(shape, 77, dtype=torch.int32, device=dev),
           "voxels": torch.full((shape[0] * shape[1] * shape[2] // 4, 4), 77, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    a, b, c = (new_map(N, res, max_chunks=8192) for _ in range(3))
    a.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    mid = a.Frontiers(origin, dims, 1, 26, 2, out=out)
    a.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4, 8)])
    b.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    b.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4, 8)])
    c.IntegrateBatch(integ, [(d_dev[i], frames[i][1], cam) for i in range(4)])
    a.synchronize()
    kept = mid["totals"]["kept_voxels"]
    got = {"state": out["state"].cpu().numpy(), "label": out["label"].cpu().numpy(), "voxels": out["voxels"][:kept].cpu().numpy(), "table": mid["table"],
           "totals": mid["totals"]}
    equal_answers(got, c.Frontiers(origin, dims, 1, 26, 2, state=True), "between the launch sets")
    equal_answers(got, fr.answer(fr.wide_states(c.fields(), N, origin, dims), 1, 26, 2), "between the launch sets, restated")
    assert kept > 100 and bool((out["voxels"][kept:] == 77).all())
    after = a.Frontiers(origin, dims, 1, 26, 2)  # (eight frames: other voxels observed than after four)
    assert (after["label"] != got["label"]).any()
    assert a.NumChunks() == b.NumChunks()
    compare_fields(b.fields(), a.fields(), a.V, False)
    assert a.counters() == b.counters()
    for m in (a, b, c):
        m.close()


def test_scratch_is_kept_grown_and_freed_with_the_map():
    """a second call of the same size allocates nothing, a larger window grows the scratch, a smaller one fits what is there, and the
    memory is back when the map is gone (cycles, as tests/test_gpu_lifetime.py measures a footprint)"""
    N = 8
    small, large = (40, 40, 40), (256, 200, 120)
    footprint = large[0] * large[1] * large[2] * 12  # roughly: three ints per voxel of the window
    second, grown, fits = [], [], []

    def cycle():
        gm = new_map(N)
        upload(gm, sparse_field(N))
        gm.Frontiers((-20, -12, -28), small)
        a = free_bytes()
        gm.Frontiers((-21, -13, -27), small, 2, 6, 4)
        second.append(a - free_bytes())
        t = gm.Frontiers((-40, -30, -50), large, label=False)
        assert t["totals"]["frontier"] > 1000
        b = free_bytes()
        grown.append(a - b)
        gm.Frontiers((-20, -12, -28), small)
        gm.Frontiers((-40, -30, -50), large, label=False)
        fits.append(b - free_bytes())
        gm.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; drift %d; second call %s; grown by %s; later calls %s" % (readings, footprint, drift, second, grown, fits))
    assert abs(drift) < footprint // 2, (readings, footprint)
    assert all(v <= 0 for v in second) and all(v <= 0 for v in fits), (second, fits)
    assert all(v >= footprint // 2 for v in grown), (grown, footprint)


def test_refusals():
    """every refusal with its code, in the header's order; nothing is touched, and the map answers afterwards"""
    from cvids_amd import capi
    from cvids_amd import chisel as ch
    N = 8
    gm = sparse_map(N)
    origin, dims = dr.block_window(N, B_OF[N], BASE)
    before = gm.Frontiers(origin, dims, state=True)
    state, label = np.full(8, 77, np.uint8), np.full(8, 77, np.int32)
    rows, table = np.full((8, 4), 77, np.int32), np.full((8, 12), 77, np.int64)

    def refused(code, word, origin=(0, 0, 0), dims=(2, 2, 2), window=True, totals=True, cap_v=8, cap_c=8, with_rows=True, with_table=True, **knobs):
        w = frontier_window(origin, dims, **knobs) if window else None
        rc, t, msg = raw_call(gm, w, state, label, cap_v, rows if with_rows else None, cap_c, table if with_table else None, totals)
        assert rc == code and word in msg, (rc, msg)
        assert (state == 77).all() and (label == 77).all() and (rows == 77).all() and (table == 77).all() and all(v == -7 for v in t.values())

    refused(1, "null window", window=False)
    refused(1, "null totals", totals=False)
    for a in range(3):
        for bad in (0, -1):
            refused(1, "dimension", dims=tuple(bad if k == a else 2 for k in range(3)))
    for bad in (0, 7, -1):
        refused(1, "min_unknown_faces", k=bad)
    for bad in (0, 4, 8, 27):
        refused(1, "connectivity", connectivity=bad)
    for bad in (0, -5):
        refused(1, "min_voxels", min_voxels=bad)
    refused(1, "NaN", offset=float("nan"))
    refused(1, "negative", cap_v=-1)
    refused(1, "negative", cap_c=-1)
    refused(1, "voxel capacity without", with_rows=False)
    refused(1, "cluster capacity without", with_table=False)
    lim = 1 << 30
    for a in range(3):
        refused(1, "2^30", origin=tuple(lim - 1 if k == a else 0 for k in range(3)))
        refused(1, "2^30", origin=tuple(-lim if k == a else 0 for k in range(3)))
    refused(5, "more than 2^26 voxels", origin=(-500, -500, -500), dims=(512, 512, 257))
    refused(5, "more than 2^26 voxels", dims=((1 << 26) + 1, 1, 1))
    refused(1, "dimension", dims=(0, 1 << 20, 1 << 20), k=0)  # the order: a dimension in front of the knobs and of the size
    refused(1, "min_unknown_faces", dims=(1 << 10, 1 << 10, 1 << 10), k=0, connectivity=5)
    refused(1, "2^30", origin=(lim - 3, 0, 0), dims=(4, 1 << 13, 1 << 13))  # a coordinate (invalid) in front of the size (unsupported)
    with pytest.raises(capi.ChiselHipError) as e:  # ... and through the Python methods
        gm.Frontiers(origin, dims, 7)
    assert e.value.code == 1 and "min_unknown_faces" in str(e.value)
    with pytest.raises(capi.ChiselHipError) as e:
        gm.FrontiersSize(origin, dims, connectivity=8)
    assert e.value.code == 1
    with pytest.raises(capi.ChiselHipError) as e:
        gm.Frontiers(origin, (1 << 9, 1 << 9, 1 << 9))
    assert e.value.code == 5
    after = gm.Frontiers(origin, dims, state=True)
    equal_answers(after, before, "after the refusals")
    group = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, devices=[0, 0])
    with pytest.raises(capi.ChiselHipError) as e:
        group.Frontiers((0, 0, 0), (4, 4, 4))
    assert e.value.code == 5 and "group" in str(e.value)
    shard = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, n_shards=2, shard_rank=0)
    with pytest.raises(capi.ChiselHipError) as e:
        shard.Frontiers((0, 0, 0), (4, 4, 4))
    assert e.value.code == 5 and "shard" in str(e.value)
    group.close()
    shard.close()


def test_the_facade_program_answers_what_python_answers():
    """cvids_amd/open_chisel/tests/facade_frontier.cpp: chisel::Chisel::Frontiers on three frames of a wall; its totals and checksums
    are those of the Python host path on the same frames"""
    from cvids_amd import chisel as ch
    tdir = os.path.join(ROOT, "cvids_amd", "open_chisel", "tests")
    subprocess.check_call(["make", "-C", tdir, "frontier"])
    run = subprocess.run([os.path.join(tdir, "facade_frontier")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "facade_frontier ok" in run.stdout, run.stdout + run.stderr
    Wf, Hf, N, res = 64, 48, 8, 0.05
    gm = new_map(N, res)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    cam = ch.PinholeCamera(52.5, 52.5, 31.5, 23.5, Wf, Hf, 0.05, 5.0)
    pose = np.eye(4, dtype=np.float32)
    for k in range(3):
        gm.IntegrateDepthScan(integ, np.full((Hf, Wf), np.float32(1.5) + np.float32(0.1) * np.float32(k), np.float32), pose, cam)
    origin, dims = (-12, -10, 22), (24, 20, 18)
    got, _ = check_window(gm, gm.fields(), N, origin, dims, 1, 26, 2, what="facade")

    def fnv1a(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
            h = ((h ^ byte) * 1099511628211) & ((1 << 64) - 1)
        return h

    lines = run.stdout.splitlines()
    totals = [l for l in lines if l.startswith("totals")][0].split()
    assert {k: int(v) for k, v in zip(totals[1::2], totals[2::2])} == {("largest" if k == "largest_voxels" else k): v for k, v in got["totals"].items()}, run.stdout
    line = [l for l in lines if l.startswith("checksum")][0].split()
    assert line[1::2] == ["label", "voxels", "table"]
    assert [int(v, 16) for v in line[2::2]] == [fnv1a(got[k]) for k in ("label", "voxels", "table")], run.stdout
    centre = [float(v) for v in [l for l in lines if l.startswith("centre0")][0].split()[1:]]
    assert centre == got["centres"][0].tolist()
    assert got["totals"]["frontier"] > 0 and got["totals"]["kept_clusters"] > 0
    gm.close()
