"""chisel_hip_gather_chunks / chisel_hip_scatter_chunks on the GPU: many chunks out of and into the map in one launch each.

Everything is compared bit for bit (uint32 / uint8 views: NaN payloads, -0.0 and denormals count).  The reference of every comparison
is the per-chunk entries -- GetChunk (chisel_hip_download_chunk), AddChunk (chisel_hip_upload_chunk) -- and, where frames are
involved, the oracle; never the new entries themselves.  The copy kernels move tiles of 16 KiB per array (capi.CHUNK_TILE_BYTES): eight
8^3 chunks, one 16^3 chunk, an eighth of a 32^3 chunk -- the chunk counts below sit on and beside those edges."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from cvids_amd import capi, synth
from tests import hash_cases as hc
from tests import voxel_fields as vf
from tests.common import compare_fields, free_bytes, make_frames, small_camera

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.05
SIZES = (8, 16, 32)
# chunks per case: around the 8 chunks of a tile at 8^3, and 1, 2, 3 where a chunk is a tile or several
COUNTS = {8: (7, 8, 9, 19), 16: (1, 2, 3, 5), 32: (1, 2, 3)}
assert capi.CHUNK_TILE_BYTES == 8 * 8 ** 3 * 4 == 16 ** 3 * 4  # (what the counts are chosen around)
NAN_BITS = (0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFFFFFFF)  # quiet and signalling NaNs with payloads, both signs
_FIELDS = {}


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def hand_field(N, seed=5):
    """27 (8^3), 8 (16^3, 32^3) chunks of voxel_fields.thresholds -- +-0.0, denormals, weights around the mesher's thresholds -- with NaN
    payloads and -0.0 written into distances and weights by hand, at the first and the last voxel too; ids around the origin, both
    signs.  Built once per chunk size; never changed."""
    if N not in _FIELDS:
        B = 3 if N == 8 else 2
        f = vf.thresholds(N, B, seed + N, res=RES, base=(-1, -1, -1))
        V = N ** 3
        for k, cid in enumerate(sorted(f)):
            s, w, c = f[cid]
            su, wu = s.view(np.uint32), w.view(np.uint32)
            for j, bits in enumerate(NAN_BITS):
                su[(k * 37 + j * 101) % V] = bits
                wu[(k * 53 + j * 211 + 7) % V] = bits
            su[0], su[V - 1], wu[V - 1] = 0x80000000, NAN_BITS[k % 4], 0x80000000
        _FIELDS[N] = f
    return _FIELDS[N]


def new_map(N, color, max_chunks=256, **kw):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), RES, color, max_chunks=max_chunks, **kw)


def upload_loop(gm, field, ids=None):
    for cid in (ids if ids is not None else field):
        s, w, c = field[tuple(cid)]
        gm.AddChunk(cid, s, w, c if gm.use_color else None)


def pack(field, ids, color=True):
    """the packed set of the ids, from the field's own arrays"""
    ids = [tuple(int(v) for v in c) for c in ids]
    V = len(next(iter(field.values()))[0])
    sdf = np.stack([field[c][0] for c in ids]) if ids else np.zeros((0, V), np.float32)
    w = np.stack([field[c][1] for c in ids]) if ids else np.zeros((0, V), np.float32)
    rgbw = (np.stack([field[c][2] for c in ids]) if ids else np.zeros((0, V, 4), np.uint8)) if color else None
    return np.array(ids, np.int32).reshape(-1, 3), sdf, w, rgbw


def stack_of_get_chunk(gm, ids):
    """the reference of a gather: GetChunk per id, stacked"""
    got = [gm.GetChunk(c) for c in ids]
    V = gm.V
    sdf = np.stack([g[0] for g in got]) if got else np.zeros((0, V), np.float32)
    w = np.stack([g[1] for g in got]) if got else np.zeros((0, V), np.float32)
    rgbw = (np.stack([g[2] for g in got]) if got else np.zeros((0, V, 4), np.uint8)) if gm.use_color else None
    return sdf, w, rgbw


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got), bits(want)
    assert np.array_equal(g, w), "%s: %d of %d values differ in their bits" % (what, int((g != w).sum()), g.size)


def assert_gather(gm, res, ids, what):
    """a gather's dict against GetChunk over `ids`"""
    ids = [tuple(int(v) for v in c) for c in ids]
    assert list(map(tuple, res["ids"].tolist())) == ids, what
    sdf, w, rgbw = stack_of_get_chunk(gm, ids)
    for name, want in (("sdf", sdf), ("weight", w), ("rgbw", rgbw)):
        if res.get(name) is not None:
            got = res[name].cpu().numpy()[:len(ids)] if hasattr(res[name], "is_cuda") else res[name]
            assert_same(got, want, "%s: %s" % (what, name))


def fields_bits_equal(a, b, what):
    assert sorted(a) == sorted(b), "%s: resident ids differ" % what
    for cid in a:
        for k, name in enumerate(("sdf", "weight", "rgbw")):
            if a[cid][k] is None:
                assert b[cid][k] is None
                continue
            assert_same(a[cid][k], b[cid][k], "%s: chunk %s %s" % (what, cid, name))


def meshes_equal(a, b, what):
    """every mesh of both maps, array by array, bit for bit -> the vertices compared"""
    ia, ib = sorted(map(tuple, a.GetMeshIDs().tolist())), sorted(map(tuple, b.GetMeshIDs().tolist()))
    assert ia == ib, "%s: mesh ids differ (%d, %d)" % (what, len(ia), len(ib))
    nv = 0
    for cid in ia:
        ma, mb = a.GetMesh(cid), b.GetMesh(cid)
        assert sorted(ma) == sorted(mb)
        for key in ma:
            if ma[key] is None:
                assert mb[key] is None
                continue
            assert_same(np.asarray(ma[key]), np.asarray(mb[key]), "%s: mesh %s %s" % (what, cid, key))
        nv += len(ma["vertices"])
    return nv


def to_update(gm):
    return sorted(map(tuple, gm.GetMeshesToUpdate().tolist()))


def expand27(ids):
    return sorted({(x + dx, y + dy, z + dz) for x, y, z in ids for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)})


def same_readout(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("hash_keys", "hash_vals", "slot_key", "free_list")) and a["free_top"] == b["free_top"]


def refused(call, code, word=None):
    with pytest.raises(capi.ChiselHipError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    return str(e.value)


def integrated(oracle_mod, n_frames, color=True, N=8, start=0, om=None, gm=None, max_chunks=4096):
    """96 x 72 sphere_room frames of two agents into an oracle map and a map -> (om, gm, integ, cam, colour image, frames)"""
    from tests.test_gpu_parity import _mk
    integ = None
    if om is None:
        om, gm, integ = _mk(oracle_mod, N, RES, color, max_chunks=max_chunks)
    cam = small_camera(96, 72)
    cimg = synth.render_color(96, 72, 3) if color else None
    frames = make_frames("sphere_room", n_frames, 96, 72, agents=2, start=start)
    return om, gm, integ, cam, cimg, frames


def run(om, gm, integ, cam, cimg, frames):
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    for d, p in frames:
        if cimg is None:
            if om is not None:
                om.integrate_depth(d, p, intr, cam.near_plane, cam.far_plane)
            gm.IntegrateDepthScan(integ, d, p, cam)
        else:
            if om is not None:
                om.integrate_depth_color(d, p, intr, cimg, near=cam.near_plane, far=cam.far_plane)
            gm.IntegrateDepthScanColor(integ, d, p, cam, cimg, p, cam)


# ---- gather = download ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", (False, True), ids=("plain", "colour"))
@pytest.mark.parametrize("N", SIZES)
def test_gather_equals_download(N, color):
    """every selection, each array alone and together, into host arrays: the stack of GetChunk over the same ids"""
    field = hand_field(N)
    gm = new_map(N, color)
    upload_loop(gm, field)
    resident = list(map(tuple, gm.GetChunkIDs().tolist()))
    assert resident == sorted(field)
    # all: GetChunkIDs' order; the size query
    assert gm.GatherChunksSize() == len(resident)
    res = gm.GatherChunks()
    assert (res["rgbw"] is not None) == color
    assert_gather(gm, res, resident, "all")
    # each array alone
    for name in ("sdf", "weight") + (("rgbw",) if color else ()):
        one = gm.GatherChunks(sdf=name == "sdf", weight=name == "weight", rgbw=name == "rgbw")
        assert [k for k in ("sdf", "weight", "rgbw") if one[k] is not None] == [name]
        assert_gather(gm, one, resident, "all, %s alone" % name)
    # the caller's lists: scrambled, with duplicates, of every count around the tile's edge; a single chunk
    rng = np.random.default_rng(N)
    for n in COUNTS[N]:
        pick = [resident[int(i)] for i in rng.permutation(len(resident))[:max(n - 1, 1)]]
        pick = (pick + [pick[0]])[:n]  # a duplicate where there is room for one
        rng.shuffle(pick)
        assert gm.GatherChunksSize(ids=pick) == n
        assert_gather(gm, gm.GatherChunks(ids=pick), pick, "a list of %d" % n)
    assert_gather(gm, gm.GatherChunks(ids=[resident[-1]]), [resident[-1]], "a single chunk")
    # boxes: one cutting through the block, one chunk exactly, one holding nothing
    for lo, hi in (((-1, 0, -1), (0, 0, 1)), ((0, 0, 0), (0, 0, 0)), ((-1, -1, -1), (5, 5, 5)), ((40, 40, 40), (50, 50, 50))):
        inside = [c for c in resident if all(lo[a] <= c[a] <= hi[a] for a in range(3))]
        assert gm.GatherChunksSize(box=(lo, hi)) == len(inside)
        assert_gather(gm, gm.GatherChunks(box=(lo, hi)), inside, "box %s %s" % (lo, hi))
    assert len(gm.GatherChunks(box=((40, 40, 40), (50, 50, 50)))["ids"]) == 0
    with pytest.raises(KeyError) as e:
        gm.GatherChunks(ids=[resident[0], (9, 9, 9), resident[1]])
    assert "id 1 " in str(e.value)
    gm.close()


@pytest.mark.parametrize("N", SIZES)
def test_gather_into_device_tensors_leaves_their_surroundings_alone(N):
    """device outputs at a 16-byte-aligned offset inside larger tensors: the live range equals GetChunk, the sentinels before and behind
    it survive -- for every chunk count around the tile's edge"""
    import torch
    field = hand_field(N)
    gm = new_map(N, True)
    upload_loop(gm, field)
    resident = list(map(tuple, gm.GetChunkIDs().tolist()))
    V, dev = gm.V, torch.device("cuda:0")
    for n in COUNTS[N]:
        pick = resident[:n] if n <= len(resident) else (resident + resident)[:n]
        pad = 8  # floats / colour words in front: 32 bytes
        fl = [torch.full((pad + n * V + pad,), -7.25, dtype=torch.float32, device=dev) for _ in range(2)]
        cb = torch.full((4 * (pad + n * V + pad),), 0xA5, dtype=torch.uint8, device=dev)
        out = {"sdf": fl[0][pad:pad + n * V].view(n, V), "weight": fl[1][pad:pad + n * V].view(n, V), "rgbw": cb[4 * pad:4 * (pad + n * V)].view(n, V, 4)}
        assert all(t.data_ptr() % 16 == 0 for t in out.values())
        res = gm.GatherChunks(ids=pick, out=out)
        gm.synchronize()
        assert_gather(gm, res, pick, "device, %d chunks" % n)
        for t in fl:
            h = t.cpu().numpy()
            assert (h[:pad] == -7.25).all() and (h[pad + n * V:] == -7.25).all(), "a float sentinel was overwritten (%d chunks)" % n
        h = cb.cpu().numpy()
        assert (h[:4 * pad] == 0xA5).all() and (h[4 * (pad + n * V):] == 0xA5).all(), "a colour sentinel was overwritten (%d chunks)" % n
        # a tensor with room to spare: the rows behind the selection are not written
        roomy = {"sdf": torch.full((n + 2, V), 3.5, dtype=torch.float32, device=dev)}
        gm.GatherChunks(ids=pick, out=roomy)
        gm.synchronize()
        assert (roomy["sdf"][n:].cpu().numpy() == 3.5).all()
        assert_same(roomy["sdf"][:n].cpu().numpy(), stack_of_get_chunk(gm, pick)[0], "roomy")
    gm.close()


# ---- scatter = upload loop ------------------------------------------------------------------------------------------------------------
def compare_maps(a, b, ids, what):
    """the upload-loop map `a` against the scattered map `b`: ids, voxels, meshes-to-update, meshes, the hash's invariants"""
    assert list(map(tuple, a.GetChunkIDs().tolist())) == list(map(tuple, b.GetChunkIDs().tolist())), what
    assert a.NumChunks() == b.NumChunks()
    fields_bits_equal(a.fields(), b.fields(), what)
    assert to_update(a) == to_update(b), what
    for m in (a, b):
        m.UpdateMeshes(force=True)
    meshes_equal(a, b, what + ", UpdateMeshes(force)")
    for m in (a, b):
        m.UpdateMeshesOf(ids)
    nv = meshes_equal(a, b, what + ", UpdateMeshesOf")
    assert hc.check_invariants(a.hash_table(), what) == hc.check_invariants(b.hash_table(), what) == a.NumChunks()
    return nv


@pytest.mark.parametrize("source", ("host", "device"))
@pytest.mark.parametrize("color", (False, True), ids=("plain", "colour"))
@pytest.mark.parametrize("N", SIZES)
def test_scatter_equals_upload_loop(N, color, source):
    """into an empty map and into one that holds half of the ids with other voxels; every chunk count around the tile's edge"""
    import torch
    field, other = hand_field(N), vf.dense(N, 3 if N == 8 else 2, 77, res=RES, base=(-1, -1, -1))
    all_ids = sorted(field)
    nv = 0
    a, b = new_map(N, color), new_map(N, color)
    for n in COUNTS[N]:
        ids = all_ids[:n]
        for prefill in (False, True):
            held = ids[::2] + all_ids[n:n + 2] if prefill else []  # half of the call's ids, and two it does not name
            for m in (a, b):
                m.Reset()
                upload_loop(m, other, held)
            upload_loop(a, field, ids)
            i, s, w, c = pack(field, ids[::-1], color)  # (the order of a call does not matter to the result)
            if source == "device":
                s, w = torch.from_numpy(s).cuda(), torch.from_numpy(w).cuda()
                c = torch.from_numpy(c).cuda() if color else None
                torch.cuda.synchronize()
            created = b.ScatterChunks(i, s, w, c)
            assert created == len(set(ids) - set(held)), (n, prefill, created)
            nv += compare_maps(a, b, ids, "%d chunks, prefill %s" % (n, prefill))
            # the gather of the same ids reads back what went in
            got = b.GatherChunks(ids=ids)
            want = pack(field, ids, color)
            for name, arr in zip(("sdf", "weight", "rgbw"), want[1:]):
                if arr is not None:
                    assert_same(got[name], arr, "gather after scatter: %s" % name)
    a.close()
    b.close()
    assert nv > 0  # (meshes were compared)


@pytest.mark.parametrize("source", ("host", "device"))
def test_scatter_without_colours_into_a_map_with_colour_writes_zeros(source):
    import torch
    N = 8
    field, other = hand_field(N), vf.dense(N, 3, 78, res=RES, base=(-1, -1, -1))
    ids = sorted(field)[:9]
    a, b = new_map(N, True), new_map(N, True)
    for m in (a, b):
        upload_loop(m, other, ids[:4])  # colours that must go
    for cid in ids:
        a.AddChunk(cid, field[cid][0], field[cid][1], None)
    i, s, w, _ = pack(field, ids)
    if source == "device":
        s, w = torch.from_numpy(s).cuda(), torch.from_numpy(w).cuda()
        torch.cuda.synchronize()
    assert b.ScatterChunks(i, s, w, None) == 5
    assert not b.GatherChunks(ids=ids)["rgbw"].any()
    compare_maps(a, b, ids, "rgbw=None")
    a.close()
    b.close()


# ---- mark_updated ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (8, 16))
def test_mark_updated_leaves_the_chunks_as_an_integration_does(N):
    field = hand_field(N)
    all_ids = sorted(field)
    base, ids = all_ids[:6], all_ids[3:8]  # three of the call's chunks are resident, two are created; three residents are neighbours only
    a, b, plain = new_map(N, True), new_map(N, True), new_map(N, True)
    for m in (a, b, plain):
        upload_loop(m, field, base)
        assert to_update(m) == []
    upload_loop(a, field, ids)
    assert b.ScatterChunks(*pack(field, ids), mark_updated=True) == 2
    assert plain.ScatterChunks(*pack(field, ids)) == 2
    # without the flag: what the upload loop leaves
    assert to_update(plain) == to_update(a) == []
    # with it: the 27-neighbourhoods of the call's ids, as Chisel::IntegrateDepthScan* leaves them (Chisel.h:175-189) -- whose resident
    # part is every resident chunk that has one of the ids in its neighbourhood
    resident = set(map(tuple, b.GetChunkIDs().tolist()))
    got = to_update(b)
    assert [c for c in got if c in resident] == [c for c in expand27(ids) if c in resident]
    assert set(ids) <= set(got) and len([c for c in got if c in resident]) > len(ids)
    assert got == expand27(ids)
    fields_bits_equal(a.fields(), b.fields(), "mark_updated")
    # the next recompute meshes them: the upload-loop map is told the same ids by hand
    b.UpdateMeshes(force=True)
    a.UpdateMeshesOf([c for c in expand27(ids) if c in resident])
    assert meshes_equal(a, b, "recompute after mark_updated") > 0
    assert to_update(b) == []
    hc.check_invariants(b.hash_table(), "mark_updated")
    for m in (a, b, plain):
        m.close()


# ---- a round trip through HBM between launch sets -----------------------------------------------------------------------------------
def test_round_trip_through_device_tensors_and_resume(oracle_mod):
    """test_checkpoint_and_resume without the file: map A integrates frames 0-5, its chunks go through device tensors into a fresh map
    B with no synchronise in between beyond the entries' own, B integrates frames 6-9 and equals A continued, and the oracle"""
    import torch
    om, A, integ, cam, cimg, frames = integrated(oracle_mod, 5, N=8)  # 2 agents: 10 frames
    assert len(frames) == 10
    run(om, A, integ, cam, cimg, frames[:6])
    n = A.GatherChunksSize()
    assert 20 < n < 2000
    dev = torch.device("cuda:0")
    out = {"sdf": torch.empty((n, A.V), dtype=torch.float32, device=dev), "weight": torch.empty((n, A.V), dtype=torch.float32, device=dev),
           "rgbw": torch.empty((n, A.V, 4), dtype=torch.uint8, device=dev)}
    done = torch.cuda.Event()
    done.record()
    res = A.GatherChunks(out=out)
    A.record_event(done.cuda_event)
    B = new_map(8, True, max_chunks=4096)
    B.wait_event(done.cuda_event)  # (two maps, two streams: the order between them is the caller's)
    assert B.ScatterChunks(res["ids"], out["sdf"], out["weight"], out["rgbw"]) == n
    assert_gather(A, res, A.GetChunkIDs(), "the integrated map, all, into device tensors")
    run(om, A, integ, cam, cimg, frames[6:])
    run(None, B, integ, cam, cimg, frames[6:])
    assert om.num_chunks() == A.NumChunks() == B.NumChunks()
    compare_fields(om.fields(), B.fields(), om.V, True, what="resumed against the oracle")
    fields_bits_equal(A.fields(), B.fields(), "resumed against the uninterrupted map")
    hc.check_invariants(B.hash_table(), "resumed")
    A.close()
    B.close()


# ---- the crowded hash -------------------------------------------------------------------------------------------------------------------
def test_scatter_into_a_crowded_hash():
    """ids that share a home bucket and a run across the table's end, created by one scatter into buckets a GarbageCollect left as
    tombstones; then every second one collected, so that the others' probe paths pass tombstones, and all of them scattered again --
    found behind the tombstones or created into them.  The reach is asserted on the device's own read-out; then the invariants, the
    voxels against the upload-loop map, and a gather of the same ids."""
    N, V = 8, 512
    a, b = new_map(N, True, max_chunks=512), new_map(N, True, max_chunks=512)
    cap = b.hash_table()["capacity"]
    assert cap == 1024
    colliding = hc.colliding_ids(cap)                                        # 32 ids on 3 homes, one of them the last bucket
    run_end = [hc.far_ids(h, 1, cap)[0] for h in list(range(cap - 40, cap - 1)) + list(range(1, 8))]  # one per bucket across the end (the colliding ids have the last and the first)
    first = [hc.far_ids(h, 1, cap, skip=1)[0] for h in range(cap - 40, cap - 1)]  # ... and a layer on the same homes that goes in first and is partly collected
    assert len(set(colliding + run_end + first)) == len(colliding) + len(run_end) + len(first)
    field = {cid: hc.blocker_voxels(k, V, True) for k, cid in enumerate(colliding + run_end + first)}
    for m in (a, b):
        upload_loop(m, field, first)
        m.GarbageCollect(first[::2])  # tombstones in the run's buckets: the creates take them
    assert hc.n_tombstones(b.hash_table()) == len(first[::2])
    ids = colliding + run_end
    upload_loop(a, field, ids)
    assert b.ScatterChunks(*pack(field, ids)) == len(ids)
    t = b.hash_table()
    r = hc.reach(t, ids)
    print("reach of the scattered ids: %s; %d tombstones left" % (r, hc.n_tombstones(t)))
    assert r["off_home"] >= 40 and r["cross"] >= 10 and r["long"] >= 10, r
    assert hc.check_invariants(t, "crowded") == len(ids) + len(first) - len(first[::2]) == b.NumChunks()
    assert hc.resident_ids(t) == hc.resident_ids(a.hash_table())
    fields_bits_equal(a.fields(), b.fields(), "crowded")
    # every second id collected: the others now sit behind tombstones
    gone, stay = ids[1::2], ids[::2]
    for m in (a, b):
        m.GarbageCollect(gone)
    t = b.hash_table()
    r = hc.reach(t, stay)
    print("after the collection: %s; %d tombstones" % (r, hc.n_tombstones(t)))
    assert r["tomb"] >= 10 and r["cross"] >= 5, r
    rng = np.random.default_rng(1)
    pick = [stay[int(i)] for i in rng.permutation(len(stay))]
    assert_gather(b, b.GatherChunks(ids=pick), pick, "gather from behind the tombstones")
    # all of them again, with other voxels: found behind the tombstones, or created into them
    again = {cid: hc.blocker_voxels(100 + k, V, True) for k, cid in enumerate(ids)}
    upload_loop(a, again, ids)
    order = [ids[int(i)] for i in rng.permutation(len(ids))]
    assert b.ScatterChunks(*pack(again, order)) == len(gone)
    t = b.hash_table()
    assert hc.check_invariants(t, "scattered again") == len(ids) + len(first) - len(first[::2]) == b.NumChunks()
    assert hc.resident_ids(t) == hc.resident_ids(a.hash_table())
    fields_bits_equal(a.fields(), b.fields(), "scattered again")
    assert_gather(b, b.GatherChunks(ids=order), order, "gather of the same ids")
    # overwrite in place: nothing is created, the table is what it was
    assert b.ScatterChunks(*pack(again, pick)) == 0
    assert same_readout(t, b.hash_table())
    a.close()
    b.close()


# ---- the pool -------------------------------------------------------------------------------------------------------------------------
def test_scatter_grows_a_growable_pool():
    N = 16
    gm = new_map(N, False, max_chunks=-64)
    info = gm.pool_info()
    assert info["growable"] and info["grown"] == 0
    n = info["committed"] + 40
    assert n <= info["limit"]
    rng = np.random.default_rng(4)
    ids = [(x, y, z) for x in range(8) for y in range(8) for z in range(8)][:n]
    sdf = rng.standard_normal((n, gm.V)).astype(np.float32)
    w = rng.uniform(0, 2, (n, gm.V)).astype(np.float32)
    assert gm.ScatterChunks(ids, sdf, w) == n
    after = gm.pool_info()
    assert after["grown"] >= 1 and after["committed"] >= n and gm.NumChunks() == n
    for k in (0, info["committed"] - 1, info["committed"], n - 1):  # on both sides of the first commitment
        gs, gw, _ = gm.GetChunk(ids[k])
        assert_same(gs, sdf[k], "chunk %d" % k)
        assert_same(gw, w[k], "chunk %d" % k)
    got = gm.GatherChunks()
    order = np.lexsort((np.array(ids)[:, 2], np.array(ids)[:, 1], np.array(ids)[:, 0]))
    assert_same(got["sdf"], sdf[order], "all after growth")
    hc.check_invariants(gm.hash_table(), "grown")
    gm.close()


def test_scatter_into_a_full_fixed_pool_is_all_or_nothing():
    N, V = 8, 512
    gm = new_map(N, True, max_chunks=64)
    info = gm.pool_info()
    cap = info["committed"]
    assert cap == info["limit"] == 64 and not info["growable"]
    ids = [hc.far_ids(h, 1, 1024)[0] for h in range(cap + 4)]
    field = {cid: hc.blocker_voxels(k, V, True) for k, cid in enumerate(ids)}
    held = ids[:cap - 3]
    upload_loop(gm, field, held)
    before, t0 = gm.fields(), gm.hash_table()
    # three free slots, four absent ids among resident ones
    msg = refused(lambda: gm.ScatterChunks(*pack(field, held[:5] + ids[cap - 3:cap + 1])), 3)
    assert "pool" in msg
    assert gm.NumChunks() == len(held)
    fields_bits_equal(before, gm.fields(), "after the refusal")
    assert same_readout(t0, gm.hash_table())
    # exactly what fits is taken
    assert gm.ScatterChunks(*pack(field, held[:5] + ids[cap - 3:cap])) == 3
    assert gm.NumChunks() == cap and hc.check_invariants(gm.hash_table(), "full") == cap
    # the refusal was not latched as "map incomplete": after room is made, an integration that creates chunks reports nothing
    from cvids_amd import chisel as ch
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    gm.GarbageCollect(ids[4:cap])
    assert gm.NumChunks() == 4
    cam = small_camera(32, 24)
    gm.IntegrateDepthScan(integ, np.full((24, 32), 0.4, np.float32), synth.pose_yaw(0.0), cam)
    gm.synchronize()  # (a latched pool error would be raised here)
    assert 4 < gm.NumChunks() <= cap
    hc.check_invariants(gm.hash_table(), "after the integration")
    gm.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_as_it_was():
    import torch
    N = 8
    field = hand_field(N)
    ids = sorted(field)[:6]
    gm, plain = new_map(N, True), new_map(N, False)
    upload_loop(gm, field, ids)
    upload_loop(plain, field, ids[:2])
    before, t0 = gm.fields(), gm.hash_table()
    i, s, w, c = pack(field, ids)
    L, h = gm.L, gm.h
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    n_out, created = C.c_int64(-5), C.c_int64(-5)
    req = capi.ChunkRequest()
    gather = lambda handle, r, cap, ps, pw, pc, dev=0, ids_out=None: capi.check(L.chisel_hip_gather_chunks(handle, r, cap, ps, pw, pc, dev, ids_out, C.byref(n_out)))
    scatter = lambda handle, pi, n, ps, pw, pc, dev=0: capi.check(L.chisel_hip_scatter_chunks(handle, pi, n, ps, pw, pc, dev, 0, C.byref(created)))
    sd, wd, cd = s.ctypes.data, w.ctypes.data, c.ctypes.data
    # ---- gather
    refused(lambda: gather(None, C.byref(req), 6, sd, wd, None), 1, "null")
    refused(lambda: gather(h, None, 6, sd, wd, None), 1, "null")
    bad = capi.ChunkRequest()
    bad.ids_xyz, bad.n_ids = ip(i), -1
    refused(lambda: gather(h, C.byref(bad), 6, sd, wd, None), 1, "negative")
    bad.n_ids = 0
    refused(lambda: gather(h, C.byref(bad), 6, sd, wd, None), 1, "without a count")
    bad = capi.ChunkRequest()
    bad.n_ids = 3
    refused(lambda: gather(h, C.byref(bad), 6, sd, wd, None), 1, "without an id list")
    refused(lambda: gm.GatherChunks(ids=ids, box=((0, 0, 0), (1, 1, 1))), 1, "box together")
    refused(lambda: gm.GatherChunks(box=((0, 2, 0), (1, 1, 1))), 1, "lo > hi")
    assert "id 2 " in refused(lambda: gm.GatherChunks(ids=[ids[0], ids[1], (0, hc.ID_MAX + 1, 0)]), 1, "range")
    refused(lambda: gather(h, C.byref(req), 6, None, None, None), 1, "no output")
    refused(lambda: gather(plain.h, C.byref(req), 6, sd, None, cd), 1, "without colour")
    dev_buf = torch.zeros(6 * gm.V + 8, dtype=torch.float32, device="cuda:0")
    refused(lambda: gather(h, C.byref(req), 6, dev_buf.data_ptr() + 4, None, None, dev=1), 1, "aligned")
    with pytest.raises(KeyError):
        gm.GatherChunks(ids=[ids[0], (3, 3, 3)])
    n_out.value = -5
    sentinel = s.copy()
    refused(lambda: gather(h, C.byref(req), 5, sd, wd, None), 1, "capacity")
    assert n_out.value == 6 and np.array_equal(bits(s), bits(sentinel))  # (the count for the retry; nothing written)
    gather(h, C.byref(req), 0, None, None, None)  # the size query
    assert n_out.value == 6
    only_ids = np.zeros((6, 3), np.int32)
    gather(h, C.byref(req), 6, None, None, None, ids_out=ip(only_ids))  # the ids alone
    assert list(map(tuple, only_ids.tolist())) == ids
    # ---- scatter
    refused(lambda: scatter(None, ip(i), 6, sd, wd, cd), 1, "null")
    refused(lambda: scatter(h, None, 6, sd, wd, cd), 1, "null")
    refused(lambda: scatter(h, ip(i), 6, None, wd, cd), 1, "null")
    refused(lambda: scatter(h, ip(i), 6, sd, None, cd), 1, "null")
    refused(lambda: scatter(h, ip(i), -1, sd, wd, cd), 1, "negative")
    created.value = -5
    scatter(h, None, 0, None, None, None)  # a successful no-op
    assert created.value == 0
    far = i.copy()
    far[4, 2] = hc.ID_MIN - 1
    assert "id 4 " in refused(lambda: scatter(h, ip(far), 6, sd, wd, cd), 1, "range")
    dup = i.copy()
    dup[5] = dup[1]
    assert "id 5 " in refused(lambda: scatter(h, ip(dup), 6, sd, wd, cd), 1, "repeats")
    refused(lambda: scatter(plain.h, ip(i), 6, sd, wd, cd), 1, "without colour")
    refused(lambda: scatter(h, ip(i), 6, dev_buf.data_ptr() + 8, dev_buf.data_ptr(), None, dev=1), 1, "aligned")
    grp = None
    try:
        from cvids_amd import chisel as ch
        grp = ch.Chisel((N, N, N), RES, True, max_chunks=256, devices=[0, 0])
        refused(lambda: scatter(grp.h, ip(i), 6, sd, wd, cd), 5, "group")
        refused(lambda: gather(grp.h, C.byref(req), 6, sd, wd, None), 5, "group")
    finally:
        if grp is not None:
            grp.close()
    # ---- nothing happened
    assert gm.NumChunks() == 6 and plain.NumChunks() == 2
    fields_bits_equal(before, gm.fields(), "after the refusals")
    assert same_readout(t0, gm.hash_table())
    gm.close()
    plain.close()


def test_one_shard_of_two_serves_its_own_chunks_and_refuses_the_others():
    from cvids_amd import chisel as ch
    N = 8
    field = hand_field(N)
    ids = sorted(field)
    shards = [new_map(N, True, n_shards=2, shard_rank=r) for r in range(2)]
    own = [[c for c in ids if ch.chunk_owner(c, 2, 2) == r] for r in range(2)]
    assert len(own[0]) >= 3 and len(own[1]) >= 3
    for r, m in enumerate(shards):
        assert m.ScatterChunks(*pack(field, own[r])) == len(own[r])
        t0 = m.hash_table()
        mixed = own[r][:2] + [own[1 - r][0]] + own[r][2:3]
        assert "id 2 " in refused(lambda: m.ScatterChunks(*pack(field, mixed)), 1, "another shard")
        assert same_readout(t0, m.hash_table())
        ref = new_map(N, True, n_shards=2, shard_rank=r)
        upload_loop(ref, field, own[r])
        fields_bits_equal(ref.fields(), m.fields(), "rank %d" % r)
        assert_gather(m, m.GatherChunks(), own[r], "rank %d, all" % r)
        ref.close()
    for m in shards:
        m.close()


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def file_of(gm, N, color):
    """the documented file, assembled from GetChunkIDs + GetChunk"""
    ids = gm.GetChunkIDs()
    out = [b"CHSLHIP1" + struct.pack("<ifiiq", N, RES, 1 if color else 0, 0, len(ids))]
    for cid in ids:
        s, w, c = gm.GetChunk(cid)
        out.append(struct.pack("<3i", *[int(v) for v in cid]) + s.tobytes() + w.tobytes() + (c.tobytes() if color else b""))
    return b"".join(out)


@pytest.mark.parametrize("block", (None, "2", "5"))
@pytest.mark.parametrize("N,color", ((8, True), (16, False), (32, True)))
def test_save_map_writes_the_documented_file_and_load_map_reads_it(N, color, block, tmp_path, monkeypatch):
    """SaveMap's bytes against the file assembled from the per-chunk entries, LoadMap of it into a fresh map; with a block of two
    (and of five) chunks, so that block boundaries are crossed, and with the default block"""
    field = hand_field(N)
    ids = sorted(field)[:13]
    gm = new_map(N, color)
    upload_loop(gm, field, ids[::-1])
    want = file_of(gm, N, color)
    if block:
        monkeypatch.setenv("CHISEL_HIP_MAP_BLOCK_CHUNKS", block)
    path = tmp_path / "map.chsl"
    gm.SaveMap(path)
    got = open(path, "rb").read()
    assert len(got) == len(want) and got == want
    fresh = new_map(N, color)
    upload_loop(fresh, field, sorted(field)[-2:])  # (a load replaces what is there)
    fresh.LoadMap(path)
    monkeypatch.delenv("CHISEL_HIP_MAP_BLOCK_CHUNKS", raising=False)
    fields_bits_equal(gm.fields(), fresh.fields(), "loaded")
    assert to_update(fresh) == []
    hc.check_invariants(fresh.hash_table(), "loaded")
    # a truncated file: the records in front of the cut are in the map, the load fails
    cut = tmp_path / "cut.chsl"
    record = 12 + gm.V * (12 if color else 8)
    open(cut, "wb").write(want[:32 + 5 * record + 100])
    if block:
        monkeypatch.setenv("CHISEL_HIP_MAP_BLOCK_CHUNKS", block)
    refused(lambda: fresh.LoadMap(cut), 6, "truncated")
    assert list(map(tuple, fresh.GetChunkIDs().tolist())) == ids[:5]
    # a file that names an id twice: the later record wins, as it did chunk by chunk
    twice = tmp_path / "twice.chsl"
    recs = [want[32 + k * record:32 + (k + 1) * record] for k in range(4)]
    again = struct.pack("<3i", *ids[1]) + recs[3][12:]
    open(twice, "wb").write(want[:24] + struct.pack("<q", 5) + b"".join(recs[:3]) + again + recs[3])
    fresh.LoadMap(twice)
    assert list(map(tuple, fresh.GetChunkIDs().tolist())) == ids[:4]
    assert_same(fresh.GetChunk(ids[1])[0], gm.GetChunk(ids[3])[0], "the later record")
    gm.close()
    fresh.close()


# ---- lifetime -------------------------------------------------------------------------------------------------------------------------
def test_scatter_gather_cycles_return_their_memory():
    from tests.test_gpu_lifetime import run_cycles
    N, n, max_chunks = 16, 600, 1024
    footprint = max_chunks * N ** 3 * 12  # sdf, weight and colour of the fixed pool: 50 MB
    rng = np.random.default_rng(6)
    ids = [(x, y, z) for x in range(10) for y in range(10) for z in range(6)][:n]
    sdf = rng.standard_normal((n, N ** 3)).astype(np.float32)
    w = np.ones((n, N ** 3), np.float32)

    def cycle():
        m = new_map(N, True, max_chunks=max_chunks)
        assert m.ScatterChunks(ids, sdf, w) == n  # (host arrays: 30 MB staged on the device)
        got = m.GatherChunks(sdf=True, weight=False, rgbw=False)
        assert len(got["ids"]) == n
        m.close()

    run_cycles(cycle, footprint)


# ---- the facade -----------------------------------------------------------------------------------------------------------------------
def weighted_sum(a):
    """facade_chunks.cpp's checksum: sum of (index + 1) x word over the array's 32-bit words, modulo 2^64"""
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((w * np.arange(1, len(w) + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_the_facade_program_gathers_what_python_gathers():
    """cvids_amd/open_chisel/tests/facade_chunks.cpp: ChunkManager::GatherChunks against the walk over GetChunks(), ScatterChunks into a
    second chisel::Chisel and back, std::out_of_range for an absent id -- and the ids and a checksum per array it prints against
    Python's gather of the same three frames"""
    from cvids_amd import chisel as ch
    tdir = os.path.join(ROOT, "cvids_amd", "open_chisel", "tests")
    exe = os.path.join(tdir, "facade_chunks")
    subprocess.check_call(["make", "-C", tdir, "chunks"])  # (make decides whether the binary is current)
    run_ = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run_.returncode == 0 and "facade_chunks ok" in run_.stdout, run_.stdout + run_.stderr
    lines = dict(l.split(" ", 1) for l in run_.stdout.splitlines() if " " in l)
    W, H, N = 64, 48, 8
    gm = ch.Chisel((N, N, N), RES, True)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    cam = ch.PinholeCamera(52.5, 52.5, 31.5, 23.5, W, H, 0.05, 5.0)
    v, u = np.mgrid[0:H, 0:W]
    color = np.stack([(7 * u + 13 * v + 50 * c) & 255 for c in range(3)], -1).astype(np.uint8)
    pose = np.eye(4, dtype=np.float32)
    for k in range(3):
        depth = (1.5 + 0.25 * k + 0.0078125 * u - 0.00390625 * v).astype(np.float32)  # (every term exact in binary)
        gm.IntegrateDepthScanColor(integ, depth, pose, cam, color, pose, cam)
    got = gm.GatherChunks()
    assert len(got["ids"]) >= 8
    assert [int(x) for x in lines["ids"].split()] == got["ids"].reshape(-1).tolist()
    for name in ("sdf", "weight", "rgbw"):
        assert int(lines[name], 16) == weighted_sum(got[name]), name
    gm.close()
