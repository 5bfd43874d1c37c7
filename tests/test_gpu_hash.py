"""The chunk hash under collisions, tombstones and wrap-around, on the GPU (the cases and builders: tests/hash_cases.py).

Every kernel reaches voxels through one open-addressed table whose probe loop is written out in many places (hash_find,
hash_find_quiescent, the cull kernel's look-up, create_chunk, find_chunk, ensure_chunk_kernel, remove_chunks_kernel, shell_ensure_ghost,
the merge's un-create).  The scenes of the other tests leave that table nearly empty; here it is crowded on purpose: a run of resident
"blocker" chunks across the table's end, blockers on the scene chunks' home buckets, tombstones where every second blocker was, and a
table without a single EMPTY bucket.  Each crowded test first shows on the device's own read-out (Chisel.hash_table()) that the case is
one -- scene chunks whose probe path crosses the end, is long, passes a tombstone -- and then holds the map to the oracle or to the
restatements exactly as the uncrowded tests do.  Every test ends with the table's invariants (hash_cases.check_invariants)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from cvids_amd import synth
from tests import hash_cases as hc
from tests import query_restated as qr
from tests import render_restated as rr
from tests.common import compare_fields, compare_meshes, fields_of, make_frames, same_bits, small_camera
from tests.test_gpu_parity import _mk

pytestmark = pytest.mark.gpu
N, RES, W, H = 8, 0.05, 64, 48
V = N ** 3
COUNTERS = ("sdf", "col", "col_sat", "probe", "carved", "updated_chunks")
_ORDER = {}


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def scene_ids(oracle_mod, scene):
    """the chunks the scene's first two frames create, in the oracle's order of creation (computed once per scene)"""
    if scene not in _ORDER:
        om = oracle_mod.OracleMap(N, RES, False)
        om.set_integrator(1, 2.0, 1.0, True, 0.05)
        _ORDER[scene] = hc.scene_order(om, make_frames(scene, 2, W, H), small_camera(W, H))
    return _ORDER[scene]


def stream(scene):
    """-> (the two frames that create the scene's chunks, two more and a frame that carves: a wall behind everything seen so far)"""
    frames = make_frames(scene, 4, W, H)
    return frames[:2], frames[2:] + [(np.full((H, W), 2.6, np.float32), synth.pose_yaw(0.0))]


def put_blockers(gm, om, blockers, first=0):
    for k, cid in enumerate(blockers, first):
        s, w, c = hc.blocker_voxels(k, V, gm.use_color)
        gm.AddChunk(cid, s, w, c)
        if om is not None:
            om.put_chunk(cid, s, w, c)


def drop(gm, om, ids):
    gm.GarbageCollect(ids)
    if om is not None:
        for c in ids:
            assert om.remove_chunk(c)
    hc.check_invariants(gm.hash_table(), "after a removal")


def run_frames(om, gm, integ, frames, cam, cimg=None, batch=False):
    """the frames into both maps with the checks of test_gpu_parity._run after every frame -- counters, chunk count, fields,
    meshes-to-update -- or, as one IntegrateBatch, after the batch; -> the oracle's counters summed"""
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    tot = dict.fromkeys(COUNTERS, 0)

    def check(what, want):
        got = gm.counters(reset=True)
        for k in COUNTERS:
            assert want[k] == got[k], "%s counter %s: oracle %d gpu %d" % (what, k, want[k], got[k])
        assert om.num_chunks() == gm.NumChunks(), "%s: chunk count" % what
        compare_fields(om.fields(), gm.fields(), om.V, om.use_color, what=what)
        assert sorted(map(tuple, om.meshes_to_update().tolist())) == sorted(map(tuple, gm.GetMeshesToUpdate().tolist())), what

    for i, (depth, pose) in enumerate(frames):
        if cimg is None:
            om.integrate_depth(depth, pose, intr, cam.near_plane, cam.far_plane)
        else:
            om.integrate_depth_color(depth, pose, intr, cimg, near=cam.near_plane, far=cam.far_plane)
        oc = om.counters()
        for k in COUNTERS:
            tot[k] += oc[k]
        if not batch:
            if cimg is None:
                gm.IntegrateDepthScan(integ, depth, pose, cam)
            else:
                gm.IntegrateDepthScanColor(integ, depth, pose, cam, cimg, pose, cam)
            check("frame %d" % i, oc)
    if batch:
        gm.IntegrateBatch(integ, [(d, p, cam) for d, p in frames], None if cimg is None else [(cimg, p, cam) for _, p in frames])
        check("batch", tot)
    return tot


def assert_reach(gm, ids, removed, what):
    """the floors every crowded test meets on the device's own read-out before it compares anything"""
    t = gm.hash_table()
    r = hc.reach(t, ids)
    print("%s: reach %s of %d scene chunks; %d keys, %d tombstones, %d empty buckets of %d" % (
        what, r, len(ids), len(hc.resident_keys(t)), hc.n_tombstones(t), hc.n_empty(t), t["capacity"]))
    assert r["cross"] >= 15, (what, r)
    assert r["long"] >= 20, (what, r)
    if removed:
        assert r["tomb"] >= 30, (what, r)
    return t


def crowded(oracle_mod, color, scene="wall", max_chunks=512, env=None, monkeypatch=None):
    """a map and its oracle with the run across the table's end set up: -> (om, gm, integ, scene ids, blockers, blockers to remove)"""
    if env:
        monkeypatch.setenv(env, "1")
    om, gm, integ = _mk(oracle_mod, N, RES, color, max_chunks=max_chunks)
    if env:
        monkeypatch.delenv(env, raising=False)
    cap = gm.hash_table()["capacity"]
    assert cap == 2 * max_chunks
    ids = scene_ids(oracle_mod, scene)
    blockers, removed = hc.run_across_end(cap, ids)
    assert len(blockers) + len(ids) <= max_chunks
    put_blockers(gm, om, blockers)
    return om, gm, integ, ids, blockers, removed


def crowded_after_removal(oracle_mod, color):
    """the crowded wall map after its first frames and the removal of every second blocker, its reach asserted:
    -> (om, gm, integ, cam, colour image or None, scene ids, the blockers left)"""
    om, gm, integ, ids, blockers, removed = crowded(oracle_mod, color)
    cam = small_camera(W, H)
    cimg = synth.render_color(W, H, 3) if color else None
    run_frames(om, gm, integ, stream("wall")[0], cam, cimg)
    assert_reach(gm, ids, False, "after the first frames")
    drop(gm, om, removed)
    assert_reach(gm, ids, True, "after the removal")
    gone = set(removed)
    return om, gm, integ, cam, cimg, ids, [b for b in blockers if b not in gone]


def scene_index(gm, left):
    """VoxelIndex over the scene's chunks alone: the blockers lie hundreds of chunks from every position the read paths are asked about
    (and a dense table over their box would not fit)"""
    far = set(left)
    fields = {cid: v for cid, v in gm.fields().items() if cid not in far}
    assert all(max(abs(c) for c in cid) < 100 for cid in fields)
    return rr.VoxelIndex(fields, N, RES), fields


# ---- host entries against the model ---------------------------------------------------------------------------------------------------
def test_host_entries_against_the_model():
    """400 random AddChunk / GarbageCollect / HasChunk / GetChunk on 32 ids that share 3 home buckets (one of them the last), against a
    dict and the table model; the collections hold duplicates and absent ids.  Every 50 operations: NumChunks, GetChunkIDs in ascending
    order, every chunk's voxels, and the read-out -- the model's keys, bucket for bucket (host entries run one after the other, so the
    first-EMPTY-or-TOMB rule fixes the layout)."""
    from cvids_amd import chisel as ch
    gm = ch.Chisel((N, N, N), RES, True, max_chunks=512)
    cap = gm.hash_table()["capacity"]
    ids = hc.colliding_ids(cap)
    absent = hc.far_ids(0, 1, cap, skip=10) + hc.far_ids(7, 2, cap)
    assert not set(absent) & set(ids)
    rng = np.random.default_rng(3)
    model, held = hc.TableModel(cap), {}
    wrapped = tombs = 0

    def compare(step):
        assert gm.NumChunks() == len(held), step
        assert list(map(tuple, gm.GetChunkIDs().tolist())) == sorted(held), step
        for cid, (s, w, c) in held.items():
            gs, gw, gc = gm.GetChunk(cid)
            assert np.array_equal(gs, s) and np.array_equal(gw, w) and np.array_equal(gc, c), (step, cid)
        t = gm.hash_table()
        assert hc.check_invariants(t, "step %d" % step) == len(held)
        assert hc.resident_ids(t) == model.ids() == sorted(held), step
        assert np.array_equal(t["hash_keys"], np.array(model.keys, np.uint64)), "step %d: the device's buckets are not the model's" % step
        return sum(hc.crosses_end(t, c) for c in held), sum(hc.tombstones_on_path(t, c) > 0 for c in held)

    for step in range(400):
        op = rng.random()
        c = ids[int(rng.integers(len(ids)))]
        if op < 0.4:
            s, w, col = hc.blocker_voxels(step, V, True)
            gm.AddChunk(c, s, w, col)  # (an id that is resident keeps its slot and takes the new voxels)
            held[c] = (s, w, col)
            model.insert(c)
        elif op < 0.65:
            pool = ids + absent
            pick = [pool[int(i)] for i in rng.integers(len(pool), size=int(rng.integers(1, 6)))]
            pick.append(pick[0])  # a duplicate
            gm.GarbageCollect(pick)
            for p in pick:
                held.pop(p, None)
                model.remove(p)
        elif op < 0.85:
            q = c if rng.random() < 0.8 else absent[int(rng.integers(len(absent)))]
            assert gm.HasChunk(q) == (q in held), (step, q)
        else:
            if c in held:
                gs, gw, gc = gm.GetChunk(c)
                assert np.array_equal(gs, held[c][0]) and np.array_equal(gc, held[c][2]), (step, c)
            else:
                with pytest.raises(KeyError):
                    gm.GetChunk(c)
        if (step + 1) % 50 == 0:
            a, b = compare(step)
            wrapped, tombs = wrapped + a, tombs + b
    print("over the 8 comparisons: %d resident ids across the end, %d behind a tombstone" % (wrapped, tombs))
    assert wrapped >= 8 and tombs >= 8  # (the case is one)
    gm.close()


# ---- integration in a crowded table, against the oracle -----------------------------------------------------------------------------
FORMS = {"default": None, "pipeline": "CHISEL_HIP_FORCE_PIPELINE", "uncertain": "CHISEL_HIP_FORCE_UNCERTAIN", "batch": None}
CROWDED = [("wall", color, form) for color in (False, True) for form in FORMS] + [("sphere_room", True, "default")]


def carve_only_items(env, integ, cam, monkeypatch):
    """work items of the carving frame on an empty map created under `env`: the chunks in front of the wall are absent and could only
    be carved, so the cull kernel drops them -- unless every candidate without a slot is handed to the integration kernel's look-up"""
    from cvids_amd import chisel as ch
    for k in FORMS.values():
        if k:
            monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(env, "1")
    m = ch.Chisel((N, N, N), RES, False, max_chunks=512)
    if env:
        monkeypatch.delenv(env, raising=False)
    depth, pose = stream("wall")[1][-1]
    m.IntegrateDepthScan(integ, depth, pose, cam)
    items, st = m.counters()["work_chunks"], m.launch_stats()
    m.close()
    return items, st


def assert_form_engaged(form, integ, cam, monkeypatch):
    """the environment hooks really select the forms: a map created under CHISEL_HIP_FORCE_PIPELINE never takes the single-stream form
    a waiting caller otherwise gets every time; one created under CHISEL_HIP_FORCE_UNCERTAIN also sends the candidates without a slot
    to the integration kernel's own look-up (find_chunk), which shows as work items that the other forms' cull drops"""
    hooked = any(os.environ.get(k) for k in FORMS.values() if k)  # (the suite run under a scheduling hook: no unforced form to compare with)
    plain, st_plain = carve_only_items(None, integ, cam, monkeypatch)
    assert hooked or st_plain["single_stream_sets"] == st_plain["launch_sets"] == 1
    if FORMS[form]:
        items, st = carve_only_items(FORMS[form], integ, cam, monkeypatch)
        assert st["launch_sets"] == 1 and st["single_stream_sets"] == 0, (form, st)
        print("%s: %d work items of the carving frame on an empty map, %d unforced" % (form, items, plain))
        assert hooked or ((items > plain) if form == "uncertain" else (items == plain)), (form, items, plain)
    return hooked


@pytest.mark.parametrize("scene,color,form", CROWDED, ids=lambda v: str(v))
def test_integration_in_a_crowded_table(oracle_mod, monkeypatch, scene, color, form):
    """The run across the end (blockers mirrored into the oracle), the scene's first frames, every second blocker removed on both sides,
    two more frames and one that carves and creates 160 chunks in a table full of tombstones, then the meshes.  The forced forms send
    the look-ups of the integration kernel through find_chunk; `batch` hands each group of frames to one IntegrateBatch."""
    om, gm, integ, ids, blockers, removed = crowded(oracle_mod, color, scene, 512 if scene == "wall" else 1024, FORMS[form], monkeypatch)
    cam = small_camera(W, H)
    hooked = assert_form_engaged(form, integ, cam, monkeypatch)
    cimg = synth.render_color(W, H, 3) if color else None
    first, later = stream(scene)
    run_frames(om, gm, integ, first, cam, cimg, batch=(form == "batch"))
    assert sorted(ids) == sorted(set(map(tuple, om.chunk_ids().tolist())) - set(blockers))
    assert_reach(gm, ids, False, "after the first frames")
    drop(gm, om, removed)
    assert_reach(gm, ids, True, "after the removal")
    tot = run_frames(om, gm, integ, later, cam, cimg, batch=(form == "batch"))
    assert tot["carved"] > 200 and om.num_chunks() - (len(blockers) - len(removed)) > len(ids) + 50  # (it carved, and created chunks)
    om.update_meshes(force=True)
    gm.UpdateMeshes(force=True)
    n, nv = compare_meshes(om, gm, color)
    assert n > 10 and nv > 500
    st = gm.launch_stats()  # (this map's own launches: never the single-stream form under a forced form, always for a caller that waits)
    assert st["launch_sets"] >= 2 and (hooked or st["single_stream_sets"] == (0 if FORMS[form] else st["launch_sets"])), (form, st)
    hc.check_invariants(gm.hash_table(), "at the end")
    gm.close()


# ---- a table with no empty bucket ---------------------------------------------------------------------------------------------------
def test_table_without_an_empty_bucket(oracle_mod):
    """One far id per bucket uploaded and collected, in three rounds that fit the pool: every bucket a tombstone.  Every look-up of an
    absent id is now a scan of the whole table, ended by the loop's bound alone.  The stream of the crowded test on it, HasChunk of
    100 absent ids, then the pool filled exactly: one chunk more is refused with CHISEL_HIP_ERR_POOL_FULL and the map is what it was."""
    from cvids_amd.capi import ChiselHipError
    om, gm, integ = _mk(oracle_mod, N, RES, False, max_chunks=512)
    cap = gm.hash_table()["capacity"]
    rounds = hc.saturation_rounds(cap, 400)
    assert len(rounds) == 3
    for r in rounds:
        put_blockers(gm, None, r)
        gm.GarbageCollect(r)
    t = gm.hash_table()
    assert hc.n_empty(t) == 0 and hc.n_tombstones(t) == cap and gm.NumChunks() == 0
    hc.check_invariants(t, "saturated")
    cam = small_camera(W, H)
    first, later = stream("wall")
    tot = run_frames(om, gm, integ, first + later, cam)
    assert tot["carved"] > 200
    t = gm.hash_table()
    print("after the stream: %d keys, %d tombstones, %d empty" % (len(hc.resident_keys(t)), hc.n_tombstones(t), hc.n_empty(t)))
    assert hc.n_empty(t) == 0
    om.update_meshes(force=True)
    gm.UpdateMeshes(force=True)
    n, nv = compare_meshes(om, gm, False)
    assert n > 10 and nv > 500
    for h in range(0, cap, cap // 100)[:100]:
        assert not gm.HasChunk(hc.far_ids(h, 1, cap, skip=1)[0])
    free = 512 - gm.NumChunks()
    assert 100 < free < cap
    extra = [hc.far_ids(h, 1, cap, skip=1)[0] for h in range(free)]
    put_blockers(gm, om, extra)
    assert gm.NumChunks() == 512 == gm.pool_info()["committed"]
    s, w, _ = hc.blocker_voxels(7, V)
    with pytest.raises(ChiselHipError) as e:
        gm.AddChunk(hc.far_ids(5, 1, cap, skip=2)[0], s, w)
    assert e.value.code == 3
    gm.synchronize()  # (the refusal is not latched: the map is complete)
    assert gm.NumChunks() == 512 == om.num_chunks()
    assert list(map(tuple, gm.GetChunkIDs().tolist())) == sorted(map(tuple, om.chunk_ids().tolist()))
    compare_fields(om.fields(), gm.fields(), V, False, what="full pool")
    t = gm.hash_table()
    assert hc.check_invariants(t, "full pool") == 512 and hc.n_empty(t) == 0 and t["free_top"] == 0
    assert not gm.HasChunk(hc.far_ids(5, 1, cap, skip=2)[0])
    gm.close()


# ---- read paths ---------------------------------------------------------------------------------------------------------------------
def test_read_paths_on_the_crowded_map(oracle_mod):
    """QueryPoints at 2 000 points -- two thirds around the wall, a third in absent chunks next to resident ones -- against the oracle's
    query_points (found bits, distance, gradient), the restatement (weight) and chisel_hip_shade_vertices (colour); CastRays and a
    32 x 24 RenderView against the restatements bit for bit, from the stream's pose and from one whose rays leave the scene (the box
    of created ids, opened on every side by the blockers, no longer ends them early)."""
    from tests import test_gpu_query as tgq
    from tests import test_gpu_render as tgr
    om, gm, integ, cam, cimg, ids, left = crowded_after_removal(oracle_mod, True)
    index, fields = scene_index(gm, left)
    rng = np.random.default_rng(synth.SEED)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    pose = synth.trajectory_pose(1)
    hits = rr.hit_points(pose, intr, synth.render_depth("wall", pose, intr, W, H))
    near = qr.jitter_points(hits, RES, rng, n=1334)
    resident = set(fields)
    beside = sorted({(x + dx, y + dy, z + dz) for x, y, z in resident for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)} - resident)
    pick = np.array([beside[int(i)] for i in rng.integers(len(beside), size=666)], np.float64)
    away = ((pick + rng.uniform(0.02, 0.98, pick.shape)) * (N * RES)).astype(np.float32)
    assert not (index.rows(index.chunk_ids(away)) >= 0).any()
    pts = np.concatenate([near, away])
    found, sdf, grad = om.query_points(pts)
    got = gm.QueryPoints(pts, sdf=True, weight=True, gradient=True, colors=True)
    assert np.array_equal(got["found"], found), "found differs at %d places" % int((got["found"] != found).sum())
    has, has_g = (found & 1).astype(bool), (found & 2).astype(bool)
    print("points: found %.3f, gradient %.3f" % (has.mean(), has_g.mean()))
    assert has[:1334].mean() > 0.5 and has_g.mean() > 0.2 and not found[1334:].any()
    assert np.array_equal(got["sdf"][has].view(np.uint32), sdf[has].astype(np.float32).view(np.uint32)) and np.isnan(got["sdf"][~has]).all()
    assert np.array_equal(got["gradient"][has_g].view(np.uint32), grad[has_g].view(np.uint32)) and np.isnan(got["gradient"][~has_g]).all()
    r_found, r_sdf, r_weight = qr.query_points(index, pts)
    assert np.array_equal(r_found, has)
    same_bits(got["sdf"], r_sdf, "sdf against the restatement")
    same_bits(got["weight"], r_weight, "weight")
    _, want_c = tgr.shade(gm, pts, np.zeros((len(pts), 3), np.float32))
    same_bits(got["colors"], want_c, "colours")
    assert (want_c[:1334] > 0).any()
    small = small_camera(32, 24)
    sintr = (small.fx, small.fy, small.cx, small.cy)
    for what, p, lo, hi in (("the stream's pose", pose, 0.9, 1.01), ("rays that leave the scene", synth.pose_yaw(55.0), 0.02, 0.9)):
        rays = qr.unit_rays(p, sintr, 32, 24)
        out = tgq.check_rays(gm, index, rays, 0.0, what)
        share = float((out["status"] == 1).mean())
        d = tgr.check_depth(gm, index, p, small, 0.0, what)
        print("%s: %.3f of the rays hit, %.3f of the pixels" % (what, share, float(np.isfinite(d).mean())))
        assert lo < share < hi, (what, share)
    hc.check_invariants(gm.hash_table(), "at the end")
    gm.close()


# ---- writers that share the table ---------------------------------------------------------------------------------------------------
def test_merge_into_the_crowded_map(oracle_mod):
    """MergeMap of a rotated 2^3 block into the crowded wall map (the blockers are in the destination only) against merge_restated:
    chunk-id sets, voxels, stats -- at a pose at which destination chunks are created and others created and taken out again"""
    from cvids_amd import chisel as ch
    from tests import merge_restated as mr
    from tests import voxel_fields as vf
    om, dst, integ, cam, cimg, ids, left = crowded_after_removal(oracle_mod, True)
    src_f = vf.thresholds(N, 2, 11, res=RES, base=(-1, -1, -1))
    pose = mr._pose(mr._rot(2, 25.0) @ mr._rot(1, -17.0) @ mr._rot(0, 33.0), (0.1, -0.05, 2.0))
    src = ch.Chisel((N, N, N), RES, True, max_chunks=512)
    for cid, (s, w, c) in src_f.items():
        src.AddChunk(cid, s, w, c)
    dst_f = fields_of(dst, N)
    want, wstats, _ = mr.merge(dst_f, src_f, pose, N, RES)
    uncreated = [c for c in mr.padded_candidate_ids(src_f, pose, N, RES) if c not in want]
    t0 = dst.hash_table()
    stats = dst.MergeMap(src, pose)
    print(stats, "candidates created and taken out again: %d" % len(uncreated))
    assert stats == {k: wstats[k] for k in stats}, (stats, wstats)
    assert stats["dst_chunks_created"] >= 3 and len(uncreated) >= 3 and stats["dst_chunks_updated"] > stats["dst_chunks_created"]
    mr.assert_fields_bit_equal(want, fields_of(dst, N), True, "merged")
    t1 = dst.hash_table()
    assert hc.check_invariants(t1, "after the merge") == len(want)
    assert set(hc.resident_ids(t1)) - set(hc.resident_ids(t0)) == set(want) - set(dst_f)
    assert_reach(dst, ids, True, "after the merge")
    src.close()
    dst.close()


def test_deintegration_on_the_crowded_map(oracle_mod):
    """a frame from the side into the crowded map and out again (deintegrate_gpu.take_out: the restatement over the map's own fields),
    the chunks it reports empty collected, then the frame again at a shifted pose against the oracle started from the map's fields"""
    from tests import deintegrate_restated as dr
    from tests.deintegrate_gpu import take_out
    om, gm, integ, cam, _, ids, left = crowded_after_removal(oracle_mod, False)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    rules = dr.Rules(1, 2.0, 1.0, True, 0.05, False)
    side = synth.pose_yaw(10.0, (0.3, 0.0, 0.0))
    depth = synth.render_depth("wall", side, intr, W, H)
    n0 = gm.NumChunks()
    gm.IntegrateDepthScan(integ, depth, side, cam)
    assert gm.NumChunks() >= n0 + 10  # (chunks of its own, created in front of tombstones)
    _, wstats, detail, got = take_out(gm, (depth, side, intr), rules, intr + (cam.near_plane, cam.far_plane), N)
    assert wstats["chunks_emptied"] >= 10 and wstats["chunks_touched"] > wstats["chunks_emptied"]
    hc.check_invariants(gm.hash_table(), "after the de-integration")
    gm.GarbageCollect(got["emptied_ids"])
    t = gm.hash_table()
    assert hc.check_invariants(t, "after the collection") == gm.NumChunks() < n0 + 25
    assert not set(map(tuple, got["emptied_ids"].tolist())) & set(hc.resident_ids(t))
    assert_reach(gm, ids, True, "after the collection")
    om2 = oracle_mod.OracleMap(N, RES, False)
    om2.set_integrator(1, 2.0, 1.0, True, 0.05)
    for cid, (s, w, _) in gm.fields().items():
        om2.put_chunk(cid, s, w)
    shifted = synth.pose_yaw(10.0, (0.33, 0.01, 0.0))
    om2.integrate_depth(depth, shifted, intr, cam.near_plane, cam.far_plane)
    gm.IntegrateDepthScan(integ, depth, shifted, cam)
    assert om2.num_chunks() == gm.NumChunks()
    compare_fields(om2.fields(), gm.fields(), V, False, what="the frame again")
    hc.check_invariants(gm.hash_table(), "at the end")
    gm.close()


def test_point_cloud_into_the_crowded_map(oracle_mod):
    """one coloured cloud through IntegratePointCloud against the oracle (test_gpu_cloud._step: counters, chunk count, fields,
    meshes-to-update)"""
    from tests import test_gpu_cloud as tgc
    om, gm, integ, cam, cimg, ids, left = crowded_after_removal(oracle_mod, True)
    n0 = gm.NumChunks()
    pts, col, pose = tgc._cloud("wall", 4, W, H, 1.0, True)
    oc = tgc._step(om, gm, integ, pts, col, pose, what="cloud")
    print("cloud: %d points, %d chunks created, counters %s" % (len(pts), gm.NumChunks() - n0, {k: oc[k] for k in ("sdf", "visited", "candidates")}))
    assert oc["sdf"] > 1000
    assert_reach(gm, ids, True, "after the cloud")
    hc.check_invariants(gm.hash_table(), "at the end")
    gm.close()


# ---- save and load ------------------------------------------------------------------------------------------------------------------
def test_save_and_load_of_the_crowded_map(oracle_mod, tmp_path):
    """SaveMap of the crowded map, LoadMap into a fresh map and into the same map: no tombstone afterwards, the same keys, equal
    fields, and a follow-on frame agrees with the oracle on both"""
    from cvids_amd import chisel as ch
    om, gm, integ, cam, cimg, ids, left = crowded_after_removal(oracle_mod, True)
    path = tmp_path / "crowded.map"
    gm.SaveMap(path)
    before = gm.fields()
    keys = hc.resident_ids(gm.hash_table())
    assert hc.n_tombstones(gm.hash_table()) > 100
    fresh = ch.Chisel((N, N, N), RES, True, max_chunks=512)
    fresh.LoadMap(path)
    gm.LoadMap(path)
    depth, pose = make_frames("wall", 3, W, H)[2]
    om.integrate_depth_color(depth, pose, (cam.fx, cam.fy, cam.cx, cam.cy), cimg, near=cam.near_plane, far=cam.far_plane)
    for what, m in (("a fresh map", fresh), ("the same map", gm)):
        t = m.hash_table()
        assert hc.check_invariants(t, what) == len(keys)
        assert hc.n_tombstones(t) == 0 and hc.resident_ids(t) == keys, what
        compare_fields(before, m.fields(), V, True, what=what)
        m.IntegrateDepthScanColor(integ, depth, pose, cam, cimg, pose, cam)
        assert m.NumChunks() == om.num_chunks()
        compare_fields(om.fields(), m.fields(), V, True, what=what + ", follow-on frame")
        hc.check_invariants(m.hash_table(), what + " at the end")
        m.close()


# ---- ghosts ---------------------------------------------------------------------------------------------------------------------------
def test_ghosts_in_crowded_tables(oracle_mod):
    """Two shards on one GPU, each rank's table pre-crowded with blockers it owns; five recomputes with a frame in front of each.  In
    front of each recompute the reach floors on the ranks' read-outs (at least 15 scene chunks across the end, 20 with a probe length
    >= 8, the two ranks together); after each: the invariants on every rank, the ghosts gone, and the union of the shards' meshes equal to the unsharded map's.  The
    tombstones each recompute leaves behind are printed (EXPERIMENTS.md records them)."""
    from cvids_amd import chisel as ch
    from cvids_amd.sharded import LocalShardGroup
    n_shards = 2
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    whole = ch.Chisel((N, N, N), RES, True, max_chunks=512)
    shards = [ch.Chisel((N, N, N), RES, True, max_chunks=512, n_shards=n_shards, shard_rank=r) for r in range(n_shards)]
    group = LocalShardGroup(shards)
    cam = small_camera(W, H)
    cimg = synth.render_color(W, H, 3)
    ids = scene_ids(oracle_mod, "wall")
    cap = shards[0].hash_table()["capacity"]
    for r, s_ in enumerate(shards):
        blockers, _ = hc.run_across_end(cap, ids, owner=lambda c: ch.chunk_owner(c, n_shards, 2) == r)
        put_blockers(s_, None, blockers)
        hc.check_invariants(s_.hash_table(), "rank %d crowded" % r)

    class Union:
        def GetMeshIDs(self):
            got = [s_.GetMeshIDs() for s_ in shards]
            return np.concatenate([i for i in got if len(i)], axis=0) if any(len(i) for i in got) else np.zeros((0, 3), np.int32)

        def GetMesh(self, cid):
            return shards[ch.chunk_owner(cid, n_shards, 2)].GetMesh(cid)

    class Whole:  # the unsharded map with the oracle's method names, for compare_meshes
        def mesh_ids(self):
            return whole.GetMeshIDs()

        def get_mesh(self, cid):
            return whole.GetMesh(cid)

    def reach_of_the_ranks(k, when):
        """each rank's scene chunks on its own read-out; the floors hold for the two ranks together (each owns half the scene)"""
        total = dict.fromkeys(("off_home", "long", "cross", "tomb"), 0)
        for r, s_ in enumerate(shards):
            t = s_.hash_table()
            hc.check_invariants(t, "rank %d %s recompute %d" % (r, when, k))
            own = [c for c in ids if ch.chunk_owner(c, n_shards, 2) == r and hc.bucket_of(t, c) >= 0]
            reach = hc.reach(t, own)
            print("recompute %d, %s, rank %d: %d keys, %d tombstones, reach of its %d scene chunks %s" % (
                k, when, r, len(hc.resident_keys(t)), hc.n_tombstones(t), len(own), reach))
            for key in total:
                total[key] += reach[key]
        return total

    for k, (depth, pose) in enumerate(make_frames("wall", 5, W, H)):
        for m in [whole] + shards:
            m.IntegrateDepthScanColor(integ, depth, pose, cam, cimg, pose, cam)
        total = reach_of_the_ranks(k, "before")
        assert total["cross"] >= 15 and total["long"] >= 20, (k, total)
        before = [s_.NumChunks() for s_ in shards]
        whole.UpdateMeshes(force=True)
        group.UpdateMeshes(force=True, wait_free=(k >= 2))
        for s_ in shards:
            s_.synchronize()
        n, nv = compare_meshes(Whole(), Union(), True)
        assert n > 10 and nv > 500
        assert [s_.NumChunks() for s_ in shards] == before and group.ghost_bytes > 0  # (there were ghosts, and they are gone)
        reach_of_the_ranks(k, "after")
    for m in [whole] + shards:
        m.close()


# ---- id bounds ------------------------------------------------------------------------------------------------------------------------
def _same_readout(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("hash_keys", "hash_vals", "slot_key", "free_list")) and a["free_top"] == b["free_top"]


def test_chunks_at_the_accepted_extremes():
    from cvids_amd import chisel as ch
    gm = ch.Chisel((N, N, N), RES, True, max_chunks=512)
    lo, hi = hc.ID_MIN, hc.ID_MAX
    ids = [tuple(v if a == axis else 0 for a in range(3)) for axis in range(3) for v in (lo, hi)] + [(lo, lo, lo), (hi, hi, hi), (lo, hi, -1), (hi, -1, lo)]
    put_blockers(gm, None, ids)
    assert list(map(tuple, gm.GetChunkIDs().tolist())) == sorted(ids)
    t = gm.hash_table()
    assert hc.check_invariants(t, "extremes") == len(ids) and hc.resident_ids(t) == sorted(ids)
    for k, cid in enumerate(ids):
        s, w, c = hc.blocker_voxels(k, V, True)
        gs, gw, gc = gm.GetChunk(cid)
        assert gm.HasChunk(cid) and np.array_equal(gs, s) and np.array_equal(gw, w) and np.array_equal(gc, c), cid
    assert not gm.HasChunk((hi - 1, 0, 0)) and not gm.HasChunk((0, lo + 1, 0))
    gm.GarbageCollect(ids[::2])
    assert list(map(tuple, gm.GetChunkIDs().tolist())) == sorted(ids[1::2])
    hc.check_invariants(gm.hash_table(), "half collected")
    gm.GarbageCollect(ids)
    assert gm.NumChunks() == 0 and hc.check_invariants(gm.hash_table(), "all collected") == 0
    gm.close()


def test_ids_outside_the_range_are_refused():
    """every entry that takes a chunk id from its caller answers CHISEL_HIP_ERR_INVALID for one past each bound, +-2^20, +-2^21 and
    INT32_MIN / MAX on every axis, and leaves the table as it was -- also where the id would pack to the key of a resident chunk"""
    from cvids_amd import chisel as ch
    from cvids_amd.capi import ChiselHipError
    gm = ch.Chisel((N, N, N), RES, True, max_chunks=512)
    alias_of = ((1 << 20) + 5, 0, 0)
    victim = hc.unpack_id(hc.pack_id(*alias_of))
    assert victim == (5 - (1 << 20), 1, 0) and all(hc.ID_MIN <= v <= hc.ID_MAX for v in victim)
    good = [(1, 2, 3), victim, (hc.ID_MAX, 0, 0)]
    put_blockers(gm, None, good)
    t0 = gm.hash_table()
    cam = small_camera(W, H)
    frame, keep = ch.depth_frame(np.full((H, W), 1.0, np.float32), synth.pose_yaw(0.0), cam)
    bad_values = (hc.ID_MAX + 1, hc.ID_MIN - 1, 1 << 20, -(1 << 20), 1 << 21, -(1 << 21), 2 ** 31 - 1, -(2 ** 31))
    bad = [alias_of] + [tuple(v if a == axis else (1, 2, 3)[a] for a in range(3)) for axis in range(3) for v in bad_values]
    s, w, c = hc.blocker_voxels(99, V, True)
    cid3 = lambda cid: (C.c_int * 3)(*cid)

    def entries(cid):
        upd, nv, ng = C.c_int(0), C.c_int64(0), C.c_int64(0)
        L, h, i3 = gm.L, gm.h, cid3(cid)
        mesh = {"mesh_size": lambda: ch.check(L.chisel_hip_mesh_size(h, i3, C.byref(nv), C.byref(ng))),
                "download_mesh": lambda: ch.check(L.chisel_hip_download_mesh(h, i3, None, None, None, None)),
                "generate_mesh": lambda: ch.check(L.chisel_hip_generate_mesh(h, i3, 1, 0, 0, None, None, None, None, C.byref(nv), C.byref(ng))),
                "mesh_cube": lambda: ch.check(L.chisel_hip_mesh_cube(h, i3, cid3((0, 0, 0)), (C.c_float * 3)(), None, None, C.byref(upd), C.byref(upd)))}
        return {**mesh, "AddChunk": lambda: gm.AddChunk(cid, s, w, c), "HasChunk": lambda: gm.HasChunk(cid), "GetChunk": lambda: gm.GetChunk(cid),
                "GarbageCollect": lambda: gm.GarbageCollect([good[0], cid, good[1]]), "UpdateMeshesOf": lambda: gm.UpdateMeshesOf([good[0], cid]),
                "integrate_chunk": lambda: ch.check(gm.L.chisel_hip_integrate_chunk(gm.h, cid3(cid), C.byref(frame), None, C.byref(upd))),
                "recompute_mesh": lambda: ch.check(gm.L.chisel_hip_recompute_mesh(gm.h, cid3(cid)))}

    for cid in bad:
        for name, call in entries(cid).items():
            with pytest.raises(ChiselHipError) as e:
                call()
            assert e.value.code == 1 and "range" in str(e.value), (name, cid, str(e.value))
    assert _same_readout(t0, gm.hash_table())
    assert gm.NumChunks() == 3 and list(map(tuple, gm.GetChunkIDs().tolist())) == sorted(good)
    hc.check_invariants(gm.hash_table(), "at the end")
    served = entries(good[0])  # (the same calls with an id inside the range are served)
    served["AddChunk"]()
    assert served["HasChunk"]() and np.array_equal(served["GetChunk"]()[0], s)
    gm.close()


def test_load_map_refuses_a_file_with_an_id_outside_the_range(tmp_path):
    """a file whose second chunk has an id that would pack to the key of (5 - 2^20, 1, 0): the load fails, nothing is entered under that key"""
    from cvids_amd import chisel as ch
    from cvids_amd.capi import ChiselHipError
    alias_of = ((1 << 20) + 5, 0, 0)
    victim = hc.unpack_id(hc.pack_id(*alias_of))
    path = tmp_path / "bad.map"
    with open(path, "wb") as f:  # header + records, as chisel_hip_save_map writes them (no colour)
        f.write(b"CHSLHIP1" + struct.pack("<ifiiq", N, RES, 0, 0, 3))
        for k, cid in enumerate([(1, 2, 3), alias_of, (4, 5, 6)]):
            s, w, _ = hc.blocker_voxels(k, V)
            f.write(struct.pack("<3i", *cid) + s.tobytes() + w.tobytes())
    gm = ch.Chisel((N, N, N), RES, False, max_chunks=512)
    put_blockers(gm, None, [(7, 7, 7)])
    with pytest.raises(ChiselHipError) as e:
        gm.LoadMap(path)
    assert e.value.code == 1 and "range" in str(e.value)
    t = gm.hash_table()
    hc.check_invariants(t, "after the refused load")
    assert set(hc.resident_ids(t)) <= {(1, 2, 3)} and not gm.HasChunk(victim) and not gm.HasChunk((4, 5, 6))
    good = tmp_path / "good.map"
    with open(good, "wb") as f:
        f.write(b"CHSLHIP1" + struct.pack("<ifiiq", N, RES, 0, 0, 2))
        for k, cid in enumerate([(1, 2, 3), (hc.ID_MIN, hc.ID_MAX, 0)]):
            s, w, _ = hc.blocker_voxels(k, V)
            f.write(struct.pack("<3i", *cid) + s.tobytes() + w.tobytes())
    gm.LoadMap(good)  # (the layout written here is the one the library reads)
    assert list(map(tuple, gm.GetChunkIDs().tolist())) == [(hc.ID_MIN, hc.ID_MAX, 0), (1, 2, 3)]
    assert np.array_equal(gm.GetChunk((1, 2, 3))[0], hc.blocker_voxels(0, V)[0])
    hc.check_invariants(gm.hash_table(), "after the load")
    gm.close()
