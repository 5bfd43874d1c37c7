"""One map in an in-process group (Chisel(..., devices=...): cvids_amd/csrc/host_group.h) on hand-built voxel fields (TEST INFRASTRUCTURE).

A group takes AddChunk, routed to the owner, which leaves nothing dirty, and refuses ScatterChunks; so a dirty set is made by
INTEGRATION, on the oracle and on the group alike: a depth frame that is NaN everywhere except a 3 x 3 patch at the projection of every
target chunk's centre, holding that centre's camera depth (Rig.sparse_frame), under ConstantTruncator(1.5 res), ConstantWeighter(1),
carving off.  The reference's band is the truncation plus 2 sqrt(3) res (ProjectionIntegrator.h), about five voxels either way along
the ray: with 8^3 chunks the target and its two z-neighbours change -- some of them new chunks outside the block --, with 16^3 and
32^3 chunks the target alone.  What changed, what is to be meshed and every voxel come from the whole-map oracle after the frame
(OracleSide); what a rank's meshes must be comes from the oracle on that rank's view (tests/shard_views.py), as in the sharded tests.

`python -m tests.group_fields turns|settles ...` runs a sequence in a process of its own: the hooks that force the rare routes of the
group's settle() are read once per process, and CHISEL_HIP_HOST_TIMING=1 makes the library print one line per recompute form and per
settle on stderr, which `routes` parses for the parent.
"""
import collections
import os
import re
import subprocess
import sys

import numpy as np

from cvids_amd import synth
from tests import shard_views as sv
from tests import voxel_fields as vf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1
W, H = 160, 120
OFFSET = (0.13, 0.09, -2.1)  # camera position: block centre + OFFSET x block edge, identity rotation (looking along +z)
MAX_CHUNKS = {8: 4096, 16: 1024, 32: 512}  # per shard
COUNTERS = ("sdf", "col", "col_sat", "probe", "carved", "updated_chunks")
TURN_ORDER = ("corner", "all", "line", "one_inside", "diagonal")
SETTLERS = ("GetMesh", "GetMeshIDs", "GetMeshesToUpdate", "NumChunks", "GetChunk", "AddChunk", "IntegrateDepthScan", "GarbageCollect",
            "SaveAllMeshesToPLY", "SaveMap", "counters", "Reset", "close")

Spec = collections.namedtuple("Spec", "family N B res base color offset focal")
Spec.__new__.__defaults__ = (True, OFFSET, 1.0)

# every (field, frames) the GPU tests run, with the shardings they run it on: (spec, turns, ((world, shard block), ...))
CASES = {
    "dense_origin": (Spec("dense", 8, 4, 0.03, (0, 0, 0)), ("all",), ((2, 1), (2, 2), (3, 1), (3, 2), (8, 1), (8, 2))),
    "dense_far_ids": (Spec("dense", 8, 4, 0.03, (1000, -1000, 37)), ("all",), ((2, 1), (2, 2), (3, 1), (3, 2), (8, 1), (8, 2))),
    "thresholds_origin": (Spec("thresholds", 8, 4, 0.03, (0, 0, 0)), ("all",), ((2, 1), (2, 2), (3, 1), (3, 2), (8, 1), (8, 2))),
    "thresholds_far_ids": (Spec("thresholds", 8, 4, 0.03, (1000, -1000, 37)), ("all",), ((2, 1), (2, 2), (3, 1), (3, 2), (8, 1), (8, 2))),
    "turns": (Spec("dense", 8, 4, 0.03, (-2, -2, -2)), TURN_ORDER, ((8, 1), (2, 2), (8, 2))),
    # (a checked turn of `all`, then the other four back to back with nothing but the frames between the recomputes: see main)
    "chain": (Spec("dense", 8, 4, 0.03, (-2, -2, -2)), ("all", "line", "one_inside", "diagonal", "corner"), ((8, 1), (2, 2))),
    "settles": (Spec("dense", 8, 4, 0.03, (-2, -2, -2)), ("all", "line", "one_inside"), ((3, 1),)),
    "chunks_16": (Spec("dense", 16, 3, 0.07, (0, 0, 0)), ("all",), ((3, 1),)),
    "chunks_32": (Spec("dense", 32, 2, 0.05, (0, 0, 0)), ("all",), ((2, 1),)),
    "no_colour": (Spec("thresholds", 8, 4, 0.03, (0, 0, 0), False), ("all",), ((8, 1),)),
    "far_dense": (Spec("dense", 8, 4, 0.25, (-2, -2, -2)), ("all", "line"), ((8, 1),)),
    # (res 1.0: a block edge is 32 m and the reference drops depths beyond 50 m, so the camera stands closer and sees wider)
    "far_thresholds": (Spec("thresholds", 8, 4, 1.0, (-1, -1, -1), True, (0.13, 0.09, -0.9), 0.35), ("all", "line"), ((8, 1),)),
    # (the turns of this case are `all`, OracleSide.collected_frame with `line`, `diagonal`: see main)
    "overflow": (Spec("dense", 8, 4, 0.03, (0, 0, 0)), ("all",), ((2, 1),)),
    "regrow": (Spec("dense", 16, 4, 0.03, (0, 0, 0)), ("corner", "all", "line"), ((2, 1),)),
}
# turn 1 of the far-reading cases must have more than this many far-reading vertices over all ranks, turn 2 more than that
FAR_READING = {"far_dense": (500, 100), "far_thresholds": (500, 100)}


def targets_of(name, B, base):
    """the dirty sets of tests/shard_views.py in a 4^3 block; in a smaller one `all`, `corner` and `one_inside` by the same rule"""
    if B == sv.B:
        return sv.dirty_set(name, base)
    ids = {"all": vf.block_ids(B), "corner": [(0, 0, 0)], "one_inside": [(1, 1, 1)]}[name]
    return [(int(base[0]) + x, int(base[1]) + y, int(base[2]) + z) for x, y, z in ids]


# Where the frame of `all` does not change a target and its z-neighbours: ids relative to the base that do not change / change besides.
# The four targets of column (2, 2) lie next to the optical axis and project within two pixels of each other, so the patches of the
# nearer ones are covered and only (2, 2, 2) and (2, 2, 3) are seen.  Under the wide camera of the res-1.0 case the rays are oblique:
# the band misses the z-neighbour in front of twelve targets of the nearest layer and reaches the neighbour beside four others.
_AXIS = (((2, 2, -1), (2, 2, 0), (2, 2, 1)), ())
NOT_AS_INTENDED = {
    ("regrow", "all"): (((2, 2, 0), (2, 2, 1)), ()),
    ("far_thresholds", "all"): (((0, 0, -1), (0, 1, -1), (0, 2, -1), (0, 3, -1), (1, 0, -1), (1, 2, -1), (2, 0, -1), (2, 2, -1), (3, 0, -1), (3, 1, -1),
                                 (3, 2, -1), (3, 3, -1)), ((-1, 0, 1), (-1, 1, 1), (-1, 2, 1), (-1, 3, 1))),
}
NOT_AS_INTENDED.update({(case, "all"): _AXIS for case in ("dense_origin", "dense_far_ids", "thresholds_origin", "thresholds_far_ids", "turns", "chain", "settles",
                                                          "no_colour", "far_dense", "overflow")})


def intended(case, name):
    """the chunks the sparse frame of turn `name` of a case changes: every target, with 8^3 chunks its two z-neighbours as well (the band
    reaches into them), but for the exceptions of NOT_AS_INTENDED"""
    spec = CASES[case][0]
    out = set(targets_of(name, spec.B, spec.base))
    if spec.N == 8:
        out |= {(x, y, z + d) for x, y, z in set(out) for d in (-1, 1)}
    less, more = NOT_AS_INTENDED.get((case, name), ((), ()))
    at = lambda ids: {(spec.base[0] + x, spec.base[1] + y, spec.base[2] + z) for x, y, z in ids}
    assert at(less) <= out and not (at(more) & out)
    return (out - at(less)) | at(more)


# ---- the camera and its frames --------------------------------------------------------------------------------------------------------
class Rig:
    """a pinhole camera in front of a block of B^3 chunks, its distance and far plane in block edges"""

    def __init__(self, spec):
        self.spec = spec
        self.chunk = spec.N * float(spec.res)
        self.block = spec.B * self.chunk
        fx, fy, cx, cy = synth.intrinsics(W, H)
        self.intr = (fx * spec.focal, fy * spec.focal, cx, cy)
        centre = (np.array(spec.base, np.float64) + spec.B / 2.0) * self.chunk
        self.position = centre + np.array(spec.offset, np.float64) * self.block
        self.near, self.far = 0.05, (abs(spec.offset[2]) + 0.75) * self.block

    def camera(self, intr=None, far=None):
        from cvids_amd.chisel import PinholeCamera
        fx, fy, cx, cy = self.intr if intr is None else intr
        return PinholeCamera(fx, fy, cx, cy, W, H, self.near, self.far if far is None else far)

    def pose(self, shift=(0.0, 0.0, 0.0)):
        p = np.eye(4, dtype=np.float64)
        p[:3, 3] = self.position + np.array(shift, np.float64) * self.block
        return p.astype(np.float32)

    def sparse_frame(self, targets):
        """NaN but for a 3 x 3 patch per target, written in the order of `targets` -> (depth, pose, the targets whose patch is whole).
        The targets of the column next to the optical axis project within a pixel or two of each other: a later patch covers an earlier
        one, wholly or in part, so with `all` a few targets may or may not be seen; no patch of the smaller sets touches another."""
        depth = np.full((H, W), np.nan, np.float32)
        index = np.full((H, W), -1, np.int64)
        fx, fy, cx, cy = self.intr
        for k, t in enumerate(targets):
            c = (np.array(t, np.float64) + 0.5) * self.chunk - self.position
            u, v = int(round(fx * c[0] / c[2] + cx)), int(round(fy * c[1] / c[2] + cy))
            assert 1 <= u < W - 1 and 1 <= v < H - 1 and self.near < c[2] < min(self.far, 50.0), (t, u, v, c[2])
            depth[v - 1:v + 2, u - 1:u + 2] = c[2]
            index[v - 1:v + 2, u - 1:u + 2] = k
        whole = np.bincount(index[index >= 0], minlength=len(targets)) == 9
        return depth, self.pose(), [tuple(t) for k, t in enumerate(targets) if whole[k]]

    def beside_frame(self):
        """a tilted plane seen from three block edges beside the field: chunks that no frame of a case has touched"""
        u = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
        depth = np.full((H, W), np.nan, np.float32)
        plane = (abs(self.spec.offset[2]) - 0.2) * self.block * (1.0 + 0.25 * (u - self.intr[2]) / W)
        depth[10:H - 10, 10:W - 10] = plane[10:H - 10, 10:W - 10]
        return depth, self.pose((3.0, 0.0, 0.0))

    def wide_frame(self):
        """a tilted plane over the whole image of a camera 0.35 times as long, eight block edges beside the field: a few thousand
        chunks -> (depth, pose, intrinsics, far plane)"""
        fx, fy, cx, cy = synth.intrinsics(W, H)
        u = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
        depth = (2.6 * self.block * (1.0 + 0.25 * (u - cx) / W)).astype(np.float32)
        return depth, self.pose((8.0, 0.0, 0.0)), (0.35 * fx, 0.35 * fy, cx, cy), 4.0 * self.block


# ---- the whole-map oracle, frame after frame ------------------------------------------------------------------------------------------
def _bits(arrays):
    return tuple(np.ascontiguousarray(a).tobytes() if a is not None else None for a in arrays)


def field_bits(fields):
    return {tuple(int(v) for v in cid): _bits(arrays) for cid, arrays in fields.items()}


Frame = collections.namedtuple("Frame", "targets whole depth pose field changed new jobs counters view collect")
Frame.__new__.__defaults__ = (None, ())


class OracleSide:
    """the field in the whole-map oracle; `frame` integrates one sparse frame and says what it did"""

    def __init__(self, oracle_mod, spec):
        self.oracle_mod, self.spec, self.rig = oracle_mod, spec, Rig(spec)
        field = getattr(vf, spec.family)(spec.N, spec.B, SEED, res=spec.res, base=spec.base)
        self.initial = field if spec.color else {cid: (s, w, None) for cid, (s, w, _) in field.items()}
        self.om = None
        self.reset()

    def reset(self):
        s = self.spec
        self.om = self.oracle_mod.OracleMap(s.N, s.res, s.color)
        self.om.set_integrator(self.oracle_mod.TRUNC_CONSTANT, 1.5 * s.res, 1.0, False, 0.05)
        for cid, (a, b, c) in self.initial.items():
            self.om.put_chunk(cid, a, b, c)
        assert len(self.om.meshes_to_update()) == 0

    def integrate(self, depth, pose, view=None):
        intr, far = (self.rig.intr, self.rig.far) if view is None else view
        self.om.integrate_depth(depth, pose, intr, self.rig.near, far)
        return self.om.counters()

    def collected_frame(self, keep=False):
        """the wide frame, and every chunk it changed garbage-collected again: their entries of the set to mesh stay (Chisel.h:228), so
        the set is the 27-neighbourhoods of some thousand chunks that are gone; `keep` leaves the set to mesh as it is, for a frame
        that follows in the same turn"""
        depth, pose, intr, far = self.rig.wide_frame()
        before = field_bits(self.om.fields())
        counters = self.integrate(depth, pose, (intr, far))
        after = field_bits(self.om.fields())
        changed = sorted(cid for cid in after if before.get(cid) != after[cid])
        assert all(cid not in before for cid in changed)  # (beside the field: new chunks only)
        for cid in changed:
            assert self.om.remove_chunk(cid)
        jobs = set(map(tuple, self.om.meshes_to_update().tolist()))
        if not keep:
            self.om.update_meshes(force=True)
        return Frame([], [], depth, pose, self.om.fields(), changed, changed, jobs, counters, (intr, far), changed)

    def frame(self, name):
        targets = targets_of(name, self.spec.B, self.spec.base)
        depth, pose, whole = self.rig.sparse_frame(targets)
        before = field_bits(self.om.fields())
        counters = self.integrate(depth, pose)
        field = self.om.fields()
        after = field_bits(field)
        changed = sorted(cid for cid in after if before.get(cid) != after[cid])
        assert set(before) <= set(after)
        jobs = set(map(tuple, self.om.meshes_to_update().tolist()))
        self.om.update_meshes(force=True)  # (the set is emptied as the group's recompute empties its own)
        return Frame(targets, whole, depth, pose, field, changed, [cid for cid in changed if cid not in before], jobs, counters)


def reach(field, N, jobs, world, block):
    """what a recompute of `jobs` on `field` reaches in a sharding -> (the most owners any rank receives resident ghosts from, jobs
    that are not resident, ranks without a job)"""
    owners = 0
    for r in range(world):
        ghosts = sv.ghost_masks(jobs, r, world, block, N)
        owners = max(owners, len({sv.owner(g, world, block) for g in ghosts if g in field}))
    idle = [r for r in range(world) if not sv.jobs_of(jobs, r, world, block)]
    return owners, len([j for j in jobs if j not in field]), idle


def most_entries(frame, world, block):
    """the longest dirty list a shard hands in after `collected_frame`: the 27-neighbourhoods of the chunks it owned, each id once"""
    return max(len(sv.job_ids([cid for cid in frame.collect if sv.owner(cid, world, block) == r])) for r in range(world))


def largest_segment_voxels(field, N, jobs, world, block):
    """the voxels of the largest (owner -> rank) segment, from the boxes of the definition alone (resident ghosts only)"""
    most = 0
    for r in range(world):
        per = collections.Counter()
        for g, mask in sv.ghost_masks(jobs, r, world, block, N).items():
            if g in field:
                per[sv.owner(g, world, block)] += int(mask.sum())
        most = max([most] + list(per.values()))
    return most


# ---- the group ---------------------------------------------------------------------------------------------------------------------------
Expected = collections.namedtuple("Expected", "frame ranks mesh_ids earlier")


class _MeshesOf:
    """an oracle as compare_meshes sees it, its meshes of `ids` only"""

    def __init__(self, om, ids):
        self.om, self.ids = om, set(ids)

    def mesh_ids(self):
        return np.array([i for i in map(tuple, self.om.mesh_ids().tolist()) if i in self.ids], np.int32).reshape(-1, 3)

    def get_mesh(self, cid):
        return self.om.get_mesh(cid)


class GroupField:
    """a field in a group beside the whole-map oracle, and the assertions every recompute is held to"""

    def __init__(self, oracle_mod, spec, world, block, devices=None):
        from cvids_amd import chisel as ch
        from tests.test_gpu_group import _devices
        self.spec, self.world, self.block = spec, world, block
        self.side = OracleSide(oracle_mod, spec)
        self.cam = self.side.rig.camera()
        self.integ = ch.ProjectionIntegrator(ch.ConstantTruncator(1.5 * spec.res), ch.ConstantWeighter(1.0), 0.05, False)
        self.grp = ch.Chisel((spec.N,) * 3, spec.res, spec.color, max_chunks=MAX_CHUNKS[spec.N], shard_block=block,
                             devices=_devices(world) if devices is None else devices)
        self.upload()

    def close(self):
        self.grp.close()

    def upload(self):
        for cid, (s, w, c) in self.side.initial.items():
            self.grp.AddChunk(cid, s, w, c)
        assert len(self.grp.GetMeshesToUpdate()) == 0  # (AddChunk leaves nothing dirty)
        assert self.grp.NumChunks() == len(self.side.initial)
        self.grp.counters(reset=True)

    def owner(self, cid):
        return sv.owner(cid, self.world, self.block)

    def mesh_bits(self):
        return {cid: {k: (v.tobytes() if v is not None else None) for k, v in self.grp.GetMesh(cid).items()}
                for cid in map(tuple, self.grp.GetMeshIDs().tolist())}

    def integrate(self, depth, pose, counters, view=None, then=lambda: None):
        """one frame into the group; its counters are the oracle's (`then` is called between the frame and the read of the counters)"""
        self.grp.IntegrateDepthScan(self.integ, depth, pose, self.cam if view is None else self.side.rig.camera(*view))
        then()
        got = self.grp.counters(reset=True)
        for k in COUNTERS:
            assert counters[k] == got[k], "counter %s: oracle %d group %d" % (k, counters[k], got[k])
        assert counters["created"] - counters["collected"] == got["new_chunks"], (counters["created"], counters["collected"], got["new_chunks"])

    def same_voxels(self, what):
        """chunk count, chunk set and every voxel of the group equal the whole-map oracle's, bit for bit"""
        want, got = field_bits(self.side.om.fields()), field_bits(self.grp.fields())
        assert self.grp.NumChunks() == self.side.om.num_chunks() == len(got), (what, self.grp.NumChunks(), self.side.om.num_chunks(), len(got))
        assert sorted(want) == sorted(got), "%s: chunk ids differ" % what
        for cid in want:
            assert want[cid] == got[cid], "%s: voxels of %s differ" % (what, cid)

    def expectation(self, frame, earlier):
        """per rank (its jobs, the oracle on its view with those jobs meshed), and the mesh ids the group must list afterwards"""
        s = self.spec
        ranks, ids = [], {cid for cid in earlier if cid not in frame.jobs}
        for r in range(self.world):
            mine = sv.jobs_of(frame.jobs, r, self.world, self.block)
            view = sv.rank_view(frame.field, s.N, r, self.world, self.block, frame.jobs)
            om = sv.oracle_of(self.side.oracle_mod, view, s.N, s.res, s.color, mine)
            ranks.append((mine, view, om))
            ids |= set(map(tuple, om.mesh_ids().tolist()))
        return Expected(frame, ranks, ids, earlier)

    def far_reading(self, exp):
        total = 0
        for mine, view, om in exp.ranks:
            verts = [om.get_mesh(cid)["vertices"] for cid in map(tuple, om.mesh_ids().tolist())]
            if verts:
                total += int(sv.far_reading(view, exp.frame.field, self.spec.N, self.spec.res, np.concatenate(verts)).sum())
        return total

    def begin(self, name):
        """the frame into the oracle and the group, the expectations, UpdateMeshes(force) -- and no call into the group after it"""
        frames = [self.side.frame(name)] if isinstance(name, str) else list(name)  # (frames of one turn: the last one holds the field and the whole set)
        name = name if isinstance(name, str) else "frames of its own"
        for frame in frames:
            self.integrate(frame.depth, frame.pose, frame.counters, frame.view)
            if len(frame.collect):
                self.grp.GarbageCollect(np.array(frame.collect, np.int32))
        assert sorted(map(tuple, self.grp.GetMeshesToUpdate().tolist())) == sorted(frame.jobs), "%s: the sets to mesh differ" % name
        self.same_voxels("after the frame of " + name)
        exp = self.expectation(frame, self.mesh_bits())
        self.grp.UpdateMeshes(force=True)
        return exp

    def check(self, exp, dirty=(), collected=None):
        """everything a finished recompute is held to -> (job meshes compared, vertices compared); `dirty`: what a frame after the
        recompute left to mesh; `collected`: a job's chunk that was garbage-collected after it"""
        from tests.common import compare_meshes
        from tests.test_gpu_shard_fields import JobsOf
        grp, jobs = self.grp, exp.frame.jobs
        listed = set(map(tuple, grp.GetMeshIDs().tolist()))
        assert listed == exp.mesh_ids or (collected is not None and listed == exp.mesh_ids - {collected}), (
            "mesh ids: %d listed, %d expected" % (len(listed), len(exp.mesh_ids)))
        n = nv = 0
        for r, (mine, view, om) in enumerate(exp.ranks):
            assert all(self.owner(j) == r for j in mine)
            if collected is not None and collected not in listed and collected in mine:
                mine = [j for j in mine if j != collected]
                om = sv.oracle_of(self.side.oracle_mod, view, self.spec.N, self.spec.res, self.spec.color, mine)
            a, b = compare_meshes(om, JobsOf(grp, mine), self.spec.color)
            n, nv = n + a, nv + b
        after = self.mesh_bits()
        for cid, arrays in exp.earlier.items():
            if cid not in jobs:
                assert after[cid] == arrays, "the mesh of %s, no job, changed" % (cid,)
        assert sorted(map(tuple, grp.GetMeshesToUpdate().tolist())) == sorted(dirty)
        self.same_voxels("after the recompute")  # (no ghost stayed, no voxel changed)
        return n, nv

    def turn(self, name):
        return self.check(self.begin(name))

    def back_to_back(self, names):
        """IntegrateDepthScan, UpdateMeshes(force) per name and nothing else in between -- no read-out that would synchronise the shards,
        so the event chains between consecutive recomputes and the settle inside the next frame are all that orders them --, then
        everything checked at once: a job's mesh is that of the last recompute that had it as a job, on the rank's view of the field
        as it was then -> (job meshes compared, vertices compared)"""
        from tests.common import compare_meshes
        from tests.test_gpu_shard_fields import JobsOf
        earlier = self.mesh_bits()
        self.grp.counters(reset=True)
        frames = [self.side.frame(name) for name in names]
        exps = [self.expectation(f, earlier) for f in frames]
        for f in frames:
            self.grp.IntegrateDepthScan(self.integ, f.depth, f.pose, self.cam)
            self.grp.UpdateMeshes(force=True)
        got = self.grp.counters(reset=True)
        for k in COUNTERS:
            assert sum(f.counters[k] for f in frames) == got[k], (k, got[k])
        n = nv = 0
        later, listed = set(), {cid for cid in earlier}
        for exp in reversed(exps):
            for r, (mine, view, om) in enumerate(exp.ranks):
                last = [j for j in mine if j not in later]  # the jobs this recompute was the last to mesh
                a, b = compare_meshes(_MeshesOf(om, last), JobsOf(self.grp, last), self.spec.color)
                n, nv = n + a, nv + b
            later |= exp.frame.jobs
        for exp in exps:  # (in order: a job without a mesh loses the one it had)
            listed = {cid for cid in listed if cid not in exp.frame.jobs} | {cid for _, _, om in exp.ranks for cid in map(tuple, om.mesh_ids().tolist())}
        after = self.mesh_bits()
        assert set(after) == listed, (len(after), len(listed))
        for cid, arrays in earlier.items():
            if cid not in later:
                assert after[cid] == arrays, "the mesh of %s, no job, changed" % (cid,)
        assert len(self.grp.GetMeshesToUpdate()) == 0
        self.same_voxels("after %d recomputes back to back" % len(names))
        return n, nv

    def finish(self):
        """a frame well beside the field -- its chunks take slots the ghosts left, and the voxels an integration does not write must be
        the default voxels a free slot holds --, then one AddChunk per shard that reads back as uploaded"""
        depth, pose = self.side.rig.beside_frame()
        before = self.side.om.num_chunks()
        self.integrate(depth, pose, self.side.integrate(depth, pose))
        created = self.side.om.num_chunks() - before
        assert created >= 20, created
        self.same_voxels("after a frame beside the field")
        rng = np.random.default_rng(SEED + 7)
        V = self.spec.N ** 3
        top = max(self.side.initial)
        for r in range(self.world):
            cid = next((top[0] + 400 + k, top[1], top[2]) for k in range(200) if self.owner((top[0] + 400 + k, top[1], top[2])) == r)
            s, w = rng.normal(size=V).astype(np.float32), rng.uniform(0, 3, V).astype(np.float32)
            c = rng.integers(0, 256, (V, 4), dtype=np.uint8) if self.spec.color else None
            count = self.grp.NumChunks()
            self.grp.AddChunk(cid, s, w, c)
            gs, gw, gc = self.grp.GetChunk(cid)
            assert self.grp.NumChunks() == count + 1
            assert gs.tobytes() == s.tobytes() and gw.tobytes() == w.tobytes() and (c is None or gc.tobytes() == c.tobytes()), (r, cid)
        return created


# ---- who settles: the first call into the group after a wait-free UpdateMeshes ----------------------------------------------------------
def settle_case(oracle_mod, who, tmp, note=lambda text: None):
    """the turns of CASES["settles"]; after the last UpdateMeshes the first call into the group is `who`: a reader must see the finished
    recompute, a writer must act on the map after it"""
    spec, turns, ((world, block),) = CASES["settles"]
    m = GroupField(oracle_mod, spec, world, block)
    om = m.side.om
    for name in turns[:-1]:
        note("turn " + name)
        m.turn(name)
    note("last " + who)
    exp = m.begin(turns[-1])
    job = next(j for mine, _, o in exp.ranks for j in mine if o.get_mesh(j) is not None and j in exp.frame.field)  # a job with a chunk and a mesh
    dirty, collected = (), None
    done = lambda: note("after " + who)  # right after the first call: whatever settles must have settled by then
    rng = np.random.default_rng(SEED + 11)
    V = spec.N ** 3
    far_chunk = ((spec.base[0] + 40, spec.base[1] - 40, spec.base[2] + 7), rng.normal(size=V).astype(np.float32), rng.uniform(0, 3, V).astype(np.float32),
                 rng.integers(0, 256, (V, 4), dtype=np.uint8))
    nxt = m.side.frame("corner") if who == "IntegrateDepthScan" else None
    if who == "GetMesh":
        got = m.grp.GetMesh(job)
        done()
        want = exp.ranks[m.owner(job)][2].get_mesh(job)
        for key in ("vertices", "normals", "colors", "grids"):
            assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), (job, key)
    elif who == "GetMeshIDs":
        got = m.grp.GetMeshIDs()
        done()
        assert set(map(tuple, got.tolist())) == exp.mesh_ids
    elif who == "GetMeshesToUpdate":
        got = m.grp.GetMeshesToUpdate()
        done()
        assert len(got) == 0
    elif who == "NumChunks":
        got = m.grp.NumChunks()
        done()
        assert got == om.num_chunks()
    elif who == "GetChunk":
        got = m.grp.GetChunk(job)
        done()
        assert _bits(got) == _bits(om.get_chunk(job))
    elif who == "AddChunk":
        m.grp.AddChunk(*far_chunk)
        done()
        om.put_chunk(*far_chunk)
    elif who == "IntegrateDepthScan":
        m.integrate(nxt.depth, nxt.pose, nxt.counters, then=done)
        dirty = nxt.jobs
    elif who == "GarbageCollect":
        m.grp.GarbageCollect(np.array([job], np.int32))
        done()
        assert om.remove_chunk(job)
        collected = job
    elif who in ("SaveAllMeshesToPLY", "SaveMap"):
        getattr(m.grp, who)(os.path.join(tmp, "first"))
        done()
    elif who == "counters":
        got = m.grp.counters()
        done()
        assert got["sdf"] == 0 and got["new_chunks"] == 0  # (read and reset after the frame: the recompute counts nothing)
    elif who == "Reset":
        m.grp.Reset()
        done()
        assert m.grp.NumChunks() == 0 and len(m.grp.GetMeshIDs()) == 0 and len(m.grp.GetMeshesToUpdate()) == 0
        m.side.reset()
        m.upload()
        note("again")
        m.turn("all")  # an empty group takes a field and a turn again
        m.turn("line")
        m.close()
        return
    elif who == "close":
        m.close()
        done()
        return
    else:
        raise ValueError(who)
    n, nv = m.check(exp, dirty, collected)
    assert n > 0 and nv > 0
    if who in ("SaveAllMeshesToPLY", "SaveMap"):  # the file written first thing equals the file of the recompute that has been checked
        getattr(m.grp, who)(os.path.join(tmp, "second"))
        first, second = (open(os.path.join(tmp, f), "rb").read() for f in ("first", "second"))
        assert len(first) > 1000 and first == second
    m.close()


# ---- a sequence in a process of its own ---------------------------------------------------------------------------------------------------
BLOCKING, WAIT_FREE = "blocking", "wait-free"
_LINES = ((re.compile(r"^chisel_hip group recompute, host us:"), lambda mt: BLOCKING),
          (re.compile(r"^chisel_hip group recompute \(wait-free\), host us:"), lambda mt: WAIT_FREE),
          (re.compile(r"^chisel_hip group settle, host us:.*\| status (-?\d+)\s*$"), lambda mt: int(mt.group(1))),
          (re.compile(r"^## (.*)$"), lambda mt: "## " + mt.group(1)))


def routes(stderr):
    """the library's timing lines and the child's own section marks, in order: BLOCKING, WAIT_FREE, a settle's status word (int), '## mark'"""
    out = []
    for line in stderr.splitlines():
        for pattern, what in _LINES:
            mt = pattern.match(line.strip())
            if mt:
                out.append(what(mt))
    return out


def sections(events):
    """-> [(mark, [events after it])]"""
    out = [("", [])]
    for e in events:
        if isinstance(e, str) and e.startswith("## "):
            out.append((e[3:], []))
        else:
            out[-1][1].append(e)
    return out


def run_child(args, hooks, timeout):
    """python -m tests.group_fields `args` in a fresh process with `hooks` set -> (CompletedProcess, routes of its stderr)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CHISEL_HIP_GROUP_") and k not in ("CHISEL_HIP_MESH_TINY",)}
    env.update(hooks, CHISEL_HIP_HOST_TIMING="1")
    out = subprocess.run([sys.executable, "-m", "tests.group_fields"] + list(args), cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    return out, routes(out.stderr)


def _note(text):
    sys.stdout.flush()
    print("## " + text, file=sys.stderr, flush=True)


def main(argv):
    import tempfile
    import oracle
    oracle.build()
    failed = 0
    if argv[0] == "turns":  # turns WORLD BLOCK: the five dirty sets on one group
        spec, turns, _ = CASES["turns"]
        m = GroupField(oracle, spec, int(argv[1]), int(argv[2]))
        for name in turns:
            _note("turn " + name)
            n, nv = m.turn(name)
            assert n > 0 and nv > 0, name
        _note("finish")
        m.finish()
        m.close()
    elif argv[0] == "chain":  # chain WORLD BLOCK: a checked turn, then recomputes back to back with only a frame between them
        spec, turns, _ = CASES["chain"]
        m = GroupField(oracle, spec, int(argv[1]), int(argv[2]))
        _note("turn " + turns[0])
        m.turn(turns[0])
        _note("turn chain")
        n, nv = m.back_to_back(turns[1:])
        assert n > 0 and nv > 0
        _note("finish")
        m.finish()
        m.close()
    elif argv[0] == "overflow":  # a turn, then a set to mesh that is longer than a shard's list
        spec, _, ((world, block),) = CASES["overflow"]
        m = GroupField(oracle, spec, world, block)
        _note("turn all")
        m.turn("all")
        frame = m.side.collected_frame(keep=True)
        assert most_entries(frame, world, block) > 4096
        line = m.side.frame("line")
        assert line.jobs == frame.jobs | sv.job_ids(line.changed)
        _note("turn collected")
        n, nv = m.check(m.begin([frame, line]))
        assert n > 0 and nv > 0
        _note("turn diagonal")
        m.turn("diagonal")
        _note("finish")
        m.finish()
        m.close()
    elif argv[0] == "settles":  # settles WHO...: one group per first call
        for who in argv[1:]:
            with tempfile.TemporaryDirectory() as tmp:
                try:
                    settle_case(oracle, who, tmp, _note)
                except AssertionError:  # a mismatch: the next case has a group of its own
                    import traceback
                    traceback.print_exc()
                    print("FAILED " + who, flush=True)
                    failed += 1
                    continue
                # (any other exception ends the process: an error of the library or the device serves no further case)
            print("ok " + who, flush=True)
        if failed:
            return 1
    else:
        raise SystemExit("usage: python -m tests.group_fields turns WORLD BLOCK | chain WORLD BLOCK | overflow | settles WHO...")
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
