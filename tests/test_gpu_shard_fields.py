"""The sharded mesh recompute on hand-built voxel fields, every rank against the oracle on its own view (tests/shard_views.py).

The sharded tests of tests/test_gpu_mesh.py run on one smooth integrated scene with every chunk dirty.  Here the fields
of tests/voxel_fields.py -- every border cube occupied, every shipped voxel changing some output element -- go into shards of one map
(Chisel(..., n_shards, shard_rank, shard_block) on device 0, driven by LocalShardGroup: shell_jobs_kernel / shell_items_kernel, the
export kernels, shell_ensure_ghosts* and the box writers, update_meshes_planned, shell_reset_boxes_kernel / shell_remove_ghosts_kernel).
A field is uploaded with AddChunk on the owners, which leaves nothing dirty; a dirty set is marked by scattering those chunks' own voxels
back with mark_updated.  Per rank the expectation is an OracleMap of rank_view -- the rank's chunks plus the shell boxes by their
definition, default voxels elsewhere -- with the rank's jobs meshed: every array of every job equal as uint32, element for element, the
far-reading vertices included; everything that is no job untouched; no ghost and no residue left behind.
"""
import numpy as np
import pytest

from tests import shard_views as sv
from tests import voxel_fields as vf
from tests.common import compare_meshes

pytestmark = pytest.mark.gpu

SEED = 1
MAX_CHUNKS = 1024


class JobsOf:
    """one shard as compare_meshes sees a map: the meshes of this recompute's jobs only (the shard keeps those of earlier turns)"""

    def __init__(self, shard, jobs):
        self.shard, self.jobs = shard, set(jobs)

    def GetMeshIDs(self):
        ids = [i for i in map(tuple, self.shard.GetMeshIDs().tolist()) if i in self.jobs]
        return np.array(ids, np.int32).reshape(-1, 3)

    def GetMesh(self, cid):
        return self.shard.GetMesh(cid)


def mesh_bytes(shard):
    return {cid: {k: (v.tobytes() if v is not None else None) for k, v in shard.GetMesh(cid).items()} for cid in map(tuple, shard.GetMeshIDs().tolist())}


def field_bytes(shard):
    return {cid: tuple(a.tobytes() if a is not None else None for a in arrays) for cid, arrays in shard.fields().items()}


class ShardedField:
    """a field in the shards of one map, and the assertions every recompute is held to"""

    def __init__(self, oracle_mod, field, N, res, world, block, color=True):
        from cvids_amd import chisel as ch
        from cvids_amd.sharded import LocalShardGroup
        self.oracle_mod, self.N, self.res, self.world, self.block, self.color = oracle_mod, N, res, world, block, color
        self.field = field if color else {cid: (s, w, None) for cid, (s, w, _) in field.items()}
        self.shards = [ch.Chisel((N, N, N), res, color, device_id=0, max_chunks=MAX_CHUNKS, n_shards=world, shard_rank=r, shard_block=block)
                       for r in range(world)]
        self.group = LocalShardGroup(self.shards)
        for cid, (s, w, c) in self.field.items():
            self.shards[sv.owner(cid, world, block)].AddChunk(cid, s, w, c)
        for s_ in self.shards:
            assert len(s_.GetMeshesToUpdate()) == 0  # (AddChunk leaves nothing dirty)
        assert sum(s_.NumChunks() for s_ in self.shards) == len(field)

    def close(self):
        for s_ in self.shards:
            s_.close()

    def expectation(self, dirty):
        """-> (jobs, per rank (its jobs, its view, the oracle on that view with those jobs meshed))"""
        jobs = sv.job_ids(dirty)
        ranks = []
        for r in range(self.world):
            mine = sv.jobs_of(jobs, r, self.world, self.block)
            view = sv.rank_view(self.field, self.N, r, self.world, self.block, jobs)
            ranks.append((mine, view, sv.oracle_of(self.oracle_mod, view, self.N, self.res, self.color, mine)))
        return jobs, ranks

    def far_reading(self, ranks):
        """far-reading vertices of all ranks, from the oracle's vertex positions alone"""
        total = 0
        for mine, view, om in ranks:
            verts = [om.get_mesh(cid)["vertices"] for cid in map(tuple, om.mesh_ids().tolist())]
            if verts:
                total += int(sv.far_reading(view, self.field, self.N, self.res, np.concatenate(verts)).sum())
        return total

    def mark(self, dirty):
        """the chunks' own voxels scattered back on their owners, marked updated"""
        for r, s_ in enumerate(self.shards):
            ids = [i for i in dirty if sv.owner(i, self.world, self.block) == r]
            if not ids:
                continue
            rgbw = np.stack([self.field[i][2] for i in ids]) if self.color else None
            created = s_.ScatterChunks(ids, np.stack([self.field[i][0] for i in ids]), np.stack([self.field[i][1] for i in ids]), rgbw, mark_updated=True)
            assert created == 0
            assert len(s_.GetMeshesToUpdate()) > 0

    def turn(self, dirty, expected=None, **how):
        """one recompute of `dirty` and everything asserted after it -> (chunks compared, vertices compared, what UpdateMeshes returned)"""
        jobs, ranks = expected if expected is not None else self.expectation(dirty)
        self.mark(dirty)
        chunks = [s_.NumChunks() for s_ in self.shards]
        voxels = [field_bytes(s_) for s_ in self.shards]
        meshes = [mesh_bytes(s_) for s_ in self.shards]
        status = self.group.UpdateMeshes(force=True, **how)
        n = nv = 0
        for r, (s_, (mine, view, om)) in enumerate(zip(self.shards, ranks)):
            a, b = compare_meshes(om, JobsOf(s_, mine), self.color)
            n, nv = n + a, nv + b
            after = mesh_bytes(s_)
            assert all(sv.owner(cid, self.world, self.block) == r for cid in after)
            assert {cid for cid in after if cid not in jobs} == {cid for cid in meshes[r] if cid not in jobs}
            for cid, arrays in meshes[r].items():
                if cid not in jobs:
                    assert after[cid] == arrays, "rank %d: the mesh of %s, no job, changed" % (r, cid)
            assert len(s_.GetMeshesToUpdate()) == 0
            assert s_.NumChunks() == chunks[r], "rank %d: %d chunks before, %d after" % (r, chunks[r], s_.NumChunks())
            assert field_bytes(s_) == voxels[r], "rank %d: voxels changed" % r
        assert n == len([j for j in jobs if j in self.field])  # (every chunk of these fields has a surface: each resident job has a mesh)
        return n, nv, status

    def integrate_into_freed_slots(self):
        """a small point cloud beside the field: the chunks it creates take the slots the ghosts left, and an integration writes only
        the voxels of its band -- the others must be the default voxels a free slot holds (the pool invariant), as in the oracle"""
        from cvids_amd import chisel as ch
        from cvids_amd import synth
        from tests.common import compare_fields
        om = self.oracle_mod.OracleMap(self.N, self.res, self.color)
        om.set_integrator(self.oracle_mod.TRUNC_CONSTANT, 3.0 * self.res, 1.0, False, 0.05)
        for cid, (s, w, c) in self.field.items():
            om.put_chunk(cid, s, w, c)
        integ = ch.ProjectionIntegrator(ch.ConstantTruncator(3.0 * self.res), ch.ConstantWeighter(1.0), 0.05, False)
        edge = self.N * self.res
        top = np.array(max(self.field), np.float64) * edge
        g = np.linspace(-2.0 * edge, 2.0 * edge, 41)
        x, y = (a.reshape(-1) for a in np.meshgrid(g, g))
        # a tilted patch 1.5 m in front of a sensor at the origin, six chunks beside the field (depth limit: 2 m without colours)
        pts = np.stack([top[0] + 6.0 * edge + x, top[1] + 6.0 * edge + y, 1.5 + 0.3 * x], axis=1).astype(np.float32)
        col = np.random.default_rng(SEED + 3).random((len(pts), 3)).astype(np.float32) if self.color else None
        pose = synth.pose_yaw(0.0)
        before = sum(s_.NumChunks() for s_ in self.shards)
        om.integrate_pointcloud(pts, pose, col, 3.0 * self.res, 10.0)
        self.group.IntegratePointCloud(integ, (pts, col), pose, 3.0 * self.res, 10.0)
        got = {}
        for r, s_ in enumerate(self.shards):
            f = s_.fields()
            assert all(sv.owner(cid, self.world, self.block) == r for cid in f) and not (set(f) & set(got))
            got.update({cid: (a, b, c if c is not None else np.zeros((self.N ** 3, 4), np.uint8)) for cid, (a, b, c) in f.items()})
        created = len(got) - before
        assert created >= 40 and len(got) == om.num_chunks(), (created, len(got), om.num_chunks())
        compare_fields(om.fields(), got, om.V, self.color, atol=0.0, what="after a sharded recompute")
        return created

    def reuse_freed_slots(self):
        """one new owned chunk per shard, into a slot a ghost may have held: it reads back as uploaded"""
        rng = np.random.default_rng(SEED + 7)
        V = self.N ** 3
        top = max(self.field)
        for r, s_ in enumerate(self.shards):  # (ids in a row far beyond the field and beyond what integrate_into_freed_slots creates)
            cid = next((top[0] + 400 + k, top[1], top[2]) for k in range(200) if sv.owner((top[0] + 400 + k, top[1], top[2]), self.world, self.block) == r)
            s, w = rng.normal(size=V).astype(np.float32), rng.uniform(0, 3, V).astype(np.float32)
            c = rng.integers(0, 256, (V, 4), dtype=np.uint8) if self.color else None
            before = s_.NumChunks()
            s_.AddChunk(cid, s, w, c)
            gs, gw, gc = s_.GetChunk(cid)
            assert s_.NumChunks() == before + 1
            assert gs.tobytes() == s.tobytes() and gw.tobytes() == w.tobytes() and (not self.color or gc.tobytes() == c.tobytes()), (r, cid)


@pytest.fixture
def sharded(oracle_mod):
    made = []

    def make(family, N, edge, res, base, world, block, color=True):
        field = getattr(vf, family)(N, edge, SEED, res=res, base=base)
        made.append(ShardedField(oracle_mod, field, N, res, world, block, color))
        return made[-1]

    yield make
    for m in made:
        m.close()


# ---- a. every sharding, every chunk dirty ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [(0, 0, 0), (1000, -1000, 37)])
@pytest.mark.parametrize("world,block", [(2, 1), (2, 2), (3, 1), (3, 2), (8, 1), (8, 2)])
@pytest.mark.parametrize("family", ["dense", "thresholds"])
def test_every_sharding(sharded, family, world, block, base):
    """8^3 chunks, 4^3 of them, at res 0.03: a world that is no power of two, shard block 1, negative and large block coordinates in
    chunk_owner; in the dense field every cube on every chunk face is occupied, so every voxel of every shell changes a vertex, a
    normal or a colour"""
    m = sharded(family, 8, 4, 0.03, base, world, block)
    n, nv, _ = m.turn(sv.dirty_set("all", base))
    assert n == 64 and nv > 50000
    m.reuse_freed_slots()


# ---- b. dirty sets smaller than the map, turn after turn ---------------------------------------------------------------------------------
@pytest.mark.parametrize("world,block", [(8, 1), (2, 2)])
def test_dirty_sets_turn_after_turn(sharded, world, block):
    """the five dirty sets on one group, across the origin: `diagonal`, then `line`, whose jobs overlap the first turn's and whose ghosts
    reuse its slots, then the others.  Only here does the covering rule meet a face job that is missing or another rank's, neighbours that
    are not resident (found = 0) and job ids that are not resident (tests/test_shard_views.py asserts that these cases reach all of it)."""
    base = (-2, -2, -2)
    m = sharded("dense", 8, 4, 0.03, base, world, block)
    first = sv.job_ids(sv.dirty_set("diagonal", base))
    assert first & sv.job_ids(sv.dirty_set("line", base))
    for name in ("diagonal", "line", "one_inside", "corner", "all"):
        n, nv, _ = m.turn(sv.dirty_set(name, base))
        assert n > 0 and nv > 0, name
    m.integrate_into_freed_slots()
    m.reuse_freed_slots()


# ---- c. larger chunks: look-ups that land inside the map ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,edge,res,world", [(16, 3, 0.07, 3), (32, 2, 0.05, 2)])
def test_larger_chunks(sharded, N, edge, res, world):
    """16^3 and 32^3 chunks, shard block 1: InterpolateColor's look-ups at voxel indices taken for metres land inside the map (317 and
    369 far-reading vertices: tests/test_shard_views.py counts them on the same fields)"""
    m = sharded("dense", N, edge, res, (0, 0, 0), world, 1)
    dirty = vf.block_ids(edge)
    n, nv, _ = m.turn(dirty)
    assert n == edge ** 3
    m.reuse_freed_slots()


# ---- d. the cases with the most far-reading vertices -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,res,base", [("dense", 0.25, (-2, -2, -2)), ("thresholds", 1.0, (-1, -1, -1))])
def test_far_reading_vertices(sharded, family, res, base):
    """more than 500 vertices whose normal or colour is read outside what the shells serve (counted from the oracle's positions before
    anything is meshed on the device): the shard must answer them as the oracle on its view does -- default voxels in a ghost outside
    its boxes, no chunk where the rank holds none -- not as the whole map would"""
    m = sharded(family, 8, 4, res, base, 8, 1)
    dirty = sv.dirty_set("all", base)
    expected = m.expectation(dirty)
    far = m.far_reading(expected[1])
    print("%s res %g base %s: %d far-reading vertices" % (family, res, base, far))
    assert far > 500
    n, nv, _ = m.turn(dirty, expected)
    assert n == 64
    # a second turn with fewer, smaller ghosts in the slots the first turn's ghosts left: the far reads that land in a ghost outside its
    # boxes must find default voxels there, not what a ghost of the turn before held (shell_reset_boxes_kernel)
    dirty = sv.dirty_set("line", base)
    expected = m.expectation(dirty)
    assert m.far_reading(expected[1]) > 100
    n, nv, _ = m.turn(dirty, expected)
    assert n > 0 and nv > 0


# ---- e. a map without colour -------------------------------------------------------------------------------------------------------------
def test_map_without_colour(sharded):
    """8-byte payloads: the segments carry no colour plane"""
    m = sharded("thresholds", 8, 4, 0.03, (0, 0, 0), 8, 1, color=False)
    n, nv, _ = m.turn(sv.dirty_set("all"))
    assert n == 64 and nv > 0
    m.integrate_into_freed_slots()
    m.reuse_freed_slots()


# ---- f. the wait-free form ---------------------------------------------------------------------------------------------------------------
def test_wait_free_form(sharded):
    """turn 1 has nothing to size its segments from and takes the blocking form, turn 2 is wait-free, turn 3 gets segments of 64 bytes:
    called off on the device -- no ghost, no mesh, no flag cleared -- and made again the blocking way"""
    m = sharded("dense", 8, 4, 0.03, (0, 0, 0), 8, 1)
    _, _, st = m.turn(sv.dirty_set("all"), wait_free=True)
    assert st is None
    _, _, st = m.turn(sv.dirty_set("line"), wait_free=True)
    assert st[0] == 0 and st[3] > 0 and st[4] > 0
    assert getattr(m.group, "wait_free_aborts", 0) == 0
    _, _, st = m.turn(sv.dirty_set("diagonal"), wait_free=True, stride=64)
    assert st[0] == 4
    assert m.group.wait_free_aborts == 1
    m.integrate_into_freed_slots()
    m.reuse_freed_slots()


# ---- g. buffers that do not fit ----------------------------------------------------------------------------------------------------------
def test_recompute_that_outgrows_its_buffers(sharded, monkeypatch):
    """a triangle list of 256 entries and an arena of 4096 floats (CHISEL_HIP_MESH_TINY): the mesh step is emitted a second time, and
    the ghosts must still be there when it is"""
    monkeypatch.setenv("CHISEL_HIP_MESH_TINY", "1")
    m = sharded("dense", 8, 4, 0.03, (0, 0, 0), 2, 1)
    m.shards[0].set_profiling(True)
    n, nv, _ = m.turn(sv.dirty_set("all"))
    assert n == 64
    assert m.shards[0].profile()["mesh"]["launches"] >= 4  # count, emit, and both again (test_dense_recompute_that_outgrows_its_buffers)
    m.reuse_freed_slots()
