"""The mesh, query and ray kernels against the oracle on hand-built voxel fields (tests/voxel_fields.py).

The integrated scenes of the other GPU tests are smooth: 29 of the 256 marching-cubes configurations, no weight in (0, 0.5], no
crossing edge with a difference below 6.8e-5, no -0.0, no denormal, a few dozen occupied cubes per sub-job, everything next to the
origin (DESIGN.md "What the mesh tests cover").  Here the same arrays go into the GPU map (Chisel.AddChunk) and into the oracle
(OracleMap.put_chunk), the listed chunks are meshed on both sides (UpdateMeshesOf / recompute_meshes) and the meshes are held to the
mesher's existing contract: identical id sets, vertices, normals, colours and grid entries equal as uint32, element for element
(tests.common.compare_meshes).  Every condition on a field is asserted on the very field that is meshed, from the field and
the oracle's output alone; the GPU is never asked what a test covers.
"""
import time

import numpy as np
import pytest

from cvids_amd import synth
from tests import query_restated as qr
from tests import render_restated as rr
from tests import voxel_fields as vf
from tests.common import compare_fields, compare_meshes, same_bits, small_camera, upload

pytestmark = pytest.mark.gpu

BLOCKS = {8: 4, 16: 3, 32: 2}      # chunk edge -> block edge: 64 chunks of 8^3, 27 of 16^3, 8 of 32^3
RES = {8: 0.03, 16: 0.07, 32: 0.05}  # one non-dyadic resolution per chunk size
SEED = 1
MAX_CHUNKS = 1024


def absent_ids(B, base):
    """ids that are not resident: next to the block, and far away"""
    b = np.asarray(base)
    return [tuple(int(v) for v in b + (B, 0, 0)), tuple(int(v) for v in b - (1, 1, 1)), tuple(int(v) for v in b + (500, -500, 500))]


def new_gpu_map(N, res):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), res, True, max_chunks=MAX_CHUNKS)


class Sides:
    """the fields of this module with their two maps, each built once, only read afterwards and released when the module is done"""

    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        self.oracle, self.gpu = {}, {}

    def oracle_side(self, family, N, res, base=(0, 0, 0)):
        """-> (field, ids meshed -- the block's and three absent ones --, the oracle's map with these meshes, the field's Cubes, seconds
        the oracle's recompute took); the field's conditions are asserted before anything is meshed"""
        key = (family, N, float(res), tuple(base))
        if key not in self.oracle:
            B = BLOCKS[N]
            field = getattr(vf, family)(N, B, SEED, res=res, base=base)
            cubes = (vf.check_dense if family == "dense" else vf.check_thresholds)(field, N)
            om = self.oracle_mod.OracleMap(N, res, True)
            for cid, (s, w, c) in field.items():
                om.put_chunk(cid, s, w, c)
            ids = vf.block_ids(B, base) + absent_ids(B, base)
            t0 = time.perf_counter()
            om.recompute_meshes(ids)
            seconds = time.perf_counter() - t0
            assert len(om.meshes_to_update()) == 0
            self.oracle[key] = (field, ids, om, cubes, seconds)
        return self.oracle[key]

    def gpu_side(self, family, N, res, base=(0, 0, 0)):
        """the GPU map of the same field with the same ids meshed"""
        key = (family, N, float(res), tuple(base))
        if key not in self.gpu:
            field, ids = self.oracle_side(family, N, res, base)[:2]
            gm = new_gpu_map(N, res)
            upload(gm, field)
            gm.UpdateMeshesOf(ids)
            self.gpu[key] = gm
        return self.gpu[key]

    def release(self):
        for gm in self.gpu.values():
            gm.close()
        self.gpu.clear()
        self.oracle.clear()


@pytest.fixture(scope="module")
def sides(oracle_mod):
    s = Sides(oracle_mod)
    yield s
    s.release()


def triangle_totals(om, cubes, counts):
    """the oracle's triangles over all meshes, checked against the field's own count"""
    total = sum(len(om.get_mesh(cid)["vertices"]) for cid in map(tuple, om.mesh_ids().tolist())) // 3
    assert total == cubes.triangles(counts), (total, cubes.triangles(counts))
    return total


@pytest.fixture(scope="module")
def vertex_counts(oracle_mod):
    return [int((row >= 0).sum()) for row in oracle_mod.triangle_table()]


# ---- a. every configuration through both kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", sorted(BLOCKS))
def test_every_configuration_through_both_kernels(sides, oracle_mod, vertex_counts, N):
    """dense field: all 256 configurations in the interior and on each of the three planes, every cube fully observed, more than two
    triangles per cube of the block -- the load at which the packed budgets of a sub-job (s_list, TriRec::code / rel, cnt, job_acc) and
    the partition cursors are nearest their limits"""
    field, ids, om, cubes, seconds = sides.oracle_side("dense", N, RES[N])
    gm = sides.gpu_side("dense", N, RES[N])
    n, nv = compare_meshes(om, gm, True)
    assert n == BLOCKS[N] ** 3
    total = triangle_totals(om, cubes, vertex_counts)
    assert 3 * total == nv and total > 2 * (BLOCKS[N] * N) ** 3, total
    print("dense N = %d: %d triangles, %.2f per cube of the block, oracle recompute %.2f s" % (N, total, total / (BLOCKS[N] * N) ** 3, seconds))


# ---- b. thresholds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", sorted(BLOCKS))
def test_thresholds(sides, oracle_mod, vertex_counts, N):
    """weights on both sides of 0.5 and of 1e-12, crossing edges below InterpolateVertex's 1e-6 (vertices 1.5 times as far from the
    origin as their cube: normals and colours from chunks far outside the job's neighbourhood), -0.0 and denormal corners"""
    field, ids, om, cubes, seconds = sides.oracle_side("thresholds", N, RES[N])
    gm = sides.gpu_side("thresholds", N, RES[N])
    n, nv = compare_meshes(om, gm, True)
    assert n == BLOCKS[N] ** 3
    total = triangle_totals(om, cubes, vertex_counts)
    assert 3 * total == nv and total > 0
    print("thresholds N = %d: %d triangles, oracle recompute %.2f s" % (N, total, seconds))


# ---- c. placement -----------------------------------------------------------------------------------------------------------------------
def test_placement(sides, oracle_mod):
    """the 16^3 thresholds field across the origin, far out at large and negative chunk ids, and at res = 1 -- the one resolution at
    which InterpolateColor's voxel indices taken for metres (ChunkManager.cpp:506-520) land inside the block.  Its two branches are
    counted on the oracle's vertices by the eight residency look-ups alone."""
    N = 16
    trilinear = fallback = 0
    for res, base in ((RES[N], (-2, -2, -2)), (RES[N], (1000, -1000, 37)), (1.0, (-1, -1, -1))):
        field, ids, om, _, _ = sides.oracle_side("thresholds", N, res, base)
        gm = sides.gpu_side("thresholds", N, res, base)
        n, nv = compare_meshes(om, gm, True)
        assert n == BLOCKS[N] ** 3 and nv > 0
        index = rr.VoxelIndex(field, N, res)
        verts = np.concatenate([om.get_mesh(cid)["vertices"] for cid in sorted(field)])
        branch = vf.color_branch(index, verts)
        print("res %g base %s: %d vertices, %d trilinear" % (res, base, len(verts), int(branch.sum())))
        trilinear += int(branch.sum())
        fallback += int((~branch).sum())
    assert trilinear >= 0.1 * (trilinear + fallback) and fallback >= 0.1 * (trilinear + fallback), (trilinear, fallback)


# ---- d. in place, twice -----------------------------------------------------------------------------------------------------------------
def test_in_place_twice(sides, oracle_mod):
    """one map through three recomputes of all its chunks: the dense field, the thresholds field uploaded over it, then three chunks
    uploaded again -- one with another seed, one with all weights 0, one unchanged.  The chunk that lost its surface keeps an empty
    mesh on both sides; job_acc, the cursors and cnt come back clean from the dense recompute."""
    N, res, B = 16, RES[16], BLOCKS[16]
    dense, ids = sides.oracle_side("dense", N, res)[:2]
    field = sides.oracle_side("thresholds", N, res)[0]
    other = vf.thresholds(N, B, SEED + 1, res=res)
    om = oracle_mod.OracleMap(N, res, True)
    gm = new_gpu_map(N, res)
    for stage in (dense, field):
        upload(gm, stage)
        for cid, (s, w, c) in stage.items():
            om.put_chunk(cid, s, w, c)
        gm.UpdateMeshesOf(ids)
        om.recompute_meshes(ids)
        assert compare_meshes(om, gm, True)[0] == B ** 3
    reseeded, emptied, same = (1, 1, 1), (0, 0, 0), (2, 2, 2)
    changes = {reseeded: other[reseeded], emptied: (field[emptied][0], np.zeros(N ** 3, np.float32), field[emptied][2]), same: field[same]}
    upload(gm, changes)
    for cid, (s, w, c) in changes.items():
        om.put_chunk(cid, s, w, c)
    before = om.get_mesh(reseeded)["vertices"].copy()
    gm.UpdateMeshesOf(ids)
    om.recompute_meshes(ids)
    assert compare_meshes(om, gm, True)[0] == B ** 3
    assert before.tobytes() != om.get_mesh(reseeded)["vertices"].tobytes()
    for side in (om.get_mesh(emptied), gm.GetMesh(emptied)):
        assert len(side["vertices"]) == 0 and len(side["grids"]) == 0
    compare_fields(om.fields(), gm.fields(), om.V, True)


# ---- e. buffers that do not fit ---------------------------------------------------------------------------------------------------------
def test_dense_recompute_that_outgrows_its_buffers(sides, oracle_mod, monkeypatch):
    """the dense 16^3 field with a triangle list of 256 entries and an arena of 4096 floats (CHISEL_HIP_MESH_TINY): the recompute runs
    into the overflow flag, grows its lists, counts again and emits again.  That it did is read off the profile, which counts the
    steps of a recompute: count kernel and triangle kernel, the triangle kernel once more when the arena was too small (9.1 M floats
    here against a first arena of 4 M: so also without the switch), and the count kernel once more only when the triangle list
    overflowed -- at least four steps with the switch, at most three for the same field on a map created without it."""
    N = 16
    field, ids, om, _, _ = sides.oracle_side("dense", N, RES[N])
    steps = {}
    for tiny in (True, False):
        if tiny:
            monkeypatch.setenv("CHISEL_HIP_MESH_TINY", "1")
        else:
            monkeypatch.delenv("CHISEL_HIP_MESH_TINY")
        gm = new_gpu_map(N, RES[N])
        upload(gm, field)
        gm.set_profiling(True)
        gm.UpdateMeshesOf(ids)
        assert compare_meshes(om, gm, True)[0] == BLOCKS[N] ** 3
        steps[tiny] = gm.profile()["mesh"]["launches"]
        gm.close()
    print("profiled mesh steps: %d with buffers too small, %d without the switch" % (steps[True], steps[False]))
    assert steps[True] >= 4 and 2 <= steps[False] <= 3 and steps[False] < steps[True], steps


# ---- f. points --------------------------------------------------------------------------------------------------------------------------
def block_points(N, B, res, base=(0, 0, 0)):
    """every voxel centre of the block and of a margin of one voxel around it, x fastest"""
    r = np.float32(res)
    axes = [(np.arange(base[a] * N - 1, (base[a] + B) * N + 1).astype(np.float32) + np.float32(0.5)) * r for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float32)


@pytest.mark.parametrize("N", [8, 16])
def test_points(sides, oracle_mod, N):
    """QueryPoints against get_sdf / get_sdf_and_gradient at every voxel centre of the block and its margin, at the same set shifted
    off the centres, and at mesh vertices: found bits equal, sdf and gradient equal as bits where found, weight that of the uploaded
    voxel.  Weights on both sides of 1e-12 decide what is found."""
    res, B = RES[N], BLOCKS[N]
    field, _, om, _, _ = sides.oracle_side("thresholds", N, res)
    gm = sides.gpu_side("thresholds", N, res)
    centres = block_points(N, B, res)
    shifted = (centres + np.array([0.37, -0.41, 0.23], np.float32) * np.float32(res)).astype(np.float32)
    verts = np.concatenate([om.get_mesh(cid)["vertices"] for cid in sorted(field)])[:5000]
    assert len(verts) == 5000
    pts = np.concatenate([centres, shifted, verts])
    found, sdf, grad = om.query_points(pts)
    for outcome in (0, 1, 3):
        share = float((found == outcome).mean())
        print("N = %d: outcome %d at %.3f of %d points" % (N, outcome, share, len(pts)))
        assert share >= 0.01, (outcome, share)
    assert not (found == 2).any()
    got = gm.QueryPoints(pts, sdf=True, weight=True, gradient=True)
    assert np.array_equal(got["found"], found), "found differs at %d places" % int((got["found"] != found).sum())
    has, has_g = (found & 1).astype(bool), (found & 2).astype(bool)
    assert np.array_equal(got["sdf"][has].view(np.uint32), sdf[has].astype(np.float32).view(np.uint32))
    assert (sdf[has].astype(np.float32).astype(np.float64) == sdf[has]).all()  # (the oracle's doubles are widened floats)
    assert np.isnan(got["sdf"][~has]).all()
    assert np.array_equal(got["gradient"][has_g].view(np.uint32), grad[has_g].view(np.uint32))
    assert np.isnan(got["gradient"][~has_g]).all()
    # the voxel GetSDF reads, by the restatement's index arithmetic over the uploaded arrays -- which the oracle's answers confirm
    index = rr.VoxelIndex(field, N, res)
    r_found, r_sdf, r_weight = qr.query_points(index, pts)
    assert np.array_equal(r_found, has)
    assert np.array_equal(r_sdf[has].view(np.uint32), sdf[has].astype(np.float32).view(np.uint32))
    assert np.array_equal(got["weight"][has].view(np.uint32), r_weight[has].view(np.uint32))
    same_bits(got["weight"], r_weight, "weight")
    # the single-point entries at 200 of them
    pick = np.random.default_rng(SEED).choice(len(pts), 200, replace=False)
    kinds = set()
    for i in pick:
        ok_o, d_o = om.get_sdf(pts[i])
        ok_g, d_g = gm.GetSDF(pts[i])
        assert ok_o == ok_g and (not ok_o or np.float64(d_o).tobytes() == np.float64(d_g).tobytes()), (i, pts[i])
        ok_o, d_o, g_o = om.get_sdf_and_gradient(pts[i])
        ok_g, d_g, g_g = gm.GetSDFAndGradient(pts[i])
        assert ok_o == ok_g and (not ok_o or (np.float64(d_o).tobytes() == np.float64(d_g).tobytes() and g_o.tobytes() == g_g.tobytes())), (i, pts[i])
        kinds.add(int(found[i]))
    assert kinds == {0, 1, 3}


# ---- g. rays ----------------------------------------------------------------------------------------------------------------------------
def test_rays(sides, oracle_mod):
    """RenderView from outside at the block's centre and CastRays of 2 000 rays through the block, on the 16^3 thresholds field across
    the origin, bit for bit against the restatements: a ray ends at the first observed sample (weight above 1e-12) that is <= 0 --
    -0.0 and negative denormals included"""
    N, res, base, B = 16, RES[16], (-2, -2, -2), BLOCKS[16]
    field = sides.oracle_side("thresholds", N, res, base)[0]
    gm = sides.gpu_side("thresholds", N, res, base)
    index = rr.VoxelIndex(field, N, res)
    edge = N * res
    lo, hi = np.array(base) * edge, (np.array(base) + B) * edge
    centre = (lo + hi) / 2
    cam = small_camera(64, 48)
    pose = synth.pose_yaw(0.0, (centre[0], centre[1], lo[2] - 1.5))
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    want = rr.render_depth(index, pose, intr, 64, 48, cam.near_plane, cam.far_plane)
    hits = float(np.isfinite(want).mean())
    print("view: %.3f of the rays hit" % hits)
    assert hits >= 0.2
    same_bits(gm.RenderView(pose, cam)["depth"], want, "depth")
    rng = np.random.default_rng(SEED)
    d = rng.normal(size=(2000, 3))
    origins = centre + 4.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    aim = rng.uniform(lo, hi, (2000, 3)) - origins
    rays = qr.pack(origins, aim / np.linalg.norm(aim, axis=1, keepdims=True), 0.0, 8.0)
    t_hit, status = qr.cast_rays(index, rays)
    print("rays: %d hit, %d end behind a surface, %d never end" % tuple(int((status == k).sum()) for k in (1, 2, 0)))
    assert (status == 1).mean() >= 0.2 and (status == 2).sum() >= 100
    got = gm.CastRays(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    same_bits(got["t_hit"], t_hit, "t_hit")
    assert np.array_equal(got["status"], status), "status differs at %d places" % int((got["status"] != status).sum())


# ---- h. dump and restore ----------------------------------------------------------------------------------------------------------------
def test_dump_and_restore(sides, oracle_mod, tmp_path):
    """SaveMap -> LoadMap into a fresh map: the voxels come back byte for byte (-0.0, denormals and the weights around 1e-12 included)
    and mesh to the same arrays"""
    N = 8
    field, ids, om, _, _ = sides.oracle_side("thresholds", N, RES[N])
    gm = sides.gpu_side("thresholds", N, RES[N])
    path = str(tmp_path / "fields.chsl")
    gm.SaveMap(path)
    g2 = new_gpu_map(N, RES[N])
    g2.LoadMap(path)
    a, b = gm.fields(), g2.fields()
    assert sorted(a) == sorted(b) == sorted(field)
    for cid in field:
        for x, y, z in zip(a[cid], b[cid], field[cid]):
            assert x.tobytes() == y.tobytes() == z.tobytes(), cid
    g2.UpdateMeshesOf(ids)
    assert compare_meshes(om, g2, True)[0] == BLOCKS[N] ** 3


# ---- i. surface on a chunk face, by integration -----------------------------------------------------------------------------------------
def test_surface_on_a_chunk_face(sides, oracle_mod):
    """a wall at z = 1.2 = the face between the chunks with z-id 2 and 3 (8^3, 5 cm): every observed voxel on the near side is positive,
    every one on the far side negative, so a z-id-2 chunk's own summary holds one sign only and its triangles all come from its max-z
    plane, whose corners lie in the chunk behind -- what slot_summary must not cut short (uploads bypass it with SUM_ANY)"""
    from tests.test_gpu_parity import _mk
    N, res = 8, 0.05
    om, gm, integ = _mk(oracle_mod, N, res, False, trunc=("constant", 0.12))
    cam = small_camera(64, 48)
    depth, pose = np.full((48, 64), 1.2, np.float32), synth.pose_yaw(0.0)
    om.integrate_depth(depth, pose, (cam.fx, cam.fy, cam.cx, cam.cy), cam.near_plane, cam.far_plane)
    gm.IntegrateDepthScan(integ, depth, pose, cam)
    fields = om.fields()
    compare_fields(fields, gm.fields(), om.V, False)
    seen = {2: 0, 3: 0}
    for cid, (s, w, _) in fields.items():
        obs = w > 0
        if cid[2] == 2:
            assert (s[obs] > 0).all(), cid
        elif cid[2] == 3:
            assert (s[obs] < 0).all(), cid
        if cid[2] in seen:
            seen[cid[2]] += int(obs.sum())
    assert seen[2] > 1000 and seen[3] > 1000, seen
    om.update_meshes(force=True)
    gm.UpdateMeshes(force=True)
    n, nv = compare_meshes(om, gm, False)
    r = np.float32(res)
    top = (np.float32(N - 1) * r + r * np.float32(0.5)) + np.float32(N * 2) * r  # centroid of the chunk's last z-layer (ChunkManager.cpp:50-66)
    # the z-id-2 chunks in view, from the voxels alone: a cube of the max-z plane away from the chunk's x and y faces has its eight
    # corners in the chunk's last layer and the first layer of the chunk behind; all eight observed -> it crosses the wall
    in_view = set()
    for cid, (s, w, _) in fields.items():
        behind = fields.get((cid[0], cid[1], 3))
        if cid[2] != 2 or behind is None:
            continue
        near, far = w.reshape(N, N, N)[N - 1] > 0.5, behind[1].reshape(N, N, N)[0] > 0.5
        both = near & far
        if (both[:-1, :-1] & both[1:, :-1] & both[:-1, 1:] & both[1:, 1:]).any():
            in_view.add(cid)
    assert len(in_view) >= 4, in_view
    meshed = set()
    for cid in map(tuple, om.mesh_ids().tolist()):
        grids = om.get_mesh(cid)["grids"]
        assert cid[2] == 2 or len(grids) == 0, cid
        if len(grids):
            meshed.add(cid)
            assert (grids[:, 2] == top).all(), cid
    assert in_view <= meshed, sorted(in_view - meshed)
    for cid in in_view:
        assert len(gm.GetMesh(cid)["grids"]) > 0 and len(gm.GetMesh(cid)["vertices"]) > 0, cid
    assert nv > 500, nv
