"""The hand-built voxel fields meet their conditions, and the oracle's entries for caller-filled chunks work (CPU only).

The conditions are conditions on the input: tests/test_gpu_mesh_fields.py asserts them again on the very fields it meshes."""
import numpy as np
import pytest

from tests import voxel_fields as vf

# chunk edge, block edge: the smallest blocks at which a dense field reaches all 256 configurations in all four sections
BLOCKS = {8: 4, 16: 3, 32: 2}
SEED = 1


@pytest.mark.parametrize("N", sorted(BLOCKS))
def test_dense_fields_hold_every_configuration_in_every_section(N):
    seeds = (1, 2) if N == 8 else (1, 2, 3)
    for seed in seeds:
        field = vf.dense(N, BLOCKS[N], seed)
        assert len(field) == BLOCKS[N] ** 3
        cubes = vf.check_dense(field, N)
        assert len(cubes.config) == (BLOCKS[N] * N - 1) ** 3
        for s, w, c in field.values():
            assert s.dtype == np.float32 and w.dtype == np.float32 and c.dtype == np.uint8 and c.shape == (N ** 3, 4)
            assert (w == 1).all() and (np.abs(s) >= np.float32(0.05 * 0.05) * (1 - 1e-6)).all() and (np.abs(s) <= np.float32(0.05)).all()


@pytest.mark.parametrize("N", sorted(BLOCKS))
def test_thresholds_fields_hold_their_classes(N):
    field = vf.thresholds(N, BLOCKS[N], SEED)
    cubes = vf.check_thresholds(field, N)
    classes = vf.weight_classes(field)
    assert set(classes) == set(float(v) for v in np.concatenate([vf.HIGH_WEIGHTS, vf.LOW_WEIGHTS]))
    values, n = vf.value_classes(field), (BLOCKS[N] * N) ** 3
    print("N = %d: value classes %s" % (N, values))
    # the shares the field is drawn with: 50 % band, 20 % tiny, 10 % zero (half of them -0.0), 10 % denormal, 10 % large; half negative
    # but for the zeros.  Binomial spread at n >= 32 768 is below 0.3 %; 1 % is asked.
    for name, share in (("band", 0.5), ("tiny", 0.2), ("+0.0", 0.05), ("-0.0", 0.05), ("denormal", 0.1), ("large", 0.1), ("negative", 0.45)):
        assert abs(values[name] / n - share) < 0.01, (name, values[name] / n)
    assert values["non-finite"] == 0
    print("N = %d: %d cubes, %.1f %% fully observed, %d rejected only by small weights, %d tiny crossing edges, observed denormal / -0.0 "
          "corners %s" % (N, len(cubes.config), 100 * cubes.observed.mean(), cubes.rejected_only_by_small_weights(),
                          cubes.tiny_crossing_edges(), cubes.observed_corners()))


def test_fields_do_not_depend_on_their_base():
    a, b = vf.thresholds(8, 2, 5, res=0.03), vf.thresholds(8, 2, 5, res=0.03, base=(1000, -1000, 37))
    assert set(b) == set(vf.block_ids(2, (1000, -1000, 37)))
    for (x, y, z), va in a.items():
        vb = b[(x + 1000, y - 1000, z + 37)]
        assert all(p.tobytes() == q.tobytes() for p, q in zip(va, vb))


def test_sections_and_traversal_order():
    """one chunk with all its neighbours: 7^3 interior cubes, 7 x 8 on the max-x plane, 7 x 7 on the max-y plane, 8 x 8 on the max-z
    plane (ChunkManager.cpp:381-447)"""
    N = 4
    cubes = vf.Cubes(vf.dense(N, 2, 3), N)
    rows = cubes.traversal_order((0, 0, 0))
    assert len(rows) == N ** 3
    sec = cubes.section[rows]
    assert [int((sec == k).sum()) for k in range(4)] == [(N - 1) ** 3, (N - 1) * N, (N - 1) ** 2, N * N]
    assert (np.diff(sec) >= 0).all()
    assert cubes.local[rows[0]].tolist() == [0, 0, 0] and cubes.local[rows[1]].tolist() == [1, 0, 0]
    assert cubes.local[rows[(N - 1) ** 3]].tolist() == [N - 1, 0, 0] and cubes.local[rows[(N - 1) ** 3 + 1]].tolist() == [N - 1, 1, 0]
    # the chunk at the far corner of the block has no neighbour on any of its three planes: interior cubes only
    assert len(cubes.traversal_order((1, 1, 1))) == (N - 1) ** 3


def test_put_chunk_keeps_the_bits(oracle_mod):
    N = 8
    field = vf.thresholds(N, 2, SEED, res=0.03, base=(-1, 5, -7))
    om = oracle_mod.OracleMap(N, 0.03, True)
    for cid, (s, w, c) in field.items():
        om.put_chunk(cid, s, w, c)
    assert sorted(map(tuple, om.chunk_ids().tolist())) == sorted(field)
    assert len(om.meshes_to_update()) == 0 and len(om.mesh_ids()) == 0
    for cid, (s, w, c) in field.items():
        gs, gw, gc = om.get_chunk(cid)
        assert gs.tobytes() == s.tobytes() and gw.tobytes() == w.tobytes() and gc.tobytes() == c.tobytes()
    # a second put overwrites the resident chunk in place; without colours the colour voxels are the defaults
    cid = sorted(field)[0]
    s, w, _ = field[sorted(field)[1]]
    om.put_chunk(cid, s, w)
    gs, gw, gc = om.get_chunk(cid)
    assert gs.tobytes() == s.tobytes() and gw.tobytes() == w.tobytes() and not gc.any()
    assert om.num_chunks() == len(field)


def test_recompute_meshes_is_mesh_cube_over_the_traversal(oracle_mod):
    """dense field, non-dyadic resolution, block across the origin: every chunk's vertices and grid entries equal oracle.mesh_cube
    over its cubes in GenerateMesh's order (normals and colours are replaced by the shading afterwards and are not looked at)"""
    N, B, res, base = 8, 4, 0.03, (-2, -2, -2)
    field = vf.dense(N, B, SEED, res=res, base=base)
    cubes = vf.check_dense(field, N)
    om = oracle_mod.OracleMap(N, res, True)
    for cid, (s, w, c) in field.items():
        om.put_chunk(cid, s, w, c)
    absent = [(50, 50, 50), (-3, -2, -2)]
    ids = vf.block_ids(B, base)
    om.recompute_meshes(ids + absent)
    assert sorted(map(tuple, om.mesh_ids().tolist())) == sorted(ids)
    assert len(om.meshes_to_update()) == 0 and om.num_chunks() == len(ids)
    r = np.float32(res)
    total = 0
    for cid in ids:
        mesh = om.get_mesh(cid)
        verts, grids = [], []
        origin = (np.array(cid, np.int32) * N).astype(np.float32) * r  # Chunk.cpp:43
        for row in cubes.traversal_order(cid):
            centre = (cubes.local[row].astype(np.float32) * r + r * np.float32(0.5)) + origin  # ChunkManager.cpp:50-66, :399
            v, _ = oracle_mod.mesh_cube(cubes.s[:, row], centre, res)
            if len(v):
                verts.append(v)
                grids.append(centre)
        verts, grids = np.concatenate(verts), np.stack(grids)
        assert mesh["vertices"].tobytes() == verts.tobytes(), cid
        assert mesh["grids"].tobytes() == grids.astype(np.float32).tobytes(), cid
        total += len(verts)
    assert total > 0


def test_recompute_meshes_leaves_the_dirty_set_and_absent_ids_alone(oracle_mod):
    """meshes_to_update() as an integration left it stays as it is; an absent id changes nothing; a chunk that lost its surface keeps
    its mesh object, empty (ChunkManager.cpp:91-128)"""
    N, res = 8, 0.05
    om = oracle_mod.OracleMap(N, res, True)
    om.set_integrator(oracle_mod.TRUNC_CONSTANT, 0.12, 1.0, True, 0.05)
    from cvids_amd import synth
    om.integrate_depth(np.full((48, 64), 1.2, np.float32), synth.pose_yaw(0.0), synth.intrinsics(64, 48))
    dirty = sorted(map(tuple, om.meshes_to_update().tolist()))
    assert len(dirty) > 0
    field = vf.dense(N, 2, SEED, res=res, base=(20, 20, 20))
    for cid, (s, w, c) in field.items():
        om.put_chunk(cid, s, w, c)
    assert sorted(map(tuple, om.meshes_to_update().tolist())) == dirty
    n_chunks = om.num_chunks()
    om.recompute_meshes([(77, 0, 0)])
    assert len(om.mesh_ids()) == 0 and om.num_chunks() == n_chunks
    om.recompute_meshes(sorted(field))
    assert sorted(map(tuple, om.mesh_ids().tolist())) == sorted(field)
    assert sorted(map(tuple, om.meshes_to_update().tolist())) == dirty
    before = {cid: om.get_mesh(cid) for cid in field}
    om.recompute_meshes([(77, 0, 0), (20, 20, 19)])
    for cid in field:
        assert all(before[cid][k].tobytes() == om.get_mesh(cid)[k].tobytes() for k in ("vertices", "normals", "colors", "grids"))
    cid = (20, 20, 20)
    om.put_chunk(cid, field[cid][0], np.zeros(N ** 3, np.float32), field[cid][2])
    om.recompute_meshes([cid])
    assert cid in set(map(tuple, om.mesh_ids().tolist())) and len(om.get_mesh(cid)["vertices"]) == 0 and len(om.get_mesh(cid)["grids"]) == 0
    # a chunk without a surface that never had a mesh gets none
    om.put_chunk((40, 0, 0), np.ones(N ** 3, np.float32), np.ones(N ** 3, np.float32))
    om.recompute_meshes([(40, 0, 0)])
    assert (40, 0, 0) not in set(map(tuple, om.mesh_ids().tolist()))


def test_query_points_equals_the_single_point_entries(oracle_mod):
    N, res = 8, 0.07
    field = vf.thresholds(N, 2, SEED, res=res, base=(-1, -1, -1))
    om = oracle_mod.OracleMap(N, res, True)
    for cid, (s, w, c) in field.items():
        om.put_chunk(cid, s, w, c)
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1.2 * N * res, 1.2 * N * res, (400, 3)).astype(np.float32)
    found, sdf, grad = om.query_points(pts)
    kinds = set()
    for i, p in enumerate(pts):
        ok, d = om.get_sdf(p)
        okg, _, g = om.get_sdf_and_gradient(p)
        assert (int(ok) | (int(okg) << 1)) == int(found[i])
        kinds.add(int(found[i]))
        assert (np.float64(d).tobytes() == sdf[i].tobytes()) if ok else np.isnan(sdf[i])
        assert (g.tobytes() == grad[i].tobytes()) if okg else np.isnan(grad[i]).all()
    assert kinds == {0, 1, 3}
    f2, s2, g2 = om.query_points(pts, gradient=False)
    assert g2 is None and np.array_equal(f2, found & 1) and s2.tobytes() == sdf.tobytes()


def test_color_branch_counts_residency_only():
    """res = 1: a vertex's voxel indices taken for metres are its own voxel, so inside the block all eight exist; at 0.05 they are
    20 times as far out and none exists"""
    from tests import render_restated as rr
    N = 8
    v = np.array([[3.5, 3.5, 3.5], [15.6, 3.5, 3.5], [-0.5, 2.0, 2.0], [14.5, 14.5, 14.5]], np.float32)
    index = rr.VoxelIndex(vf.dense(N, 2, 1, res=1.0), N, 1.0)
    assert vf.color_branch(index, v).tolist() == [True, False, False, True]
    index = rr.VoxelIndex(vf.dense(N, 2, 1, res=0.05), N, 0.05)
    assert not vf.color_branch(index, v * np.float32(0.05)).any()
