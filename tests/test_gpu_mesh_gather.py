"""chisel_hip_gather_meshes (Chisel.GatherMeshes) on hand-built maps: every comparison is same_bits against GetMesh over the same ids,
i.e. against the unchanged per-chunk entry (tests/mesh_gather_restated.py concatenates what GetMesh returns and restates the marker
colours); the gather is never checked against itself.  What a case reaches is asserted from the totals, the table and GetMesh
before anything is compared.  The maps are blocks of vf.dense chunks (thousands of triangles per chunk at N = 16) and chunks with
one negative voxel (8, 4, 2 or 1 triangles, by how many of the voxel's cubes lie inside the chunk)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mesh_gather_restated as R
from tests import voxel_fields as vf
from tests.common import compare_fields, fields_of, free_bytes, same_bits, small_camera, upload

pytestmark = pytest.mark.gpu

RES = {8: 0.03, 16: 0.07}
DENSE_BASE = (-1, 0, 2)
ARRAYS = ("vertices", "normals", "colors", "rgba", "grids")
WIDTH = {"vertices": 3, "normals": 3, "colors": 3, "rgba": 4, "grids": 3}
# where the one negative voxel sits -> triangles of an isolated chunk's mesh: the voxel's cubes that lie inside the chunk, one each
ONE_VOXEL = {"interior": ((3, 3, 3), 8), "face": ((0, 3, 3), 4), "edge": ((0, 0, 3), 2), "corner": ((0, 0, 0), 1)}
SMALL_IDS = {"interior": (40, 0, 0), "face": (44, 0, 0), "edge": (48, 0, 0), "corner": (52, 0, 0)}
OTHER_LIGHTS = {"light0": (0.3, -1.7, 0.4), "light1": (2.5, 0.25, -0.125), "diffuse": 0.375, "ambient": 0.0625}


def new_map(N, color=False, max_chunks=256):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), RES[N], color, max_chunks=max_chunks)


def one_voxel_chunk(N, voxels, seed=0):
    """every voxel +0.8 res with weight 1 but `voxels` {(x, y, z): sdf}; random colours"""
    s = np.full((N, N, N), 0.8 * RES[N], np.float32)
    for (x, y, z), v in voxels.items():
        s[z, y, x] = v
    rgbw = np.random.default_rng(seed).integers(0, 256, (N ** 3, 4), dtype=np.uint8)
    return s.reshape(-1), np.ones(N ** 3, np.float32), rgbw


def small_field(N):
    return {SMALL_IDS[k]: one_voxel_chunk(N, {pos: -0.2 * RES[N]}, seed=i) for i, (k, (pos, _)) in enumerate(ONE_VOXEL.items())}


@functools.lru_cache(maxsize=None)
def whole_map(N, color):
    """a 2 x 2 x 2 block of dense chunks and the four one-voxel chunks, meshed in one recompute (only ever read)"""
    gm = new_map(N, color)
    field = dict(vf.dense(N, 2, 3, res=RES[N], base=DENSE_BASE))
    field.update(small_field(N))
    upload(gm, field)
    gm.UpdateMeshesOf(sorted(field))
    return gm


def reference(gm, ids, lights=None):
    """what the gather must return for `ids`, from GetMesh alone"""
    return R.gather([gm.GetMesh(tuple(int(v) for v in cid)) for cid in ids], lights)


def check_against(got, want, names, what):
    for name in names:
        same_bits(np.ascontiguousarray(got[name]), want[name], "%s: %s" % (what, name))


def device_tensors(names, V, G, fill=None):
    """tensors for `out`; a fill is torch's work on torch's stream, which the map's stream knows nothing of: it is over on return"""
    import torch
    out = {}
    for name in names:
        rows = G if name == "grids" else V
        out[name] = torch.empty((rows, WIDTH[name]), dtype=torch.float32, device="cuda") if fill is None else \
            torch.full((rows, WIDTH[name]), fill, dtype=torch.float32, device="cuda")
    if fill is not None:
        torch.cuda.synchronize()
    return out


# ---- 1. the whole map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,color", [(8, False), (8, True), (16, False), (16, True)])
def test_whole_map_host_and_device_and_every_subset(N, color):
    import torch
    gm = whole_map(N, color)
    ids = gm.GetMeshIDs()
    lights = gm.MARKER_LIGHTS
    want = reference(gm, ids, lights)
    names = [n for n in ARRAYS if color or n != "colors"]
    V, G = len(want["vertices"]), len(want["grids"])
    # reach: twelve meshes, thousands of vertices, more tiles than one, one arena
    size = gm.GatherMeshesSize()
    assert size["meshes"] == len(ids) == 12 and size["meshes_nonempty"] == 12 and size["vertices"] == V and size["grids"] == G and size["arenas_read"] == 1
    assert V > 2000 and G > 500 and want["table"][:, 1].min() == 3  # (the corner chunk's one triangle)
    host = gm.GatherMeshes(rgba=True)
    assert host["totals"]["vertices"] == V and host["totals"]["tiles"] == -(-(V * (10 + 3 * color) + G * 3) // 4096) > 5
    assert np.array_equal(host["table"], want["table"]) and np.array_equal(host["ids"], ids)
    check_against(host, want, names, "host")
    assert (host["colors"] is None) == (not color)
    dev = gm.GatherMeshes(out=device_tensors(names, V, G, fill=-7.0))
    gm.synchronize()
    check_against({k: dev[k].cpu().numpy() for k in names}, want, names, "device")
    assert np.array_equal(dev["table"], want["table"])
    for left_out in names:  # every subset that leaves one out; rows to spare are left alone
        some = [n for n in names if n != left_out]
        out = gm.GatherMeshes(out=device_tensors(some, V + 3, G + 2, fill=-7.0))
        gm.synchronize()
        got = {k: out[k].cpu().numpy() for k in some}
        check_against({k: got[k][:(G if k == "grids" else V)] for k in some}, want, some, "without %s" % left_out)
        assert all((got[k][(G if k == "grids" else V):] == -7.0).all() for k in some)
    torch.cuda.synchronize()


# ---- 2. three arenas with dead space ------------------------------------------------------------------------------------------------
def test_three_arenas_with_dead_space():
    N = 8
    gm = new_map(N)
    field = vf.dense(N, 2, 11, res=RES[N], base=DENSE_BASE)
    upload(gm, field)
    ids = sorted(field)
    A, B = ids[:4], ids[4:]
    gm.UpdateMeshesOf(A)
    gm.UpdateMeshesOf(B)
    old = {cid: gm.GetMesh(cid) for cid in A[:2]}
    other = vf.dense(N, 2, 12, res=RES[N], base=DENSE_BASE)
    for cid in A[:2]:  # other voxels: another draw of the same family
        s, w, c = other[cid]
        gm.AddChunk(cid, s, w, None)
    gm.UpdateMeshesOf(A[:2])  # the first arena keeps A[2:] alive and holds the dead meshes of A[:2]
    want = reference(gm, gm.GetMeshIDs())
    got = gm.GatherMeshes()
    assert got["totals"]["arenas_read"] == 3 and got["totals"]["meshes"] == 8
    for cid in A[:2]:  # the re-meshed chunks' new meshes are the ones returned
        new = gm.GetMesh(cid)
        assert len(new["vertices"]) > 100 and not (new["vertices"].shape == old[cid]["vertices"].shape and np.array_equal(new["vertices"], old[cid]["vertices"]))
        row = got["table"][[tuple(r) for r in got["ids"].tolist()].index(cid)]
        same_bits(np.ascontiguousarray(got["vertices"][row[0]:row[0] + row[1]]), new["vertices"], "re-meshed %s" % (cid,))
    assert np.array_equal(got["table"], want["table"])
    check_against(got, want, ("vertices", "normals", "grids"), "three arenas")
    picked = [B[3], A[0], A[3], B[0], A[1]]  # a selection across the three arenas, in the caller's order
    got = gm.GatherMeshes(ids=picked)
    assert got["totals"]["arenas_read"] == 3
    check_against(got, reference(gm, picked), ("vertices", "normals", "grids"), "picked")
    gm.close()


# ---- 3. tile edges -------------------------------------------------------------------------------------------------------------------
def test_tile_edges():
    """One dense chunk of N = 16 (its mesh spans many tiles), then one-voxel meshes by the hundred: as many of 8 triangles and then of
    1 triangle as bring the vertex array's end EXACTLY onto a tile edge (9 floats per triangle: the triangles before the edge are a
    multiple of the tile), then three more."""
    from cvids_amd import capi
    T = capi.GATHER_TILE_FLOATS
    N = 16
    gm = new_map(N)
    dense_id = (7, -3, 1)
    field = dict(vf.dense(N, 1, 5, res=RES[N], base=dense_id))
    field.update(small_field(N))
    upload(gm, field)
    gm.UpdateMeshesOf(sorted(field))
    tris = {k: len(gm.GetMesh(SMALL_IDS[k])["vertices"]) // 3 for k in ONE_VOXEL}
    assert tris == {k: t for k, (_, t) in ONE_VOXEL.items()}, tris
    D = len(gm.GetMesh(dense_id)["vertices"]) // 3
    assert D > 3000
    lack = -D % T  # triangles up to the next multiple of the tile: 9 (D + lack) floats end on an edge
    picked = [dense_id] + [SMALL_IDS["interior"]] * (lack // 8) + [SMALL_IDS["corner"]] * (lack % 8) + [SMALL_IDS["face"], SMALL_IDS["edge"], SMALL_IDS["interior"]]
    want = reference(gm, picked)
    table = want["table"]
    end = 3 * (table[:, 0] + table[:, 1])  # every mesh's last float + 1 in the vertex array, which is first in the tile space
    start = 3 * table[:, 0]
    assert (end[0] - 1) // T - start[0] // T >= 2, "the dense mesh spans at least three tiles"
    whole = np.bincount((start // T)[(start // T) == ((end - 1) // T)])
    assert whole.max() >= 4, "some tile holds at least four whole meshes"
    assert (end % T == 0).any() and end[-4] % T == 0, "a mesh ends exactly on a tile edge"
    assert end[-1] % T != 0 and (2 * end[-1] + 3 * (table[-1, 2] + table[-1, 3])) % T != 0, "the total is no multiple of the tile"
    got = gm.GatherMeshes(ids=picked)
    assert np.array_equal(got["table"], table) and got["totals"]["arenas_read"] == 1
    check_against(got, want, ("vertices", "normals", "grids"), "tile edges")
    got = gm.GatherMeshes(ids=picked, normals=False, grids=False, rgba=True, lights=OTHER_LIGHTS)  # rgba tiles cut vertices: 4 per vertex behind 9 D + ...
    check_against(got, reference(gm, picked, OTHER_LIGHTS), ("vertices", "rgba"), "tile edges, rgba")
    gm.close()


# ---- 4. empty and absent -------------------------------------------------------------------------------------------------------------
def raw_gather(gm, ids, cap_v, cap_g, arrays, marker=False, n_ids=None):
    """the C entry as it is -> (code, message, totals); arrays: five numpy arrays or None"""
    from cvids_amd import capi
    req = capi.MeshRequest()
    keep = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1, 3)) if ids is not None else None
    if keep is not None:
        req.ids_xyz = keep.ctypes.data_as(C.POINTER(C.c_int))
        req.n_ids = len(keep) if n_ids is None else n_ids
    if marker:
        req.marker_colors = 1
        req.light0[:], req.light1[:], req.diffuse, req.ambient = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), 0.5, 0.2
    t = capi.MeshTotals()
    rc = gm.L.chisel_hip_gather_meshes(gm.h, C.byref(req), cap_v, cap_g, *[a.ctypes.data if a is not None else None for a in arrays], 0, None, None, C.byref(t))
    return rc, gm.L.chisel_hip_last_error().decode(), t


def test_empty_and_absent():
    N = 8
    gm = new_map(N)
    empty = gm.GatherMeshes(rgba=True)  # an empty map: zero totals, nothing launched
    assert empty["totals"] == {k: 0 for k in empty["totals"]} and empty["vertices"].shape == (0, 3) and empty["table"].shape == (0, 4)
    assert gm.GatherMeshesSize() == empty["totals"]
    field = small_field(N)
    upload(gm, field)
    ids = sorted(field)
    gm.UpdateMeshesOf(ids)
    gone = SMALL_IDS["face"]
    s, w, c = field[gone]
    gm.AddChunk(gone, np.abs(s), w, None)  # all positive: the mesh is regenerated to empty
    gm.UpdateMeshesOf([gone])
    assert tuple(gone) in [tuple(r) for r in gm.GetMeshIDs().tolist()] and len(gm.GetMesh(gone)["vertices"]) == 0 and len(gm.GetMesh(gone)["grids"]) == 0
    got = gm.GatherMeshes()
    want = reference(gm, gm.GetMeshIDs())
    k = [tuple(r) for r in got["ids"].tolist()].index(gone)
    assert tuple(got["table"][k]) == (0, 0, 0, 0) and got["totals"]["meshes"] == 4 and got["totals"]["meshes_nonempty"] == 3
    assert np.array_equal(got["table"], want["table"])
    check_against(got, want, ("vertices", "normals", "grids"), "with an empty mesh")
    dup = [ids[0], gone, ids[0], ids[3], ids[0], gone]  # duplicated ids
    got = gm.GatherMeshes(ids=dup)
    check_against(got, reference(gm, dup), ("vertices", "normals", "grids"), "duplicates")
    assert np.array_equal(got["table"], reference(gm, dup)["table"]) and np.array_equal(got["ids"], np.asarray(dup, np.int32))
    # an id without a mesh is refused with its index, and the outputs are untouched
    arrays = [np.full((64, 3), 77.0, np.float32), np.full((64, 3), 77.0, np.float32), None, None, np.full((64, 3), 77.0, np.float32)]
    rc, msg, _ = raw_gather(gm, [ids[0], ids[1], (9, 9, 9), ids[2]], 64, 64, arrays)
    assert rc == 4 and "id 2 " in msg, (rc, msg)
    rc, msg, _ = raw_gather(gm, [ids[0]], 64, 64, arrays, n_ids=0)  # n_ids = 0 with a non-null list
    assert rc == 1 and "without a count" in msg, (rc, msg)
    assert all((a == 77.0).all() for a in arrays if a is not None)
    with pytest.raises(KeyError):
        gm.GatherMeshes(ids=[(9, 9, 9)])
    gm.close()


# ---- 5. rgba -------------------------------------------------------------------------------------------------------------------------
def test_rgba_of_a_colour_map_is_the_mesh_colour():
    gm = whole_map(8, True)
    ids = gm.GetMeshIDs()
    want = reference(gm, ids, gm.MARKER_LIGHTS)
    got = gm.GatherMeshes(rgba=True, normals=False, grids=False)
    assert len(np.unique(want["colors"])) > 100
    same_bits(got["rgba"], want["rgba"], "rgba of a colour map")
    same_bits(np.ascontiguousarray(got["rgba"][:, :3]), np.concatenate([gm.GetMesh(tuple(c))["colors"] for c in ids.tolist()]), "rgb = GetMesh's colours")
    assert (got["rgba"][:, 3] == 1.0).all()


def test_rgba_without_colour_is_the_restated_rule_with_nan_normals():
    """a +inf voxel beside the negative one gives vertices at NaN and with them NaN normals (asserted from GetMesh): s_k = 0 there"""
    N = 8
    gm = new_map(N)
    field = dict(vf.dense(N, 2, 13, res=RES[N], base=DENSE_BASE))
    field.update(small_field(N))
    nan_id = (60, 1, -2)
    field[nan_id] = one_voxel_chunk(N, {(3, 3, 3): -0.2 * RES[N], (4, 3, 3): np.inf})
    upload(gm, field)
    gm.UpdateMeshesOf(sorted(field))
    nan_rows = int(np.isnan(gm.GetMesh(nan_id)["normals"]).any(axis=1).sum())
    assert nan_rows >= 1, "the field yields no NaN normal"
    ids = gm.GetMeshIDs()
    for lights in (gm.MARKER_LIGHTS, OTHER_LIGHTS):
        want = reference(gm, ids, lights)
        assert int(np.isnan(want["normals"]).any(axis=1).sum()) == nan_rows and not np.isnan(want["rgba"]).any()
        assert len(np.unique(want["rgba"][:, 0])) > 100 and (want["rgba"][:, 0] == np.float32(1.0)).any() == (lights is OTHER_LIGHTS)
        got = gm.GatherMeshes(rgba=True, lights=lights)
        same_bits(got["rgba"], want["rgba"], "rgba by the restated rule")
        same_bits(got["normals"], want["normals"], "normals")
        same_bits(got["rgba"], R.marker_rgba(got["normals"], **lights), "rgba of the gathered normals")
        dev = gm.GatherMeshes(out=device_tensors(("rgba",), len(want["vertices"]), 0), lights=lights)  # rgba alone: the normals are not gathered
        gm.synchronize()
        same_bits(dev["rgba"].cpu().numpy(), want["rgba"], "rgba alone, device")
    gm.close()


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------------
def test_a_gather_nobody_waited_for_survives_the_arena_being_rewritten():
    import torch
    N = 16
    gm = new_map(N)
    field = vf.dense(N, 2, 17, res=RES[N], base=DENSE_BASE)
    upload(gm, field)
    ids = sorted(field)
    gm.UpdateMeshesOf(ids)
    want = reference(gm, gm.GetMeshIDs())  # the meshes as downloaded before the recomputes
    V, G = len(want["vertices"]), len(want["grids"])
    gm.synchronize()
    out = gm.GatherMeshes(out=device_tensors(("vertices", "normals", "grids"), V, G))  # no wait
    for round_ in range(3):  # every chunk altered, full recomputes: the first arena loses its meshes, is pooled and written again
        other = vf.dense(N, 2, 18 + round_, res=RES[N], base=DENSE_BASE)
        for cid in ids:
            s, w, c = other[cid]
            gm.AddChunk(cid, s, w, None)
        gm.UpdateMeshesOf(ids)
    assert gm.GatherMeshesSize()["arenas_read"] == 1  # (resolves the last recompute: the earlier arenas are released)
    gm.synchronize()
    torch.cuda.synchronize()
    check_against({k: out[k].cpu().numpy() for k in ("vertices", "normals", "grids")}, want, ("vertices", "normals", "grids"), "before the recomputes")
    after = reference(gm, gm.GetMeshIDs())
    assert after["vertices"].shape != want["vertices"].shape or not np.array_equal(after["vertices"], want["vertices"])
    gm.close()


# ---- 7. capacity and read-only -------------------------------------------------------------------------------------------------------
def test_capacity_one_short_and_the_map_is_only_read():
    from cvids_amd import synth
    from cvids_amd.chisel import ConstantWeighter, InverseTruncator, ProjectionIntegrator
    N = 8
    gm = new_map(N, max_chunks=4096)
    field = dict(vf.dense(N, 2, 19, res=RES[N], base=(30, 30, 30)))
    upload(gm, field)
    ids = sorted(field)
    gm.UpdateMeshesOf(ids[:6])
    depth, pose = next(iter(synth.stream("wall", 1, 64, 48)))  # something in the dirty set: one integrated frame
    gm.IntegrateDepthScan(ProjectionIntegrator(InverseTruncator(2.0), ConstantWeighter(1.0), 0.05, True), depth, pose, small_camera(64, 48))
    before = (fields_of(gm, N), gm.counters(), sorted(map(tuple, gm.GetMeshesToUpdate().tolist())))
    size = gm.GatherMeshesSize()
    V, G = size["vertices"], size["grids"]
    assert V > 1000 and G > 100
    arrays = [np.full((V, 3), 77.0, np.float32), np.full((V, 3), 77.0, np.float32), None, np.full((V, 4), 77.0, np.float32), np.full((G, 3), 77.0, np.float32)]
    for cap_v, cap_g in ((V - 1, G), (V, G - 1)):
        rc, msg, t = raw_gather(gm, None, cap_v, cap_g, arrays, marker=True)
        assert rc == 1 and "capacity" in msg and t.vertices == V and t.grids == G and t.meshes == 6, (rc, msg)
        assert all((a == 77.0).all() for a in arrays if a is not None)
    rc, msg, t = raw_gather(gm, None, V, G, arrays, marker=True)
    assert rc == 0 and t.vertices == V and t.tiles == -(-(V * 10 + G * 3) // 4096)
    want = reference(gm, gm.GetMeshIDs(), {"light0": (0.0, 0.0, 1.0), "light1": (1.0, 0.0, 0.0), "diffuse": 0.5, "ambient": 0.2})
    for a, name in zip(arrays, ARRAYS):
        if a is not None:
            same_bits(a, want[name], "exact capacity: %s" % name)
    gm.GatherMeshes(rgba=True)
    gm.GatherMeshes(out=device_tensors(("vertices", "grids"), V, G))
    gm.synchronize()
    after = (fields_of(gm, N), gm.counters(), sorted(map(tuple, gm.GetMeshesToUpdate().tolist())))
    compare_fields(before[0], after[0], N ** 3, False, what="read-only")
    assert before[1] == after[1] and before[2] == after[2] and len(before[2]) >= 1
    gm.close()


def test_refusals_that_need_the_map():
    from cvids_amd import capi
    gm = whole_map(8, False)
    v = np.full((8, 3), 77.0, np.float32)
    rc, msg, _ = raw_gather(gm, None, 1 << 20, 1 << 20, [v, None, v, None, None])
    assert rc == 1 and "colour" in msg, (rc, msg)
    rc, msg, _ = raw_gather(gm, None, 1 << 20, 1 << 20, [None, None, None, np.full((8, 4), 77.0, np.float32), None])
    assert rc == 1 and "marker_colors" in msg, (rc, msg)
    rc, msg, _ = raw_gather(gm, None, 1 << 20, 1 << 20, [None] * 5)
    assert rc == 1 and "no output" in msg, (rc, msg)
    rc, msg, _ = raw_gather(gm, [(0, 0, 0), (1 << 20, 0, 0)], 1 << 20, 1 << 20, [v, None, None, None, None])
    assert rc == 1 and "id 1" in msg and "range" in msg, (rc, msg)
    assert gm.L.chisel_hip_gather_meshes(gm.h, None, 0, 0, v.ctypes.data, None, None, None, None, 0, None, None, None) == 1
    assert gm.L.chisel_hip_gather_meshes(None, C.byref(capi.MeshRequest()), 0, 0, v.ctypes.data, None, None, None, None, 0, None, None, None) == 1
    assert (v == 77.0).all()


# ---- 8. scratch lifetime -------------------------------------------------------------------------------------------------------------
def test_gather_cycles_return_their_memory():
    N = 8
    field = small_field(N)
    n = 60000
    picked = np.tile(np.asarray([SMALL_IDS["corner"], SMALL_IDS["edge"]], np.int32), (n // 2, 1))
    footprint = 4 * n * 32  # the device copy of the segment table: four arrays, 32 bytes a segment (7.7 MB)

    def cycle():
        gm = new_map(N)
        upload(gm, field)
        gm.UpdateMeshesOf(sorted(field))
        V = (3 + 6) * (n // 2)
        out = gm.GatherMeshes(ids=picked, out=device_tensors(("vertices", "normals", "rgba", "grids"), V, 3 * (n // 2)))
        assert out["totals"]["vertices"] == V
        got = gm.GatherMeshes(ids=picked[:100], rgba=True)  # a second, smaller call fits the scratch
        assert got["totals"]["meshes"] == 100
        gm.close()

    readings = []
    for _ in range(4):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; drift %d" % (readings, footprint, drift))
    assert abs(drift) < footprint // 2, (readings, footprint)


# ---- 9. the binary PLY ---------------------------------------------------------------------------------------------------------------
def parse_ply(path):
    """-> (format, vertices (V, 3) float32, colours (V, 3) uint8 or None, faces (F, 3) int32) of a file written by either writer"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    fmt = lines[1].split()[1]
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    color = any("uchar red" in l for l in lines)
    props = [l for l in lines if l.startswith("property") or l.startswith("element")]
    if fmt == "ascii":
        rows = body.decode().split("\n")
        vals = np.array([r.split() for r in rows[:nv]], dtype=object).reshape(nv, 6 if color else 3)
        v = np.array([float(x) for x in vals[:, :3].reshape(-1)], np.float32).reshape(nv, 3)
        c = vals[:, 3:].astype(int).astype(np.uint8) if color else None
        f = np.array([r.split()[1:4] for r in rows[nv:nv + nf]], dtype=np.int32).reshape(nf, 3)
        return fmt, props, v, c, f
    vt = np.dtype([("v", "<f4", 3)] + ([("c", "u1", 3)] if color else []))
    ft = np.dtype([("n", "u1"), ("i", "<i4", 3)])
    verts = np.frombuffer(body, vt, nv)
    faces = np.frombuffer(body, ft, nf, offset=nv * vt.itemsize)
    assert len(body) == nv * vt.itemsize + nf * ft.itemsize and (faces["n"] == 3).all()
    return fmt, props, verts["v"].copy(), verts["c"].copy() if color else None, faces["i"].copy()


@pytest.mark.parametrize("color", [False, True])
def test_binary_ply_holds_what_the_text_ply_holds(tmp_path, color):
    gm = whole_map(8, color)
    text, binary = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    assert gm.SaveAllMeshesToPLY(text) and gm.SaveAllMeshesToPLYBinary(binary)
    tf, tprops, tv, tc, tfaces = parse_ply(text)
    bf, bprops, bv, bc, bfaces = parse_ply(binary)
    assert tf == "ascii" and bf == "binary_little_endian" and tprops == bprops
    got = gm.GatherMeshes(normals=False, grids=False)
    same_bits(bv, got["vertices"], "the binary file's vertices are the gather's")
    # the text holds each float at operator<<'s six significant digits: the binary vertices after the same round trip
    rounded = np.array([float("%.6g" % x) for x in bv.reshape(-1)], np.float32).reshape(-1, 3)
    assert len(tv) == len(bv) > 2000 and np.array_equal(tv, rounded)
    assert np.array_equal(tfaces, bfaces) and np.array_equal(bfaces.reshape(-1), np.arange(len(bv), dtype=np.int32))
    assert (tc is None) == (bc is None) == (not color)
    if color:
        assert np.array_equal(tc, bc) and len(np.unique(bc)) > 50
    assert not gm.SaveAllMeshesToPLYBinary(str(tmp_path / "no_such_dir" / "c.ply"))


def test_the_facade_program_gathers_what_it_walks(tmp_path):
    """cvids_amd/open_chisel/tests/facade_gather.cpp: ChunkManager::GatherMeshes against the per-mesh walk over GetAllMeshes(), the
    marker colours with ChiselServer's lights against the same arithmetic in C++, and the file SaveAllMeshesToPLYBinary writes"""
    import os
    import subprocess
    tdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cvids_amd", "open_chisel", "tests")
    ply = str(tmp_path / "facade.ply")
    run = subprocess.run([os.path.join(tdir, "facade_gather"), ply], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "facade_gather ok" in run.stdout, run.stdout + run.stderr
    fmt, props, v, c, faces = parse_ply(ply)
    n = int(run.stdout.split(" meshes, ")[1].split(" vertices")[0])
    assert fmt == "binary_little_endian" and c is None and len(v) == n > 300 and np.isfinite(v).all() and len(faces) == n // 3


# ---- 10. a group is refused, a shard is served ----------------------------------------------------------------------------------------
def test_group_handle_is_refused_and_a_shard_is_served():
    from cvids_amd import capi
    from cvids_amd import chisel as ch
    group = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, devices=[0, 0])
    for call in (lambda: group.GatherMeshes(), lambda: group.GatherMeshesSize(), lambda: group.SaveAllMeshesToPLYBinary("/dev/null")):
        with pytest.raises(capi.ChiselHipError) as e:
            call()
        assert e.value.code == 5 and "group" in str(e.value)
    group.close()
    shard = ch.Chisel((16, 16, 16), 0.04, False, max_chunks=4096, n_shards=2, shard_rank=0)
    got = shard.GatherMeshes()  # one shard of several: its meshes are its own (none yet)
    assert got["totals"]["meshes"] == 0
    shard.close()
