"""What one rank of a sharded map sees while it meshes its jobs, from the definitions alone (TEST INFRASTRUCTURE, numpy only).

A sharded recompute moves SHELLS: of a neighbour G = J + d of a job J that another rank owns, the meshing rank receives the box of
voxels with coordinates {0, 1} along an axis with d = +1, {N - 1} along an axis with d = -1 and all of them along an axis with
d = 0, and installs it as a ghost chunk that holds default voxels (99999, 0, 0) everywhere else.  The rank then meshes its jobs on
that VIEW -- its own chunks, whole, plus the ghosts.  Nothing here restates how the product plans the exchange (no covering rule, no
merging of boxes, nothing of cvids_amd/sharded.py): a view is the union of the boxes over every (job, direction), written down once.

The view is not the whole map, and two reads of the reference leave the 27-neighbourhood the shells serve: the `v1 + 0.5 v2` vertex
of InterpolateVertex's degenerate branch (MarchingCubes.h:135-146) lies 1.5 times as far from the origin as its cube, so its normal
and colour are read chunks away; and InterpolateColor (ChunkManager.cpp:506-520) takes voxel indices for metres, so near the origin
its eight look-ups land in chunks that are resident in the whole map but belong to another rank.  `far_reading` names the vertices at
which a view can answer differently from the whole map, from the voxel addresses alone.

A field is what tests/voxel_fields.py builds: dict chunk id -> (sdf[N^3], weight[N^3], rgbw[N^3, 4] or None), voxel id = (z N + y) N + x.
"""
import numpy as np

from tests import align_restated as ar
from tests import query_restated as qr
from tests import render_restated as rr

F = np.float32
DEFAULT_SDF = F(99999.0)
DIRECTIONS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy or dz]
DIRTY_SETS = ("one_inside", "corner", "line", "diagonal", "all")
B = 4  # the block the dirty sets are written for


# ---- who owns what, and what is meshed ---------------------------------------------------------------------------------------------
def owner(cid, world, block):
    """(bx + 3 by + 5 bz) mod world on the floor-divided blocks of the id (python's // and % are floor division and its remainder)"""
    if world <= 1:
        return 0
    return (cid[0] // block + 3 * (cid[1] // block) + 5 * (cid[2] // block)) % world


def job_ids(dirty, flags=None):
    """the ids a recompute meshes: the 27-neighbourhood of every flag-0 id, a flag-1 id as it is -- resident or not"""
    dirty = [tuple(int(v) for v in i) for i in dirty]
    flags = [0] * len(dirty) if flags is None else [int(f) for f in flags]
    jobs = set()
    for (x, y, z), flag in zip(dirty, flags):
        if flag:
            jobs.add((x, y, z))
        else:
            jobs.update((x + dx, y + dy, z + dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
    return jobs


def jobs_of(jobs, rank, world, block):
    return sorted(j for j in jobs if owner(j, world, block) == rank)


def dirty_set(name, base=(0, 0, 0)):
    """the dirty sets of the sharded tests, in the coordinates of a 4 x 4 x 4 block based at `base`"""
    ids = {"one_inside": [(1, 1, 1)], "corner": [(0, 0, 0)], "line": [(x, 1, 2) for x in range(B)], "diagonal": [(0, 0, 0), (3, 3, 3)],
           "all": [(x, y, z) for z in range(B) for y in range(B) for x in range(B)]}[name]
    return [(int(base[0]) + x, int(base[1]) + y, int(base[2]) + z) for x, y, z in ids]


# ---- the box of a direction ----------------------------------------------------------------------------------------------------------
def _axis(d, N):
    return [0, 1] if d > 0 else ([N - 1] if d < 0 else list(range(N)))


def box_mask(d, N):
    """what a job reads of its neighbour in direction d: (N, N, N) bool indexed [z, y, x]"""
    m = np.zeros((N, N, N), bool)
    m[np.ix_(_axis(d[2], N), _axis(d[1], N), _axis(d[0], N))] = True
    return m


def box_code(d):
    """the 6-bit name the product gives box(d): per axis 2 bits, 0 = all, 1 = {0, 1}, 2 = {N - 1} (x lowest)"""
    return sum((1 if v > 0 else (2 if v < 0 else 0)) << (2 * a) for a, v in enumerate(d))


def shell_requests(jobs, rank, world, block):
    """every (J, d, G) of the definition: J a job of `rank`, d != 0, G = J + d owned by another rank (resident or not)"""
    out = []
    for j in jobs_of(jobs, rank, world, block):
        for d in DIRECTIONS:
            g = (j[0] + d[0], j[1] + d[1], j[2] + d[2])
            if owner(g, world, block) != rank:
                out.append((j, d, g))
    return out


def ghost_masks(jobs, rank, world, block, N):
    """{ghost id: (N, N, N) bool}: per neighbour another rank owns, the union of box(d) over every (J, d) that names it"""
    out = {}
    for _, d, g in shell_requests(jobs, rank, world, block):
        if g not in out:
            out[g] = np.zeros((N, N, N), bool)
        out[g] |= box_mask(d, N)
    return out


# ---- the view ------------------------------------------------------------------------------------------------------------------------
def rank_view(field, N, rank, world, block, jobs):
    """dict id -> (sdf, weight, rgbw): the rank's own chunks, whole; and for every job J of the rank (resident or not), every d != 0 and
    G = J + d that is resident in `field` and owned by another rank, box(d) of G in a chunk of default voxels -- the union over all (J, d)"""
    view = {cid: v for cid, v in field.items() if owner(cid, world, block) == rank}
    for g, mask in ghost_masks(jobs, rank, world, block, N).items():
        if g not in field:
            continue
        s, w, c = field[g]
        m = mask.reshape(-1)
        gs, gw = np.full(N ** 3, DEFAULT_SDF, np.float32), np.zeros(N ** 3, np.float32)
        gs[m], gw[m] = np.asarray(s, np.float32)[m], np.asarray(w, np.float32)[m]
        gc = None
        if c is not None:
            gc = np.zeros((N ** 3, 4), np.uint8)
            gc[m] = np.asarray(c, np.uint8).reshape(-1, 4)[m]
        view[g] = (gs, gw, gc)
    return view


def oracle_of(oracle_mod, field, N, res, color, ids):
    """an OracleMap that holds `field` with `ids` meshed (RecomputeMeshes skips the ids that are not resident)"""
    om = oracle_mod.OracleMap(N, res, color)
    for cid, (s, w, c) in field.items():
        om.put_chunk(cid, s, w, c if color else None)
    om.recompute_meshes(np.asarray(sorted(ids), np.int32).reshape(-1, 3))
    return om


# ---- where a view can answer differently ---------------------------------------------------------------------------------------------
def _differing(view, whole, N, res):
    """a VoxelIndex over the chunks of `whole` whose "weight" is 1 at every voxel that the view does not hold with the same bits -- a
    chunk the view lacks differs everywhere -- and 0 elsewhere: sample_weight then answers "does this address differ" with the
    address arithmetic of the restated GetSDF / GetColorVoxel"""
    diff = {}
    for cid, (s, w, c) in whole.items():
        if cid not in view:
            d = np.ones(N ** 3, bool)
        else:
            vs, vw, vc = view[cid]
            d = (np.asarray(s, np.float32).view(np.uint32) != np.asarray(vs, np.float32).view(np.uint32)) | \
                (np.asarray(w, np.float32).view(np.uint32) != np.asarray(vw, np.float32).view(np.uint32))
            if c is not None and vc is not None:
                d |= (np.asarray(c, np.uint8).reshape(-1, 4) != np.asarray(vc, np.uint8).reshape(-1, 4)).any(1)
        diff[cid] = (np.zeros(N ** 3, np.float32), d.astype(np.float32), None)
    return rr.VoxelIndex(diff, N, res)


def far_reading(view, whole, N, res, vertices):
    """(n,) bool: True where one of the voxel addresses that GetSDFAndGradient(p) (the voxel centre and its six neighbours,
    ChunkManager.cpp:449-474) or InterpolateColor(p) (the eight look-ups at voxel indices taken for metres, and the nearest voxel of
    the fallback, :501-573) forms lies in a chunk that is resident in `whole` and holds other values there than in the view.  A
    superset of the vertices whose normal or colour differs; only the positions enter."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    index = _differing(view, whole, N, res)
    far = np.zeros(len(v), bool)
    if not len(v):
        return far

    def look(pos):
        ok, w = qr.sample_weight(index, pos)
        return ok & (np.where(ok, w, F(0)) > 0)

    # Fifteen of the sixteen positions depend on floorf(p / r) alone -- the voxel centre is floorf(p / r) r + r / 2, the look-ups start
    # at (int)floorf(p / r) --, and the vertices of a chunk share a few thousand values of it: they are formed once per value, from the
    # first vertex that has it, by the same restated functions.
    r = index.res
    i0 = np.floor(v / r).astype(np.int32)  # (as voxel_fields.color_branch forms them)
    if (np.abs(i0.astype(np.int64)) < (1 << 20)).all():  # (one sortable key per row: much faster than a row-wise unique)
        k = i0.astype(np.int64) + (1 << 20)
        _, first, inverse = np.unique((k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2], return_index=True, return_inverse=True)
    else:
        _, first, inverse = np.unique(i0, axis=0, return_index=True, return_inverse=True)
    rep, j0 = v[first], i0[first]
    some = np.zeros(len(rep), bool)
    c = ar.voxel_centre(index, rep)
    some |= look(c)
    for axis in range(3):
        for sign in (1, -1):
            q = c.copy()
            q[:, axis] = c[:, axis] + r if sign > 0 else c[:, axis] - r
            some |= look(q)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                some |= look((j0 + np.array([dx, dy, dz], np.int32)).astype(np.float32))
    far |= some[np.asarray(inverse).reshape(-1)]
    far |= look(v)
    return far


def differing_rows(a, b):
    """(n,) bool: rows of two (n, 3) float32 arrays that differ in their bits"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint32) != b.view(np.uint32)).any(1) if len(a) else np.zeros(0, bool)


def view_against_whole(oracle_mod, field, N, res, world, block, dirty, whole_om=None, color=True):
    """mesh every job of every rank on its view and on the whole map, on the oracle alone: positions and grid entries must be equal
    everywhere, every normal / colour row that differs must be far-reading.
    -> {"vertices", "far", "normals", "colors"}: counts over all ranks"""
    jobs = job_ids(dirty)
    if whole_om is None:
        whole_om = oracle_of(oracle_mod, field, N, res, color, jobs)
    counts = {"vertices": 0, "far": 0, "normals": 0, "colors": 0}
    meshed = set()
    for rank in range(world):
        mine = jobs_of(jobs, rank, world, block)
        view = rank_view(field, N, rank, world, block, jobs)
        om = oracle_of(oracle_mod, view, N, res, color, mine)
        ids = sorted(map(tuple, om.mesh_ids().tolist()))
        assert ids == [j for j in mine if whole_om.get_mesh(j) is not None], (rank, len(ids))
        meshed.update(ids)
        got, want = [om.get_mesh(cid) for cid in ids], [whole_om.get_mesh(cid) for cid in ids]
        for cid, a, b in zip(ids, got, want):
            for key in ("vertices", "grids"):
                assert a[key].shape == b[key].shape and np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (rank, cid, key)
        if not ids:
            continue
        rows = lambda meshes, key: np.concatenate([m[key] for m in meshes])
        far = far_reading(view, field, N, res, rows(got, "vertices"))
        dn = differing_rows(rows(got, "normals"), rows(want, "normals"))
        dc = differing_rows(rows(got, "colors"), rows(want, "colors")) if color else np.zeros(len(dn), bool)
        assert not (dn & ~far).any(), "rank %d: %d normals differ at vertices that are not far-reading" % (rank, int((dn & ~far).sum()))
        assert not (dc & ~far).any(), "rank %d: %d colours differ at vertices that are not far-reading" % (rank, int((dc & ~far).sum()))
        counts["vertices"] += len(far)
        counts["far"] += int(far.sum())
        counts["normals"] += int(dn.sum())
        counts["colors"] += int(dc.sum())
    assert meshed == {j for j in jobs if whole_om.get_mesh(j) is not None}
    return counts
