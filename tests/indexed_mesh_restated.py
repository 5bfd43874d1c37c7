"""The indexed mesh of DESIGN.md 3.15 restated (TEST INFRASTRUCTURE, numpy only: every cube, dictionaries keyed by (owner, lattice
point, axis), no masks and no prefixes).  The cube walk is the coarse restatement's (tests/coarse_mesh_restated.py: cubes_of,
cube_coords), the triangle table the oracle's (oracle.triangle_table).

A lattice point l in [0, M)^3 of chunk o owns the three edges l -> l + e_a.  An edge is USED when its two distances differ in
(sdf < 0) and a MESHED cube of a selected chunk has it among its twelve.  Its vertex is InterpolateVertex(P, Q, sdf_lo, sdf_hi) with P
the centre of voxel s l of o and Q = P + step e_a.  Owners: the selection in its order, then the + neighbours in the field that are not
selected, ascending.  Vertex ids: owners in that order, inside an owner ascending (a, lk, lj, li).  Triangles: the coarse mesh's rows.
"""
import numpy as np

from tests import coarse_mesh_restated as cr
from tests import voxel_fields as vf

F = np.float32


def edge_key(N, s, cid, ijk, e):
    """edge e of cube ijk of chunk cid -> (owner id, (li, lj, lk), axis), lower corner, upper corner"""
    M = N // s
    c0, c1 = vf.EDGES[e]
    o0, o1 = vf.CORNERS[c0], vf.CORNERS[c1]
    axis = [a for a in range(3) if o0[a] != o1[a]]
    assert len(axis) == 1
    a = axis[0]
    lo, hi = (c0, c1) if o0[a] < o1[a] else (c1, c0)
    l = [ijk[b] + vf.CORNERS[lo][b] for b in range(3)]
    owner = list(cid)
    for b in range(3):
        if l[b] == M:
            l[b] = 0
            owner[b] += 1
    return (tuple(owner), tuple(l), a), lo, hi


def interpolate_vertex(p, q, s1, s2):
    """MarchingCubes::InterpolateVertex, one float32 operation at a time ("vertex1 + 0.5 * vertex2" included)"""
    with np.errstate(all="ignore"):
        diff = F(F(s1) - F(s2))
        if np.abs(diff) < vf.MIN_DIFF:
            return (p + q * F(0.5)).astype(np.float32)
        t = F(F(s1) / diff)
        return (p + (q - p) * t).astype(np.float32)


def extras_of(field, ids):
    """the + neighbours of the selected chunks that are in the field and not selected, each once, ascending"""
    chosen = set(ids)
    found = set()
    for x, y, z in ids:
        for d in range(1, 8):
            nb = (x + (d & 1), y + ((d >> 1) & 1), z + (d >> 2))
            if nb in field and nb not in chosen:
                found.add(nb)
    return sorted(found)


def indexed_mesh(oracle_mod, field, N, res, s, selection=None, box=None):
    """-> {"vertices": (V, 3) float32, "indices": (T, 3) int32, "table": (n, 2) int64 (first triangle, triangles), "owner_table": (owners, 2)
    int64 (first vertex, vertices), "owner_ids": (owners, 3) int32, "totals": {...}, "degenerate": (V,) bool -- vertices of edges under
    InterpolateVertex's 1e-6}; KeyError for a selected id that is not in the field"""
    assert 1 <= s <= N and N % s == 0
    table = oracle_mod.triangle_table()
    ids = cr.selection_all(field, box) if selection is None else [tuple(int(v) for v in c) for c in selection]
    assert len(set(ids)) == len(ids)
    for cid in ids:
        if cid not in field:
            raise KeyError(cid)
    G = cr.grids(field, N)
    used, triangles, rows = {}, [], []
    cubes_meshed = 0
    for cid in ids:
        first = len(triangles)
        for ijk, state, sdf8, _ in cr.cubes_of(G, N, s, cid):
            if state != cr.MESHED:
                continue
            cubes_meshed += 1
            index = sum((1 << d) for d in range(8) if sdf8[d] < 0)
            row = table[index]
            keys = {}
            for e in range(12):
                key, lo, hi = edge_key(N, s, cid, ijk, e)
                if (sdf8[lo] < 0) != (sdf8[hi] < 0):
                    used[key] = (sdf8[lo], sdf8[hi])
                    keys[e] = key
            t = 0
            while t < 16 and row[t] != -1:
                triangles.append((keys[int(row[t + 2])], keys[int(row[t + 1])], keys[int(row[t])]))
                t += 3
        rows.append((first, len(triangles) - first))
    owners = list(ids) + (extras_of(field, ids) if (selection is not None or box is not None) else [])
    step = F(s) * F(res)
    by_owner = {o: [] for o in owners}
    for key in used:
        by_owner[key[0]].append(key)
    number, verts, degenerate, owner_rows = {}, [], [], []
    for o in owners:
        mine = sorted(by_owner[o], key=lambda k: (k[2], k[1][2], k[1][1], k[1][0]))
        owner_rows.append((len(verts), len(mine)))
        for key in mine:
            _, l, a = key
            p = cr.cube_coords(N, res, s, o, l)
            q = p.copy()
            q[a] = q[a] + step
            lo, hi = used[key]
            number[key] = len(verts)
            verts.append(interpolate_vertex(p, q, lo, hi))
            with np.errstate(all="ignore"):
                degenerate.append(bool(np.abs(F(F(lo) - F(hi))) < vf.MIN_DIFF))
    indices = np.array([[number[k] for k in tri] for tri in triangles], np.int32).reshape(-1, 3)
    vertices = np.array(verts, np.float32).reshape(-1, 3)
    return {"vertices": vertices, "indices": indices, "table": np.array(rows, np.int64).reshape(-1, 2),
            "owner_table": np.array(owner_rows, np.int64).reshape(-1, 2), "owner_ids": np.array(owners, np.int32).reshape(-1, 3),
            "degenerate": np.array(degenerate, bool),
            "totals": {"chunks": len(ids), "owners": len(owners), "cubes_meshed": cubes_meshed, "vertices": len(vertices), "triangles": len(indices)}}


def deindexed(mesh):
    """(3 T, 3): the soup the indexed mesh stands for, in the coarse mesh's row order"""
    return mesh["vertices"][mesh["indices"].reshape(-1)].reshape(-1, 3)


def edge_uses(indices):
    """undirected edge (low id, high id) -> number of triangles that have it"""
    uses = {}
    for a, b, c in np.asarray(indices).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            k = (min(u, v), max(u, v))
            uses[k] = uses.get(k, 0) + 1
    return uses


def sphere(N, B, radius, centre, res, base=(0, 0, 0)):
    """a fully observed block of B^3 chunks whose distance is |voxel - centre| - radius in voxel units (centre off the lattice)"""
    n = N * B
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    d = np.sqrt((x - F(centre[0])) ** 2 + (y - F(centre[1])) ** 2 + (z - F(centre[2])) ** 2).astype(np.float32) - F(radius)
    sdf = (d * F(res)).astype(np.float32)
    field = {}
    for cx, cy, cz in vf.block_ids(B):
        part = sdf[cz * N:(cz + 1) * N, cy * N:(cy + 1) * N, cx * N:(cx + 1) * N]
        rgbw = np.zeros((N ** 3, 4), np.uint8)
        rgbw[:, 0] = 40 + 20 * cx
        rgbw[:, 1] = 40 + 20 * cy
        rgbw[:, 2] = 40 + 20 * cz
        rgbw[:, 3] = 255
        field[(cx + base[0], cy + base[1], cz + base[2])] = (np.ascontiguousarray(part).reshape(-1), np.ones(N ** 3, np.float32), rgbw)
    return field
