"""The mesh components and the filter of DESIGN.md 3.16 restated (TEST INFRASTRUCTURE, plain Python and numpy: a dictionary of
parents, the numbering by sorted roots, the filter as boolean masks), and the cases the tests of both sides share.

A triangle is VALID when its three ids lie in [0, V).  The components are those of the graph on the V vertices whose edges are the sides
of the valid triangles; a component's root is its smallest vertex; components are numbered by ascending root.  Component c is KEPT when
it has at least min_triangles valid triangles and, with largest_only, is the one with the most (the lowest number of equals).
"""
import numpy as np

from tests import indexed_mesh_restated as ir
from tests import voxel_fields as vf

F = np.float32
TILE = 256  # elements one workgroup of the device's scans takes (components_checks.h: COMPONENTS_TILE)
TOTALS = ("vertices", "triangles", "invalid_triangles", "components", "largest_triangles", "kept_components", "kept_vertices", "kept_triangles")


def as_triangles(indices):
    return np.asarray(indices, np.int64).reshape(-1, 3)


def valid_rows(V, indices):
    idx = as_triangles(indices)
    return ((idx >= 0) & (idx < V)).all(1)


def components(V, indices):
    """-> {"vertex_component": (V,) int32, "triangle_component": (T,) int32, "table": (C, 3) int64 (root, vertices, valid triangles),
    "totals"}"""
    idx = as_triangles(indices)
    valid = valid_rows(V, idx)
    parent = {v: v for v in range(V)}

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:  # (everything on the way points at the root afterwards: the walks stay short, the sets are the same)
            parent[x], x = r, parent[x]
        return r

    for a, b, c in idx[valid].tolist():
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    root_of = np.array([find(v) for v in range(V)], np.int64)
    least = np.full(V, V, np.int64)
    np.minimum.at(least, root_of, np.arange(V))
    assert V == 0 or (least[root_of] == root_of).all()  # a root is the smallest vertex of its set
    roots = np.array(sorted(set(root_of.tolist())), np.int64)
    number = {int(r): k for k, r in enumerate(roots)}
    vertex_component = np.array([number[int(r)] for r in root_of], np.int32)
    triangle_component = np.full(len(idx), -1, np.int32)
    if valid.any():
        triangle_component[valid] = vertex_component[idx[valid, 0]]
    table = np.zeros((len(roots), 3), np.int64)
    table[:, 0] = roots
    table[:, 1] = np.bincount(vertex_component, minlength=len(roots))
    table[:, 2] = np.bincount(triangle_component[valid], minlength=len(roots))
    totals = dict.fromkeys(TOTALS, 0)
    totals.update(vertices=V, triangles=len(idx), invalid_triangles=int((~valid).sum()), components=len(roots),
                  largest_triangles=int(table[:, 2].max()) if len(roots) else 0)
    return {"vertex_component": vertex_component, "triangle_component": triangle_component, "table": table, "totals": totals}


def filter_mesh(V, indices, min_triangles=1, largest_only=False, rows=None):
    """rows: {"vertices" | "normals" | "colors": (V, 3) float32 or None} -> {"indices", "vertex_map", "triangle_map", "totals", and every
    array of `rows`}: boolean masks over what components() says"""
    assert min_triangles >= 1
    idx = as_triangles(indices)
    comp = components(V, idx)
    counts = comp["table"][:, 2]
    kept = counts >= min_triangles
    if largest_only and len(counts):
        kept &= np.arange(len(counts)) == int(np.argmax(counts))  # (argmax: the first of equals, the lowest number)
    keep_v = kept[comp["vertex_component"]] if V else np.zeros(0, bool)
    keep_t = np.zeros(len(idx), bool)
    valid = comp["triangle_component"] >= 0
    keep_t[valid] = kept[comp["triangle_component"][valid]]
    vertex_map = np.where(keep_v, np.cumsum(keep_v) - 1, -1).astype(np.int32)
    triangle_map = np.where(keep_t, np.cumsum(keep_t) - 1, -1).astype(np.int32)
    out = {"indices": vertex_map[idx[keep_t]].astype(np.int32).reshape(-1, 3), "vertex_map": vertex_map, "triangle_map": triangle_map}
    for name, a in (rows or {}).items():
        out[name] = None if a is None else np.ascontiguousarray(np.asarray(a)[:V][keep_v])
    totals = dict(comp["totals"])
    totals.update(kept_components=int(kept.sum()), kept_vertices=int(keep_v.sum()), kept_triangles=int(keep_t.sum()))
    out["totals"] = totals
    return out


def hook_walks(V, indices):
    """The device's hook rule run sequentially in array order, without any shortening of paths: a valid triangle unites (a, b) and
    (a, c); a union links the larger root under the smaller.  -> (the longest find walk of a union, the longest walk from a vertex to its
    root afterwards, the parents)"""
    idx = as_triangles(indices)
    parent = list(range(V))
    longest = 0

    def find(x):
        steps = 0
        while parent[x] != x:
            x, steps = parent[x], steps + 1
        return x, steps

    for a, b, c in idx[valid_rows(V, idx)].tolist():
        for u, w in ((a, b), (a, c)):
            (ru, su), (rw, sw) = find(u), find(w)
            longest = max(longest, su, sw)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    depth = [0] * V
    for v in range(V):  # (a parent is smaller than its child: it has its depth already)
        depth[v] = 0 if parent[v] == v else depth[parent[v]] + 1
    return longest, max(depth) if V else 0, parent


# ---- index arrays made by hand ------------------------------------------------------------------------------------------------------------
def strip(first, n):
    """n triangles over the n + 2 vertices from `first` on"""
    return [(first + i, first + i + 1, first + i + 2) for i in range(n)]


def clusters(V, T, seed):
    """T triangles (x, x + 1, x + 2), x a multiple of 4 drawn at random: groups of three vertices, every fourth vertex alone, some groups
    without a triangle, many with several"""
    rng = np.random.default_rng(seed)
    x = 4 * rng.integers(0, max((V - 3) // 4, 1), T)
    return np.stack([x, x + 1, x + 2], 1).astype(np.int32)


PATH = 4097
I32_MAX = 2 ** 31 - 1


def hand_cases():
    """-> [(name, V, (T, 3) int32)]"""
    cases = [("no triangle", 5, []),
             ("one triangle", 3, [(0, 1, 2)]),
             ("a strip", 10, strip(0, 8)),
             ("a fan", 9, [(0, i, i + 1) for i in range(1, 8)]),
             ("a path, descending", PATH + 2, strip(0, PATH)[::-1]),
             ("a path, descending, then its first triangle again", PATH + 2, strip(0, PATH)[::-1] + [strip(0, PATH)[-1]]),
             ("a path, shuffled", PATH + 2, [strip(0, PATH)[i] for i in np.random.default_rng(7).permutation(PATH)]),
             ("two strips joined by the last triangle", 40, strip(0, 10) + strip(20, 12) + [(5, 25, 39)]),
             ("repeated triangles", 12, strip(0, 3) * 3 + strip(6, 2) * 2 + [(8, 7, 6), (7, 6, 8)]),
             ("equal ids", 12, [(4, 4, 5), (7, 7, 7), (1, 2, 2), (9, 8, 9), (5, 4, 4), (2, 3, 3)]),
             ("vertices no triangle names", 30, strip(3, 4) + strip(20, 2)),
             ("ids out of range", 20, strip(0, 3) + [(-1, 1, 2), (6, 20, 7), (8, 9, I32_MAX), (-1, -1, -1), (I32_MAX, 20, -5)] + strip(10, 4) + [(12, 13, 20), (-(2 ** 31), 0, 1)]),
             ("equal largest components", 40, strip(20, 5) + strip(0, 5) + strip(10, 3) + strip(30, 5)),
             ("many tiles", 66000, clusters(66000, 66100, 5))]  # (more tile sums than one batch of the scan over them)
    for V in (TILE - 1, TILE, TILE + 1):
        for T in (TILE - 1, TILE, TILE + 1):
            cases.append(("V %d T %d" % (V, T), V, clusters(V, T, V + 7 * T)))
    return [(name, V, np.array(idx, np.int64).astype(np.int32).reshape(-1, 3)) for name, V, idx in cases]


def float_rows(V, seed):
    """three (V, 3) float32 arrays of arbitrary bit patterns, NaNs with payloads, infinities and subnormals among them"""
    rng = np.random.default_rng(seed)
    return {name: rng.integers(0, 2 ** 32, (V, 3), dtype=np.uint64).astype(np.uint32).view(np.float32) for name in ("vertices", "normals", "colors")}


# ---- a field of several closed surfaces -------------------------------------------------------------------------------------------------
# five spheres in a block of 32^3 voxels (N = 8: 4^3 chunks, N = 16: 2^3), radii 1.3 ... 6 voxels, their surfaces more than two voxels
# apart and below 30 on every axis (the last lattice point of stride 2: the cubes beyond it lack their + neighbour), every centre off the
# lattice: the largest across the chunk corner (16, 16, 16) -- its vertices have
# eight owners --, the third across the chunk face x = 16
SPHERES = (((16.3, 16.4, 15.6), 6.0), ((7.3, 6.4, 6.6), 4.7), ((16.4, 5.3, 25.4), 3.5), ((26.6, 25.7, 6.3), 2.4), ((5.4, 26.3, 25.6), 1.3))
BLOCK = {8: 4, 16: 2}


def blobs(N, B, spheres, res, base=(0, 0, 0)):
    """a fully observed block of B^3 chunks whose distance is the minimum over `spheres` ((centre, radius), voxel units) of
    indexed_mesh_restated.sphere's |voxel - centre| - radius"""
    n = N * B
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    d = None
    for centre, radius in spheres:
        one = np.sqrt((x - F(centre[0])) ** 2 + (y - F(centre[1])) ** 2 + (z - F(centre[2])) ** 2).astype(np.float32) - F(radius)
        d = one if d is None else np.minimum(d, one)
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


def closed(indices):
    """every undirected edge of the triangles is used exactly twice"""
    return set(ir.edge_uses(indices).values()) == {2}
