"""The adjacency, the vertex normals and the smoothing of DESIGN.md 3.17 restated plainly (TEST INFRASTRUCTURE: dictionaries of sets,
sorted(), numpy float32 scalars with one operation per line; no CSR tricks), and the cases the tests of both sides share.

A triangle is VALID when its three ids lie in [0, V).  INCIDENCE: row v is the ascending list of the valid triangles that name v, each
once.  NEIGHBOURS: row v is the ascending list of the distinct ids u != v named by the triangles of row v; c(v, u) is the number of
triangles of row v that name u.  FLAGS: bit 0 BOUNDARY some c(v, u) == 1, bit 1 NONMANIFOLD some c(v, u) > 2, bit 2 ISOLATED no triangle.
"""
import numpy as np

from tests import mesh_components_restated as mc

F = np.float32
MAX_INCIDENT = 32  # adjacency_checks.h: MESH_MAX_INCIDENT
BOUNDARY, NONMANIFOLD, ISOLATED = 1, 2, 4
TOTALS = ("vertices", "triangles", "invalid_triangles", "incidences", "neighbors", "max_incident", "max_neighbors", "boundary_vertices",
          "nonmanifold_vertices", "isolated_vertices", "pinned_vertices", "reserved")


def rows_of(V, indices):
    """-> (incidence: [sorted list of triangles] per vertex, counts: [{u: c(v, u)}] per vertex, number of invalid triangles)"""
    idx = mc.as_triangles(indices)
    valid = mc.valid_rows(V, idx)
    named = {v: set() for v in range(V)}
    for t, ids in enumerate(idx.tolist()):
        if valid[t]:
            for v in ids:
                named[v].add(t)
    incidence = [sorted(named[v]) for v in range(V)]
    counts = []
    for v in range(V):
        c = {}
        for t in incidence[v]:
            for u in set(idx[t].tolist()) - {v}:
                c[u] = c.get(u, 0) + 1
        counts.append(c)
    return incidence, counts, int((~valid).sum())


def adjacency(V, indices, pin=None):
    """-> {"tri_offsets": (V + 1,), "tri_items", "nbr_offsets": (V + 1,), "nbr_items", "flags": (V,) all int32, "totals", and the rows
    themselves: "incidence", "neighbors" (lists of lists)}; pin: the mask whose pinned vertices are counted (None: 0 is reported)"""
    incidence, counts, invalid = rows_of(V, indices)
    neighbors = [sorted(c) for c in counts]
    flags = np.zeros(V, np.int32)
    for v in range(V):
        if any(n == 1 for n in counts[v].values()):
            flags[v] |= BOUNDARY
        if any(n > 2 for n in counts[v].values()):
            flags[v] |= NONMANIFOLD
        if not incidence[v]:
            flags[v] |= ISOLATED
    offsets = lambda rows: np.array([0] + np.cumsum([len(r) for r in rows]).tolist(), np.int64).astype(np.int32)
    flat = lambda rows: np.array([x for r in rows for x in r], np.int64).astype(np.int32)
    totals = dict.fromkeys(TOTALS, 0)
    totals.update(vertices=V, triangles=len(mc.as_triangles(indices)), invalid_triangles=invalid, incidences=sum(len(r) for r in incidence),
                  neighbors=sum(len(r) for r in neighbors), max_incident=max([len(r) for r in incidence] + [0]),
                  max_neighbors=max([len(r) for r in neighbors] + [0]), boundary_vertices=int((flags & BOUNDARY != 0).sum()),
                  nonmanifold_vertices=int((flags & NONMANIFOLD != 0).sum()), isolated_vertices=int((flags & ISOLATED != 0).sum()))
    if pin is not None:
        totals["pinned_vertices"] = int(pinned(flags, neighbors, pin).sum())
    return {"tri_offsets": offsets(incidence), "tri_items": flat(incidence), "nbr_offsets": offsets(neighbors), "nbr_items": flat(neighbors), "flags": flags,
            "totals": totals, "incidence": incidence, "neighbors": neighbors}


def pinned(flags, neighbors, pin):
    return np.array([bool(flags[v] & pin) or not neighbors[v] for v in range(len(flags))], bool)


def vertex_normals(adj, indices, vertices):
    """the area-weighted sum of the incident triangles' normals, in ascending triangle order, normalised; float32, an operation a line"""
    idx = mc.as_triangles(indices)
    P = np.asarray(vertices, F)
    out = np.zeros((len(adj["incidence"]), 3), F)
    with np.errstate(all="ignore"):
        for v, row in enumerate(adj["incidence"]):
            ax, ay, az = F(0), F(0), F(0)
            for t in row:
                i0, i1, i2 = idx[t].tolist()
                pxx = F(P[i1, 0] - P[i0, 0])
                pxy = F(P[i1, 1] - P[i0, 1])
                pxz = F(P[i1, 2] - P[i0, 2])
                pyx = F(P[i2, 0] - P[i0, 0])
                pyy = F(P[i2, 1] - P[i0, 1])
                pyz = F(P[i2, 2] - P[i0, 2])
                a = F(pxy * pyz)
                b = F(pxz * pyy)
                ax = F(ax + F(a - b))
                a = F(pxz * pyx)
                b = F(pxx * pyz)
                ay = F(ay + F(a - b))
                a = F(pxx * pyy)
                b = F(pxy * pyx)
                az = F(az + F(a - b))
            xx = F(ax * ax)
            yy = F(ay * ay)
            zz = F(az * az)
            s = F(xx + yy)
            s = F(s + zz)
            length = F(np.sqrt(s))
            if length > 0:
                out[v, 0] = F(ax / length)
                out[v, 1] = F(ay / length)
                out[v, 2] = F(az / length)
    return out


def smooth_pass(adj, P, f, pin):
    """one pass with factor f: a pinned vertex is copied, any other moves towards the mean of its neighbours, in ascending order"""
    f = F(f)
    Q = P.copy()
    stays = pinned(adj["flags"], adj["neighbors"], pin)
    with np.errstate(all="ignore"):
        for v, row in enumerate(adj["neighbors"]):
            if stays[v]:
                continue
            for k in range(3):
                m = P[row[0], k]
                for u in row[1:]:
                    m = F(m + P[u, k])
                m = F(m / F(len(row)))
                d = F(m - P[v, k])
                step = F(f * d)
                Q[v, k] = F(P[v, k] + step)
    return Q


def smooth(adj, vertices, iterations, lam, mu, pin):
    """`iterations` times a pass with lam, then one with mu where mu != 0; every pass reads only the pass before it"""
    P = np.array(vertices, F).reshape(-1, 3).copy()
    for _ in range(iterations):
        P = smooth_pass(adj, P, lam, pin)
        if F(mu) != 0:
            P = smooth_pass(adj, P, mu, pin)
    return P


# ---- index arrays made by hand, beside mesh_components_restated.hand_cases() ----------------------------------------------------------------
def fan(deg):
    """`deg` triangles around vertex 0 -> (V, (deg, 3) int32): an open fan, vertex 0 has deg + 1 neighbours"""
    return deg + 2, np.array([(0, i, i + 1) for i in range(1, deg + 1)], np.int32)


def flat_grid(n):
    """(n + 1)^2 vertices at (i / 8, j / 8, 0.5), two triangles a cell, all with the same winding -> (vertices, indices)"""
    ids = lambda i, j: j * (n + 1) + i
    v = np.array([(i / 8.0, j / 8.0, 0.5) for j in range(n + 1) for i in range(n + 1)], F)
    t = []
    for j in range(n):
        for i in range(n):
            t += [(ids(i, j), ids(i + 1, j), ids(i + 1, j + 1)), (ids(i, j), ids(i + 1, j + 1), ids(i, j + 1))]
    return v, np.array(t, np.int32)


def positions(V, seed, nan_row=None):
    """(V, 3) finite float32 positions of a few units' size; nan_row: that row holds NaNs"""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((V, 3)) * 3).astype(F)
    if nan_row is not None and V:
        p[nan_row % V] = np.nan
    return p
