"""The coarse mesh of DESIGN.md 3.14 restated (TEST INFRASTRUCTURE, numpy only; MeshCube itself is the oracle's, oracle.mesh_cube).

A field is a dict of tests/voxel_fields.py: chunk id (x, y, z) -> (sdf[N^3], weight[N^3], rgbw[N^3, 4]), voxel id = (z N + y) N + x.
With s the stride and M = N / s, chunk c of the selection has the cubes (i, j, k) in [0, M)^3, walked by ascending (k M + j) M + i.  Cube
(i, j, k) has the base voxel b = s (i, j, k); corner d is the voxel b + s CORNERS[d], a component equal to N meaning voxel 0 of the
chunk one further along that axis.  A cube whose corner lies in an absent chunk, or has a weight <= 0.5, yields nothing.  The cube's
coordinates are ((float)b res + half_res) + (float)(N c) res per axis, its corner d lies at coords + (float)CORNERS[d] step with step
= (float)s res; the triangles are MeshCube's, each with its face normal three times.
"""
import numpy as np

from tests import voxel_fields as vf

F = np.float32
ABSENT, LOW_WEIGHT, MESHED = 0, 1, 2


def selection_all(field, box=None):
    """every chunk of the field, ascending by x, then y, then z (chisel_hip_list_chunks' order); box = (lo, hi): those inside"""
    ids = sorted(field)
    if box is not None:
        lo, hi = box
        ids = [c for c in ids if all(lo[a] <= c[a] <= hi[a] for a in range(3))]
    return ids


def grids(field, N):
    """chunk id -> (sdf, weight) as (N, N, N) arrays indexed [z, y, x]"""
    return {cid: (np.asarray(s, np.float32).reshape(N, N, N), np.asarray(w, np.float32).reshape(N, N, N)) for cid, (s, w, _) in field.items()}


def cubes_of(G, N, s, cid):
    """the cubes of chunk `cid` in the definition's order -> (i, j, k), state, sdf8 (None unless MESHED), chunks its corners lie in"""
    M = N // s
    for k in range(M):
        for j in range(M):
            for i in range(M):
                base = (s * i, s * j, s * k)
                sdf8 = np.zeros(8, np.float32)
                state = MESHED
                span = 1
                for a in range(3):
                    if base[a] + s == N:
                        span *= 2
                for d, off in enumerate(vf.CORNERS):
                    v = [base[a] + s * off[a] for a in range(3)]
                    nb = list(cid)
                    for a in range(3):
                        if v[a] == N:
                            v[a] = 0
                            nb[a] += 1
                    chunk = G.get(tuple(nb))
                    if chunk is None:
                        state = ABSENT
                        break
                    if chunk[1][v[2], v[1], v[0]] <= F(0.5):
                        state = min(state, LOW_WEIGHT)
                        continue  # (an absent corner further on still makes the cube one skipped for an absent neighbour)
                    sdf8[d] = chunk[0][v[2], v[1], v[0]]
                yield (i, j, k), state, (sdf8 if state == MESHED else None), span


def cube_coords(N, res, s, cid, ijk):
    """the cube's coordinates, one float32 operation per line"""
    r = F(res)
    half = r * F(0.5)
    out = np.zeros(3, np.float32)
    for a in range(3):
        x = F(s * ijk[a])
        x = x * r
        x = x + half
        o = F(N * cid[a])
        o = o * r
        out[a] = x + o
    return out


def coarse_mesh(oracle_mod, field, N, res, s, selection=None):
    """-> {"vertices": (V, 3), "normals": (V, 3) face normals, "table": (n, 2) int64, "ids": (n, 3) int32, "totals": {...}}; KeyError for
    a selected id that is not in the field"""
    assert 1 <= s <= N and N % s == 0
    ids = selection_all(field) if selection is None else [tuple(int(v) for v in c) for c in selection]
    G = grids(field, N)
    step = float(F(s) * F(res))
    verts, norms, table = [], [], []
    first = cubes_meshed = nonempty = 0
    for cid in ids:
        if cid not in G:
            raise KeyError(cid)
        count = 0
        for ijk, state, sdf8, _ in cubes_of(G, N, s, cid):
            if state != MESHED:
                continue
            cubes_meshed += 1
            v, n = oracle_mod.mesh_cube(sdf8, cube_coords(N, res, s, cid, ijk), step)
            if len(v):
                verts.append(v)
                norms.append(n)
                count += len(v)
        table.append((first, count))
        first += count
        nonempty += 1 if count else 0
    cat = lambda parts: np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 3), np.float32)
    return {"vertices": cat(verts), "normals": cat(norms), "table": np.array(table, np.int64).reshape(-1, 2),
            "ids": np.array(ids, np.int32).reshape(-1, 3),
            "totals": {"chunks": len(ids), "chunks_nonempty": nonempty, "cubes_meshed": cubes_meshed, "vertices": first}}


def decimate(field, N, s):
    """the field of chunk edge N / s that keeps the voxels at multiples of s"""
    M = N // s
    out = {}
    for cid, (sdf, w, c) in field.items():
        out[cid] = (np.ascontiguousarray(np.asarray(sdf, np.float32).reshape(N, N, N)[::s, ::s, ::s]).reshape(M ** 3),
                    np.ascontiguousarray(np.asarray(w, np.float32).reshape(N, N, N)[::s, ::s, ::s]).reshape(M ** 3),
                    np.ascontiguousarray(np.asarray(c, np.uint8).reshape(N, N, N, 4)[::s, ::s, ::s]).reshape(M ** 3, 4))
    return out


def reach(field, N, s, selection=None):
    """what the cubes of a coarse mesh contain, from the field alone: the configurations of the meshed cubes, cubes skipped for an
    absent neighbour and for a weight <= 0.5, meshed cubes by the number of chunks their corners lie in, and crossing edges of meshed
    cubes with |s1 - s2| below InterpolateVertex's 1e-6"""
    G = grids(field, N)
    out = {"configurations": set(), "meshed": 0, "absent": 0, "low_weight": 0, "span": {1: 0, 2: 0, 4: 0, 8: 0}, "tiny_edges": 0}
    for cid in (selection_all(field) if selection is None else selection):
        for _, state, sdf8, span in cubes_of(G, N, s, tuple(cid)):
            if state == ABSENT:
                out["absent"] += 1
            elif state == LOW_WEIGHT:
                out["low_weight"] += 1
            else:
                out["meshed"] += 1
                out["span"][span] += 1
                out["configurations"].add(sum((1 << d) for d in range(8) if sdf8[d] < 0))
                for a, b in vf.EDGES:
                    if (sdf8[a] < 0) != (sdf8[b] < 0) and abs(F(sdf8[a] - sdf8[b])) < vf.MIN_DIFF:
                        out["tiny_edges"] += 1
    return out


def triangles_as_bits(vertices):
    """(3 T, 3) float32 -> sorted list of 36-byte triangles: equal exactly when the multisets of triangles are, bit for bit"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 9)
    return sorted(row.tobytes() for row in v)
