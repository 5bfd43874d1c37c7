"""chisel_hip_frontiers restated in numpy (DESIGN.md 3.18 "Frontiers"), a builder of hand-built fields from state volumes, and the hand
volumes the tests of both sides share.

TEST INFRASTRUCTURE ONLY (tests/test_frontier_restated.py checks it on the CPU, tests/test_gpu_frontier.py uses it against the device).

Every array is indexed [z, y, x]; a voxel's linear index is (z ny + y) nx + x.  The states come from distance_restated.states over the
window widened by one voxel.  A FRONTIER voxel is a free voxel of the window with at least k unknown face neighbours (of the widened
window: of the map).  The clusters are the connected components of the frontier voxels of the window, numbered by ascending smallest
linear index; two labellings, scipy's and a flood fill over a dictionary, must agree.  Integers throughout: so must any kernel.
"""
import numpy as np

from tests import distance_restated as dr

F = np.float32
UNKNOWN, FREE, OCCUPIED = dr.UNKNOWN, dr.FREE, dr.OCCUPIED
TILE = (16, 16, 8)  # the labelling tile of the device, x, y, z (frontier_checks.h: FRONTIER_TILE_*)
MAX_VOXELS = 1 << 26
TOTALS = ("unknown", "free", "occupied", "frontier", "clusters", "largest_voxels", "kept_clusters", "kept_voxels")
COLUMNS = ("root", "voxels", "sum_x", "sum_y", "sum_z", "min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "unknown_faces")
SPARSE_CASES = ((8, 3), (16, 2), (32, 2), (8, 4))  # (N, B) of distance_restated.sparse
SPARSE_SEED = 7


def wide_states(fields, N, origin, dims, offset=0.0):
    """the states of the window widened by one voxel on every side, uint8 [nz + 2, ny + 2, nx + 2]"""
    return dr.states(fields, N, origin, dims, 1, offset)


def unknown_faces(wide):
    """the number of unknown face neighbours of every voxel of the window, int64 [nz, ny, nx]"""
    u = (wide == UNKNOWN).astype(np.int64)
    c = (slice(1, -1),) * 3
    n = np.zeros(tuple(s - 2 for s in wide.shape), np.int64)
    for axis in range(3):
        for side in (slice(0, -2), slice(2, None)):
            sl = list(c)
            sl[axis] = side
            n += u[tuple(sl)]
    return n


def frontier(wide, min_unknown_faces):
    """(the frontier voxels of the window, bool; unknown_faces)"""
    faces = unknown_faces(wide)
    return (dr.window_of(wide, 1) == FREE) & (faces >= int(min_unknown_faces)), faces


def offsets(connectivity):
    """the offsets with 1, <= 2, <= 3 non-zero coordinates, each in -1 ... 1, as (dz, dy, dx)"""
    level = {6: 1, 18: 2, 26: 3}[int(connectivity)]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 1 <= (dz != 0) + (dy != 0) + (dx != 0) <= level]


def renumber_by_root(lab):
    """labels > 0 of any numbering -> int64, -1 elsewhere, clusters 0 ... C - 1 by ascending smallest linear index"""
    flat = lab.ravel()
    out = np.full(flat.shape, -1, np.int64)
    at = np.flatnonzero(flat > 0)
    if len(at):
        names, first = np.unique(flat[at], return_index=True)  # first: the position in `at` of each label's first voxel (ascending linear index)
        order = np.argsort(first, kind="stable")
        number = np.empty(len(names), np.int64)
        number[order] = np.arange(len(names))
        out[at] = number[np.searchsorted(names, flat[at])]
    return out.reshape(lab.shape)


def clusters_scipy(front, connectivity):
    """scipy.ndimage.label with generate_binary_structure(3, 1 | 2 | 3), renumbered by smallest linear index (scipy's own order is not relied on)"""
    from scipy import ndimage
    lab, _ = ndimage.label(front, structure=ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[int(connectivity)]))
    return renumber_by_root(lab)


def clusters_flood(front, connectivity):
    """the same by a plain flood fill over a dictionary, visiting the voxels in ascending linear index: the k-th fill is cluster k"""
    nz, ny, nx = front.shape
    cells = {(int(z), int(y), int(x)): -1 for z, y, x in zip(*np.nonzero(front))}
    offs = offsets(connectivity)
    n = 0
    for start in sorted(cells):  # (z, y, x) ascending = the linear index ascending
        if cells[start] >= 0:
            continue
        cells[start] = n
        stack = [start]
        while stack:
            z, y, x = stack.pop()
            for dz, dy, dx in offs:
                q = (z + dz, y + dy, x + dx)
                if cells.get(q, 0) == -1:
                    cells[q] = n
                    stack.append(q)
        n += 1
    out = np.full(front.shape, -1, np.int64)
    for (z, y, x), c in cells.items():
        out[z, y, x] = c
    return out


def answer(wide, min_unknown_faces=1, connectivity=26, min_voxels=1, labeller=clusters_scipy):
    """everything chisel_hip_frontiers answers, from the states of the widened window -> {"state", "label", "voxels", "table", "totals",
    and, beyond the entry's outputs, "all": every cluster's number before the filter (-1 elsewhere), "sizes": every cluster's voxels}"""
    state = np.ascontiguousarray(dr.window_of(wide, 1))
    front, faces = frontier(wide, min_unknown_faces)
    every = labeller(front, connectivity)
    C = int(every.max()) + 1 if front.any() else 0
    sizes = np.bincount(every[front], minlength=C).astype(np.int64)
    keep = sizes >= int(min_voxels)
    new = np.where(keep, np.cumsum(keep) - 1, -2).astype(np.int64)
    label = np.full(state.shape, -1, np.int32)
    label[front] = new[every[front]]
    z, y, x = np.nonzero(label >= 0)  # ascending linear index
    c = label[z, y, x].astype(np.int64)
    voxels = np.stack([x, y, z, c], axis=1).astype(np.int32).reshape(-1, 4)
    K = int(keep.sum())
    nz, ny, nx = state.shape
    lin = (z * ny + y) * nx + x
    f = faces[z, y, x]
    table = np.zeros((K, 12), np.int64)
    if K:
        big = np.iinfo(np.int64).max
        table[:, 0], table[:, 5:8], table[:, 8:11] = big, big, -1
        np.minimum.at(table[:, 0], c, lin)
        table[:, 1] = np.bincount(c, minlength=K)
        for j, coordinate in enumerate((x, y, z)):
            np.add.at(table[:, 2 + j], c, coordinate)
            np.minimum.at(table[:, 5 + j], c, coordinate)
            np.maximum.at(table[:, 8 + j], c, coordinate)
        np.add.at(table[:, 11], c, f)
    totals = {"unknown": int((state == UNKNOWN).sum()), "free": int((state == FREE).sum()), "occupied": int((state == OCCUPIED).sum()),
              "frontier": int(front.sum()), "clusters": C, "largest_voxels": int(sizes.max()) if C else 0, "kept_clusters": K, "kept_voxels": int(len(voxels))}
    return {"state": state, "label": label, "voxels": voxels, "table": table, "totals": totals, "all": every, "sizes": sizes}


def centres(origin, table, res):
    """((origin + sum / voxels) + 0.5) * resolution, float64 (K, 3), metres"""
    table = np.asarray(table, np.int64).reshape(-1, 12)
    mean = table[:, 2:5].astype(np.float64) / np.maximum(table[:, 1:2], 1).astype(np.float64)
    return ((np.asarray(origin, np.float64)[None, :] + mean) + 0.5) * float(F(res))


def spans_tiles(table_row, tile=TILE):
    """does the cluster's box cross a tile border of the window on every axis?"""
    return all(int(table_row[5 + a]) // tile[a] != int(table_row[8 + a]) // tile[a] for a in range(3))


# ---- hand-built fields from state volumes -----------------------------------------------------------------------------------------------
def fields_from_states(volume, N, base, res=0.0625, absent=True):
    """a uint8 state volume [z, y, x] whose first voxel has the global index `base` (x, y, z; any integers) -> a field {chunk id:
    (sdf, weight, rgbw)}: unknown = weight 0, free = weight 1 and sdf +res, occupied = weight 1 and sdf -res; the voxels of the touched
    chunks outside the volume are unknown.  absent: chunks that are wholly unknown are left out; else they are there with zero weights"""
    volume = np.asarray(volume, np.uint8)
    base = np.asarray(base, np.int64)
    lo = np.floor_divide(base, N)
    hi = np.floor_divide(base + np.array(volume.shape[::-1], np.int64) - 1, N)
    n = (hi - lo + 1) * N  # x, y, z
    grid = np.zeros((int(n[2]), int(n[1]), int(n[0])), np.uint8)
    o = base - lo * N
    grid[o[2]:o[2] + volume.shape[0], o[1]:o[1] + volume.shape[1], o[0]:o[0] + volume.shape[2]] = volume
    out = {}
    for cz in range(int(hi[2] - lo[2] + 1)):
        for cy in range(int(hi[1] - lo[1] + 1)):
            for cx in range(int(hi[0] - lo[0] + 1)):
                st = grid[cz * N:(cz + 1) * N, cy * N:(cy + 1) * N, cx * N:(cx + 1) * N]
                if absent and not st.any():
                    continue
                sdf = np.where(st == OCCUPIED, -F(res), F(res)).astype(np.float32)
                w = (st != UNKNOWN).astype(np.float32)
                out[(int(lo[0]) + cx, int(lo[1]) + cy, int(lo[2]) + cz)] = (np.ascontiguousarray(sdf).reshape(-1), np.ascontiguousarray(w).reshape(-1),
                                                                           np.zeros((N ** 3, 4), np.uint8))
    return out


# ---- the hand volumes: name -> (volume of the window, the clusters at connectivity 26 / 18 / 6 with min_unknown_faces 1, or None) ------------
def serpentine(shape=(24, 40, 40)):
    """a one-voxel-wide free corridor through an unknown block [z, y, x]: along x in every second row of every second plane, joined at
    alternating ends, the planes joined likewise: every corridor voxel is a frontier voxel, all of them one cluster"""
    nz, ny, nx = shape
    v = np.zeros(shape, np.uint8)
    right = True  # where the last row ended
    rows = list(range(0, ny, 2))
    for k, z in enumerate(range(0, nz, 2)):
        ys = rows if k % 2 == 0 else rows[::-1]
        for j, y in enumerate(ys):
            v[z, y, :] = FREE
            if j + 1 < len(ys):
                x = nx - 1 if right else 0
                v[z, min(y, ys[j + 1]):max(y, ys[j + 1]) + 1, x] = FREE
                right = not right
        if z + 2 < nz:
            x = nx - 1 if right else 0
            v[z:z + 3, ys[-1], x] = FREE
            right = not right
    return v


def comb(shape=(3, 21, 40)):
    """teeth along y in every second column, joined only by the last row [z = 1]"""
    v = np.zeros(shape, np.uint8)
    v[1, :, ::2] = FREE
    v[1, -1, :] = FREE
    return v


def pair(kind):
    """two free voxels in an unknown 5 x 5 x 5 block, touching by a face, an edge or a corner only"""
    v = np.zeros((5, 5, 5), np.uint8)
    v[2, 2, 2] = FREE
    v[{"face": (2, 2, 3), "edge": (2, 3, 3), "corner": (3, 3, 3)}[kind]] = FREE
    return v


def bridge():
    """two free bars along x in an unknown block, joined only by a free voxel in the column x = 8: a window of the columns 0 ... 7
    sees two clusters, one of the columns 0 ... 8 sees one"""
    v = np.zeros((3, 5, 9), np.uint8)
    v[1, 1, :] = FREE
    v[1, 3, :] = FREE
    v[1, 2, 8] = FREE
    return v


def faces_case(k):
    """a free voxel at the centre of an occupied 3 x 3 x 3 block with exactly k unknown faces"""
    v = np.full((3, 3, 3), OCCUPIED, np.uint8)
    v[1, 1, 1] = FREE
    for at in [(1, 1, 0), (1, 1, 2), (1, 0, 1), (1, 2, 1), (0, 1, 1), (2, 1, 1)][:k]:
        v[at] = UNKNOWN
    return v


def hand_volumes():
    """name -> (volume, expected clusters at connectivity (26, 18, 6) with min_unknown_faces 1, or None)"""
    out = {"serpentine": (serpentine(), (1, 1, 1)), "comb": (comb(), (1, 1, 1)), "face": (pair("face"), (1, 1, 1)), "edge": (pair("edge"), (1, 1, 2)),
           "corner": (pair("corner"), (1, 2, 2)), "bridge": (bridge(), (1, 1, 1))}
    for k in range(7):
        out["faces%d" % k] = (faces_case(k), (min(k, 1),) * 3)
    for name, s in (("unknown", UNKNOWN), ("free", FREE), ("occupied", OCCUPIED)):
        out["all_" + name] = (np.full((9, 10, 70), s, np.uint8), None)
    return out


def hand_case(name, N, base, window=None, absent=True, res=0.0625):
    """(fields, origin, dims) of a hand volume placed at `base`; the window is the volume itself, or `window` = (lo, dims) relative to it"""
    volume = hand_volumes()[name][0]
    fields = fields_from_states(volume, N, base, res, absent)
    lo, dims = window if window is not None else ((0, 0, 0), volume.shape[::-1])
    return fields, tuple(int(base[a] + lo[a]) for a in range(3)), tuple(int(d) for d in dims)
