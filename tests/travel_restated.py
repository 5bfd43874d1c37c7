"""chisel_hip_travel_field restated (DESIGN.md 3.19 "Travel field"), three ways that must agree exactly, and the cases the tests of both
sides share.

TEST INFRASTRUCTURE ONLY (tests/test_travel_restated.py checks it on the CPU, tests/test_gpu_travel.py uses it against the device).

Every array is indexed [z, y, x]; a voxel's linear index is (z ny + y) nx + x; seeds are rows (x, y, z), targets rows (x, y, z, group).
The states come from distance_restated.states, the clearance from distance_restated.separable.  The costs are integers: `relaxation`
(whole-volume numpy relaxation to the fixed point), `heap` (heapq Dijkstra over a dictionary) and `scipy_form`
(scipy.sparse.csgraph.dijkstra on the explicit grid graph; floats, exact below 2^53) must agree, and so must any kernel.
"""
import heapq

import numpy as np

from tests import distance_restated as dr
from tests import frontier_restated as fr

UNKNOWN, FREE, OCCUPIED = dr.UNKNOWN, dr.FREE, dr.OCCUPIED
TILE = fr.TILE
INF = np.int64(1) << 40
SEED, NONE = 13, 255
TOTALS = ("unknown", "free", "occupied", "traversable", "seeds_used", "seeds_ignored", "reached", "largest_cost", "targets_reached", "targets_ignored")
DIAGNOSTICS = ("rounds", "tile_visits")  # of the implementation: never compared
COST_SETS = ((1, 1, 1), (3, 4, 5), (10, 14, 17))


def offsets(connectivity):
    """the moves as (dz, dy, dx), in ascending code (dz + 1) 9 + (dy + 1) 3 + (dx + 1)"""
    return fr.offsets(connectivity)


def code(o):
    return (o[0] + 1) * 9 + (o[1] + 1) * 3 + (o[2] + 1)


def move_cost(o, step_cost):
    return int(step_cost[sum(1 for d in o if d) - 1])


def traversable(fields, N, origin, dims, clearance=0, unknown_is_obstacle=False, offset=0.0):
    """(state of the window uint8, traversable bool): free, and with a clearance no obstacle of the map within it"""
    R = int(clearance)
    st = dr.states(fields, N, origin, dims, R, offset)
    state = np.ascontiguousarray(dr.window_of(st, R) if R else st)
    trav = state == FREE
    if R:
        trav = trav & (dr.separable(st, R, unknown_is_obstacle) == -1)
    return state, trav


def _views(shape, o):
    """(destination, source) slices: source = destination + o"""
    dst, src = [], []
    for n, d in zip(shape, o):
        dst.append(slice(max(0, -d), n - max(0, d)))
        src.append(slice(max(0, d), n - max(0, -d)))
    return tuple(dst), tuple(src)


def _seed_mask(trav, seeds):
    seeds = np.asarray(seeds, np.int64).reshape(-1, 3)
    on = trav[seeds[:, 2], seeds[:, 1], seeds[:, 0]]
    mask = np.zeros(trav.shape, bool)
    used = seeds[on]
    mask[used[:, 2], used[:, 1], used[:, 0]] = True
    return mask, int(on.sum()), int((~on).sum())


def relaxation(trav, seeds, connectivity=26, step_cost=(10, 14, 17), max_cost=1 << 30):
    """cost int32 [nz, ny, nx], -1 unreached: shifts, a minimum and the max_cost cut until nothing falls"""
    mask, _, _ = _seed_mask(trav, seeds)
    cost = np.where(mask, np.int64(0), INF)
    moves = [(o, move_cost(o, step_cost)) for o in offsets(connectivity)]
    while True:
        new = cost.copy()
        for o, c in moves:
            dst, src = _views(cost.shape, o)
            cand = cost[src] + c
            ok = trav[dst] & (cand <= int(max_cost))
            new[dst] = np.where(ok, np.minimum(new[dst], cand), new[dst])
        if np.array_equal(new, cost):
            break
        cost = new
    return np.where(cost >= INF, -1, cost).astype(np.int32)


def heap(trav, seeds, connectivity=26, step_cost=(10, 14, 17), max_cost=1 << 30):
    """the same by Dijkstra with heapq over a dictionary"""
    mask, _, _ = _seed_mask(trav, seeds)
    nz, ny, nx = trav.shape
    moves = [(o, move_cost(o, step_cost)) for o in offsets(connectivity)]
    best = {(int(z), int(y), int(x)): 0 for z, y, x in zip(*np.nonzero(mask))}
    queue = [(0, v) for v in best]
    heapq.heapify(queue)
    while queue:
        c, v = heapq.heappop(queue)
        if c > best[v]:
            continue
        for o, m in moves:
            q = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if not (0 <= q[0] < nz and 0 <= q[1] < ny and 0 <= q[2] < nx) or not trav[q]:
                continue
            n = c + m
            if n <= int(max_cost) and n < best.get(q, INF):
                best[q] = n
                heapq.heappush(queue, (n, q))
    cost = np.full(trav.shape, -1, np.int32)
    for v, c in best.items():
        cost[v] = c
    return cost


def scipy_form(trav, seeds, connectivity=26, step_cost=(10, 14, 17), max_cost=1 << 30):
    """the same by scipy.sparse.csgraph.dijkstra (min_only over the used seeds, limit = max_cost) on the explicit grid graph"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    mask, used, _ = _seed_mask(trav, seeds)
    cost = np.full(trav.shape, -1, np.int32)
    if not used:
        return cost
    n = trav.size
    lin = np.arange(n, dtype=np.int64).reshape(trav.shape)
    rows, cols, vals = [], [], []
    for o in offsets(connectivity):
        dst, src = _views(trav.shape, o)
        ok = trav[dst] & trav[src]
        rows.append(lin[src][ok])
        cols.append(lin[dst][ok])
        vals.append(np.full(int(ok.sum()), float(move_cost(o, step_cost))))
    graph = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    d = dijkstra(graph, directed=True, indices=np.flatnonzero(mask.ravel()), min_only=True, limit=float(max_cost))
    d = d.reshape(trav.shape)
    reached = np.isfinite(d)
    cost[reached] = d[reached].astype(np.int64).astype(np.int32)
    return cost


def step_of(cost, connectivity=26, step_cost=(10, 14, 17)):
    """STEP from the costs alone: 13 at cost 0, 255 at -1, else the smallest code of a move o with cost(v + o) + cost_of(o) == cost(v)"""
    cost = np.asarray(cost, np.int64)
    step = np.full(cost.shape, NONE, np.uint8)
    for o in offsets(connectivity)[::-1]:  # descending code: the smallest is written last
        dst, src = _views(cost.shape, o)
        fits = (cost[dst] > 0) & (cost[src] >= 0) & (cost[src] + move_cost(o, step_cost) == cost[dst])
        step[dst] = np.where(fits, np.uint8(code(o)), step[dst])
    step[cost == 0] = SEED
    return step


def table_of(cost, targets, n_groups):
    """(table int64 (n_groups, 4), targets reached, targets ignored)"""
    nz, ny, nx = cost.shape
    table = np.zeros((int(n_groups), 4), np.int64)
    table[:, 2:] = -1
    reached = ignored = 0
    best = {}
    for x, y, z, g in np.asarray(targets, np.int64).reshape(-1, 4):
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz and 0 <= g < n_groups):
            ignored += 1
            continue
        table[g, 0] += 1
        c = int(cost[z, y, x])
        if c < 0:
            continue
        reached += 1
        table[g, 1] += 1
        key = (c, int((z * ny + y) * nx + x))
        if g not in best or key < best[g]:
            best[g] = key
    for g, (c, v) in best.items():
        table[g, 2], table[g, 3] = c, v
    return table, reached, ignored


def answer(state, trav, seeds, connectivity=26, step_cost=(10, 14, 17), max_cost=1 << 30, targets=None, n_groups=0, form=scipy_form):
    """everything chisel_hip_travel_field answers -> {"cost", "step", "state", "table", "totals"} (totals without the diagnostics)"""
    _, used, ignored = _seed_mask(trav, seeds)
    cost = form(trav, seeds, connectivity, step_cost, max_cost)
    step = step_of(cost, connectivity, step_cost)
    table, t_reached, t_ignored = (None, 0, 0) if targets is None or not len(targets) else table_of(cost, targets, n_groups)
    totals = {"unknown": int((state == UNKNOWN).sum()), "free": int((state == FREE).sum()), "occupied": int((state == OCCUPIED).sum()),
              "traversable": int(trav.sum()), "seeds_used": used, "seeds_ignored": ignored, "reached": int((cost >= 0).sum()),
              "largest_cost": int(cost.max()) if (cost >= 0).any() else -1, "targets_reached": t_reached, "targets_ignored": t_ignored}
    return {"cost": cost, "step": step, "state": np.ascontiguousarray(state), "table": table, "totals": totals}


def walk(step, start):
    """the plain walk of chisel_hip_travel_path: (n, 3) int32 rows (x, y, z) from `start` to its seed; ValueError where the entry refuses"""
    nz, ny, nx = step.shape
    x, y, z = (int(v) for v in start)
    if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz) or step[z, y, x] == NONE:
        raise ValueError("start")
    rows = []
    while True:
        if len(rows) >= step.size:
            raise ValueError("cycle")
        rows.append((x, y, z))
        c = int(step[z, y, x])
        if c == SEED:
            break
        if c > 26:
            raise ValueError("code")
        x, y, z = x + c % 3 - 1, y + (c // 3) % 3 - 1, z + c // 9 - 1
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            raise ValueError("leaves")
    return np.asarray(rows, np.int32).reshape(-1, 3)


def walk_cost(path, step_cost):
    """the summed move costs along a walk"""
    d = np.abs(np.diff(np.asarray(path, np.int64), axis=0))
    assert d.max(initial=0) <= 1
    k = d.sum(axis=1)
    assert (k >= 1).all()
    return int(sum(int(step_cost[int(v) - 1]) for v in k))


# ---- the shared cases: name -> (state volume [z, y, x], seeds) ----------------------------------------------------------------------------
def walled(shape=(12, 36, 40)):
    """a free box with occupied walls that leave gaps at alternating ends, and an unknown pocket"""
    v = np.full(shape, FREE, np.uint8)
    nz, ny, nx = shape
    for k, x in enumerate(range(6, nx - 2, 7)):
        v[:, :, x] = OCCUPIED
        if k % 2:
            v[1:4, 1:4, x] = FREE
        else:
            v[nz - 4:nz - 1, ny - 4:ny - 1, x] = FREE
    v[5:8, 10:14, 1:4] = UNKNOWN
    return v


def corridor_first(volume):
    """the first free voxel of a volume in linear index, as a seed row (x, y, z)"""
    z, y, x = (int(a[0]) for a in np.nonzero(volume == FREE))
    return [(x, y, z)]


def seam(kind):
    """two free voxels in unknown space, (15, 15, 7) and its face, edge or corner neighbour across the tile border: a volume
    (9, 17, 17) [z, y, x]; the seed on the first"""
    v = np.zeros((9, 17, 17), np.uint8)
    v[7, 15, 15] = FREE
    v[{"face": (7, 15, 16), "edge": (7, 16, 16), "corner": (8, 16, 16)}[kind]] = FREE
    return v, [(15, 15, 7)]


def cases():
    """name -> (volume, seeds)"""
    out = {"walled": (walled(), [(1, 1, 1)]), "serpentine": (fr.serpentine(), corridor_first(fr.serpentine())),
           "small_serpentine": (fr.serpentine((6, 20, 40)), corridor_first(fr.serpentine((6, 20, 40)))),
           "comb": (fr.comb(), corridor_first(fr.comb())),
           "open_box": (np.full((12, 36, 40), FREE, np.uint8), [(0, 0, 0), (39, 35, 11)])}
    for kind in ("face", "edge", "corner"):
        out["seam_" + kind] = seam(kind)
    return out


def tile_borders_crossed(volume, seeds):
    """does the reached set of a case span more than one tile?"""
    cost = scipy_form(volume == FREE, seeds, 26, (1, 1, 1))
    z, y, x = np.nonzero(cost >= 0)
    return len(set(zip((x // TILE[0]).tolist(), (y // TILE[1]).tolist(), (z // TILE[2]).tolist())))
