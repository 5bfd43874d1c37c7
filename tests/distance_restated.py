"""chisel_hip_distance_field restated in numpy (DESIGN.md 3.11 "Distance field"), and a builder of sparse hand-built maps for it.

TEST INFRASTRUCTURE ONLY (tests/test_distance_restated.py checks it on the CPU, tests/test_gpu_distance.py uses it against the device).

A global voxel index per axis is g = chunk_id * N + voxel_coordinate.  A window is origin (x, y, z), dims (nx, ny, nz); every array here
is indexed [z, y, x].  The answer is a set of integers -- squared voxel distances -- so `brute` (the definition as written: every offset
of the ball) and `separable` (three one-dimensional passes) must agree exactly, and so must any kernel.
"""
import numpy as np

from tests import voxel_fields as vf

F = np.float32
ID_BIAS = 1 << 20
ID_MIN, ID_MAX = -ID_BIAS + 2, ID_BIAS - 2  # the chunk ids the look-up accepts, per axis
BIG = np.int32(1 << 28)
UNKNOWN, FREE, OCCUPIED = 0, 1, 2


def voxel_box(fields, N, lo, dims):
    """(sdf, weight, resident) of the box of voxels that starts at global index lo (x, y, z) and has dims (x, y, z): arrays [z, y, x];
    resident: the voxel's chunk is in `fields` and its id is one the look-up accepts"""
    lo, dims = np.asarray(lo, np.int64), np.asarray(dims, np.int64)
    shape = (int(dims[2]), int(dims[1]), int(dims[0]))
    sdf, wgt, resident = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape, bool)
    hi = lo + dims  # exclusive
    for cid, chunk in fields.items():
        c = np.asarray(cid, np.int64)
        if (c < ID_MIN).any() or (c > ID_MAX).any():
            continue
        a, b = np.maximum(c * N, lo), np.minimum((c + 1) * N, hi)  # the overlap, global
        if (a >= b).any():
            continue
        src = tuple(slice(int(a[k] - c[k] * N), int(b[k] - c[k] * N)) for k in (2, 1, 0))
        dst = tuple(slice(int(a[k] - lo[k]), int(b[k] - lo[k])) for k in (2, 1, 0))
        sdf[dst] = np.asarray(chunk[0], np.float32).reshape(N, N, N)[src]
        wgt[dst] = np.asarray(chunk[1], np.float32).reshape(N, N, N)[src]
        resident[dst] = True
    return sdf, wgt, resident


def states(fields, N, origin, dims, R, offset):
    """the state of every voxel of the window widened by R on every side: uint8 [nz + 2 R, ny + 2 R, nx + 2 R].  0 unknown: the chunk
    is not resident or the weight fails GetSDF's rule; 2 occupied: observed and sdf < offset, one float32 compare; 1 free"""
    lo = np.asarray(origin, np.int64) - R
    sdf, wgt, resident = voxel_box(fields, N, lo, np.asarray(dims, np.int64) + 2 * R)
    observed = resident & (wgt.astype(np.float64) > 1e-12)
    with np.errstate(invalid="ignore"):
        occupied = observed & (sdf < F(offset))
    return np.where(occupied, OCCUPIED, np.where(observed, FREE, UNKNOWN)).astype(np.uint8)


def window_of(st, R):
    """the window's own part of an array over the widened window"""
    return st[R:st.shape[0] - R, R:st.shape[1] - R, R:st.shape[2] - R]


def obstacles(st, unknown_is_obstacle):
    return (st == OCCUPIED) | (bool(unknown_is_obstacle) & (st == UNKNOWN))


def brute(st, R, unknown_is_obstacle=False):
    """dist2 over the window, int32 [nz, ny, nx], from the states of the widened window -- the definition as written: for every offset
    of the ball |d|^2 <= R^2, the obstacles at that offset; -1 without one"""
    obs = obstacles(st, unknown_is_obstacle)
    nz, ny, nx = (s - 2 * R for s in st.shape)
    best = np.full((nz, ny, nx), BIG, np.int32)
    for dz in range(-R, R + 1):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                d2 = dx * dx + dy * dy + dz * dz
                if d2 > R * R:
                    continue
                there = obs[R + dz:R + dz + nz, R + dy:R + dy + ny, R + dx:R + dx + nx]
                best = np.where(there & (d2 < best), np.int32(d2), best)
    return np.where(best == BIG, np.int32(-1), best).astype(np.int32)


def _pass(g, axis, R):
    """g'(i) = min over |d| <= R of g(i + R + d) + d^2 along `axis`, which loses R entries at either end"""
    n = g.shape[axis] - 2 * R
    out = None
    for d in range(-R, R + 1):
        sl = [slice(None)] * 3
        sl[axis] = slice(R + d, R + d + n)
        term = g[tuple(sl)] + np.int32(d * d)
        out = term if out is None else np.minimum(out, term)
    return out


def separable(st, R, unknown_is_obstacle=False):
    """the same by three one-dimensional passes (x, y, z) and the final threshold at R^2"""
    g = np.where(obstacles(st, unknown_is_obstacle), np.int32(0), BIG).astype(np.int32)
    for axis in (2, 1, 0):
        g = _pass(g, axis, R)
    return np.where(g > R * R, np.int32(-1), g).astype(np.int32)


def distance(dist2, res):
    """(float)(sqrt((double)dist2) * (double)res), +inf where dist2 is -1"""
    d = np.sqrt(np.maximum(dist2, 0).astype(np.float64)) * np.float64(F(res))
    return np.where(dist2 < 0, F(np.inf), d.astype(np.float32)).astype(np.float32)


def centres(origin, dims, res):
    """the centres ((float)g + 0.5f) * res of the window's voxels, (n, 3) float32 in the order of the outputs"""
    ax = [((np.arange(dims[k], dtype=np.int64) + int(origin[k])).astype(np.float32) + F(0.5)) * F(res) for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


def sparse(N, B, seed, res=0.0625, p=0.003, base=(0, 0, 0)):
    """a B^3 block of chunks at any base id: every voxel observed (weight 1) with |sdf| uniform in [0.05 res, res], negative with
    probability p; 0.5 % of the weights 1e-12 (unobserved by GetSDF's rule); a slab of zero weights across the block; two chunks of
    the block absent.  The voxels are drawn for the block as one grid and do not depend on the base."""
    rng = np.random.default_rng(seed)
    n = B * N
    mag = rng.uniform(0.05 * res, res, (n, n, n))
    sign = np.where(rng.random((n, n, n)) < p, -1.0, 1.0)
    w = np.where(rng.random((n, n, n)) < 0.005, vf.W_EDGE, F(1)).astype(np.float32)
    z0 = n // 3 + 1
    w[z0:z0 + max(2, N // 4), :, :] = 0  # the slab
    field = vf._cut((sign * mag).astype(np.float32), w, np.zeros((n, n, n, 4), np.uint8), N, B, base)
    ids = vf.block_ids(B, base)
    for k in rng.choice(len(ids), 2, replace=False):
        del field[ids[int(k)]]
    return field


def block_window(N, B, base, over_lo=(3, 7, 5), over_hi=(9, 4, 6)):
    """(origin, dims) of a window that overhangs the block by over_lo voxels below and over_hi above, per axis"""
    lo = np.asarray(base, np.int64) * N - np.asarray(over_lo, np.int64)
    hi = (np.asarray(base, np.int64) + B) * N + np.asarray(over_hi, np.int64)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo)


def reach(state, dist2, R):
    """what an answer contains: the share of each state, the share of -1, the distinct values of dist2"""
    n = float(state.size)
    return {"unknown": float((state == UNKNOWN).sum()) / n, "free": float((state == FREE).sum()) / n, "occupied": float((state == OCCUPIED).sum()) / n,
            "none": float((dist2 < 0).sum()) / n, "values": np.unique(dist2[dist2 >= 0])}


def check_reach(state, dist2, R):
    """the reach conditions of a sparse map's answer without the flag: every state in at least 0.05 % of the window; at R = 5, -1 in
    30 ... 80 % of it and at least 20 distinct values with 0, 1 and 25 among them; at R = 13 at least 100 distinct values and 169"""
    r = reach(state, dist2, R)
    assert min(r["unknown"], r["free"], r["occupied"]) >= 0.0005, r
    vals = set(r["values"].tolist())
    if R == 5:
        assert 0.30 <= r["none"] <= 0.80, r
        assert len(vals) >= 20 and {0, 1, 25} <= vals, sorted(vals)
    if R == 13:
        assert len(vals) >= 100 and 169 in vals, sorted(vals)
    return r
