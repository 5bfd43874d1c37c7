"""chisel_hip_cast_rays and the voxel read-out of chisel_hip_query_points, restated in numpy (TEST INFRASTRUCTURE: DESIGN.md
"Querying points and rays" is the definition), and the point and ray sets the CPU and the GPU tests share.

Built on tests/render_restated.py: VoxelIndex.sample is ChunkManager::GetSDF; everything is float32, one rounding per operation, in
the order the definition writes it.  cast_rays runs every sample of every ray that has not ended -- nothing is skipped, no state is
shared between rays: the full march the kernel's shortcuts must agree with bit for bit.

A ray is a row of 8 float32: origin, direction, t_near, t_far (chisel_hip_ray)."""
import numpy as np

from tests import render_restated as rr

F = np.float32
MAX_SAMPLES = rr.MAX_SAMPLES


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def sample_counts(rays, step):
    """K_r = floorf((t_far - t_near) / step) + 1, capped at 65536; 0 where the quotient is negative or NaN, or the origin, the
    direction or t_near is not finite.  -> (n,) int64"""
    rays = np.asarray(rays, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = np.floor((rays[:, 7] - rays[:, 6]) / F(step))
        ok = (q >= 0) & np.isfinite(rays[:, :7]).all(1)
        K = np.where(ok, np.minimum(np.where(ok, q, 0), MAX_SAMPLES - 1) + 1, 0)
    return K.astype(np.int64)


def cast_rays(index, rays, step=0.0):
    """-> (t_hit (n,) float32, NaN unless status is 1; status (n,) uint8: 1 hit, 2 ended behind a surface, 0 never ended).
    index: a render_restated.VoxelIndex; step <= 0: the map's resolution."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    step = F(step) if step > 0 else index.res
    n = len(rays)
    o, d, t_near = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
    K = sample_counts(rays, step)
    t_hit = np.full(n, np.nan, np.float32)
    status = np.zeros(n, np.uint8)
    prev_obs = np.zeros(n, bool)
    prev_s = np.zeros(n, np.float32)
    alive = np.ones(n, bool)
    for k in range(int(K.max()) if n else 0):
        alive &= K > k
        a = np.flatnonzero(alive)
        if not len(a):
            break
        with np.errstate(invalid="ignore", over="ignore"):
            t = t_near[a] + F(k) * step  # from k, never accumulated
            pos = o[a] + t[:, None] * d[a]
        fin = np.isfinite(pos).all(1)  # (t d overflowed: no voxel contains the sample)
        obs, s, _ = index.sample(np.where(fin[:, None], pos, F(0)))
        obs &= fin
        with np.errstate(invalid="ignore"):
            end = obs & (s <= 0)
            hit = end & prev_obs[a] & (prev_s[a] > 0)
        if hit.any():
            ps = prev_s[a][hit]
            t_prev = t_near[a][hit] + F(k - 1) * step
            t_hit[a[hit]] = t_prev + step * (ps / (ps - s[hit]))
        status[a[end]] = 2
        status[a[hit]] = 1
        prev_obs[a] = obs
        prev_s[a] = s
        alive[a[end]] = False
    return t_hit, status


def sample_weight(index, pos):
    """the voxel ChunkManager::GetSDF reads for each position, as VoxelIndex.sample addresses it: -> (in range (n,) bool: chunk
    resident and linear voxel id in [0, N^3); weight (n,) float32, NaN where not in range).  A position with a non-finite component is
    in no voxel."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    fin = np.isfinite(pos).all(1)
    pos = np.where(fin[:, None], pos, F(0))
    N = index.N
    ids = index.chunk_ids(pos)
    row = index.rows(ids)
    origin = (N * ids).astype(np.float32) * index.res
    c = np.floor((pos - origin) * index.rf_voxel).astype(np.int32).astype(np.int64)
    vid = (c[:, 2] * N + c[:, 1]) * N + c[:, 0]
    ok = fin & (row >= 0) & (vid >= 0) & (vid < N ** 3)
    w = index.wgt[np.where(ok, row, 0), np.where(ok, vid, 0)]
    return ok, np.where(ok, w, F(np.nan)).astype(np.float32)


def query_points(index, pos):
    """-> found bit 0 (n,) bool, sdf (n,) float32 (NaN where not found), weight (n,) float32 (NaN where the voxel does not exist)"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    fin = np.isfinite(pos).all(1)
    obs, s, _ = index.sample(np.where(fin[:, None], pos, F(0)))
    obs &= fin
    _, w = sample_weight(index, pos)
    return obs, np.where(obs, s, F(np.nan)).astype(np.float32), w


# ---- ray sets --------------------------------------------------------------------------------------------------------------------
def pack(origins, directions, t_near, t_far):
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    rays = np.empty((len(d), 8), np.float32)
    rays[:, 0:3] = np.asarray(origins, np.float32)
    rays[:, 3:6] = d
    rays[:, 6] = np.asarray(t_near, np.float32)
    rays[:, 7] = np.asarray(t_far, np.float32)
    return rays


def view_rays(pose, intr, W, H, near, far):
    """the rays chisel_hip_render_view marches for this view, row-major: t is z-depth"""
    o, d = rr.rays(pose, intr, W, H)
    return pack(o, d, near, far)


def unit_rays(pose, intr, W, H, t_near=0.0, t_far=6.0):
    """the same directions normalised (float32): t is Euclidean range"""
    o, d = rr.rays(pose, intr, W, H)
    d = (d / np.sqrt((d * d).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
    return pack(o, d, t_near, t_far)


def hit_points_of(rays, t):
    """o + t d per ray, float32: where chisel_hip_cast_rays shades a hit"""
    rays = np.asarray(rays, np.float32)
    return (rays[:, 0:3] + np.asarray(t, np.float32).reshape(-1, 1) * rays[:, 3:6]).astype(np.float32)


def interleave(*sets):
    """ray i of the result is ray i // m of set i % m: neighbouring lanes march rays of different kinds"""
    n = min(len(s) for s in sets)
    return np.stack([s[:n] for s in sets], axis=1).reshape(-1, 8)


def plane_chunk(N, res, z0, sign):
    """one chunk (0, 0, 0) with sdf = sign * (z0 - z_centre), every voxel observed (tests/test_render_restated.py's)"""
    zc = (np.arange(N, dtype=np.float64) + 0.5) * res
    sdf = np.broadcast_to((sign * (z0 - zc))[:, None, None], (N, N, N)).astype(np.float32).reshape(-1)  # voxel id = (z N + y) N + x
    return {(0, 0, 0): (sdf, np.ones(N ** 3, np.float32), None)}


# ---- point sets ------------------------------------------------------------------------------------------------------------------
N_POINTS = 20000


def jitter_points(hit_points, res, rng, n=N_POINTS):
    """n of the view's hit points (drawn with replacement among the finite ones), each moved by N(0, 2 voxels) per axis"""
    p = hit_points[np.isfinite(hit_points).all(1)]
    pick = rng.integers(0, len(p), n)
    return (p[pick] + rng.normal(0.0, 2.0 * res, (n, 3))).astype(np.float32)


def box_points(chunk_ids, N, res, rng, n=N_POINTS):
    """uniform in the box of the resident chunk ids grown by one chunk on every side"""
    ids = np.asarray(chunk_ids, np.int64).reshape(-1, 3)
    edge = N * res
    lo, hi = (ids.min(0) - 1) * edge, (ids.max(0) + 2) * edge
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32)


def hand_points(anchor, N, res):
    """64 positions around `anchor` (an observed position): on every axis exact multiples of res and of N res next to it, and the
    floats one ulp below and above them; the same around the origin with both signs; the anchor snapped to the voxel grid in all
    eight octants; the origin; a NaN, a +Inf and a -Inf component; a position 100 m away"""
    res = F(res)
    a = np.asarray(anchor, np.float32)
    j = np.round(a / res).astype(np.int64)
    c = np.floor(a / (F(N) * res)).astype(np.int64)
    pts = []

    def three(axis, v, base):
        for x in (v, np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf))):
            p = base.copy()
            p[axis] = x
            pts.append(p)

    for axis in range(3):
        for v in (F(j[axis]) * res, F(j[axis] + 1) * res, F(N * c[axis]) * res, F(N * (c[axis] + 1)) * res):
            three(axis, v, a)                                               # 36
    for v in (F(0), res, -res, F(N) * res, -(F(N) * res)):
        three(0, v, a)                                                      # 15
    snapped = j.astype(np.float32) * res
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                pts.append(snapped * np.array([sx, sy, sz], np.float32))    # 8
    pts.append(np.zeros(3, np.float32))
    for bad in (np.nan, np.inf, -np.inf):
        p = a.copy()
        p[1] = bad
        pts.append(p)
    pts.append(a + F(100.0))
    out = np.stack(pts).astype(np.float32)
    assert out.shape == (64, 3)
    return out
