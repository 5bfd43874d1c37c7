"""chisel_hip_merge_map restated in numpy (TEST INFRASTRUCTURE: DESIGN.md 3.9 "Merging maps" is the definition), and the cases the CPU
and the GPU tests share.

Everything is float32, one rounding per operation, in the order the definition writes it (numpy neither contracts a * b + c nor
reorders).  The source voxel of a position is found with render_restated.VoxelIndex's own chunk-id and row look-up (its `sample` is
ChunkManager::GetSDF; here the weight and the colour are wanted beside the distance, so the linear id is formed as `sample` forms it).
There is no candidate logic: EVERY chunk id of the transformed source's bounding box plus a margin of one chunk is visited, and every
chunk the destination holds.

A field is a dict chunk id (x, y, z) -> (sdf[V], weight[V], rgbw[V, 4]), as voxel_fields builds it and Chisel.AddChunk /
OracleMap.put_chunk take it.
"""
import functools
import itertools

import numpy as np

from tests import render_restated as rr
from tests import voxel_fields as vf

F = np.float32
DEFAULT_SDF = F(99999.0)
RES = {8: 0.03, 16: 0.07, 32: 0.05}  # one non-dyadic resolution per chunk size (tests/test_gpu_mesh_fields.py)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def inverse_rigid(src_to_dst):
    """rule 1: M = (R^T, -R^T t) in double, products and sums left to right, each entry rounded to float32 -> (3, 4) float32"""
    a = np.asarray(src_to_dst, np.float32)[:3, :4].astype(np.float64)
    M = np.empty((3, 4), np.float32)
    for i in range(3):
        for j in range(3):
            M[i, j] = F(a[j, i])
        M[i, 3] = F(-((a[0, i] * a[0, 3] + a[1, i] * a[1, 3]) + a[2, i] * a[2, 3]))
    return M


def centres(cid, N, res):
    """rule 2: c = ((float)i res + half_res) + (float)(N id) res for the voxels of chunk `cid` in voxel-id order -> (V, 3) float32"""
    res = F(res)
    half = res * F(0.5)  # ChunkManager.cpp:52
    i = np.arange(N, dtype=np.float32)
    ax = [(i * res + half) + (F(N * int(cid[a])) * res) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float32)


def source_positions(M, c):
    """rule 2: p = ((m0 c.x + m1 c.y) + m2 c.z) + m3 per row of M -> (n, 3) float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((M[r, 0] * c[:, 0] + M[r, 1] * c[:, 1]) + M[r, 2] * c[:, 2]) + M[r, 3] for r in range(3)], axis=1).astype(np.float32)


class Source:
    """the source map: VoxelIndex for the look-up, and the colours stacked in the same row order"""

    def __init__(self, field, N, res):
        self.index = rr.VoxelIndex(field, N, res)
        self.N = N
        ids = sorted(field)
        self.rgbw = np.zeros((max(1, len(ids)), N ** 3, 4), np.uint8)
        for r, cid in enumerate(ids):
            if field[cid][2] is not None:
                self.rgbw[r] = np.asarray(field[cid][2], np.uint8).reshape(-1, 4)

    def pick(self, p):
        """rule 3: the voxel ChunkManager::GetSDF reads at p -> (observed, sdf, weight, rgbw, located) per position; located: the chunk is
        resident and the linear voxel id in range (weight, sdf and rgbw mean something)"""
        ix, N = self.index, self.N
        finite = np.isfinite(p).all(1)
        q = np.where(finite[:, None], p, F(0))
        ids = ix.chunk_ids(q)
        row = ix.rows(ids)
        origin = (N * ids).astype(np.float32) * ix.res
        c = np.floor((q - origin) * ix.rf_voxel).astype(np.int32).astype(np.int64)
        vid = (c[:, 2] * N + c[:, 1]) * N + c[:, 0]
        ok = finite & (row >= 0) & (vid >= 0) & (vid < N ** 3)
        r, v = np.where(ok, row, 0), np.where(ok, vid, 0)
        w, s = ix.wgt[r, v], ix.sdf[r, v]
        with np.errstate(invalid="ignore"):
            obs = ok & (w.astype(np.float64) > 1e-12)
        return obs, s, w, self.rgbw[r, v], ok


def dist_integrate(sdf, w, d, wu):
    """DistVoxel::Integrate (DistVoxel.h:52-60) on float32 arrays"""
    with np.errstate(all="ignore"):
        new = (w * sdf + wu * d) / (wu + w)
        return new.astype(np.float32), (w + wu).astype(np.float32)


def color_integrate(rgbw, src):
    """ColorVoxel::Integrate (ColorVoxel.h:65-85) on (n, 4) uint8 arrays, src = (r, g, b, weightUpdate) -> (new rgbw, early return taken)"""
    w, wu = rgbw[:, 3].astype(np.int32), src[:, 3].astype(np.int32)
    early = w >= 255 - wu
    out = rgbw.copy()
    den = (wu + w).astype(np.float32)
    for ch in range(3):
        old = rgbw[:, ch].astype(np.float32)
        with np.errstate(all="ignore"):
            val = (w.astype(np.float32) * old + (wu * src[:, ch].astype(np.int32)).astype(np.float32)) / den
        val = np.minimum(np.maximum(np.nan_to_num(val, nan=0.0), F(0)), F(255))  # Saturate
        out[:, ch] = np.where(early, rgbw[:, ch], val.astype(np.uint8))
    out[:, 3] = np.where(early, rgbw[:, 3], (w + wu).astype(np.uint8))
    return out, early


def brute_force_ids(src_field, dst_field, pose, N, res):
    """every chunk id of the transformed source's bounding box plus a margin of one chunk, and every id of the destination"""
    ids = set(dst_field)
    if src_field:
        a = np.array(sorted(src_field), np.int64)
        edge = float(F(N) * F(res))
        lo, hi = a.min(0) * edge, (a.max(0) + 1) * edge
        T = np.asarray(pose, np.float32)[:3, :4].astype(np.float64)
        corners = np.array([[(lo, hi)[k][ax] for ax, k in enumerate(sel)] for sel in itertools.product((0, 1), repeat=3)])
        moved = corners @ T[:, :3].T + T[:, 3]
        i0 = np.floor(moved.min(0) / edge).astype(np.int64) - 1
        i1 = np.floor(moved.max(0) / edge).astype(np.int64) + 1
        ids |= set(itertools.product(*(range(int(i0[k]), int(i1[k]) + 1) for k in range(3))))
    return sorted(ids)


def merge(dst_field, src_field, pose, N, res, dst_color=True, src_color=True):
    """-> (merged field, stats, detail).  stats: the four counts of chisel_hip_merge_stats and "col", the ColorVoxel::Integrate
    executions.  detail: what the reach predicates and the oracle comparison need, per visited chunk id."""
    V = N ** 3
    M = inverse_rigid(pose)
    src = Source(src_field, N, res)
    color = dst_color and src_color
    out, detail = {}, {}
    stats = {"src_chunks": len(src_field), "dst_chunks_created": 0, "dst_chunks_updated": 0, "voxels_updated": 0, "col": 0}
    for cid in brute_force_ids(src_field, dst_field, pose, N, res):
        p = source_positions(M, centres(cid, N, res))
        obs, s, w, c, located = src.pick(p)
        held = cid in dst_field
        n = int(obs.sum())
        detail[cid] = {"p": p, "observed": obs, "sdf": s, "weight": w, "located": located, "held": held, "updates": n}
        if not held and n == 0:
            continue
        if held:
            ds, dw, dc = (np.array(a) for a in dst_field[cid])
            ds, dw = ds.astype(np.float32), dw.astype(np.float32)
            dc = np.asarray(dc, np.uint8).reshape(-1, 4)
        else:
            ds, dw, dc = np.full(V, DEFAULT_SDF), np.zeros(V, np.float32), np.zeros((V, 4), np.uint8)
        if n:
            ns, nw = dist_integrate(ds[obs], dw[obs], s[obs], w[obs])
            ds[obs], dw[obs] = ns, nw
            stats["dst_chunks_updated"] += 1
            stats["voxels_updated"] += n
            stats["dst_chunks_created"] += 0 if held else 1
            if color:
                paint = obs & (c[:, 3] > 0)
                new, early = color_integrate(dc[paint], c[paint])
                dc[paint] = new
                stats["col"] += int(paint.sum())
                detail[cid].update(color_early=int(early.sum()), color_applied=int((~early).sum()), color_weight_zero=int((obs & (c[:, 3] == 0)).sum()))
        out[cid] = (ds, dw, dc)
    return out, stats, detail


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _pose(R, t):
    p = np.zeros((3, 4), np.float32)
    p[:, :3] = np.asarray(R, np.float64).astype(np.float32)
    p[:, 3] = np.asarray(t, np.float64).astype(np.float32)
    return p


def poses(res):
    """name -> src_to_dst (3, 4) float32, for a map of voxel size `res`"""
    rpy = _rot(2, 25.0) @ _rot(1, -17.0) @ _rot(0, 33.0)  # yaw, pitch, roll
    r = float(F(res))
    return {
        "identity": _pose(np.eye(3), (0, 0, 0)),
        "shift_voxels": _pose(np.eye(3), (3 * r, -5 * r, 9 * r)),
        "shift_half": _pose(np.eye(3), (0.5 * r, 0.5 * r, 0.5 * r)),  # positions sit on voxel faces
        "z90": _pose(np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64), (0, 0, 0)),  # entries exactly 0 and +-1
        "x45": _pose(_rot(0, 45.0), (0, 0, 0)),
        "rpy_neg": _pose(rpy, (-1.3, -0.7, -2.1)),
        "rpy_far": _pose(rpy, (-1.3 + 30.0, -0.7, -2.1)),  # the destination 30 m from the origin
    }


ROTATED = ("z90", "x45", "rpy_neg", "rpy_far")
SRC_BASE = {2: (-1, -1, -1), 1: (-1, 2, 0)}  # block edge -> base: the 2^3 block straddles the origin; the single chunk sits where the general
                                             # pose leaves candidate ids untouched (asserted in tests/test_merge_restated.py)


def case_names():
    """(N, pose name, destination kind): every pose at N = 8 (B = 2), identity and the general pose at 16 and 32 (B = 1), each into a dense
    block that overlaps half of the moved source and into an empty map"""
    out = []
    for N, names in ((8, tuple(poses(RES[8]))), (16, ("identity", "rpy_neg")), (32, ("identity", "rpy_neg"))):
        out += [(N, name, kind) for name in names for kind in ("dense", "empty")]
    return out


@functools.lru_cache(maxsize=None)
def case(N, name, kind):
    """-> (src field, dst field, pose, res).  The source: a voxel_fields.thresholds block; the destination: a voxel_fields.dense block based
    at the chunk that holds the moved source's centre, one chunk down in y and z -- about half of the moved source -- or nothing."""
    res = RES[N]
    B = 2 if N == 8 else 1
    base = SRC_BASE[B]
    src = vf.thresholds(N, B, 11, res=res, base=base)
    pose = poses(res)[name]
    dst = {}
    if kind == "dense":
        edge = float(F(N) * F(res))
        centre = (np.array(base, np.float64) + B / 2.0) * edge
        moved = pose[:, :3].astype(np.float64) @ centre + pose[:, 3].astype(np.float64)
        at = np.floor(moved / edge).astype(np.int64)
        dst = vf.dense(N, B, 12, res=res, base=(int(at[0]), int(at[1]) - (B - 1), int(at[2]) - (B - 1)))
    return src, dst, pose, res


@functools.lru_cache(maxsize=None)
def merged(N, name, kind, dst_color=True, src_color=True):
    """the restated result of a case, computed once and only read afterwards"""
    src, dst, pose, res = case(N, name, kind)
    return merge(dst, src, pose, N, res, dst_color, src_color)


def padded_candidate_ids(src_field, pose, N, res):
    """for the reach predicate of the rotated cases only: per source chunk the ids its moved cube's bounding box, padded by one voxel,
    meets (double arithmetic on the pose as given)"""
    edge = float(F(N) * F(res))
    T = np.asarray(pose, np.float32)[:3, :4].astype(np.float64)
    ids = set()
    for cid in src_field:
        corners = (np.array(cid, np.float64) + np.array(list(itertools.product((0, 1), repeat=3)), np.float64)) * edge
        moved = corners @ T[:, :3].T + T[:, 3]
        i0 = np.floor((moved.min(0) - float(F(res))) / edge).astype(np.int64)
        i1 = np.floor((moved.max(0) + float(F(res))) / edge).astype(np.int64)
        ids |= set(itertools.product(*(range(int(i0[k]), int(i1[k]) + 1) for k in range(3))))
    return ids


def reach(N, name, kind, dst_color=True, src_color=True):
    """what a case reaches, from the restatement alone"""
    src, dst, pose, res = case(N, name, kind)
    out, stats, detail = merged(N, name, kind, dst_color, src_color)
    used_w = np.concatenate([d["weight"][d["observed"]] for d in detail.values()] + [np.zeros(0, np.float32)])
    looked_w = np.concatenate([d["weight"][d["located"]] for d in detail.values()] + [np.zeros(0, np.float32)])
    r = {
        "created": stats["dst_chunks_created"],
        "candidates_not_created": len([c for c in padded_candidate_ids(src, pose, N, res) if c not in out]),
        "updated_in_existing": sum(d["updates"] for d in detail.values() if d["held"]),
        "weight_edge_below": int((looked_w == vf.W_EDGE).sum()),       # read as unobserved
        "weight_edge_above": int((used_w == vf.W_EDGE_NEXT).sum()),    # read as observed
        "color_early": sum(d.get("color_early", 0) for d in detail.values()),
        "color_applied": sum(d.get("color_applied", 0) for d in detail.values()),
        "color_weight_zero": sum(d.get("color_weight_zero", 0) for d in detail.values()),
    }
    return r


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_fields_bit_equal(want, got, use_color, what=""):
    """chunk-id sets equal; sdf and weight equal as uint32, colours as bytes"""
    assert sorted(want) == sorted(got), "%s: chunk ids differ: %s" % (what, sorted(set(want) ^ set(got))[:8])
    for cid in sorted(want):
        ws, ww, wc = want[cid]
        gs, gw, gc = got[cid]
        for key, x, y in (("sdf", ws, gs), ("weight", ww, gw)):
            x, y = np.asarray(x, np.float32).reshape(-1), np.asarray(y, np.float32).reshape(-1)
            bad = np.flatnonzero(x.view(np.uint32) != y.view(np.uint32))
            assert not len(bad), "%s chunk %s: %s differs at %d voxels, first %d: %r vs %r" % (what, cid, key, len(bad), bad[0], x[bad[0]], y[bad[0]])
        if use_color:
            x, y = np.asarray(wc, np.uint8).reshape(-1, 4), np.asarray(gc, np.uint8).reshape(-1, 4)
            bad = np.flatnonzero((x != y).any(1))
            assert not len(bad), "%s chunk %s: colour differs at %d voxels, first %d: %r vs %r" % (what, cid, len(bad), bad[0], x[bad[0]], y[bad[0]])
