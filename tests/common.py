"""Shared helpers of the parity tests: run the same frames through the oracle and the HIP path."""
import numpy as np

from cvids_amd import synth

DEFAULT_SDF = np.float32(99999.0)


def small_camera(W=64, H=48, near=0.05, far=5.0):
    from cvids_amd.chisel import PinholeCamera
    fx, fy, cx, cy = synth.intrinsics(W, H)
    return PinholeCamera(fx, fy, cx, cy, W, H, near, far)


def make_frames(scene, n, W, H, agents=1, nan_fraction=0.0, noise=False, start=0):
    return list(synth.stream(scene, n, W, H, agents=agents, nan_fraction=nan_fraction, noise=noise, start=start))


def compare_fields(ref, got, V, use_color, atol=0.0, what=""):
    """ref/got: dict id -> (sdf, w, rgbw).  Absent chunk == all (99999, 0, 0).  Returns max |dsdf|, |dw|."""
    ids = set(ref) | set(got)
    max_ds = 0.0
    max_dw = 0.0
    for cid in sorted(ids):
        rs, rw, rc = ref.get(cid, (None, None, None))
        gs, gw, gc = got.get(cid, (None, None, None))
        if rs is None:
            rs, rw = np.full(V, DEFAULT_SDF), np.zeros(V, np.float32)
            rc = np.zeros((V, 4), np.uint8)
        if gs is None:
            gs, gw = np.full(V, DEFAULT_SDF), np.zeros(V, np.float32)
            gc = np.zeros((V, 4), np.uint8)
        # NaN-aware comparison, for voxels that did not come from depth images (AddChunk / put_chunk take whatever the caller holds).
        # ProjectionIntegrator.h:51-99 itself cannot store a NaN: a NaN depth fails `depth > 50`, both band tests and the carving test
        # (:74-88), depth 0 with the inverse truncator gives truncation 1 / (inf * inf) = 0, not NaN (InverseTruncator.h:42-46), and
        # DistVoxel::Integrate only averages finite updates from weight 0 on.  An infinite distance is possible (a huge negative depth
        # under an infinite truncation sums to -inf).
        same_nan_s = np.isnan(rs) == np.isnan(gs)
        same_nan_w = np.isnan(rw) == np.isnan(gw)
        assert same_nan_s.all() and same_nan_w.all(), "%s chunk %s: NaN pattern differs" % (what, cid)
        fin = np.isfinite(rs) & np.isfinite(gs)
        assert (np.isfinite(rs) == np.isfinite(gs)).all(), "%s chunk %s: inf pattern differs" % (what, cid)
        ds = float(np.abs(rs[fin] - gs[fin]).max()) if fin.any() else 0.0
        finw = np.isfinite(rw) & np.isfinite(gw)
        dw = float(np.abs(rw[finw] - gw[finw]).max()) if finw.any() else 0.0
        max_ds, max_dw = max(max_ds, ds), max(max_dw, dw)
        if atol == 0.0:
            assert np.array_equal(rs[fin], gs[fin]), "%s chunk %s: sdf differs (max %g)" % (what, cid, ds)
            assert np.array_equal(rw[finw], gw[finw]), "%s chunk %s: weight differs (max %g)" % (what, cid, dw)
        else:
            assert ds <= atol and dw <= atol, "%s chunk %s: |dsdf| %g |dw| %g > %g" % (what, cid, ds, dw, atol)
        if use_color:
            assert np.array_equal(rc, gc), "%s chunk %s: colour voxels differ" % (what, cid)
    return max_ds, max_dw


def triangle_multiset(vertices, decimals=5):
    """mesh -> its triangles as a multiset, in a form that compares equal exactly when the multisets do: every triangle's 3 vertices
    (rounded) rotated to a canonical start -- the lexicographically smallest vertex, the first of them where two are equal --, the
    triangles sorted (by their bytes: any total order serves) and packed into one bytes object."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3, 3).round(decimals) + 0.0
    rows = np.arange(len(v))
    k = np.zeros(len(v), np.int64)
    for j in (1, 2):
        a, b = v[:, j], v[rows, k]
        less = (a[:, 0] < b[:, 0]) | ((a[:, 0] == b[:, 0]) & ((a[:, 1] < b[:, 1]) | ((a[:, 1] == b[:, 1]) & (a[:, 2] < b[:, 2]))))
        k = np.where(less, j, k)
    tri = np.ascontiguousarray(v[rows[:, None], (k[:, None] + np.arange(3)) % 3].reshape(-1, 9))
    return np.sort(tri.view(np.dtype((np.void, 72))).ravel()).tobytes()


def compare_meshes(om, gm, color):
    """the oracle's meshes against the map's: the same chunk ids, every array bit for bit -> (chunks, vertices)"""
    oids = sorted(map(tuple, om.mesh_ids().tolist()))
    gids = sorted(map(tuple, gm.GetMeshIDs().tolist()))
    assert oids == gids, "mesh id sets differ: %d vs %d" % (len(oids), len(gids))
    nv = 0
    for cid in oids:
        a, b = om.get_mesh(cid), gm.GetMesh(cid)
        for key in ("vertices", "normals", "grids") + (("colors",) if color else ()):
            x, y = np.asarray(a[key]), np.asarray(b[key])
            assert x.shape == y.shape, "chunk %s %s: %s vs %s" % (cid, key, x.shape, y.shape)
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "chunk %s: %s differ (max %g)" % (
                cid, key, np.abs(x - y).max() if x.size else 0)
        assert triangle_multiset(a["vertices"]) == triangle_multiset(b["vertices"])
        nv += len(a["vertices"])
    return len(oids), nv


def same_bits(got, want, what):
    """NaN masks equal, uint32 views equal elsewhere, no pixel left out"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN masks differ at %d places" % (what, int((gn != wn).sum()))
    g, w = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    assert np.array_equal(g, w), "%s: %d of %d values differ in their bits (max |d| %g)" % (
        what, int((g != w).sum()), g.size, float(np.abs(got[~gn].astype(np.float64) - want[~wn].astype(np.float64)).max()))


def upload(gm, field):
    """a field (dict id -> (sdf, w, rgbw)) into a map, chunk by chunk; the colours only where the map keeps any"""
    for cid, (s, w, c) in field.items():
        gm.AddChunk(cid, s, w, c if gm.use_color else None)


def fields_of(gm, N):
    """Chisel.fields() with a zero colour array where the map has none, so that both kinds compare alike"""
    return {cid: (s, w, c if c is not None else np.zeros((N ** 3, 4), np.uint8)) for cid, (s, w, c) in gm.fields().items()}


def free_bytes():
    import torch
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]
