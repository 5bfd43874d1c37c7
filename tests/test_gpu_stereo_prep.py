"""GPU tests of the stereo matcher's raw-image path (chisel_hip_stereo_set_camera / set_reference_image / update_image /
bind_sparse_points / output_image; StereoMapper.InitIntrinsic ... OutputImage; DepthEstimator): every prepared input and the
camera-size depth bit-exact against tests/stereo_prep_restated.py chained into the float-input restatement, the raw path against
the float path fed with the restated images, recovery of a distorted textured plane through DepthEstimator into the TSDF,
determinism and argument checks."""
import ctypes as C

import numpy as np
import pytest

import stereo_prep_restated as pr
import stereo_restated as sr

pytestmark = pytest.mark.gpu
f32 = np.float32

# EuRoC cam0 (752 x 480): the camera the reference's configuration is written for
EUROC_K = (458.654, 457.296, 367.215, 248.375)
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)


def camera(real_w, real_h):
    s = real_w / 752.0
    return (EUROC_K[0] * s, EUROC_K[1] * s, EUROC_K[2] * s, EUROC_K[3] * real_h / 480.0), EUROC_D


def random_image(rng, w, h):
    """smooth random texture, uint8"""
    g = rng.uniform(0, 255, (h // 4 + 2, w // 4 + 2))
    ys, xs = np.linspace(0, g.shape[0] - 1.001, h), np.linspace(0, g.shape[1] - 1.001, w)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    img = (g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0 + 1][:, x0] * fy * (1 - fx) + g[y0][:, x0 + 1] * (1 - fy) * fx +
           g[y0 + 1][:, x0 + 1] * fy * fx)
    return np.clip(img + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)


def random_pose(rng, scale=1.0):
    a = rng.normal(0, 0.03 * scale, 3)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + Kx + Kx @ Kx / 2
    q, r = np.linalg.qr(R)
    R = q * np.sign(np.diag(r))
    return R, rng.normal(0, 0.05 * scale, 3) + np.array([0.1, 0.0, 0.0])


def random_points(rng, n, real_w, real_h):
    d = rng.uniform(0.8, 6.0, n)
    xy = np.stack([rng.uniform(-3, real_w + 3, n), rng.uniform(-3, real_h + 3, n)], axis=1)
    xy[: n // 4, 0] = rng.uniform(real_w - 12, real_w + 2, n // 4)   # near the right edge: reads wrap into the next row
    return d, xy


class GpuRaw:
    """RawStereo's interface over cvids_amd.chisel.StereoMapper"""

    def __init__(self, W, H):
        from cvids_amd.chisel import StereoMapper
        self.m = StereoMapper(W, H)

    def set_camera(self, real_w, real_h, K1, D1, K2, D2):
        self.m.InitIntrinsic(K1, D1, K2, D2, (real_w, real_h))

    def set_reference_image(self, raw):
        self.m.InitReferenceImage(raw)

    def update_image(self, raw, ref_pose, match_pose):
        self.m.UpdateImage(raw, ref_pose, match_pose)

    def bind_sparse_points(self, d, xy):
        self.m.BindSparsePoints(d, xy)

    def output_image(self):
        return self.m.OutputImage()

    def clear(self):
        self.m.ClearRawCost()

    P = lambda which: property(lambda self: self.m.debug_prep(which))
    ref, match, p2w = P(0), P(1), P(2)
    mask_x, mask_y, sparse_depth, sparse_dist = P(3), P(4), P(5), P(6)
    depth = property(lambda self: self.m.read(self.m.DEPTH))
    depth_real = property(lambda self: self.m.read(self.m.DEPTH_REAL))


def run_raw_sequence(obj, W, H, real_w, real_h, seed, n_points):
    """set_camera, reference, then match frames with and without points, with and without ClearRawCost; -> [(name, array)]"""
    rng = np.random.default_rng(seed)
    K, D = camera(real_w, real_h)
    obj.set_camera(real_w, real_h, K, D, K, D)
    out = []
    ref_pose = random_pose(rng)
    obj.set_reference_image(random_image(rng, real_w, real_h))
    out += [("ref", obj.ref), ("p2w", obj.p2w), ("mask_x", obj.mask_x), ("mask_y", obj.mask_y)]
    for step, (pts, clear) in enumerate([(True, False), (False, False), (True, True)]):
        obj.update_image(random_image(rng, real_w, real_h), ref_pose, random_pose(rng))
        out.append(("match", obj.match))
        obj.bind_sparse_points(*(random_points(rng, n_points, real_w, real_h) if pts else (np.zeros(0), np.zeros((0, 2)))))
        obj.output_image()
        out += [("sparse_depth", obj.sparse_depth), ("sparse_dist", obj.sparse_dist), ("depth", obj.depth),
                ("depth_real", obj.depth_real)]
        out = [(k, np.array(v, copy=True)) for k, v in out]   # (the restatement's arrays are its live state)
        if clear:
            obj.clear()
    return out


SIZES = [(160, 120, 200, 150), (640, 480, 752, 480)]


@pytest.mark.parametrize("W,H,real_w,real_h", SIZES)
def test_raw_path_matches_the_restatement_bit_for_bit(hip_lib, W, H, real_w, real_h):
    n = 500 if W == 640 else 120
    want = run_raw_sequence(pr.RawStereo(sr.VectorisedStereo(W, H), W, H), W, H, real_w, real_h, 3, n)
    got = run_raw_sequence(GpuRaw(W, H), W, H, real_w, real_h, 3, n)
    assert [k for k, _ in got] == [k for k, _ in want]
    for i, ((name, g), (_, w)) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if not sr.same_bits(g, w):
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            idx = tuple(np.argwhere(bad)[0])
            pytest.fail("state %d (%s): %d entries differ, first at %s: gpu %r cpu %r" % (i, name, bad.sum(), idx, g[idx], w[idx]))
    named = dict(want)
    assert named["mask_x"].mean() > 0.02 and named["mask_y"].mean() > 0.02
    assert (dict(want)["sparse_depth"] > 0).sum() > 100 if W == 640 else True
    assert all((d != 1000).mean() > 0.2 for k, d in want if k == "depth")


def test_raw_depth_equals_the_float_path_fed_the_restated_images(hip_lib):
    """the raw entries vs set_reference / update / output given the restatement's prepared images, P2 map and sparse maps"""
    from cvids_amd.chisel import StereoMapper
    W, H, real_w, real_h = 640, 480, 752, 480
    rng = np.random.default_rng(8)
    K, D = camera(real_w, real_h)
    ref_img, match_img = random_image(rng, real_w, real_h), random_image(rng, real_w, real_h)
    ref_pose, match_pose = random_pose(rng), random_pose(rng)
    d, xy = random_points(rng, 400, real_w, real_h)
    raw = StereoMapper(W, H)
    raw.InitIntrinsic(K, D, K, D, (real_w, real_h))
    raw.InitReferenceImage(ref_img)
    raw.UpdateImage(match_img, ref_pose, match_pose)
    raw.BindSparsePoints(d, xy)
    real = raw.OutputImage()

    Ks = pr.scale_intrinsics(K, real_w, real_h, W, H)
    ref = pr.prepare(ref_img, W, H, Ks, D)
    p2w, mx, my = pr.reference_maps(ref)
    match = pr.prepare(match_img, W, H, Ks, D)
    R, t = pr.homography(Ks, Ks, ref_pose[0], ref_pose[1], match_pose[0], match_pose[1])
    sd, sdist = pr.sparse_maps_vectorised(d, xy, mx, my, W, H, real_w, real_h)
    flt = StereoMapper(W, H)
    flt.InitReference(ref, p2w)
    flt.Update(match, R, t)
    want = flt.Output(sd, sdist)
    assert raw.read(raw.DEPTH).tobytes() == want.tobytes()
    assert real.tobytes() == pr.resize_f32(want, real_w, real_h).tobytes()
    assert np.array_equal(raw.read(raw.DEPTH_REAL64), real.astype(np.float64))


def render_plane(real_w, real_h, K, D, pose_wc, plane_z):
    """mono8 image of the textured plane z = plane_z (world) seen by a camera with distortion D at pose (R_wc, t_wc): for every
    distorted pixel the undistorted ray (fixed-point inversion of the k1 k2 p1 p2 model), its hit on the plane, the texture there"""
    fx, fy, cx, cy = K
    k1, k2, p1, p2 = D[:4]
    u, v = np.meshgrid(np.arange(real_w, dtype=np.float64), np.arange(real_h, dtype=np.float64))
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(20):
        r2 = x * x + y * y
        kr = 1 + k1 * r2 + k2 * r2 * r2
        dx, dy = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) / kr, (yd - dy) / kr
    R, t = pose_wc
    rays = np.stack([x, y, np.ones_like(x)], axis=-1) @ np.asarray(R).T
    s = (plane_z - t[2]) / rays[..., 2]
    X, Y = t[0] + s * rays[..., 0], t[1] + s * rays[..., 1]
    tex = (128 + 45 * np.sin(23.0 * X + 3.1 * Y) + 35 * np.sin(41.0 * Y - 7.0 * X + 1.0) + 25 * np.sin(67.0 * X + 59.0 * Y + 2.0) +
           15 * np.sin(97.0 * X - 89.0 * Y))
    return np.clip(np.rint(tex), 0, 255).astype(np.uint8)


def test_depth_estimator_recovers_a_distorted_plane_and_integrates_it(hip_lib):
    """DepthEstimator on EuRoC-size frames (752 x 480, EuRoC distortion) of a textured plane 2 m away: three match frames fused,
    every step in HBM; the filter's depth within 3 % on at least 80 % of the interior, and the depth map integrated into a TSDF"""
    import torch
    from cvids_amd import chisel as ch
    real_w, real_h, Z = 752, 480, 2.0
    K, D = EUROC_K, EUROC_D
    I = np.eye(3)
    ref_pose = (I, np.zeros(3))
    ref = torch.from_numpy(render_plane(real_w, real_h, K, D, ref_pose, Z)).cuda()
    est = ch.DepthEstimator(ref, ref_pose, *K, *D[:4])
    for tx, ty in [(0.10, 0.0), (0.12, 0.02), (0.09, -0.015)]:
        pose = (I, np.array([tx, ty, 0.0]))
        est.FuseNewFrame(torch.from_numpy(render_plane(real_w, real_h, K, D, pose, Z)).cuda(), pose)
    depth = torch.empty((real_h, real_w), dtype=torch.float64, device="cuda")
    est.read(ch.DepthFilter.DEPTH, out=depth)
    dh = depth.cpu().numpy()
    interior = dh[60:real_h - 60, 100:real_w - 100]
    ok = np.abs(interior / Z - 1.0) < 0.03
    assert ok.mean() >= 0.8, (ok.mean(), np.median(interior))

    d32 = torch.empty((real_h, real_w), dtype=torch.float32, device="cuda")
    intr = (C.c_double * 4)(*K)
    assert hip_lib.chisel_hip_condition_depth(depth.data_ptr(), real_w, real_h, 1, d32.data_ptr(), real_w, real_h, 1, intr, None) == 0
    cam = ch.PinholeCamera(*K, real_w, real_h, 0.05, 5.0)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    tsdf = ch.Chisel((16, 16, 16), 0.05, False)
    tsdf.IntegrateDepthScan(integ, d32, np.eye(4), cam)
    assert len(tsdf.fields()) > 10


def test_raw_path_is_deterministic(hip_lib):
    a = run_raw_sequence(GpuRaw(160, 120), 160, 120, 200, 150, 21, 150)
    b = run_raw_sequence(GpuRaw(160, 120), 160, 120, 200, 150, 21, 150)
    for (_, x), (_, y) in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_raw_path_rejects_bad_state_and_arguments(hip_lib):
    import torch
    from cvids_amd.chisel import StereoMapper
    W, H, rw, rh = 64, 48, 80, 60
    m = StereoMapper(W, H)
    img = np.zeros((rh, rw), np.uint8)
    I9, Z3 = (C.c_double * 9)(*np.eye(3).reshape(9)), (C.c_double * 3)()
    K4, D5 = (C.c_double * 4)(60.0, 60.0, 40.0, 30.0), (C.c_double * 5)()
    pts = np.zeros(2)
    out = np.empty((rh, rw), np.float32)
    # before set_camera: every raw entry and the camera-size read-outs refuse
    assert hip_lib.chisel_hip_stereo_set_reference_image(m.h, img.ctypes.data, rw, 0) == 1
    assert hip_lib.chisel_hip_stereo_update_image(m.h, img.ctypes.data, rw, I9, Z3, I9, Z3, 0) == 1
    assert hip_lib.chisel_hip_stereo_bind_sparse_points(m.h, pts.ctypes.data, pts.ctypes.data, 1) == 1
    assert hip_lib.chisel_hip_stereo_output_image(m.h) == 1
    assert hip_lib.chisel_hip_stereo_read(m.h, 4, out.ctypes.data, 0) == 1
    assert hip_lib.chisel_hip_debug_stereo_prep(m.h, 3, out.ctypes.data) == 1
    with pytest.raises(AssertionError):
        m.InitReferenceImage(img)
    # a work size too small for the 9-tap border
    small = StereoMapper(8, 8)
    assert hip_lib.chisel_hip_stereo_set_camera(small.h, rw, rh, K4, D5, K4, D5) == 1
    assert hip_lib.chisel_hip_stereo_set_camera(m.h, 1, rh, K4, D5, K4, D5) == 1
    assert hip_lib.chisel_hip_stereo_set_camera(m.h, rw, rh, None, D5, K4, D5) == 1
    m.InitIntrinsic((60.0, 60.0, 40.0, 30.0), (0.0,) * 4, (60.0, 60.0, 40.0, 30.0), (0.0,) * 4, (rw, rh))
    # match before reference, bad step, null image, n < 0
    assert hip_lib.chisel_hip_stereo_update_image(m.h, img.ctypes.data, rw, I9, Z3, I9, Z3, 0) == 1
    assert hip_lib.chisel_hip_stereo_set_reference_image(m.h, img.ctypes.data, rw - 1, 0) == 1
    assert hip_lib.chisel_hip_stereo_set_reference_image(m.h, None, rw, 0) == 1
    assert hip_lib.chisel_hip_stereo_bind_sparse_points(m.h, pts.ctypes.data, pts.ctypes.data, -1) == 1
    assert hip_lib.chisel_hip_stereo_bind_sparse_points(m.h, None, None, 3) == 1
    assert hip_lib.chisel_hip_stereo_read(m.h, 6, out.ctypes.data, 0) == 1
    # the binding: dtype and shape, numpy and torch
    with pytest.raises(AssertionError):
        m.InitReferenceImage(img.astype(np.float32))
    with pytest.raises(AssertionError):
        m.InitReferenceImage(np.zeros((rh, rw + 1), np.uint8))
    with pytest.raises(AssertionError):
        m.InitReferenceImage(torch.zeros((rh, rw), dtype=torch.float32, device="cuda"))
    with pytest.raises(AssertionError):
        m.BindSparsePoints([1.0, 2.0], [(1.0, 2.0)])
    assert (m.read(m.COST) == 0).all()          # nothing was launched
    # the right types go through, with a row step (a column slice of a wider device image)
    wide = torch.zeros((rh, rw + 16), dtype=torch.uint8, device="cuda")
    assert hip_lib.chisel_hip_stereo_set_reference_image(m.h, wide.data_ptr(), rw + 16, 1) == 0
    m.InitReferenceImage(torch.zeros((rh, rw), dtype=torch.uint8, device="cuda"))
    m.UpdateImage(img, (np.eye(3), np.zeros(3)), (np.eye(3), np.array([0.1, 0, 0])))
    m.BindSparsePoints([], np.zeros((0, 2)))
    assert m.OutputImage().shape == (rh, rw)
