"""GPU tests of the stereo matcher (chisel_hip_stereo_*, StereoMapper): bit-exact parity with the vectorised CPU restatement
(tests/stereo_restated.py) through a whole InitReference / Update / Output / ClearRawCost sequence, recovery of a known plane,
the device-resident chain into the depth filter and the TSDF, determinism and argument checks."""
import ctypes as C

import numpy as np
import pytest

import stereo_restated as sr
from test_stereo_restated import random_pose, run_sequence

pytestmark = pytest.mark.gpu
f32 = np.float32


class GpuStereo:
    """the restatement's interface over cvids_amd.chisel.StereoMapper, state read back after every step"""

    def __init__(self, W, H):
        from cvids_amd.chisel import StereoMapper
        self.m = StereoMapper(W, H)

    def set_reference(self, ref, p2w):
        self.m.InitReference(ref, p2w)

    def update(self, match, R, t):
        self.m.Update(match, R, t)

    def output(self, sparse_depth=None, sparse_dist=None):
        return self.m.Output(sparse_depth, sparse_dist)

    def clear(self):
        self.m.ClearRawCost()

    cost = property(lambda self: self.m.read(self.m.COST))
    sgm = property(lambda self: self.m.read(self.m.SGM))
    depth = property(lambda self: self.m.read(self.m.DEPTH))


@pytest.mark.parametrize("W,H", [(160, 120), (640, 480)])
def test_stereo_matches_the_restatement_bit_for_bit(hip_lib, W, H):
    want = run_sequence(sr.VectorisedStereo, W, H, 7)
    got = run_sequence(GpuStereo, W, H, 7)
    assert [n for n, _ in got] == [n for n, _ in want]
    for k, ((name, g), (_, w)) in enumerate(zip(got, want)):
        if not sr.same_bits(g, w):
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            idx = np.argwhere(bad)[0]
            pytest.fail("state %d (%s): %d entries differ, first at %s: gpu %r cpu %r" % (k, name, bad.sum(), tuple(idx), g[tuple(idx)],
                                                                                        w[tuple(idx)]))
    depths = [x for n, x in want if n == "depth"]
    assert all((d != 1000).mean() > 0.2 for d in depths)


def plane_pair(W, H, index):
    """a fronto-parallel plane whose inverse depth is `index` steps of DEP_SAMPLE, the match camera 0.11 m to the right, both
    rotations identity.  The texture varies with x only and is flat over the match image's first 8 columns: the quirky taps r and
    ru, which land near the match image's top-left corner, read a constant, and the mirrored u and d taps see equal rows.
    Disparity in pixels = 0.11 fx / Z = index (fx = 460.95, the reference's FOCAL): the ref image is the match image shifted
    right by `index`."""
    from cvids_amd.chisel import stereo_homography
    fx = 460.95
    K = np.array([[fx, 0, W / 2.0], [0, fx, H / 2.0], [0, 0, 1.0]])
    R, t = stereo_homography(K, K, np.eye(3), np.zeros(3), np.eye(3), np.array([0.11, 0.0, 0.0]))

    def tex(u):  # increasing past the flat part, so a 3 x 3 window has one match within the 128 hypotheses
        s = np.maximum(u - 8.0, 0.0)
        return 40.0 + 0.3 * s + 8.0 * np.sin(0.031 * s)

    u = np.arange(W, dtype=np.float64)
    disparity = index * float(sr.DEP_SAMPLE) * 0.11 * fx
    match = np.broadcast_to(tex(u), (H, W)).astype(np.float32)
    ref = np.broadcast_to(tex(u - disparity), (H, W)).astype(np.float32)
    return ref, match, R, t


def test_stereo_recovers_a_plane(hip_lib):
    from cvids_amd.chisel import StereoMapper
    W, H, index = 640, 480, 40.37
    ref, match, R, t = plane_pair(W, H, index)
    p2w = np.ones((H, W), np.float32)
    m = StereoMapper(W, H)
    m.InitReference(ref, p2w)
    m.Update(match, R, t)
    depth = m.Output()
    cpu = sr.VectorisedStereo(W, H)
    cpu.set_reference(ref, p2w)
    cpu.update(match, R, t)
    valid = ~(cpu.cost < 0).any(axis=2)
    truth = 1.0 / (index * float(sr.DEP_SAMPLE))
    assert 100 <= (~valid[H // 2]).sum() <= 140              # the left columns where some hypothesis leaves the match image
    assert (depth[~valid] == 1000).all()
    ok = np.abs(depth[valid] / truth - 1.0) < 0.02
    assert ok.mean() >= 0.9, ok.mean()


def test_stereo_device_chain_into_filter_and_tsdf(hip_lib):
    """stereo -> read(3) in HBM -> chisel_hip_depth_filter_update(reciprocal = 1, on_device = 1) -> filter read 6 -> condition_depth
    -> integrate, against the same chain through host copies: the voxels are identical"""
    import torch
    from cvids_amd import chisel as ch
    W, H = 320, 240
    intr = (460.95, 460.95, W / 2.0, H / 2.0)     # plane_pair's camera
    ref, match, R, t = plane_pair(W, H, 40.37)
    m = ch.StereoMapper(W, H)
    m.InitReference(torch.from_numpy(ref).cuda(), torch.from_numpy(np.ones((H, W), np.float32)).cuda())
    m.Update(torch.from_numpy(match).cuda(), R, t)
    m.Output()
    pose = np.eye(4)
    cam = ch.PinholeCamera(*intr, W, H, 0.05, 5.0)
    integ = ch.ProjectionIntegrator(ch.InverseTruncator(2.0), ch.ConstantWeighter(1.0), 0.05, True)
    K = (C.c_double * 4)(*intr)

    # on the device end to end
    d64 = torch.empty((H, W), dtype=torch.float64, device="cuda")
    m.read(m.DEPTH64, out=d64)
    fd = ch.DepthFilter(H, W)
    assert hip_lib.chisel_hip_depth_filter_update(fd.h, d64.data_ptr(), None, C.c_double((3 * float(sr.DEP_SAMPLE)) ** 2), 1, 1) == 0
    dmap = torch.empty((H, W), dtype=torch.float64, device="cuda")
    fd.read(fd.DEPTH, out=dmap)
    d32 = torch.empty((H, W), dtype=torch.float32, device="cuda")
    assert hip_lib.chisel_hip_condition_depth(dmap.data_ptr(), W, H, 1, d32.data_ptr(), W, H, 1, K, None) == 0
    gd = ch.Chisel((16, 16, 16), 0.02, False)
    gd.IntegrateDepthScan(integ, d32, pose, cam)

    # through the host
    h64 = m.read(m.DEPTH64)
    assert np.array_equal(h64, m.read(m.DEPTH).astype(np.float64))
    fh = ch.DepthFilter(H, W)
    fh.Update(h64, (3 * float(sr.DEP_SAMPLE)) ** 2, reciprocal=True)
    hmap = fh.read(fh.DEPTH)
    h32, _ = ch.condition_depth(hmap, W, H, intr)
    gh = ch.Chisel((16, 16, 16), 0.02, False)
    gh.IntegrateDepthScan(integ, h32, pose, cam)

    assert np.array_equal(dmap.cpu().numpy(), hmap)
    assert np.array_equal(d32.cpu().numpy(), h32, equal_nan=True)
    fa, fb = gd.fields(), gh.fields()
    assert set(fa) == set(fb) and len(fa) > 10
    for cid in fa:
        for x, y in zip(fa[cid], fb[cid]):            # sdf, weight, colour (None: a map without colour)
            assert (x is None and y is None) or x.tobytes() == y.tobytes()


def test_stereo_runs_are_deterministic(hip_lib):
    a = run_sequence(GpuStereo, 160, 120, 11)
    b = run_sequence(GpuStereo, 160, 120, 11)
    for (_, x), (_, y) in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_stereo_rejects_bad_arguments(hip_lib):
    """the library: null handles and pointers, a bad size or parameter at create, a bad read-out, an update before the
    reference -- CHISEL_HIP_ERR_INVALID, nothing launched.  (The ABI takes no image sizes: those the binding checks, below.)"""
    from cvids_amd import capi
    from cvids_amd.chisel import StereoMapper
    h = C.c_void_p()
    assert hip_lib.chisel_hip_stereo_create(1, 48, None, 0, C.byref(h)) == 1
    assert hip_lib.chisel_hip_stereo_create(64, 48, None, 0, None) == 1
    bad = capi.StereoParams()
    hip_lib.chisel_hip_stereo_default_params(C.byref(bad))
    bad.dep_sample = 0.0
    assert hip_lib.chisel_hip_stereo_create(64, 48, C.byref(bad), 0, C.byref(h)) == 1
    m = StereoMapper(64, 48)
    img = np.zeros((48, 64), np.float32)
    R = (C.c_float * 9)(*np.eye(3, dtype=np.float32).reshape(9).tolist())
    t = (C.c_float * 3)(0.0, 0.0, 0.0)
    assert hip_lib.chisel_hip_stereo_update(m.h, img.ctypes.data, R, t, 0) == 1      # no reference yet
    assert hip_lib.chisel_hip_stereo_set_reference(m.h, None, img.ctypes.data, 0) == 1
    assert hip_lib.chisel_hip_stereo_set_reference(None, img.ctypes.data, img.ctypes.data, 0) == 1
    m.InitReference(img, img)
    assert hip_lib.chisel_hip_stereo_update(m.h, None, R, t, 0) == 1
    assert hip_lib.chisel_hip_stereo_update(m.h, img.ctypes.data, None, t, 0) == 1
    assert hip_lib.chisel_hip_stereo_output(m.h, img.ctypes.data, None, 0) == 1          # sparse depth without distance
    assert hip_lib.chisel_hip_stereo_output(None, None, None, 0) == 1
    assert hip_lib.chisel_hip_stereo_clear(None) == 1
    out = np.empty((48, 64), np.float32)
    assert hip_lib.chisel_hip_stereo_read(m.h, 4, out.ctypes.data, 0) == 1
    assert hip_lib.chisel_hip_stereo_read(m.h, 2, None, 0) == 1
    # nothing was launched: the state is still the created one
    assert (m.read(m.COST) == 0).all() and (m.read(m.DEPTH) == 0).all()


def test_stereo_binding_checks_shape_and_dtype(hip_lib):
    """cvids_amd.chisel.StereoMapper: an image of another size, or a CUDA tensor that is not float32 (used in place, it would be
    read as float32), is refused before the library is called"""
    import torch
    from cvids_amd.chisel import StereoMapper
    m = StereoMapper(64, 48)
    img = np.zeros((48, 64), np.float32)
    with pytest.raises(AssertionError):
        m.InitReference(np.zeros((47, 64), np.float32), img)
    m.InitReference(img, img)
    with pytest.raises(AssertionError):
        m.Update(np.zeros((48, 65), np.float32), np.eye(3), np.zeros(3))
    with pytest.raises(AssertionError):
        m.Update(torch.zeros((48, 64), dtype=torch.float64, device="cuda"), np.eye(3), np.zeros(3))
    with pytest.raises(AssertionError):
        m.Output(torch.zeros((48, 64), dtype=torch.float16, device="cuda"), torch.zeros((48, 64), device="cuda"))
    assert (m.read(m.COST) == 0).all()
    m.Update(torch.zeros((48, 64), dtype=torch.float32, device="cuda"), np.eye(3), np.zeros(3))   # the right type goes through
