"""GPU tests of who frees what: each of the three device objects (stereo matcher, depth filter, map) is created, used and
destroyed four times, and the free device memory after the first cycle is compared with that after the fourth.  An object that
is not freed, or one of its large buffers, shows as three footprints; the two readings may differ by less than half of one.  The
footprint is computed here from the test's own sizes and counts the object's large arrays only (a lower bound: the stricter side).
The first cycle is not compared with the state before it: the runtime keeps what it loaded for the first kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CYCLES = 4


def free_bytes():
    import torch
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


def run_cycles(cycle, footprint):
    readings = []
    for _ in range(CYCLES):
        cycle()
        readings.append(free_bytes())
    drift = readings[0] - readings[-1]
    print("free after each cycle: %s; footprint %d; cycle 1 - cycle %d = %d" % (readings, footprint, CYCLES, drift))
    assert abs(drift) < footprint // 2, (readings, footprint)


def test_stereo_cycles_return_their_memory():
    from cvids_amd.chisel import StereoMapper
    W, H = 256, 192
    footprint = 2 * W * H * StereoMapper.DEP_CNT * 4  # the cost and the SGM volume, float32: 50 MB
    K, D = (458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)
    rng = np.random.default_rng(7)
    ref = rng.integers(0, 256, (288, 384), dtype=np.uint8)
    match = np.roll(ref, 3, axis=1)
    eye = np.eye(3)

    def cycle():
        s = StereoMapper(W, H)
        s.InitIntrinsic(K, D, K, D, (320, 240))
        s.InitIntrinsic(K, D, K, D, (384, 288))  # another camera size: the three camera-size buffers are released and made again
        s.InitReferenceImage(ref)
        s.UpdateImage(match, (eye, np.zeros(3)), (eye, np.array([0.1, 0.0, 0.0])))
        depth = s.OutputImage()
        depth64 = s.read(StereoMapper.DEPTH_REAL64)  # the read-out that is staged on the device before it reaches the host
        assert depth.shape == depth64.shape == (288, 384) and np.array_equal(depth.astype(np.float64), depth64, equal_nan=True)
        s.close()

    run_cycles(cycle, footprint)


def test_depth_filter_cycles_return_their_memory():
    from cvids_amd.chisel import DepthFilter
    H = W = 1024
    footprint = 7 * H * W * 8  # a, b, mu, cov and three staging arrays, float64: 59 MB
    rng = np.random.default_rng(8)
    mu, cov = rng.uniform(0.5, 4.0, (H, W)), rng.uniform(0.01, 0.1, (H, W))

    def cycle():
        f = DepthFilter(H, W)
        f.Update(mu, cov)
        inv_depth = f.GetInvDepth()
        assert inv_depth.shape == (H, W)
        f.close()

    run_cycles(cycle, footprint)


def test_map_cycles_return_their_memory():
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    W, H, N, max_chunks = 160, 120, 16, 1024
    footprint = max_chunks * N ** 3 * (4 + 4 + 4)  # sdf, weight and colour of a fixed pool: 50 MB
    intr = synth.intrinsics(W, H)
    cam = PinholeCamera(*intr, W, H, 0.05, 5.0)
    color = synth.render_color(W, H, 3)
    integ = ProjectionIntegrator(InverseTruncator(2.0), ConstantWeighter(1.0), 0.05, True)
    frames = list(synth.stream("sphere_room", 2, W, H))
    cloud_pose = synth.trajectory_pose(2)
    cloud_intr = synth.intrinsics(64, 48)
    pts, cols = synth.depth_to_cloud(synth.render_depth("sphere_room", cloud_pose, cloud_intr, 64, 48), cloud_intr, 0.6, colors=True)

    def cycle():
        m = Chisel((N, N, N), 0.04, True, device_id=0, max_chunks=max_chunks)
        for depth, pose in frames:
            m.IntegrateDepthScanColor(integ, depth, pose, cam, color, pose, cam)
        m.UpdateMeshes()
        m.IntegratePointCloud(integ, (pts, cols), cloud_pose, 0.1, 5.0)
        m.synchronize()
        assert len(m.fields()) > 10
        m.close()

    run_cycles(cycle, footprint)
