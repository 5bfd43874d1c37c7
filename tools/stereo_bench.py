#!/usr/bin/env python3
"""Time the stereo matcher (chisel_hip_stereo_*) at the reference's working size, inputs in HBM, after warm-up.

    python tools/stereo_bench.py [--width 640 --height 480 --iters 20 --warmup 3 --out FILE]

Per match frame the reference's driver runs Update then Output (depth_estimator.cpp:234-253); this reports the device time of each
(events on the null stream the library uses), the bytes each must move at the least (below) and their rate over 8 TB/s HBM.
  update:  cost volume read + written (from the second measurement on) + the match image
  output:  SGM -- cost read by each of 4 passes, SGM volume written by the first and read + written by the other three --
           then the winner-takes-all pass reading the SGM volume and writing the depth map (no sparse prior)
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/stereo_bench.py`.

    python tools/stereo_bench.py --raw [--real-width 752 --real-height 480 --points 500 ...]

times the raw-image path instead (chisel_hip_stereo_set_camera and after), mono8 camera frames in HBM, one line per camera size:
  ref_prep:    set_reference_image -- 8-bit resize, undistort remap, three Sobel maps with their sums, P2 map and masks
  match_prep:  update_image minus update (the float path's cost pass on the same images): resize + remap of the match image
  raster:      output_image with the bound points minus output_image with none: the two rasteriser kernels plus FuseSparseInfo
  out_resize:  output_image without points minus output without a prior: the empty rasteriser pass plus the final resize
The differences are of medians; the rocprofv3 run above gives the kernels' own times."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--raw", action="store_true", help="time the raw-image path (see above)")
    ap.add_argument("--real-width", type=int, nargs="*", default=[640, 752])
    ap.add_argument("--real-height", type=int, default=480)
    ap.add_argument("--points", type=int, default=500)
    a = ap.parse_args()
    if a.raw:
        return raw_main(a)

    import torch
    from cvids_amd.chisel import StereoMapper, stereo_homography
    W, H, D = a.width, a.height, StereoMapper.DEP_CNT
    rng = np.random.default_rng(0)
    fx = 460.95 * W / 640.0
    K = np.array([[fx, 0, W / 2.0], [0, fx, H / 2.0], [0, 0, 1.0]])
    R, t = stereo_homography(K, K, np.eye(3), np.zeros(3), np.eye(3), np.array([0.11, 0.01, 0.02]))
    ref = torch.from_numpy(rng.uniform(0, 255, (H, W)).astype(np.float32)).cuda()
    match = torch.from_numpy(rng.uniform(0, 255, (H, W)).astype(np.float32)).cuda()
    p2w = torch.from_numpy((0.8 + rng.uniform(0, 1.5, (H, W))).astype(np.float32)).cuda()
    m = StereoMapper(W, H)
    m.InitReference(ref, p2w)
    depth = torch.empty((H, W), dtype=torch.float32, device="cuda")
    for _ in range(a.warmup):
        m.Update(match, R, t)
        m.Output(out=depth)
    torch.cuda.synchronize()

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_upd, t_out = [], []
    for _ in range(a.iters):
        ev[0].record()
        m.Update(match, R, t)
        ev[1].record()
        check = m.L.chisel_hip_stereo_output(m.h, None, None, 0)
        assert check == 0
        ev[2].record()
        ev[2].synchronize()
        t_upd.append(ev[0].elapsed_time(ev[1]) * 1e3)
        t_out.append(ev[1].elapsed_time(ev[2]) * 1e3)
    vol = W * H * D * 4
    bytes_upd = 2 * vol + W * H * 4
    bytes_out = 4 * vol + vol + 3 * 2 * vol + vol + W * H * 4
    us_upd, us_out = float(np.median(t_upd)), float(np.median(t_out))
    res = {
        "width": W, "height": H, "dep_cnt": D, "iters": a.iters,
        "update_us": round(us_upd, 1), "update_us_min": round(float(np.min(t_upd)), 1),
        "output_us": round(us_out, 1), "output_us_min": round(float(np.min(t_out)), 1),
        "frame_us": round(us_upd + us_out, 1),
        "update_bytes": bytes_upd, "output_bytes": bytes_out,
        "update_hbm_fraction": round(bytes_upd / (us_upd * 1e-6) / HBM_BYTES_PER_S, 3),
        "output_hbm_fraction": round(bytes_out / (us_out * 1e-6) / HBM_BYTES_PER_S, 3),
        "valid_depth_fraction": round(float((depth.cpu().numpy() != 1000).mean()), 3),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def _median_us(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        t.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return float(np.median(t))


def raw_main(a):
    import torch
    from cvids_amd.chisel import StereoMapper, stereo_homography
    from cvids_amd import capi
    W, H, D = a.width, a.height, StereoMapper.DEP_CNT
    lines = []
    for real_w in a.real_width:
        real_h = a.real_height
        rng = np.random.default_rng(0)
        s = real_w / 752.0
        K = (458.654 * s, 457.296 * s, 367.215 * s, 248.375 * real_h / 480.0)      # EuRoC cam0, scaled to the frame
        Dist = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)
        m = StereoMapper(W, H)
        m.InitIntrinsic(K, Dist, K, Dist, (real_w, real_h))
        ref = torch.from_numpy(rng.integers(0, 256, (real_h, real_w), dtype=np.uint8)).cuda()
        match = torch.from_numpy(rng.integers(0, 256, (real_h, real_w), dtype=np.uint8)).cuda()
        I, t0, t1 = np.eye(3), np.zeros(3), np.array([0.11, 0.01, 0.02])
        d = lambda v: (capi.C.c_double * len(v))(*[float(x) for x in v])
        Rr, tr, Rm, tm = d(I.reshape(9)), d(t0), d(I.reshape(9)), d(t1)
        Ks = (K[0] * W / real_w, K[1] * H / real_h, K[2] * W / real_w, K[3] * H / real_h)
        Km = np.array([[Ks[0], 0, Ks[2]], [0, Ks[1], Ks[3]], [0, 0, 1.0]])
        R, t = stereo_homography(Km, Km, I, t0, I, t1)
        Rf = (capi.C.c_float * 9)(*R.reshape(9).tolist())
        tf = (capi.C.c_float * 3)(*t.tolist())
        fmatch = torch.from_numpy(rng.uniform(0, 255, (H, W)).astype(np.float32)).cuda()
        L, h = m.L, m.h

        def ok(rc):
            assert rc == 0, L.chisel_hip_last_error()
        ref_prep = _median_us(lambda: ok(L.chisel_hip_stereo_set_reference_image(h, ref.data_ptr(), real_w, 1)), a.iters, a.warmup)
        upd_img = _median_us(lambda: ok(L.chisel_hip_stereo_update_image(h, match.data_ptr(), real_w, Rr, tr, Rm, tm, 1)), a.iters, a.warmup)
        upd = _median_us(lambda: ok(L.chisel_hip_stereo_update(h, fmatch.data_ptr(), Rf, tf, 1)), a.iters, a.warmup)
        m.BindSparsePoints(np.zeros(0), np.zeros((0, 2)))
        out_none = _median_us(lambda: ok(L.chisel_hip_stereo_output_image(h)), a.iters, a.warmup)
        out_float = _median_us(lambda: ok(L.chisel_hip_stereo_output(h, None, None, 0)), a.iters, a.warmup)
        pts = np.stack([rng.uniform(0, real_w, a.points), rng.uniform(0, real_h, a.points)], axis=1)
        m.BindSparsePoints(rng.uniform(0.5, 8.0, a.points), pts)
        out_pts = _median_us(lambda: ok(L.chisel_hip_stereo_output_image(h)), a.iters, a.warmup)
        res = {"width": W, "height": H, "real_width": real_w, "real_height": real_h, "points": a.points, "iters": a.iters,
               "ref_prep_us": round(ref_prep, 1), "update_image_us": round(upd_img, 1), "update_us": round(upd, 1),
               "match_prep_us": round(upd_img - upd, 1), "output_image_us": round(out_none, 1), "output_us": round(out_float, 1),
               "output_image_points_us": round(out_pts, 1), "raster_us": round(out_pts - out_none, 1),
               "out_resize_us": round(out_none - out_float, 1)}
        lines.append(json.dumps(res))
        print(lines[-1])
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
