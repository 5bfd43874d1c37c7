#!/usr/bin/env python3
"""Time the stereo matcher (chisel_hip_stereo_*) at the reference's working size, inputs in HBM, after warm-up.

    python tools/stereo_bench.py [--width 640 --height 480 --iters 20 --warmup 3 --out FILE]

Per match frame the reference's driver runs Update then Output (depth_estimator.cpp:234-253); this reports the device time of each
(events on the null stream the library uses), the bytes each must move at the least (below) and their rate over 8 TB/s HBM.
  update:  cost volume read + written (from the second measurement on) + the match image
  output:  SGM -- cost read by each of 4 passes, SGM volume written by the first and read + written by the other three --
           then the winner-takes-all pass reading the SGM volume and writing the depth map (no sparse prior)
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/stereo_bench.py`."""
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
    a = ap.parse_args()

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


if __name__ == "__main__":
    main()
