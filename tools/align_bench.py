#!/usr/bin/env python3
"""Time chisel_hip_align_terms and chisel_hip_align_depth on the map of bench.py's default stream (sphere_room, 640 x 480 depth +
colour, 1 cm voxels, 16^3 chunks, InverseTruncator(1), carving 0.05 m) after 220 frames, the depth image in HBM, after warm-up.

    python tools/align_bench.py [--frames 220 --iters 20 --warmup 3 --out profiles/align_bench.json]

The frame is the last pose's depth image at 160 x 120 and at 640 x 480; the guess is that pose moved by 1 cm and 0.5 degrees.  Per size:
  align_terms/device   device time of one call with the 32 doubles left in HBM (events on the map's stream around the call, nothing
                       waited for in between): the launch chain alone
  align_terms/host     wall time of one call that returns the 32 doubles to the host (what an iteration of a caller's own loop pays)
  query_reduce/host    wall time of what a caller could do before this entry existed, on the same points, until the same numbers are
                       on the host: Chisel.QueryPoints(found, sdf, gradient) into device tensors, then in torch (float64) J = (g, p x g),
                       the 21 sums of J J^T as J^T J and the 6 of J sdf as J^T sdf, over the found points.  (It takes the stored distance
                       for the residual and leaves the order of the sums to torch: it is the cheaper computation.)
  align_depth/iteration  wall time of chisel_hip_align_depth with 10 iterations (stop thresholds 0: all ten run), divided by 10
Medians and minima in microseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES, CHUNK, NEAR, FAR = 0.01, 16, 0.05, 5.0
W, H = 640, 480
SIZES = ((160, 120), (640, 480))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    from tests import align_restated as ar
    from tests import render_restated as rr
    dev = torch.device("cuda:0")
    gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    color = torch.from_numpy(synth.render_color(W, H, 3)).to(dev)
    batch = []
    for depth, pose in synth.stream("sphere_room", a.frames, W, H):
        batch.append((torch.from_numpy(depth).to(dev), pose, cam))
        if len(batch) == 10:
            gm.IntegrateBatch(integ, batch, [(color, p, cam) for _, p, _ in batch])
            gm.synchronize()
            batch = []
    if batch:
        gm.IntegrateBatch(integ, batch, [(color, p, cam) for _, p, _ in batch])
    gm.synchronize()

    true_pose = synth.trajectory_pose(a.frames - 1)
    guess = ar.start_pose(true_pose, (0.006, -0.006, 0.006, 0.3, -0.3, 0.3))
    res = {"frames": a.frames, "chunks": gm.NumChunks(), "voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "sizes": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        e.record()  # (creates the hipEvent_t the map records below)
    torch.cuda.synchronize()

    def stats(t):
        return {"us": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1)}

    def device_time(call):
        for _ in range(a.warmup):
            call()
        gm.synchronize()
        t = []
        for _ in range(a.iters):
            gm.record_event(ev[0].cuda_event)
            call()
            gm.record_event(ev[1].cuda_event)
            ev[1].synchronize()
            t.append(ev[0].elapsed_time(ev[1]) * 1e3)
        return stats(t)

    def wall_time(call, per=1):
        for _ in range(a.warmup):
            call()
        t = []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            gm.synchronize()
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6 / per)
        return stats(t)

    for w, h in SIZES:
        c = PinholeCamera(*synth.intrinsics(w, h), w, h, NEAR, FAR)
        depth_h = synth.render_depth("sphere_room", true_pose, synth.intrinsics(w, h), w, h)
        depth = torch.from_numpy(depth_h).to(dev)
        out = torch.zeros(32, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        r = {"pixels": w * h}
        r["align_terms/device"] = device_time(lambda: gm.AlignTerms(depth, guess, c, out=out))
        terms = gm.AlignTerms(depth, guess, c)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), terms.view(np.uint64))
        r["used_share"] = round(float(terms[28] / terms[29]), 4)
        r["align_terms/host"] = wall_time(lambda: gm.AlignTerms(depth, guess, c))

        # the same points through the existing entry and torch
        pts = torch.from_numpy(rr.hit_points(np.asarray(guess, np.float32), (c.fx, c.fy, c.cx, c.cy), depth_h)).to(dev)
        n = w * h
        q = {"found": torch.zeros(n, dtype=torch.uint8, device=dev), "sdf": torch.zeros(n, dtype=torch.float32, device=dev),
             "gradient": torch.zeros((n, 3), dtype=torch.float32, device=dev)}
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()

        def query_reduce():
            gm.QueryPoints(pts, out=q)
            gm.order_stream_after_map(stream)
            use = (q["found"] & 2) != 0
            g = torch.where(use[:, None], q["gradient"], torch.zeros_like(q["gradient"])).double()
            p = pts.double()
            J = torch.cat([g, torch.linalg.cross(p, g)], dim=1)
            rho = torch.where(use, q["sdf"], torch.zeros_like(q["sdf"])).double()
            sums = torch.cat([(J.T @ J).reshape(-1), J.T @ rho, use.sum(dtype=torch.float64)[None]])
            host = sums.cpu().numpy()
            gm.order_map_after_stream(stream)  # (the next query overwrites what these kernels read)
            return host

        host = query_reduce()
        assert host[36 + 6] == terms[28], (host[36 + 6], terms[28])
        assert abs(host[0] - terms[0]) <= 1e-9 * terms[28]
        r["query_reduce/host"] = wall_time(query_reduce)
        run = gm.AlignDepth(depth, guess, c, max_iterations=10, min_translation=0.0, min_rotation=0.0)
        assert run["iterations"] == 10, run["status"]
        r["align_depth/iteration"] = wall_time(lambda: gm.AlignDepth(depth, guess, c, max_iterations=10, min_translation=0.0, min_rotation=0.0), per=10)
        res["sizes"]["%dx%d" % (w, h)] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
