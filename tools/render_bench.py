#!/usr/bin/env python3
"""Time chisel_hip_render_view on the map of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3
chunks, InverseTruncator(1), carving 0.05 m) after 220 frames, outputs in HBM, after warm-up.

    python tools/render_bench.py [--frames 220 --iters 20 --warmup 3 --out FILE]

Four views, in this order:
  vga_depth     640 x 480 from the last pose of the stream, depth only
  vga_shaded    the same with normals and colours
  hd_depth      1280 x 720 from the same pose, depth only
  vga_unseen    640 x 480 from the last position, turned by 180 degrees: into space no frame has observed
Per view: the median and minimum device time of a call in microseconds (events recorded on the map's stream around the call, nothing
waited for in between) and the share of the pixels with a hit.

For the kernel's own times run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/render_bench.py` and then

    python tools/render_bench.py --summarize-trace DIR [--iters 20 --warmup 3] --out profiles/render_kernel_stats.csv

which cuts the trace's render_view_kernel dispatches into the four views by their order (warm-up + iters dispatches each).

    python tools/render_bench.py --count-samples [--frames 220] --out FILE

needs no GPU: it builds the same map with the CPU oracle (whose voxels the GPU's equal bit for bit: tests/test_gpu_parity.py) and runs
the numpy restatement of the march (tests/render_restated.py) over the 640 x 480 views: samples evaluated before the rays ended, and
how many of them lie in resident chunks (the others are what the kernel jumps over), against W H K."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES, CHUNK, NEAR, FAR = 0.01, 16, 0.05, 5.0
VIEWS = ("vga_depth", "vga_shaded", "hd_depth", "vga_unseen")


def views(frames):
    """name -> (pose, width, height, normals and colours)"""
    from cvids_amd import synth
    k = frames - 1
    last = synth.trajectory_pose(k)
    away = synth.pose_yaw(0.5 * k + 180.0, (0.01 * k, 0.0, 0.0))
    return {"vga_depth": (last, 640, 480, False), "vga_shaded": (last, 640, 480, True), "hd_depth": (last, 1280, 720, False),
            "vga_unseen": (away, 640, 480, False)}


def summarize_trace(a):
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "render_view_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = a.warmup + a.iters
    assert len(rows) == per * len(VIEWS), "%d render_view_kernel dispatches in the trace, expected %d" % (len(rows), per * len(VIEWS))
    out = open(a.out, "w") if a.out else sys.stdout
    w = csv.writer(out)
    w.writerow(["view", "kernel", "calls", "median_us", "min_us", "max_us"])
    for i, name in enumerate(VIEWS):
        part = rows[i * per + a.warmup:(i + 1) * per]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in part]
        kernel = part[0]["Kernel_Name"].split("(")[0].replace("void ", "").replace("chisel_hip::", "")
        w.writerow([name, kernel, len(us), "%.1f" % np.median(us), "%.1f" % min(us), "%.1f" % max(us)])


def count_samples(a):
    import oracle
    from cvids_amd import synth
    from tests import render_restated as rr
    W, H = 640, 480
    intr = synth.intrinsics(W, H)
    om = oracle.OracleMap(CHUNK, RES, False)
    om.set_integrator(oracle.TRUNC_INVERSE, 100 * RES, 1.0, True, 0.05)
    for depth, pose in synth.stream("sphere_room", a.frames, W, H):
        om.integrate_depth(depth, pose, intr, NEAR, FAR)
    index = rr.VoxelIndex(om.fields(), CHUNK, RES)
    res = {"frames": a.frames, "chunks": om.num_chunks()}
    for name, (pose, w, h, _) in views(a.frames).items():
        if (w, h) != (W, H) or name == "vga_shaded":
            continue
        st = {}
        d = rr.render_depth(index, pose, intr, W, H, NEAR, FAR, stats=st)
        st["full_march"] = st["rays"] * st["K"]
        st["hit_share"] = round(float(np.isfinite(d).mean()), 4)
        res[name] = st
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarize-trace", metavar="DIR", default=None)
    ap.add_argument("--count-samples", action="store_true")
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a)
    if a.count_samples:
        return count_samples(a)

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    W, H = 640, 480
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

    res = {"frames": a.frames, "chunks": gm.NumChunks(), "voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "views": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        e.record()  # (creates the hipEvent_t the map records below)
    torch.cuda.synchronize()
    for name, (pose, w, h, shaded) in views(a.frames).items():
        c = PinholeCamera(*synth.intrinsics(w, h), w, h, NEAR, FAR)
        out = {"depth": torch.empty((h, w), dtype=torch.float32, device=dev)}
        if shaded:
            out["normals"] = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            out["colors"] = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            gm.RenderView(pose, c, out=out)
        gm.synchronize()
        t = []
        for _ in range(a.iters):
            gm.record_event(ev[0].cuda_event)
            gm.RenderView(pose, c, out=out)
            gm.record_event(ev[1].cuda_event)
            ev[1].synchronize()
            t.append(ev[0].elapsed_time(ev[1]) * 1e3)
        depth = out["depth"].cpu().numpy()
        K = int(np.floor((np.float32(FAR) - np.float32(NEAR)) / np.float32(RES))) + 1
        res["views"][name] = {"width": w, "height": h, "samples_per_ray": K, "call_us": round(float(np.median(t)), 1), "call_us_min": round(float(np.min(t)), 1),
                              "hit_share": round(float(np.isfinite(depth).mean()), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
