#!/usr/bin/env python3
"""Time chisel_hip_distance_field on the map of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3
chunks, InverseTruncator(1), carving 0.05 m) after 220 frames, outputs in HBM, after warm-up.

    python tools/distance_bench.py [--frames 220 --iters 10 --warmup 2 --out profiles/distance_bench.txt]

Windows: 128 x 128 x 32 voxels at R = 16 and 256 x 256 x 64 at R = 32, centred on the surface point the central pixel of the last
pose sees, state + dist2 + distance, occupied voxels as obstacles.  Per window: the median, minimum and maximum device time of a call
in microseconds (events recorded on the map's stream around the call, nothing waited for in between), and beside it the only route
a caller has without the entry, once, wall time: chisel_hip_query_points at every voxel centre of the widened window (host arrays,
the read-back included) plus tests/distance_restated.separable on the host -- whose dist2 must equal the call's.

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/distance_bench.py --skip-route` and then

    python tools/distance_bench.py --summarize-trace DIR [--iters 10 --warmup 2] --out profiles/distance_bench.txt

which cuts the trace's dispatches into the windows by their order (warm-up + iters dispatches each) and appends the table."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES, CHUNK, NEAR, FAR = 0.01, 16, 0.05, 5.0
W, H = 640, 480
WINDOWS = [((128, 128, 32), 16), ((256, 256, 64), 32)]
KERNELS = ("distance_seed_kernel", "distance_x_kernel", "distance_axis_kernel<false>", "distance_axis_kernel<true>")


def summarize_trace(a):
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = a.warmup + a.iters
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nper kernel, from rocprofv3 --kernel-trace --stats (a run of its own: %d warm-up + %d timed calls per window)\n" % (a.warmup, a.iters))
    out.write("%-22s %-30s %6s %10s %10s %10s\n" % ("window", "kernel", "calls", "median_us", "min_us", "max_us"))
    for kernel in KERNELS:
        part = [r for r in rows if kernel in r["Kernel_Name"].replace("(bool)0", "false").replace("(bool)1", "true")]
        assert len(part) == per * len(WINDOWS), "%d %s dispatches in the trace, expected %d" % (len(part), kernel, per * len(WINDOWS))
        for i, (dims, R) in enumerate(WINDOWS):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in part[i * per + a.warmup:(i + 1) * per]]
            out.write("%-22s %-30s %6d %10.1f %10.1f %10.1f\n" % ("%dx%dx%d R=%d" % (dims + (R,)), kernel, len(us), np.median(us), min(us), max(us)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-route", action="store_true", help="leave out the QueryPoints + host transform route (under the profiler)")
    ap.add_argument("--summarize-trace", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a)

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    from tests import distance_restated as dr
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

    pose = np.asarray(synth.trajectory_pose(a.frames - 1), np.float64)
    view = gm.RenderView(synth.trajectory_pose(a.frames - 1), cam)["depth"]
    z = float(view[H // 2, W // 2])
    assert np.isfinite(z), "the central pixel of the last pose sees no surface"
    hit = pose[:3, :3] @ np.array([(W // 2 + 0.5 - cam.cx) / cam.fx * z, (H // 2 + 0.5 - cam.cy) / cam.fy * z, z]) + pose[:3, 3]
    res = {"frames": a.frames, "chunks": gm.NumChunks(), "voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "warmup": a.warmup, "windows": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        e.record()  # (creates the hipEvent_t the map records below)
    torch.cuda.synchronize()
    for dims, R in WINDOWS:
        origin = tuple(int(np.floor(hit[k] / RES)) - dims[k] // 2 for k in range(3))
        shape = (dims[2], dims[1], dims[0])
        out = {"state": torch.empty(shape, dtype=torch.uint8, device=dev), "dist2": torch.empty(shape, dtype=torch.int32, device=dev),
               "distance": torch.empty(shape, dtype=torch.float32, device=dev)}
        torch.cuda.synchronize()
        call = lambda: gm.DistanceField(origin, dims, R, out=out)
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
        state, dist2 = out["state"].cpu().numpy(), out["dist2"].cpu().numpy()
        voxels = dims[0] * dims[1] * dims[2]
        r = {"origin": origin, "voxels": voxels, "widened_voxels": int(np.prod([d + 2 * R for d in dims])),
             "call_us": round(float(np.median(t)), 1), "call_us_min": round(float(np.min(t)), 1), "call_us_max": round(float(np.max(t)), 1),
             "ns_per_voxel": round(float(np.median(t)) * 1e3 / voxels, 3),
             "unknown": round(float((state == 0).mean()), 4), "free": round(float((state == 1).mean()), 4), "occupied": round(float((state == 2).mean()), 4),
             "without_obstacle": round(float((dist2 < 0).mean()), 4), "distinct_dist2": int(len(np.unique(dist2)))}
        if not a.skip_route:
            wo, wd = tuple(o - R for o in origin), tuple(d + 2 * R for d in dims)
            t0 = time.perf_counter()
            q = gm.QueryPoints(dr.centres(wo, wd, RES))
            t1 = time.perf_counter()
            with np.errstate(invalid="ignore"):
                st = np.where(q["found"] & 1, np.where(q["sdf"] < np.float32(0), 2, 1), 0).astype(np.uint8).reshape(wd[2], wd[1], wd[0])
            want = dr.separable(st, R)
            t2 = time.perf_counter()
            # (1 cm is no power of two: a centre computed in fp32 may fall into the neighbour voxel, so the route's answer is compared as a share)
            r["route"] = {"query_and_readback_ms": round((t1 - t0) * 1e3, 1), "host_transform_ms": round((t2 - t1) * 1e3, 1),
                          "wall_ms": round((t2 - t0) * 1e3, 1), "dist2_equal_share": round(float((want == dist2).mean()), 6)}
            r["route_over_call"] = round((t2 - t0) * 1e6 / r["call_us"], 1)
        res["windows"]["%dx%dx%d R=%d" % (dims + (R,))] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("python tools/distance_bench.py   (one MI355X; the map of bench.py's default stream -- sphere_room, 640 x 480 depth + colour, 1 cm voxels,\n"
                    "16^3 chunks -- after %d frames; %d warm-up + %d timed calls per window, state + dist2 + distance into device tensors;\n"
                    "call_us = hipEvent time over the map's stream around chisel_hip_distance_field; route = chisel_hip_query_points at every centre of\n"
                    "the widened window with the read-back, plus tests/distance_restated.separable on the host, once, wall time)\n\n" % (a.frames, a.warmup, a.iters))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
