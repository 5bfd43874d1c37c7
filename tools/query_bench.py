#!/usr/bin/env python3
"""Time chisel_hip_cast_rays and chisel_hip_query_points on the map of bench.py's default stream (sphere_room, 640 x 480 depth +
colour, 1 cm voxels, 16^3 chunks, InverseTruncator(1), carving 0.05 m) after 220 frames, inputs and outputs in HBM, after warm-up.

    python tools/query_bench.py [--frames 220 --iters 20 --warmup 3 --out profiles/query_bench.json]

Rays: the 640 x 480 rays of the last pose ("seen") and of the same position turned by 180 degrees into space no frame has observed
("unseen"), each in three orders -- row-major, 8 x 8 tiles (the order in which chisel_hip_render_view's waves take their pixels) and
shuffled -- beside chisel_hip_render_view of the same view, and the ratio to it.
Points: 1 M positions of the "jitter" kind (hit points of the last view moved by N(0, 2 voxels)) and of the "box" kind (uniform in
the box of the resident chunks grown by one chunk), each with sdf only, with the gradient, with gradient and colour; and the time
per call of 1000 chisel_hip_get_sdf calls.
Per case: the median and minimum device time of a call in microseconds (events recorded on the map's stream around the call, nothing
waited for in between).

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/query_bench.py` and then

    python tools/query_bench.py --summarize-trace DIR [--iters 20 --warmup 3] --out profiles/query_kernel_stats.csv

which cuts the trace's dispatches into the cases by their order (warm-up + iters dispatches each)."""
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
ORDERS = ("row_major", "tiles_8x8", "shuffled")
VIEWS = ("seen", "unseen")
POINT_KINDS = ("jitter", "box")
POINT_OUTPUTS = {"sdf": ("found", "sdf"), "sdf_gradient": ("found", "sdf", "gradient"), "sdf_gradient_colour": ("found", "sdf", "gradient", "colors")}
N_POINTS = 1 << 20
SEED = 20260102
# the order in which the cases dispatch their kernels
RAY_CASES = [(v, o) for v in VIEWS for o in ORDERS]
POINT_CASES = [(k, o) for k in POINT_KINDS for o in POINT_OUTPUTS]


def orders(rng):
    """name -> permutation of the W * H row-major ray indices"""
    idx = np.arange(W * H).reshape(H // 8, 8, W // 8, 8)
    return {"row_major": np.arange(W * H), "tiles_8x8": idx.transpose(0, 2, 1, 3).reshape(-1), "shuffled": rng.permutation(W * H)}


def summarize_trace(a):
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = a.warmup + a.iters
    out = open(a.out, "w") if a.out else sys.stdout
    w = csv.writer(out)
    w.writerow(["case", "kernel", "calls", "median_us", "min_us", "max_us"])

    def emit(kernel, names):
        part = [r for r in rows if kernel in r["Kernel_Name"]]
        assert len(part) == per * len(names), "%d %s dispatches in the trace, expected %d" % (len(part), kernel, per * len(names))
        for i, name in enumerate(names):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in part[i * per + a.warmup:(i + 1) * per]]
            w.writerow([name, kernel, len(us), "%.1f" % np.median(us), "%.1f" % min(us), "%.1f" % max(us)])

    emit("render_view_kernel", ["render_view/" + v for v in VIEWS])
    emit("cast_rays_kernel", ["cast_rays/%s/%s" % c for c in RAY_CASES])
    emit("query_points_kernel", ["query_points/%s/%s" % c for c in POINT_CASES])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarize-trace", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a)

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator, pack_rays
    from tests import render_restated as rr
    dev = torch.device("cuda:0")
    gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
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

    k = a.frames - 1
    poses = {"seen": synth.trajectory_pose(k), "unseen": synth.pose_yaw(0.5 * k + 180.0, (0.01 * k, 0.0, 0.0))}
    res = {"frames": a.frames, "chunks": gm.NumChunks(), "voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "rays": W * H, "points": N_POINTS,
           "render_view": {}, "cast_rays": {}, "query_points": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        e.record()  # (creates the hipEvent_t the map records below)
    torch.cuda.synchronize()

    def timed(call):
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
        return {"call_us": round(float(np.median(t)), 1), "call_us_min": round(float(np.min(t)), 1)}

    # chisel_hip_render_view of both views: what the rays are compared with
    depth_of = {}
    for name, pose in poses.items():
        out = {"depth": torch.empty((H, W), dtype=torch.float32, device=dev)}
        torch.cuda.synchronize()
        r = timed(lambda: gm.RenderView(pose, cam, out=out))
        depth_of[name] = out["depth"].cpu().numpy()
        r["hit_share"] = round(float(np.isfinite(depth_of[name]).mean()), 4)
        res["render_view"][name] = r
    rng = np.random.default_rng(SEED)
    perm = orders(rng)
    for view, order in RAY_CASES:
        o, d = rr.rays(poses[view], intr, W, H)
        rays = torch.from_numpy(pack_rays(o, d, NEAR, FAR)[perm[order]]).to(dev)
        out = {"t_hit": torch.empty(W * H, dtype=torch.float32, device=dev), "status": torch.empty(W * H, dtype=torch.uint8, device=dev)}
        torch.cuda.synchronize()
        r = timed(lambda: gm.CastRays(rays, None, None, None, out=out))
        t_hit = np.empty(W * H, np.float32)
        t_hit[perm[order]] = out["t_hit"].cpu().numpy()
        want = depth_of[view].reshape(-1)
        assert np.array_equal(np.isnan(t_hit), np.isnan(want)) and np.array_equal(t_hit[~np.isnan(t_hit)], want[~np.isnan(want)]), (view, order)
        r["to_render_view"] = round(r["call_us"] / res["render_view"][view]["call_us"], 3)
        res["cast_rays"]["%s/%s" % (view, order)] = r

    hits = rr.hit_points(poses["seen"], intr, depth_of["seen"])
    hits = hits[np.isfinite(hits).all(1)]
    ids = gm.GetChunkIDs().astype(np.int64)
    edge = CHUNK * RES
    sets = {"jitter": (hits[rng.integers(0, len(hits), N_POINTS)] + rng.normal(0.0, 2.0 * RES, (N_POINTS, 3))).astype(np.float32),
            "box": rng.uniform((ids.min(0) - 1) * edge, (ids.max(0) + 2) * edge, (N_POINTS, 3)).astype(np.float32)}
    for kind, outputs in POINT_CASES:
        pts = torch.from_numpy(sets[kind]).to(dev)
        out = {name: torch.empty((N_POINTS,) + ((3,) if name in ("gradient", "colors") else ()), dtype=torch.uint8 if name == "found" else torch.float32,
                                 device=dev) for name in POINT_OUTPUTS[outputs]}
        torch.cuda.synchronize()
        r = timed(lambda: gm.QueryPoints(pts, out=out))
        found = out["found"].cpu().numpy()
        r["ns_per_point"] = round(r["call_us"] * 1e3 / N_POINTS, 3)
        r["found_share"] = round(float((found & 1).mean()), 4)
        if "gradient" in out:
            r["gradient_share"] = round(float((found >> 1).mean()), 4)
        res["query_points"]["%s/%s" % (kind, outputs)] = r

    # the single-point entry: one launch and one wait per position
    gm.GetSDF(sets["jitter"][0])
    t0 = time.perf_counter()
    for p in sets["jitter"][:1000]:
        gm.GetSDF(p)
    res["get_sdf_us_per_call"] = round((time.perf_counter() - t0) * 1e6 / 1000, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
