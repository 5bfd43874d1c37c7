#!/usr/bin/env python3
"""Time chisel_hip_frontiers on the maps of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3 chunks,
InverseTruncator(1), carving 0.05 m) after 220 frames (the default window's map) and after 620 (the late window's), after warm-up.

    python tools/frontier_bench.py [--frames 220 620 --iters 10 --warmup 2 --out profiles/frontier_bench.txt]

Windows: those of tools/distance_bench.py, 128 x 128 x 32 and 256 x 256 x 64 voxels centred on the surface point the central pixel of
the last pose sees.  Per window, connectivity (6, 18, 26) and min_voxels (1, 16), min_unknown_faces 1:
  device_us   wall time of one chisel_hip_frontiers call -- label and the voxel list into device tensors, the table, capacities known
              from an earlier size query, as a planner that keeps its buffers calls it -- until a synchronise of the map returns
  host_us     wall time of Chisel.Frontiers into numpy arrays (a size query, then the call with exact capacities)
and beside it, once per window and connectivity 26, the only route a caller has without the entry, wall time: DistanceField(state) over
the window widened by one voxel, the read-back, scipy.ndimage.label plus numpy (tests/frontier_restated.answer) -- whose label, list
and table must equal the call's.

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/frontier_bench.py
--frames 220 --skip-route` and then

    python tools/frontier_bench.py --summarize-trace DIR --out profiles/frontier_bench.txt

which appends, per kernel, the calls and the median, the sum and the share of the device time over the whole run."""
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
WINDOWS = [(128, 128, 32), (256, 256, 64)]
KNOBS = [(c, m) for c in (6, 18, 26) for m in (1, 16)]


def summarize_trace(a):
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    per = {}
    for r in rows:
        name = r["Kernel_Name"]
        mine = next((k for k in ("frontier_", "report_words_kernel") if k in name), None)  # (the control words' way to the host is the shared kernel)
        if mine is None:
            continue
        name = mine if mine == "report_words_kernel" else name[name.index(mine):].split("(")[0]
        per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    total = sum(sum(v) for v in per.values())
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nper kernel, from rocprofv3 --kernel-trace --stats (a run of its own: every call of the run, both windows, all knobs)\n")
    out.write("%-34s %7s %10s %10s %12s %7s\n" % ("kernel", "calls", "median_us", "max_us", "sum_us", "share"))
    for name, us in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        out.write("%-34s %7d %10.1f %10.1f %12.1f %6.1f%%\n" % (name, len(us), np.median(us), max(us), sum(us), 100.0 * sum(us) / total))


def build_map(frames):
    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    dev = torch.device("cuda:0")
    gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    color = torch.from_numpy(synth.render_color(W, H, 3)).to(dev)
    batch = []
    for depth, pose in synth.stream("sphere_room", frames, W, H):
        batch.append((torch.from_numpy(depth).to(dev), pose, cam))
        if len(batch) == 10:
            gm.IntegrateBatch(integ, batch, [(color, p, cam) for _, p, _ in batch])
            gm.synchronize()
            batch = []
    if batch:
        gm.IntegrateBatch(integ, batch, [(color, p, cam) for _, p, _ in batch])
    gm.synchronize()
    for last in range(frames - 1, -1, -1):  # the latest pose whose central pixel sees a surface (the late window's last ones look past it)
        pose = np.asarray(synth.trajectory_pose(last), np.float64)
        z = float(gm.RenderView(synth.trajectory_pose(last), cam)["depth"][H // 2, W // 2])
        if np.isfinite(z):
            break
    assert np.isfinite(z), "no pose whose central pixel sees a surface"
    hit = pose[:3, :3] @ np.array([(W // 2 + 0.5 - cam.cx) / cam.fx * z, (H // 2 + 0.5 - cam.cy) / cam.fy * z, z]) + pose[:3, 3]
    return gm, hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[220, 620])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-route", action="store_true", help="leave out the host route and the host-array calls (under the profiler)")
    ap.add_argument("--summarize-trace", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a)

    import torch
    from tests import frontier_restated as fr
    dev = torch.device("cuda:0")
    res = {"voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "warmup": a.warmup, "maps": {}}
    for frames in a.frames:
        gm, hit = build_map(frames)
        per_map = {"chunks": gm.NumChunks(), "windows": {}}
        for dims in WINDOWS:
            origin = tuple(int(np.floor(hit[k] / RES)) - dims[k] // 2 for k in range(3))
            shape = (dims[2], dims[1], dims[0])
            voxels = dims[0] * dims[1] * dims[2]
            label = torch.empty(shape, dtype=torch.int32, device=dev)
            r = {"origin": origin, "voxels": voxels, "knobs": {}}
            for connectivity, min_voxels in KNOBS:
                size = gm.FrontiersSize(origin, dims, 1, connectivity, min_voxels)
                rows = torch.empty((max(size["kept_voxels"], 1), 4), dtype=torch.int32, device=dev)
                table = np.zeros((max(size["kept_clusters"], 1), 12), np.int64)
                w = gm._frontier_window(origin, dims, 1, connectivity, min_voxels, 0.0)
                torch.cuda.synchronize()

                def call():
                    gm._frontier_call(w, None, label.data_ptr(), rows.shape[0], rows.data_ptr(), len(table), table, 1)
                    gm.synchronize()

                def timed(f, n):
                    t = []
                    for _ in range(n):
                        t0 = time.perf_counter()
                        f()
                        t.append((time.perf_counter() - t0) * 1e6)
                    return t

                timed(call, a.warmup)
                t = timed(call, a.iters)
                k = {"frontier": size["frontier"], "clusters": size["clusters"], "kept_clusters": size["kept_clusters"], "largest_voxels": size["largest_voxels"],
                     "device_us": round(float(np.median(t)), 1), "device_us_min": round(float(np.min(t)), 1), "device_us_max": round(float(np.max(t)), 1),
                     "ns_per_voxel": round(float(np.median(t)) * 1e3 / voxels, 3)}
                if not a.skip_route:
                    host = lambda: gm.Frontiers(origin, dims, 1, connectivity, min_voxels)
                    timed(host, 1)
                    k["host_us"] = round(float(np.median(timed(host, max(a.iters // 2, 1)))), 1)
                r["knobs"]["c%d m%d" % (connectivity, min_voxels)] = k
            if not a.skip_route:
                got = gm.Frontiers(origin, dims, 1, 26, 1)
                wo, wd = tuple(o - 1 for o in origin), tuple(d + 2 for d in dims)
                t0 = time.perf_counter()
                wide = gm.DistanceField(wo, wd, 1, dist2=False)["state"]
                t1 = time.perf_counter()
                want = fr.answer(wide, 1, 26, 1)
                t2 = time.perf_counter()
                equal = all(np.array_equal(got[key], want[key]) for key in ("label", "voxels", "table")) and got["totals"] == want["totals"]
                r["route"] = {"state_and_readback_ms": round((t1 - t0) * 1e3, 1), "host_label_and_table_ms": round((t2 - t1) * 1e3, 1),
                              "wall_ms": round((t2 - t0) * 1e3, 1), "equal": bool(equal)}
                r["route_over_call"] = round((t2 - t0) * 1e6 / r["knobs"]["c26 m1"]["device_us"], 1)
                t = got["totals"]
                r["shares"] = {key: round(t[key] / voxels, 4) for key in ("unknown", "free", "occupied", "frontier")}
            per_map["windows"]["%dx%dx%d" % dims] = r
        res["maps"]["frames 0-%d" % (frames - 1)] = per_map
        gm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("python tools/frontier_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour, 1 cm voxels,\n"
                    "16^3 chunks -- after the frames named; %d warm-up + %d timed calls per window and knob set (c = connectivity, m = min_voxels),\n"
                    "min_unknown_faces 1; device_us = wall time of one chisel_hip_frontiers call, label and list into device tensors plus the table,\n"
                    "until a synchronise returns; host_us = Chisel.Frontiers into numpy arrays, a size query and the call; route = DistanceField(state)\n"
                    "over the widened window with the read-back, plus scipy.ndimage.label and numpy on the host, once, wall time)\n\n" % (a.warmup, a.iters))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
