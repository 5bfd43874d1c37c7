#!/usr/bin/env python3
"""Time chisel_hip_gather_meshes against the per-mesh walk it replaces, on the maps of bench.py's default stream (sphere_room,
640 x 480 depth + colour, 1 cm voxels, 16^3 chunks, InverseTruncator(1), carving 0.05 m, UpdateMeshes every 10 frames): after frames
0-219 (the default window's map, after its last recompute) and after frames 0-619 (the late window's).

    python tools/mesh_gather_bench.py [--frames 220,620 --iters 15 --warmup 3 --out profiles/mesh_gather_bench.txt]

Per map, alternating in one process, wall time in microseconds (median and the p10-p90 range):
  walk         GetMeshIDs + GetMesh over every id: the way to the same data without the entry (two C calls and three host copies
               per mesh).  walk_first is the one walk that follows the recompute and copies every live arena to the host, whole;
               the timed walks find those copies cached (arena_on_host), so they are the walk's floor, not its cost per recompute
  host         GatherMeshes() into numpy arrays (vertices, normals, colours, grids), complete on return
  device       GatherMeshes(out=...) into torch tensors: enqueue (the host's time in the call, nothing waited for) and the time
               until a synchronise behind it returns
  rgba         the time between two events on the map's stream around the call: the marker colours in the same launch against a
               launch of their own (rgba alone) behind a launch without them
The host arrays are checked equal, bit for bit, to the walk's concatenation before anything is timed.

For the kernel's own time run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mesh_gather_bench.py --device-only`
and then `python tools/mesh_gather_bench.py --summarize-trace DIR --out profiles/mesh_gather_bench.txt`, which appends the table
(bytes moved = 2 x 4 x the floats gathered, over the kernel's time, as a share of 8 TB/s)."""
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
NAMES = ("vertices", "normals", "colors", "grids")
WIDTH = {"vertices": 3, "normals": 3, "colors": 3, "rgba": 4, "grids": 3}


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1), "p90": round(float(np.percentile(us, 90)), 1)}


def summarize_trace(a):
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows = [r for r in rows if "gather_meshes_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\ngather_meshes_kernel, from rocprofv3 --kernel-trace (a run of its own, --device-only); grid = tiles of 4096 floats; bytes = 8 per float gathered\n")
    out.write("%-10s %6s %10s %10s %10s %12s %10s\n" % ("tiles", "calls", "median_us", "min_us", "max_us", "GB/s", "of 8 TB/s"))
    groups = {}
    for r in rows:
        tiles = int(r.get("Grid_Size_X") or r["Grid_Size"]) // int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
        groups.setdefault(tiles, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for tiles, us in sorted(groups.items()):
        gbs = tiles * 4096 * 8 / (np.median(us) * 1e-6) / 1e9  # (the last tile is partial: an upper bound by less than one tile)
        out.write("%-10d %6d %10.1f %10.1f %10.1f %12.0f %9.1f%%\n" % (tiles, len(us), np.median(us), min(us), max(us), gbs, gbs / 80.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="220,620")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help="the device-output calls alone (under the profiler)")
    ap.add_argument("--summarize-trace", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a)

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    from tests.common import same_bits
    dev = torch.device("cuda:0")
    gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    color = torch.from_numpy(synth.render_color(W, H, 3)).to(dev)
    marks = sorted(int(v) for v in a.frames.split(","))
    res = {"voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "warmup": a.warmup, "maps": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        e.record()  # (creates the hipEvent_t the map records below)
    torch.cuda.synchronize()
    done = 0
    for mark in marks:
        batch = []
        for depth, pose in synth.stream("sphere_room", mark - done, W, H, start=done):
            batch.append((torch.from_numpy(depth).to(dev), pose, cam))
            if len(batch) == 10:
                gm.IntegrateBatch(integ, batch, [(color, p, cam) for _, p, _ in batch])
                gm.UpdateMeshes(force=True)  # the reference's keyframe cadence (Chisel.cpp:54)
                batch = []
        assert not batch, "--frames: multiples of 10"
        done = mark
        gm.synchronize()
        size = gm.GatherMeshesSize()
        V, G = size["vertices"], size["grids"]
        floats = 9 * V + 3 * G
        r = {"chunks": gm.NumChunks(), "totals": size, "floats": floats, "MB": round(floats * 4 / 1e6, 1)}

        def walk():
            ids = gm.GetMeshIDs()
            return ids, [gm.GetMesh(tuple(c)) for c in ids.tolist()]

        out = {n: torch.empty((G if n == "grids" else V, WIDTH[n]), dtype=torch.float32, device=dev) for n in NAMES}
        out_rgba = dict(out, rgba=torch.empty((V, 4), dtype=torch.float32, device=dev))
        only_rgba = {"rgba": out_rgba["rgba"]}

        def device_us(call):
            gm.record_event(ev[0].cuda_event)
            call()
            gm.record_event(ev[1].cuda_event)
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3

        t = {k: [] for k in ("walk", "host", "enqueue", "device_wall", "rgba_same_launch", "without_rgba", "rgba_alone")}
        if not a.device_only:
            t0 = time.perf_counter()
            ids, meshes = walk()  # the first walk after the recompute: every live arena is copied to the host
            r["walk_first_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            got = gm.GatherMeshes()
            for n in NAMES:  # the same data, bit for bit
                same_bits(got[n], np.concatenate([m[n] for m in meshes]) if meshes else np.zeros((0, 3), np.float32), n)
            assert np.array_equal(got["ids"], ids)
        for i in range(a.warmup + a.iters):
            keep = i >= a.warmup
            if not a.device_only:
                t0 = time.perf_counter()
                walk()
                t1 = time.perf_counter()
                gm.GatherMeshes()
                t2 = time.perf_counter()
                gm.GatherMeshes(out=out)
                t3 = time.perf_counter()
                gm.synchronize()
                t4 = time.perf_counter()
                if keep:
                    t["walk"].append((t1 - t0) * 1e6); t["host"].append((t2 - t1) * 1e6); t["enqueue"].append((t3 - t2) * 1e6); t["device_wall"].append((t4 - t2) * 1e6)
            for key, o in (("rgba_same_launch", out_rgba), ("without_rgba", out), ("rgba_alone", only_rgba)):
                us = device_us(lambda: gm.GatherMeshes(out=o))
                if keep:
                    t[key].append(us)
        r.update({k: stats(v) for k, v in t.items() if v})
        if not a.device_only:
            r["walk_over_host"] = round(r["walk"]["median"] / r["host"]["median"], 2)
            r["walk_first_over_host"] = round(r["walk_first_us"] / r["host"]["median"], 2)
            r["walk_over_device_wall"] = round(r["walk"]["median"] / r["device_wall"]["median"], 2)
        res["maps"]["frames 0-%d" % (mark - 1)] = r
    line = json.dumps(res)
    print(line)
    if a.out and not a.device_only:
        with open(a.out, "w") as f:
            f.write("python tools/mesh_gather_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour, 1 cm\n"
                    "voxels, 16^3 chunks, UpdateMeshes every 10 frames -- after the frames named; %d warm-up + %d timed rounds per map, the walk, the host\n"
                    "gather and the device gathers alternating in one process; microseconds, median and p10-p90; walk / host / enqueue / device_wall are\n"
                    "host wall times, the others hipEvent times over the map's stream around one Chisel.GatherMeshes(out=...) call, size call included)\n\n"
                    % (a.warmup, a.iters))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
