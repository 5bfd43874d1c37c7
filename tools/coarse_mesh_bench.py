#!/usr/bin/env python3
"""Time chisel_hip_coarse_mesh on the maps of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3
chunks, InverseTruncator(1), carving 0.05 m, UpdateMeshes every 10 frames): after frames 0-219 (the default window's map) and after
frames 0-619 (the late window's) -- the maps of tools/mesh_gather_bench.py.

    python tools/coarse_mesh_bench.py [--frames 220,620 --iters 15 --warmup 3 --out profiles/coarse_mesh_bench.txt]

Per map, in one process, every timed region fenced by a synchronise on both sides; wall time in microseconds (median, p10-p90):
  stride 1, 2, 4   Chisel.CoarseMesh(s, out=...) into torch tensors (vertices, gradient normals, colours) of every resident chunk:
                   `host` is the time in the call (the listing, the count and the one wait for the totals; emit and shade are only
                   queued), `wall` the time until a synchronise behind it returns; vertices and bytes (36 per vertex)
  yardstick        what the map offers for the same purpose without the entry: UpdateMeshes(force) + GatherMeshes(out=...) into
                   torch tensors (vertices, normals, colours, grids), until a synchronise returns; its bytes.  Nothing is due for
                   meshing at that point (the stream's last frames were followed by a recompute), so this is the gather of meshes
                   that exist
  remesh_all       UpdateMeshesOf(every resident chunk) + GatherMeshes(out=...): the mesher's two kernels over the chunks a coarse
                   mesh at stride 1 walks, then the gather

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/coarse_mesh_bench.py --device-only` and then `python tools/coarse_mesh_bench.py --summarize-trace DIR --out
profiles/coarse_mesh_bench.txt`, which appends the table (same --frames, --iters, --warmup in both)."""
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
STRIDES = (1, 2, 4)
COARSE_KERNELS = ("coarse_count_kernel", "coarse_scan_kernel", "coarse_emit_kernel", "shade_vertices_kernel")
MESHER_KERNELS = ("mesh_count_kernel", "mesh_triangle_kernel", "gather_meshes_kernel")


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1), "p90": round(float(np.percentile(us, 90)), 1)}


def summarize_trace(a):
    """the run's order: per map the strides in turn, warmup + iters calls each, then warmup + iters of remesh_all, then the yardsticks"""
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    named = lambda name: [r for r in rows if name in r["Kernel_Name"]]
    rounds, marks = a.warmup + a.iters, [int(v) for v in a.frames.split(",")]
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nkernel times from rocprofv3 --kernel-trace (a run of its own, --device-only), microseconds, median (min - max) over %d calls\n" % a.iters)
    out.write("%-14s %-10s %-24s %10s %10s %10s\n" % ("map", "call", "kernel", "median_us", "min_us", "max_us"))
    counts = named("coarse_count_kernel")
    # (count and scan also run once for the size query in front of every stride's calls)
    assert len(counts) == len(marks) * len(STRIDES) * (rounds + 1), "the trace does not hold the device-only run of these arguments (%d count launches)" % len(counts)
    for m, mark in enumerate(marks):
        last = 0
        for k, s in enumerate(STRIDES):
            for name in COARSE_KERNELS:
                per = rounds + 1 if name in COARSE_KERNELS[:2] else rounds
                block = named(name)[(m * len(STRIDES) + k) * per:(m * len(STRIDES) + k + 1) * per][per - rounds + a.warmup:]
                t = [us(r) for r in block]
                last = max([last] + [int(r["End_Timestamp"]) for r in block])
                out.write("%-14s %-10s %-24s %10.1f %10.1f %10.1f\n" % ("frames 0-%d" % (mark - 1), "stride %d" % s, name, np.median(t), min(t), max(t)))
        for name in MESHER_KERNELS:
            block = [r for r in named(name) if int(r["Start_Timestamp"]) > last][:rounds][a.warmup:]
            t = [us(r) for r in block]
            out.write("%-14s %-10s %-24s %10.1f %10.1f %10.1f\n" % ("frames 0-%d" % (mark - 1), "remesh_all", name, np.median(t), min(t), max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="220,620")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help="the calls alone, without the host clock's bookkeeping (under the profiler)")
    ap.add_argument("--summarize-trace", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a)

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    dev = torch.device("cuda:0")
    gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    color = torch.from_numpy(synth.render_color(W, H, 3)).to(dev)
    marks = sorted(int(v) for v in a.frames.split(","))
    res = {"voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "warmup": a.warmup, "maps": {}}
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
        r = {"chunks": gm.NumChunks()}
        print("map after frames 0-%d: %d chunks" % (mark - 1, r["chunks"]), file=sys.stderr, flush=True)
        for s in STRIDES:
            size = gm.CoarseMeshSize(s)
            V = size["vertices"]
            out = {n: torch.empty((V, 3), dtype=torch.float32, device=dev) for n in ("vertices", "normals", "colors")}
            host, wall = [], []
            for i in range(a.warmup + a.iters):
                gm.synchronize()
                t0 = time.perf_counter()
                got = gm.CoarseMesh(s, out=out)
                t1 = time.perf_counter()
                gm.synchronize()
                t2 = time.perf_counter()
                assert got["totals"] == size
                if i >= a.warmup:
                    host.append((t1 - t0) * 1e6); wall.append((t2 - t0) * 1e6)
            r["stride %d" % s] = {"totals": size, "MB": round(V * 36 / 1e6, 2), "host": stats(host), "wall": stats(wall)}
        size = gm.GatherMeshesSize()
        V, G = size["vertices"], size["grids"]
        gout = {n: torch.empty((G if n == "grids" else V, 3), dtype=torch.float32, device=dev) for n in ("vertices", "normals", "colors", "grids")}
        ids = gm.GetChunkIDs()
        for key, remesh in (("remesh_all", lambda: gm.UpdateMeshesOf(ids)), ("yardstick", lambda: gm.UpdateMeshes(force=True))):
            wall = []
            for i in range(a.warmup + a.iters):
                gm.synchronize()
                t0 = time.perf_counter()
                remesh()
                gm.GatherMeshes(out=gout)
                gm.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    wall.append((t1 - t0) * 1e6)
            now = gm.GatherMeshesSize()
            assert (now["vertices"], now["grids"]) == (V, G)
            r[key] = {"totals": now, "MB": round((9 * V + 3 * G) * 4 / 1e6, 2), "wall": stats(wall)}
        r["stride_1_wall_over_remesh_all"] = round(r["stride 1"]["wall"]["median"] / r["remesh_all"]["wall"]["median"], 2)
        for s in STRIDES[1:]:
            r["stride %d" % s]["bytes_of_stride_1"] = round(r["stride %d" % s]["totals"]["vertices"] / max(r["stride 1"]["totals"]["vertices"], 1), 4)
        r["stride_1_wall_over_yardstick"] = round(r["stride 1"]["wall"]["median"] / r["yardstick"]["wall"]["median"], 2)
        res["maps"]["frames 0-%d" % (mark - 1)] = r
    line = json.dumps(res)
    print(line)
    if a.out and not a.device_only:
        with open(a.out, "w") as f:
            f.write("python tools/coarse_mesh_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour, 1 cm\n"
                    "voxels, 16^3 chunks, UpdateMeshes every 10 frames -- after the frames named; %d warm-up + %d timed calls per figure, a synchronise on\n"
                    "both sides of every timed region; microseconds, median and p10-p90 of host wall times.  stride s: Chisel.CoarseMesh(s, out=...) of\n"
                    "every resident chunk into device tensors (vertices, gradient normals, colours: 36 bytes a vertex) -- host: the time in the call, wall:\n"
                    "until a synchronise behind it returns.  yardstick: UpdateMeshes(force) + GatherMeshes(out=...) into device tensors until a synchronise\n"
                    "returns.)\n\n" % (a.warmup, a.iters))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
