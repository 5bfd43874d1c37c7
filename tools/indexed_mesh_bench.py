#!/usr/bin/env python3
"""Time chisel_hip_indexed_mesh beside chisel_hip_coarse_mesh on the maps of bench.py's default stream (sphere_room, 640 x 480 depth +
colour, 1 cm voxels, 16^3 chunks, InverseTruncator(1), carving 0.05 m, UpdateMeshes every 10 frames): after frames 0-219 (the default
window's map) and after frames 0-619 (the late window's) -- the maps of tools/coarse_mesh_bench.py.

    python tools/indexed_mesh_bench.py [--frames 220,620 --iters 10 --warmup 2 --out profiles/indexed_mesh_bench.txt]

Per map and stride (1, 2, 4), in one process, every timed region fenced by a synchronise on both sides; wall time in microseconds
(median, p10-p90):
  indexed   Chisel.IndexedMesh(s, out=...) into torch tensors (vertices, indices, gradient normals, colours) of every resident chunk:
            `host` is the time in the call (the listing, mark / rows / scan and the one wait for the totals; the rest is only
            queued), `wall` the time until a synchronise behind it returns; vertices, triangles and bytes (36 a vertex + 12 a triangle)
  coarse    Chisel.CoarseMesh(s, out=...) into torch tensors (vertices, gradient normals, colours) in the same run: the same triangles
            as a soup, 108 bytes each

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/indexed_mesh_bench.py --device-only` and then `python tools/indexed_mesh_bench.py --summarize-trace DIR --out
profiles/indexed_mesh_bench.txt`, which appends the table (same --frames, --iters, --warmup in both)."""
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
# (kernel, launches per call that is a size query, launches per full call)
INDEXED_KERNELS = (("indexed_owner_kernel", 1, 1), ("indexed_mark_kernel", 1, 1), ("indexed_rows_kernel", 1, 1), ("indexed_scan_kernel", 1, 1),
                   ("indexed_vertex_kernel", 0, 1), ("indexed_index_kernel", 0, 1))
COARSE_KERNELS = (("coarse_count_kernel", 1, 1), ("coarse_scan_kernel", 1, 1), ("coarse_emit_kernel", 0, 1))


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1), "p90": round(float(np.percentile(us, 90)), 1)}


def summarize_trace(a):
    """the run's order: per map the strides in turn; per stride one size query of each entry, then warmup + iters coarse calls, then
    warmup + iters indexed calls.  The shade kernel runs once per full call of either entry."""
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    named = lambda name: [r for r in rows if name in r["Kernel_Name"]]
    rounds, marks = a.warmup + a.iters, [int(v) for v in a.frames.split(",")]
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nkernel times from rocprofv3 --kernel-trace (a run of its own, --device-only), microseconds, median (min - max) over %d calls\n" % a.iters)
    out.write("%-14s %-10s %-28s %10s %10s %10s\n" % ("map", "stride", "kernel", "median_us", "min_us", "max_us"))
    marks_launched = named("indexed_mark_kernel")
    assert len(marks_launched) == len(marks) * len(STRIDES) * (rounds + 1), "the trace does not hold the device-only run of these arguments (%d mark launches)" % len(marks_launched)

    def line(m, k, label, block):
        t = [us(r) for r in block]
        out.write("%-14s %-10s %-28s %10.1f %10.1f %10.1f\n" % ("frames 0-%d" % (marks[m] - 1), "stride %d" % STRIDES[k], label, np.median(t), min(t), max(t)))
        return float(np.median(t))

    for m in range(len(marks)):
        for k in range(len(STRIDES)):
            at = m * len(STRIDES) + k
            sums = {}
            for entry, kernels in (("coarse", COARSE_KERNELS), ("indexed", INDEXED_KERNELS)):
                total = 0.0
                for name, in_query, _ in kernels:
                    per = rounds + in_query
                    total += line(m, k, name, named(name)[at * per:(at + 1) * per][in_query + a.warmup:])
                shade = named("shade_vertices_kernel")[at * 2 * rounds:(at + 1) * 2 * rounds]
                total += line(m, k, "shade_vertices_kernel (%s)" % entry, (shade[:rounds] if entry == "coarse" else shade[rounds:])[a.warmup:])
                sums[entry] = total
            out.write("%-14s %-10s %-28s %10.1f   (coarse %.1f)\n" % ("frames 0-%d" % (marks[m] - 1), "stride %d" % STRIDES[k], "sum of medians, indexed", sums["indexed"], sums["coarse"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="220,620")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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

    def timed(call, want):
        host, wall = [], []
        for i in range(a.warmup + a.iters):
            gm.synchronize()
            t0 = time.perf_counter()
            got = call()
            t1 = time.perf_counter()
            gm.synchronize()
            t2 = time.perf_counter()
            assert got["totals"] == want
            if i >= a.warmup:
                host.append((t1 - t0) * 1e6); wall.append((t2 - t0) * 1e6)
        return {"host": stats(host), "wall": stats(wall)}

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
            soup = gm.CoarseMeshSize(s)
            size = gm.IndexedMeshSize(s)
            V, T = size["vertices"], size["triangles"]
            assert soup["vertices"] == 3 * T and soup["cubes_meshed"] == size["cubes_meshed"]
            cout = {n: torch.empty((3 * T, 3), dtype=torch.float32, device=dev) for n in ("vertices", "normals", "colors")}
            out = {n: torch.empty((V, 3), dtype=torch.float32, device=dev) for n in ("vertices", "normals", "colors")}
            out["indices"] = torch.empty((T, 3), dtype=torch.int32, device=dev)
            coarse = timed(lambda: gm.CoarseMesh(s, out=cout), soup)
            indexed = timed(lambda: gm.IndexedMesh(s, out=out), size)
            idx = out["indices"]
            assert int(idx.min()) == 0 and int(idx.max()) == V - 1
            coarse.update(totals=soup, MB=round(3 * T * 36 / 1e6, 2))
            indexed.update(totals=size, MB=round((36 * V + 12 * T) / 1e6, 2), bytes_per_triangle=round((36 * V + 12 * T) / max(T, 1), 1),
                           bytes_of_coarse=round((36 * V + 12 * T) / max(108 * T, 1), 3),
                           wall_over_coarse=round(indexed["wall"]["median"] / coarse["wall"]["median"], 2))
            r["stride %d" % s] = {"indexed": indexed, "coarse": coarse}
            del cout, out
        res["maps"]["frames 0-%d" % (mark - 1)] = r
    line = json.dumps(res)
    print(line)
    if a.out and not a.device_only:
        with open(a.out, "w") as f:
            f.write("python tools/indexed_mesh_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour, 1 cm\n"
                    "voxels, 16^3 chunks, UpdateMeshes every 10 frames -- after the frames named; %d warm-up + %d timed calls per figure, a synchronise on\n"
                    "both sides of every timed region; microseconds, median and p10-p90 of host wall times.  indexed: Chisel.IndexedMesh(s, out=...) of\n"
                    "every resident chunk into device tensors (vertices, indices, gradient normals, colours: 36 bytes a vertex + 12 a triangle); coarse:\n"
                    "Chisel.CoarseMesh(s, out=...) in the same run (vertices, gradient normals, colours: 108 bytes a triangle) -- host: the time in the\n"
                    "call, wall: until a synchronise behind it returns.)\n\n" % (a.warmup, a.iters))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
