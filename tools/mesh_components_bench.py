#!/usr/bin/env python3
"""Time chisel_hip_mesh_components and chisel_hip_filter_mesh on the maps of bench.py's default stream (sphere_room, 640 x 480 depth +
colour, 1 cm voxels, 16^3 chunks, InverseTruncator(1), carving 0.05 m, UpdateMeshes every 10 frames): after frames 0-219 (the default
window's map) and after frames 0-619 (the late window's) -- the maps of tools/indexed_mesh_bench.py.

    python tools/mesh_components_bench.py [--frames 220,620 --iters 10 --warmup 2 --out profiles/mesh_components_bench.txt]

Per map and stride (1, 2, 4), in one process, every timed region fenced by a synchronise on both sides; wall time in microseconds
(median, p10-p90):
  indexed     Chisel.IndexedMesh(s, out=...) into torch tensors (vertices, indices, gradient normals, colours): the mesh the other
              rows work on, left on the device
  components  Chisel.MeshComponents(indices tensor, V, out=...): both label arrays on the device, table and totals on the host
  filter      Chisel.FilterMesh(mesh, min_triangles=64, out=...): vertices, indices, normals, colours and both maps on the device
              (`host` is the time in the call -- everything up to the one wait for the totals; the rest is only queued --, `wall` the
              time until a synchronise behind it returns)
  before      what a caller had before these entries: Chisel.IndexedMesh(s) into host arrays, scipy.sparse.csgraph's
              connected_components on the triangles' sides, numpy masks and a renumbering for the same threshold -- wall time, the
              mesh left on the host (the upload a caller who wants it in HBM pays is not in it)
and what was found: components, the largest one's share of the triangles, what a threshold of 64 triangles removes.

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/mesh_components_bench.py --device-only` and then `python tools/mesh_components_bench.py --summarize-trace DIR --out
profiles/mesh_components_bench.txt`, which appends the table (same --frames, --iters, --warmup in both)."""
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
MIN_TRIANGLES = 64
# (kernel, template argument or None, launches per MeshComponents call, launches per FilterMesh call)
KERNELS = (("components_init_kernel", None, 1, 1), ("components_hook_kernel", None, 1, 1), ("components_label_vertices_kernel", None, 1, 1),
           ("components_label_triangles_kernel", None, 1, 1), ("components_sums_kernel", 0, 1, 1), ("components_sums_kernel", 1, 0, 1),
           ("components_sums_kernel", 2, 0, 1), ("components_scan_sums_kernel", None, 1, 3), ("components_prefix_kernel", 0, 1, 1),
           ("components_prefix_kernel", 1, 0, 1), ("components_prefix_kernel", 2, 0, 1), ("report_words_kernel", None, 1, 1),
           ("components_write_vertices_kernel", None, 1, 0), ("components_write_triangles_kernel", None, 1, 0),
           ("components_write_table_kernel", None, 1, 0), ("filter_vertices_kernel", None, 0, 1), ("filter_triangles_kernel", None, 0, 1))


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1), "p90": round(float(np.percentile(us, 90)), 1)}


def summarize_trace(a):
    """the run's order: per map the strides in turn; per stride warmup + iters MeshComponents calls, then warmup + iters FilterMesh
    calls.  A kernel's figure is the sum of its launches in one call (the scan over the tile sums runs three times in a filter)."""
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    def named(name, arg):
        hit = lambda k: name in k and (arg is None or "<%d>" % arg in k or "ILi%dE" % arg in k)
        return [r for r in rows if hit(r["Kernel_Name"])]

    rounds, marks = a.warmup + a.iters, [int(v) for v in a.frames.split(",")]
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nkernel times from rocprofv3 --kernel-trace (a run of its own, --device-only), microseconds per call (a kernel's launches in one call\n"
              "summed), median (min - max) over %d calls\n" % a.iters)
    out.write("%-14s %-10s %-12s %-40s %10s %10s %10s\n" % ("map", "stride", "entry", "kernel", "median_us", "min_us", "max_us"))
    hooks = named("components_hook_kernel", None)
    assert len(hooks) == len(marks) * len(STRIDES) * 2 * rounds, "the trace does not hold the device-only run of these arguments (%d hook launches)" % len(hooks)
    for m in range(len(marks)):
        for k in range(len(STRIDES)):
            at = m * len(STRIDES) + k
            for entry, col in (("components", 2), ("filter", 3)):
                total = 0.0
                for kernel in KERNELS:
                    name, arg, per = kernel[0], kernel[1], kernel[col]
                    if per == 0:
                        continue
                    block_len = rounds * (kernel[2] + kernel[3])
                    block = named(name, arg)[at * block_len:(at + 1) * block_len]
                    mine = block[:rounds * kernel[2]] if entry == "components" else block[rounds * kernel[2]:]
                    calls = [sum(us(r) for r in mine[i * per:(i + 1) * per]) for i in range(a.warmup, rounds)]
                    label = name + ("<%d>" % arg if arg is not None else "") + (" x %d" % per if per > 1 else "")
                    out.write("%-14s %-10s %-12s %-40s %10.1f %10.1f %10.1f\n" % ("frames 0-%d" % (marks[m] - 1), "stride %d" % STRIDES[k], entry, label, np.median(calls),
                                                                                  min(calls), max(calls)))
                    total += float(np.median(calls))
                out.write("%-14s %-10s %-12s %-40s %10.1f\n" % ("frames 0-%d" % (marks[m] - 1), "stride %d" % STRIDES[k], entry, "sum of medians", total))


def before(gm, s):
    """the caller's way before these entries -> (kept vertices, kept triangles, components, the largest one's triangles)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    mesh = gm.IndexedMesh(s)
    idx, V = mesh["indices"], len(mesh["vertices"])
    u = np.concatenate([idx[:, 0], idx[:, 0]])
    w = np.concatenate([idx[:, 1], idx[:, 2]])
    n, label = connected_components(sp.coo_matrix((np.ones(len(u), np.int8), (u, w)), shape=(V, V)).tocsr(), directed=False)
    counts = np.bincount(label[idx[:, 0]], minlength=n)
    keep_v = counts[label] >= MIN_TRIANGLES
    keep_t = keep_v[idx[:, 0]]
    renumber = np.cumsum(keep_v, dtype=np.int32) - 1
    clean = {"vertices": mesh["vertices"][keep_v], "normals": mesh["normals"][keep_v], "colors": mesh["colors"][keep_v], "indices": renumber[idx[keep_t]]}
    return len(clean["vertices"]), len(clean["indices"]), int(n), int(counts.max()) if n else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="220,620")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help="the two entries' calls alone (under the profiler)")
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
    res = {"voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "warmup": a.warmup, "min_triangles": MIN_TRIANGLES, "maps": {}}
    done = 0

    def timed(call, check=None):
        host, wall = [], []
        for i in range(a.warmup + a.iters):
            gm.synchronize()
            t0 = time.perf_counter()
            got = call()
            t1 = time.perf_counter()
            gm.synchronize()
            t2 = time.perf_counter()
            if check is not None:
                check(got)
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
            size = gm.IndexedMeshSize(s)
            V, T = size["vertices"], size["triangles"]
            mesh_out = {n: torch.empty((V, 3), dtype=torch.float32, device=dev) for n in ("vertices", "normals", "colors")}
            mesh_out["indices"] = torch.empty((T, 3), dtype=torch.int32, device=dev)
            labels = {"vertex_component": torch.empty(V, dtype=torch.int32, device=dev), "triangle_component": torch.empty(T, dtype=torch.int32, device=dev)}
            out = {n: torch.empty_like(t) for n, t in mesh_out.items()}
            out.update(vertex_map=torch.empty(V, dtype=torch.int32, device=dev), triangle_map=torch.empty(T, dtype=torch.int32, device=dev))
            if a.device_only:
                mesh = gm.IndexedMesh(s, out=mesh_out)
                for _ in range(a.warmup + a.iters):
                    comp = gm.MeshComponents(mesh_out["indices"], n_vertices=V, out=labels)
                for _ in range(a.warmup + a.iters):
                    kept = gm.FilterMesh(mesh, MIN_TRIANGLES, out=out)
                gm.synchronize()
                continue
            indexed = timed(lambda: gm.IndexedMesh(s, out=mesh_out))
            mesh = gm.IndexedMesh(s, out=mesh_out)
            components = timed(lambda: gm.MeshComponents(mesh_out["indices"], n_vertices=V, out=labels))
            comp = gm.MeshComponents(mesh_out["indices"], n_vertices=V, out=labels)
            filtered = timed(lambda: gm.FilterMesh(mesh, MIN_TRIANGLES, out=out))
            kept = gm.FilterMesh(mesh, MIN_TRIANGLES, out=out)
            gm.synchronize()
            t = kept["totals"]
            assert comp["totals"]["components"] == t["components"] == len(comp["table"]) and t["invalid_triangles"] == 0
            found = []
            host_way = timed(lambda: before(gm, s), found.append)
            assert all(f == (t["kept_vertices"], t["kept_triangles"], t["components"], t["largest_triangles"]) for f in found), (found[0], t)
            with_triangles = int((comp["table"][:, 2] > 0).sum())
            r["stride %d" % s] = {
                "indexed": indexed, "components": components, "filter": filtered, "before": {"wall": host_way["wall"]},
                "totals": t, "components_with_triangles": with_triangles,
                "largest_share_of_triangles": round(t["largest_triangles"] / max(T, 1), 4),
                "removed_at_%d" % MIN_TRIANGLES: {"components": with_triangles - t["kept_components"], "vertices": V - t["kept_vertices"], "triangles": T - t["kept_triangles"]},
                "MB_in": round((36 * V + 12 * T) / 1e6, 2),
                "filter_wall_over_indexed": round(filtered["wall"]["median"] / indexed["wall"]["median"], 2),
                "before_over_indexed_plus_filter": round(host_way["wall"]["median"] / (indexed["wall"]["median"] + filtered["wall"]["median"]), 1)}
            del mesh_out, labels, out
        res["maps"]["frames 0-%d" % (mark - 1)] = r
    if a.device_only:
        return
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("python tools/mesh_components_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour,\n"
                    "1 cm voxels, 16^3 chunks, UpdateMeshes every 10 frames -- after the frames named; %d warm-up + %d timed calls per figure, a\n"
                    "synchronise on both sides of every timed region; microseconds, median and p10-p90 of host wall times.  indexed:\n"
                    "Chisel.IndexedMesh(s, out=...) into device tensors; components: Chisel.MeshComponents on its index tensor, labels into device\n"
                    "tensors; filter: Chisel.FilterMesh(mesh, %d, out=...) into device tensors -- host: the time in the call, wall: until a\n"
                    "synchronise behind it returns; before: IndexedMesh into host arrays + scipy.sparse.csgraph.connected_components + numpy masks\n"
                    "for the same threshold, in the same run.)\n\n" % (a.warmup, a.iters, MIN_TRIANGLES))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
