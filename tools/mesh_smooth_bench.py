#!/usr/bin/env python3
"""Time chisel_hip_mesh_adjacency, chisel_hip_mesh_vertex_normals and chisel_hip_smooth_mesh on the maps of bench.py's default stream
(sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3 chunks, InverseTruncator(1), carving 0.05 m, UpdateMeshes every 10 frames):
after frames 0-219 (the default window's map) and after frames 0-619 (the late window's) -- the maps of tools/mesh_components_bench.py.

    python tools/mesh_smooth_bench.py [--frames 220,620 --iters 10 --warmup 2 --out profiles/mesh_smooth_bench.txt]

Per map and stride (1, 2, 4), in one process, every timed region fenced by a synchronise on both sides; wall time in microseconds
(median, p10-p90):
  indexed     Chisel.IndexedMesh(s, out=...) into torch tensors (vertices, indices, gradient normals, colours): the mesh the other
              rows work on, left on the device
  filter      Chisel.FilterMesh(mesh, 64, out=...), for scale
  adjacency   Chisel.MeshAdjacency(indices tensor, V, out=...): both offset arrays, both item arrays (3 T and 6 T ints of room) and
              the flags on the device
  normals     Chisel.MeshVertexNormals(mesh, out=...)
  smooth      Chisel.SmoothMesh(mesh, 10, out=...): 20 passes, vertices and their normals on the device
              (`host` is the time in the call -- everything up to the one wait for the totals; the rest is only queued --, `wall` the
              time until a synchronise behind it returns)
  before      what a caller had before these entries: Chisel.IndexedMesh(s) into host arrays, the incidence and the neighbour matrix
              as scipy.sparse CSR, area-weighted normals by numpy's scatter-add, and 10 Taubin iterations as sparse products with the
              same pins -- wall time, everything left on the host
and what was found: the totals, and how far the host way's floats are from the device's (the host way's sums have another order).

A second, small part (--sphere) measures on the sphere of tests/indexed_mesh_restated.py the largest angle to the radial direction of the
gradient normals IndexedMesh gives and of the vertex normals, at strides 1, 2, 4.

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/mesh_smooth_bench.py --device-only` and then `python tools/mesh_smooth_bench.py --summarize-trace DIR --out
profiles/mesh_smooth_bench.txt`, which appends the table (same --frames, --iters, --warmup in both)."""
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
ITERATIONS, LAM, MU, PIN = 10, 0.5, -0.53, 3
ENTRIES = ("adjacency", "normals", "smooth")
KERNELS = ("adjacency_count_kernel", "adjacency_sums_kernel", "adjacency_scan_sums_kernel", "adjacency_prefix_kernel", "adjacency_fill_kernel",
           "adjacency_rows_kernel", "report_words_kernel", "adjacency_compact_kernel", "mesh_vertex_normals_kernel", "mesh_smooth_pass_kernel")


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1), "p90": round(float(np.percentile(us, 90)), 1)}


def summarize_trace(a):
    """the run's order: per map the strides in turn; per stride warmup + iters calls of each entry in turn.  Every call launches the
    count kernel once, first: the launches from one count kernel to the next are one call's.  A kernel's figure is the sum of its
    launches in one call (the scan kernels run twice, the pass kernel 20 times in a smoothing)."""
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    calls = []
    for r in rows:
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        if name == "adjacency_count_kernel":
            calls.append({})
        if calls:
            one = calls[-1].setdefault(name, [0, 0.0])
            one[0] += 1
            one[1] += us(r)
    rounds, marks = a.warmup + a.iters, [int(v) for v in a.frames.split(",")]
    assert len(calls) == len(marks) * len(STRIDES) * len(ENTRIES) * rounds, "the trace does not hold the device-only run of these arguments (%d calls)" % len(calls)
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nkernel times from rocprofv3 --kernel-trace (a run of its own, --device-only), microseconds per call (a kernel's launches in one call\n"
              "summed), median (min - max) over %d calls\n" % a.iters)
    out.write("%-14s %-10s %-10s %-36s %10s %10s %10s\n" % ("map", "stride", "entry", "kernel", "median_us", "min_us", "max_us"))
    at = 0
    for mark in marks:
        for s in STRIDES:
            for entry in ENTRIES:
                mine = calls[at + a.warmup:at + rounds]
                at += rounds
                total = 0.0
                for name in KERNELS:
                    if name not in mine[0]:
                        continue
                    t = [c[name][1] for c in mine]
                    label = name + (" x %d" % mine[0][name][0] if mine[0][name][0] > 1 else "")
                    out.write("%-14s %-10s %-10s %-36s %10.1f %10.1f %10.1f\n" % ("frames 0-%d" % (mark - 1), "stride %d" % s, entry, label, np.median(t), min(t), max(t)))
                    total += float(np.median(t))
                out.write("%-14s %-10s %-10s %-36s %10.1f\n" % ("frames 0-%d" % (mark - 1), "stride %d" % s, entry, "sum of medians", total))


def before(gm, s):
    """the caller's way before these entries -> (flags, normals, smoothed vertices, normals of the smoothed), numpy"""
    import scipy.sparse as sp
    mesh = gm.IndexedMesh(s)
    idx, P = mesh["indices"].astype(np.int64), mesh["vertices"]
    V, T = len(P), len(idx)
    t = np.repeat(np.arange(T), 3)
    incidence = sp.coo_matrix((np.ones(3 * T, np.int32), (idx.reshape(-1), t)), shape=(V, T)).tocsr()
    incidence.sort_indices()
    a = np.concatenate([idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 1], idx[:, 2], idx[:, 0]])
    b = np.concatenate([idx[:, 1], idx[:, 2], idx[:, 0], idx[:, 0], idx[:, 1], idx[:, 2]])
    nbr = sp.coo_matrix((np.ones(len(a), np.int32), (a, b)), shape=(V, V)).tocsr()  # (data: c(v, u); the device's meshes repeat no id in a triangle)
    nbr.sort_indices()
    flags = np.zeros(V, np.int32)
    row = np.repeat(np.arange(V), np.diff(nbr.indptr))
    flags[np.unique(row[nbr.data == 1])] |= 1
    flags[np.unique(row[nbr.data > 2])] |= 2
    flags[np.diff(incidence.indptr) == 0] |= 4

    def normals(Q):
        n = np.cross(Q[idx[:, 1]] - Q[idx[:, 0]], Q[idx[:, 2]] - Q[idx[:, 0]])
        acc = np.zeros((V, 3), np.float32)
        for k in range(3):
            np.add.at(acc, idx[:, k], n)
        length = np.sqrt((acc * acc).sum(1, dtype=np.float32))
        return np.where(length[:, None] > 0, acc / np.where(length > 0, length, 1)[:, None], 0).astype(np.float32)

    ones = nbr.copy()
    ones.data = np.ones(len(ones.data), np.float32)
    count = np.diff(nbr.indptr).astype(np.float32)
    moves = ((flags & PIN) == 0) & (count > 0)
    Q = P.copy()
    for _ in range(ITERATIONS):
        for f in (LAM, MU):
            mean = (ones @ Q) / np.where(count > 0, count, 1)[:, None]
            Q = np.where(moves[:, None], Q + np.float32(f) * (mean - Q), Q).astype(np.float32)
    return flags, normals(P), Q, normals(Q)


def sphere_part(out):
    """gradient normals against vertex normals on a sphere of radius 9.6 voxels (tests/indexed_mesh_restated.py's), 8^3 chunks"""
    from cvids_amd.chisel import Chisel
    from tests import indexed_mesh_restated as ir
    from tests.common import upload
    N, B, radius, centre, res = 8, 4, 9.6, (15.3, 16.1, 15.7), 0.03
    m = Chisel((N, N, N), res, True, max_chunks=128)
    upload(m, ir.sphere(N, B, radius, centre, res))
    c = (np.array(centre, np.float64) + 0.5) * res  # (a voxel's value belongs to its centre)
    lines = {}
    for s in STRIDES:
        mesh = m.IndexedMesh(s)
        radial = mesh["vertices"].astype(np.float64) - c
        radial /= np.linalg.norm(radial, axis=1)[:, None]

        def angle(n):
            n = n.astype(np.float64)
            length = np.linalg.norm(n, axis=1)
            cos = (n * radial).sum(1) / np.where(length > 0, length, 1)
            return np.degrees(np.arccos(np.clip(cos, -1, 1))), int((length == 0).sum())
        (g, g0), (v, v0) = angle(mesh["normals"]), angle(m.MeshVertexNormals(mesh))
        lines["stride %d" % s] = {"vertices": len(radial), "gradient_normals_max_deg": round(float(g.max()), 2), "gradient_normals_mean_deg": round(float(g.mean()), 2),
                                  "gradient_normals_zero": g0, "vertex_normals_max_deg": round(float(v.max()), 2), "vertex_normals_mean_deg": round(float(v.mean()), 2),
                                  "vertex_normals_zero": v0}
    m.close()
    out["sphere_radius_9.6_voxels"] = lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="220,620")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help="the three entries' calls alone (under the profiler)")
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
    res = {"voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "warmup": a.warmup, "iterations": ITERATIONS, "lambda": LAM, "mu": MU, "pin": PIN, "maps": {}}
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
            rows = {"tri_offsets": V + 1, "tri_items": 3 * T, "nbr_offsets": V + 1, "nbr_items": 6 * T, "flags": V}
            adj_out = {n: torch.empty(k, dtype=torch.int32, device=dev) for n, k in rows.items()}
            normals_out = torch.empty((V, 3), dtype=torch.float32, device=dev)
            smooth_out = {n: torch.empty((V, 3), dtype=torch.float32, device=dev) for n in ("vertices", "normals")}
            filter_out = {n: torch.empty_like(t) for n, t in mesh_out.items()}
            mesh = gm.IndexedMesh(s, out=mesh_out)
            entries = {"adjacency": lambda: gm.MeshAdjacency(mesh_out["indices"], n_vertices=V, out=adj_out),
                       "normals": lambda: gm.MeshVertexNormals(mesh, out=normals_out),
                       "smooth": lambda: gm.SmoothMesh(mesh, ITERATIONS, LAM, MU, PIN, out=smooth_out)}
            if a.device_only:
                for name in ENTRIES:
                    for _ in range(a.warmup + a.iters):
                        entries[name]()
                gm.synchronize()
                continue
            t = {"indexed": timed(lambda: gm.IndexedMesh(s, out=mesh_out)), "filter": timed(lambda: gm.FilterMesh(mesh, MIN_TRIANGLES, out=filter_out))}
            for name in ENTRIES:
                t[name] = timed(entries[name])
            totals = entries["smooth"]()["totals"]
            entries["adjacency"]()
            entries["normals"]()
            gm.synchronize()
            found = []
            t["before"] = {"wall": timed(lambda: before(gm, s), found.append)["wall"]}
            flags, normals, Q, Qn = found[-1]
            assert np.array_equal(adj_out["flags"].cpu().numpy(), flags), "the host way's flags are not the device's"
            P = mesh_out["vertices"].cpu().numpy()
            odd = ~np.isfinite(P).all(1)  # (a vertex that is not finite spreads along the passes, the same way on both sides)
            same_nans = bool(np.array_equal(np.isnan(smooth_out["vertices"].cpu().numpy()), np.isnan(Q)))

            def far(x, y):
                d = np.abs(x.cpu().numpy().astype(np.float64) - y)
                return float(np.nanmax(d)) if d.size else 0.0
            device = sum(t[name]["wall"]["median"] for name in ENTRIES)
            r["stride %d" % s] = dict(t, totals=totals, MB_in=round((12 * V + 12 * T) / 1e6, 2), vertices_not_finite=int(odd.sum()),
                                      smoothed_vertices_not_finite=int((~np.isfinite(Q).all(1)).sum()), host_way_nans_where_the_devices_are=same_nans,
                                      host_way_max_abs_difference={"normals": far(normals_out, normals), "smoothed_vertices_m": far(smooth_out["vertices"], Q),
                                                                   "normals_of_the_smoothed": far(smooth_out["normals"], Qn)},
                                      smooth_wall_over_indexed=round(t["smooth"]["wall"]["median"] / t["indexed"]["wall"]["median"], 2),
                                      before_over_indexed_plus_three_entries=round(t["before"]["wall"]["median"] / (t["indexed"]["wall"]["median"] + device), 1))
            del mesh_out, adj_out, normals_out, smooth_out, filter_out
        res["maps"]["frames 0-%d" % (mark - 1)] = r
    if a.device_only:
        return
    gm.close()
    sphere_part(res)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("python tools/mesh_smooth_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour,\n"
                    "1 cm voxels, 16^3 chunks, UpdateMeshes every 10 frames -- after the frames named; %d warm-up + %d timed calls per figure, a\n"
                    "synchronise on both sides of every timed region; microseconds, median and p10-p90 of host wall times.  indexed:\n"
                    "Chisel.IndexedMesh(s, out=...) into device tensors; filter: Chisel.FilterMesh(mesh, %d, out=...); adjacency, normals, smooth:\n"
                    "Chisel.MeshAdjacency / MeshVertexNormals / SmoothMesh(mesh, %d) into device tensors -- host: the time in the call, wall: until\n"
                    "a synchronise behind it returns; before: IndexedMesh into host arrays + scipy.sparse CSR matrices + numpy normals + %d Taubin\n"
                    "iterations as sparse products, in the same run.  sphere_radius_9.6_voxels: the largest and mean angle to the radial direction\n"
                    "of IndexedMesh's gradient normals and of MeshVertexNormals on a sphere, per stride.)\n\n" % (a.warmup, a.iters, MIN_TRIANGLES, ITERATIONS, ITERATIONS))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
