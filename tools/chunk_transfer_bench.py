#!/usr/bin/env python3
"""Time chisel_hip_gather_chunks / chisel_hip_scatter_chunks against the per-chunk loops they replace, and SaveMap / LoadMap, on the
maps of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3 chunks, InverseTruncator(1), carving
0.05 m): after frames 0-219 (the default window's map) and after frames 0-619 (the late window's).

    python tools/chunk_transfer_bench.py [--frames 220,620 --iters 20 --warmup 3 --out profiles/chunk_transfer_bench.txt]

Per map, alternating in one process, wall time in microseconds (median and the p10-p90 range):
  get_loop        GetChunk over GetChunkIDs(): one look-up with a wait and three blocking copies per chunk
  gather_host     GatherChunks() into numpy arrays, complete on return
  gather_device   GatherChunks(out=...) into torch tensors: enqueue (the host's time in the call) and the time until a synchronise
                  behind it returns
  add_loop        AddChunk per chunk into a second map (reset before every round, not timed)
  scatter_host    ScatterChunks from the numpy arrays into that map
  scatter_device  ScatterChunks from the torch tensors: enqueue, and until a synchronise returns
  save, load      SaveMap to a file in the temporary directory, LoadMap of it into the second map (--file-iters rounds)
Before anything is timed the gathered arrays are checked equal, bit for bit, to the loop's, and the scattered map to the source.

`--files-only` times SaveMap and LoadMap alone and uses no entry an older library lacks: run it with CHISEL_HIP_LIB naming the parent
commit's library (built into cvids_amd/ under another name) for the comparison; `--append` adds its line to --out.

For the kernels' own time run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/chunk_transfer_bench.py --device-only` and then `python tools/chunk_transfer_bench.py --summarize-trace DIR --out FILE`, which
appends the table (bytes moved = 2 x the payload, over the kernel's time, as a share of 8 TB/s)."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES, CHUNK, NEAR, FAR = 0.01, 16, 0.05, 5.0
W, H = 640, 480


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1), "p90": round(float(np.percentile(us, 90)), 1)}


def summarize_trace(a):
    from cvids_amd.capi import CHUNK_TILE_BYTES as TILE_BYTES
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nchunk_copy_kernel, from rocprofv3 --kernel-trace (a run of its own, --device-only); grid = tiles of 16 KiB x arrays; bytes = 2 x the payload\n")
    out.write("%-8s %8s %7s %6s %10s %10s %10s %10s %10s\n" % ("kernel", "tiles", "arrays", "calls", "median_us", "min_us", "max_us", "GB/s", "of 8 TB/s"))
    for tag, name in (("<false>", "gather"), ("<true>", "scatter")):
        groups = {}
        for r in rows:
            if "chunk_copy_kernel" not in r["Kernel_Name"] or (tag not in r["Kernel_Name"] and ("Lb%d" % (tag == "<true>")) not in r["Kernel_Name"]):
                continue
            tiles = int(r.get("Grid_Size_X") or r["Grid_Size"]) // int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
            arrays = int(r.get("Grid_Size_Y") or 3) // int(r.get("Workgroup_Size_Y") or 1)
            groups.setdefault((tiles, arrays), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for (tiles, arrays), us in sorted(groups.items()):
            gbs = tiles * arrays * TILE_BYTES * 2 / (np.median(us) * 1e-6) / 1e9
            out.write("%-8s %8d %7d %6d %10.1f %10.1f %10.1f %10.0f %9.1f%%\n" % (name, tiles, arrays, len(us), np.median(us), min(us), max(us), gbs, gbs / 80.0))


def build_map(gm, integ, cam, color, dev, start, stop):
    import torch
    from cvids_amd import synth
    batch = []
    for depth, pose in synth.stream("sphere_room", stop - start, W, H, start=start):
        batch.append((torch.from_numpy(depth).to(dev), pose, cam))
        if len(batch) == 10:
            gm.IntegrateBatch(integ, batch, [(color, p, cam) for _, p, _ in batch])
            batch = []
    assert not batch, "--frames: multiples of 10"
    gm.synchronize()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="220,620")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--file-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--files-only", action="store_true", help="SaveMap / LoadMap alone (any library)")
    ap.add_argument("--device-only", action="store_true", help="the device-tensor calls alone (under the profiler)")
    ap.add_argument("--summarize-trace", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a)

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    dev = torch.device("cuda:0")
    gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)
    dst = Chisel((CHUNK,) * 3, RES, True, device_id=0)
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    color = torch.from_numpy(synth.render_color(W, H, 3)).to(dev)
    marks = sorted(int(v) for v in a.frames.split(","))
    res = {"label": a.label, "library": os.environ.get("CHISEL_HIP_LIB", "libchisel_hip.so"), "voxel_m": RES, "chunk": CHUNK, "iters": a.iters,
           "warmup": a.warmup, "file_iters": a.file_iters, "maps": {}}
    path = os.path.join(tempfile.mkdtemp(), "map.chsl")
    done = 0
    for mark in marks:
        build_map(gm, integ, cam, color, dev, done, mark)
        done = mark
        ids = gm.GetChunkIDs()
        n, V = len(ids), gm.V
        r = {"chunks": n, "payload_MB": round(n * V * 12 / 1e6, 1)}
        t = {}

        def timed(key, call, sync=None, keep=True):
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if sync is not None:
                sync()
                t2 = time.perf_counter()
            if keep:
                t.setdefault(key if sync is None else key + "_enqueue", []).append((t1 - t0) * 1e6)
                if sync is not None:
                    t.setdefault(key + "_wall", []).append((t2 - t0) * 1e6)

        if not a.files_only:
            out = {"sdf": torch.empty((n, V), dtype=torch.float32, device=dev), "weight": torch.empty((n, V), dtype=torch.float32, device=dev),
                   "rgbw": torch.empty((n, V, 4), dtype=torch.uint8, device=dev)}
            host = gm.GatherChunks()
            gm.GatherChunks(out=out)
            gm.synchronize()
            if not a.device_only:  # the same data, bit for bit, both ways
                loop = [gm.GetChunk(c) for c in ids]
                for k, name in enumerate(("sdf", "weight", "rgbw")):
                    want = np.stack([c[k] for c in loop])
                    assert np.array_equal(bits(host[name]), bits(want)) and np.array_equal(bits(out[name].cpu().numpy()), bits(want)), name
                assert np.array_equal(host["ids"], ids)
                dst.Reset()
                assert dst.ScatterChunks(ids, out["sdf"], out["weight"], out["rgbw"]) == n
                back = dst.GatherChunks()
                assert np.array_equal(back["ids"], ids) and all(np.array_equal(bits(back[k]), bits(host[k])) for k in ("sdf", "weight", "rgbw"))
            for i in range(a.warmup + a.iters):
                keep = i >= a.warmup
                if not a.device_only:
                    timed("get_loop", lambda: [gm.GetChunk(c) for c in ids], keep=keep)
                    timed("gather_host", lambda: gm.GatherChunks(), keep=keep)
                timed("gather_device", lambda: gm.GatherChunks(out=out), gm.synchronize, keep=keep)
                if not a.device_only:
                    dst.Reset(); dst.synchronize()
                    timed("add_loop", lambda: [dst.AddChunk(c, host["sdf"][k], host["weight"][k], host["rgbw"][k]) for k, c in enumerate(ids)], keep=keep)
                    dst.Reset(); dst.synchronize()
                    timed("scatter_host", lambda: dst.ScatterChunks(ids, host["sdf"], host["weight"], host["rgbw"]), keep=keep)
                dst.Reset(); dst.synchronize()
                timed("scatter_device", lambda: dst.ScatterChunks(ids, out["sdf"], out["weight"], out["rgbw"]), dst.synchronize, keep=keep)
        if not a.device_only:
            for i in range(1 + a.file_iters):
                timed("save", lambda: gm.SaveMap(path), keep=i > 0)
                timed("load", lambda: dst.LoadMap(path), dst.synchronize, keep=i > 0)
            assert dst.NumChunks() == n
            t.pop("load_enqueue", None)
        r.update({k: stats(v) for k, v in t.items() if v})
        if not a.files_only and not a.device_only:
            r["get_loop_over_gather_host"] = round(r["get_loop"]["median"] / r["gather_host"]["median"], 1)
            r["get_loop_over_gather_device"] = round(r["get_loop"]["median"] / r["gather_device_wall"]["median"], 1)
            r["add_loop_over_scatter_host"] = round(r["add_loop"]["median"] / r["scatter_host"]["median"], 1)
            r["add_loop_over_scatter_device"] = round(r["add_loop"]["median"] / r["scatter_device_wall"]["median"], 1)
        res["maps"]["frames 0-%d" % (mark - 1)] = r
    os.remove(path) if os.path.exists(path) else None
    line = json.dumps(res)
    print(line)
    if a.out and not a.device_only:
        with open(a.out, "a" if a.append else "w") as f:
            if not a.append:
                f.write("python tools/chunk_transfer_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour,\n"
                        "1 cm voxels, 16^3 chunks -- after the frames named; warm-up + timed rounds per map as the line says, the loops and the packed\n"
                        "entries alternating in one process; host wall times in microseconds, median and p10-p90; *_enqueue: the host's time in the\n"
                        "call, *_wall: until a synchronise behind it returns; save / load: the file in the temporary directory)\n\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
