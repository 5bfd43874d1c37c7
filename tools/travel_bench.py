#!/usr/bin/env python3
"""Time chisel_hip_travel_field on the maps of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3 chunks,
InverseTruncator(1), carving 0.05 m) after 220 frames (the default window's map) and after 620 (the late window's), after warm-up.

    python tools/travel_bench.py [--frames 220 620 --iters 10 --warmup 2 --out profiles/travel_bench.txt]

Windows: those of tools/distance_bench.py and tools/frontier_bench.py, 128 x 128 x 32 and 256 x 256 x 64 voxels centred on the surface
point the central pixel of the last pose sees -- at 1 cm voxels the map holds chunks only in a band around the surfaces, and a window
of these sizes around the camera itself holds no observed voxel.  The seed is the voxel of the window that is traversable at
clearance 3 and nearest to the voxel of the last camera position ("seed_voxels_from_camera" says how far that is).  Per window,
connectivity (6, 26), clearance (0, 3) and with / without the kept frontier voxels of the window (Frontiers, connectivity 26,
min_voxels 16) as targets, costs (10, 14, 17):
  device_us   wall time of one chisel_hip_travel_field call -- cost and step into device tensors, the targets a device tensor, the
              table -- until the call returns (it waits for its totals)
  host_us     wall time of Chisel.TravelField into numpy arrays, the targets a numpy array
  rounds, tile_visits   the call's diagnostics
and beside it, once for the smaller window at connectivity 26 and clearance 0 (the explicit graph of the larger one has 10^8 edges), the only route a caller has without the entry, wall time:
DistanceField(state), the read-back, scipy.sparse.csgraph.dijkstra on the explicit grid graph (tests/travel_restated.answer) -- whose
cost and step must equal the call's.  Then the one number of the host loop, TRAVEL_ROUNDS_PER_WAIT: the same calls (connectivity 26,
clearance 0, no targets) and the frontier serpentine (24, 40, 40) with 8, 16, 32 and 64 round launches per wait, through the
library's tuning hook CHISEL_HIP_TRAVEL_ROUNDS_PER_WAIT.

For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/travel_bench.py
--frames 220 --skip-route` and then

    python tools/travel_bench.py --summarize-trace DIR --out profiles/travel_bench.txt

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
KNOBS = [(c, r, t) for c in (6, 26) for r in (0, 3) for t in (False, True)]
HOOK = "CHISEL_HIP_TRAVEL_ROUNDS_PER_WAIT"


def summarize_trace(a):
    rows = []
    for f in glob.glob(os.path.join(a.summarize_trace, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    per = {}
    for r in rows:
        name = r["Kernel_Name"]
        mine = next((k for k in ("travel_", "frontier_seed_kernel", "distance_", "report_words_kernel") if k in name), None)
        if mine is None:
            continue
        name = mine if mine == "report_words_kernel" else name[name.index(mine):].split("(")[0].split("<")[0]
        per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    total = sum(sum(v) for v in per.values())
    out = open(a.out, "a") if a.out else sys.stdout
    out.write("\nper kernel, from rocprofv3 --kernel-trace --stats (a run of its own: every call of the run, both windows, all knobs, the sweep)\n")
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
    return gm, np.floor(hit / RES).astype(int), np.floor(pose[:3, 3] / RES).astype(int)


def timed(f, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e6)
    return t


def sweep(call, a):
    """the median wall time of `call` per value of the host loop's number"""
    out = {}
    for per_wait in (8, 16, 32, 64):
        os.environ[HOOK] = str(per_wait)
        timed(call, a.warmup)
        out[str(per_wait)] = round(float(np.median(timed(call, a.iters))), 1)
    del os.environ[HOOK]
    return out


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
    from cvids_amd import capi
    from cvids_amd.chisel import Chisel
    from tests import frontier_restated as fr
    from tests import travel_restated as tr
    from tests.common import upload
    dev = torch.device("cuda:0")
    res = {"voxel_m": RES, "chunk": CHUNK, "iters": a.iters, "warmup": a.warmup, "rounds_per_wait": capi.TRAVEL_ROUNDS_PER_WAIT, "maps": {}}
    for frames in a.frames:
        gm, hit_voxel, cam_voxel = build_map(frames)
        per_map = {"chunks": gm.NumChunks(), "windows": {}}
        for dims in WINDOWS:
            origin = tuple(int(hit_voxel[k]) - dims[k] // 2 for k in range(3))
            # the seed: the voxel of the window that is traversable at clearance 3 and nearest to the camera
            field = gm.DistanceField(origin, dims, 3)
            ok = (field["state"] == 1) & (field["dist2"] == -1)
            z, y, x = np.nonzero(ok)
            assert len(x), "no voxel of the window is traversable at clearance 3"
            at = cam_voxel - np.asarray(origin)
            d2 = (x - at[0]) ** 2 + (y - at[1]) ** 2 + (z - at[2]) ** 2
            k = int(np.argmin(d2))
            seeds, moved = [(int(x[k]), int(y[k]), int(z[k]))], round(float(np.sqrt(d2[k])), 1)
            shape = (dims[2], dims[1], dims[0])
            voxels = dims[0] * dims[1] * dims[2]
            out = {"cost": torch.empty(shape, dtype=torch.int32, device=dev), "step": torch.empty(shape, dtype=torch.uint8, device=dev)}
            size = gm.FrontiersSize(origin, dims, 1, 26, 16)
            rows = torch.zeros((max(size["kept_voxels"], 1), 4), dtype=torch.int32, device=dev)
            front = gm.Frontiers(origin, dims, 1, 26, 16, out={"voxels": rows})
            K = max(front["totals"]["kept_clusters"], 1)
            rows = rows[:max(front["totals"]["kept_voxels"], 1)].contiguous()
            rows_host = rows.cpu().numpy()
            r = {"origin": origin, "voxels": voxels, "seed": seeds[0], "seed_voxels_from_camera": moved, "frontier_rows": int(rows.shape[0]), "groups": K, "knobs": {}}
            for connectivity, clearance, with_targets in KNOBS:
                kw = dict(connectivity=connectivity, clearance=clearance)
                call = lambda: gm.TravelField(origin, dims, seeds, targets=rows if with_targets else None, n_groups=K if with_targets else 0, out=out, **kw)
                timed(call, a.warmup)
                t = timed(call, a.iters)
                totals = call()["totals"]
                k = {"traversable": totals["traversable"], "reached": totals["reached"], "largest_cost": totals["largest_cost"], "rounds": totals["rounds"],
                     "tile_visits": totals["tile_visits"], "device_us": round(float(np.median(t)), 1), "device_us_min": round(float(np.min(t)), 1),
                     "device_us_max": round(float(np.max(t)), 1), "ns_per_voxel": round(float(np.median(t)) * 1e3 / voxels, 3)}
                if with_targets:
                    k["targets_reached"] = totals["targets_reached"]
                if not a.skip_route:
                    host = lambda: gm.TravelField(origin, dims, seeds, targets=rows_host if with_targets else None, n_groups=K if with_targets else 0, **kw)
                    timed(host, 1)
                    k["host_us"] = round(float(np.median(timed(host, max(a.iters // 2, 1)))), 1)
                r["knobs"]["c%d r%d %s" % (connectivity, clearance, "targets" if with_targets else "plain")] = k
            r["rounds_per_wait_us"] = sweep(lambda: gm.TravelField(origin, dims, seeds, out=out), a)
            if not a.skip_route and voxels <= 1 << 20:  # (the explicit grid graph of the larger window has 10^8 edges)
                got = gm.TravelField(origin, dims, seeds)
                t0 = time.perf_counter()
                state = gm.DistanceField(origin, dims, 1, dist2=False)["state"]
                t1 = time.perf_counter()
                want = tr.answer(state, state == fr.FREE, seeds)
                t2 = time.perf_counter()
                equal = all(np.array_equal(got[key], want[key]) for key in ("cost", "step"))
                r["route"] = {"state_and_readback_ms": round((t1 - t0) * 1e3, 1), "host_dijkstra_and_step_ms": round((t2 - t1) * 1e3, 1),
                              "wall_ms": round((t2 - t0) * 1e3, 1), "equal": bool(equal)}
                r["route_over_call"] = round((t2 - t0) * 1e6 / r["knobs"]["c26 r0 plain"]["device_us"], 1)
            per_map["windows"]["%dx%dx%d" % dims] = r
        res["maps"]["frames 0-%d" % (frames - 1)] = per_map
        gm.close()
    # the serpentine: many rounds, little work in each
    gm = Chisel((8, 8, 8), 0.0625, False, max_chunks=512)
    volume, seeds = tr.cases()["serpentine"]
    upload(gm, fr.fields_from_states(volume, 8, (5, -13, 9)))
    dims = volume.shape[::-1]
    call = lambda: gm.TravelField((5, -13, 9), dims, seeds, 6)
    totals = call()["totals"]
    res["serpentine"] = {"dims": dims, "rounds": totals["rounds"], "tile_visits": totals["tile_visits"], "reached": totals["reached"],
                         "rounds_per_wait_us": sweep(call, a)}
    gm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("python tools/travel_bench.py   (one MI355X; the maps of bench.py's default stream -- sphere_room, 640 x 480 depth + colour, 1 cm voxels,\n"
                    "16^3 chunks -- after the frames named; %d warm-up + %d timed calls per window and knob set (c = connectivity, r = clearance, with / without\n"
                    "the window's kept frontier voxels as targets), costs (10, 14, 17), the seed the voxel of the last camera position; device_us = wall time\n"
                    "of one chisel_hip_travel_field call, cost and step into device tensors, until it returns; host_us = Chisel.TravelField into numpy\n"
                    "arrays; route = DistanceField(state) with the read-back plus scipy.sparse.csgraph.dijkstra and the steps on the host, once, wall time;\n"
                    "rounds_per_wait_us = the median wall time of the c26 r0 plain call, and of the frontier serpentine at connectivity 6, with 8 / 16 / 32 /\n"
                    "64 round launches per host wait)\n\n" % (a.warmup, a.iters))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
