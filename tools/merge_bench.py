#!/usr/bin/env python3
"""Time chisel_hip_merge_map on the map of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3 chunks,
InverseTruncator(1), carving 0.05 m) built as two halves in two handles: the first half of the frames in one, the second in the other.

    python tools/merge_bench.py [--frames 220 --iters 7 --warmup 2 --route-chunks 1500 --out profiles/merge_bench.json]

Two things are timed:
  merge   the second half merged into a FRESH copy of the first (a new map filled by a merge of the first half at identity) at identity and
          at a general pose: hipEvent time over the destination's stream from in front of the call to behind its last kernel -- the one
          host wait in the middle of a merge is part of it -- over --iters fresh destinations after --warmup; median, minimum, maximum
  route   what exists without the entry point, for the same chunks at identity: chisel_hip_download_chunk of the source's and the
          destination's chunk, DistVoxel::Integrate / ColorVoxel::Integrate on the host (numpy), chisel_hip_upload_chunk -- wall time,
          over the first --route-chunks chunks of the source, scaled to all of them
Beside them the algorithmic bytes of a merge -- the voxels of the updated destination chunks read and written, the source's voxels read
once, 12 bytes per voxel with colour -- and bytes / time / 8 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES, CHUNK, NEAR, FAR = 0.01, 16, 0.05, 5.0
W, H = 640, 480
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route-chunks", type=int, default=1500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    from tests import merge_restated as mr
    dev = torch.device("cuda:0")
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    color = torch.from_numpy(synth.render_color(W, H, 3)).to(dev)
    frames = list(synth.stream("sphere_room", a.frames, W, H))
    halves = []
    for part in (frames[:a.frames // 2], frames[a.frames // 2:]):
        gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)
        for lo in range(0, len(part), 10):
            batch = [(torch.from_numpy(d).to(dev), p, cam) for d, p in part[lo:lo + 10]]
            gm.IntegrateBatch(integ, batch, [(color, p, cam) for _, p, _ in batch])
            gm.synchronize()
        halves.append(gm)
    first, second = halves
    n_first, n_second = first.NumChunks(), second.NumChunks()
    cap = n_first + 8 * n_second + 1024  # a fixed pool with room for every candidate chunk of the general pose
    identity = np.eye(4, dtype=np.float32)
    general = np.eye(4, dtype=np.float32)
    general[:3, :4] = mr.poses(RES)["rpy_neg"]
    general[:3, 3] = (0.11, -0.07, 0.05)
    V = CHUNK ** 3
    res = {"frames": a.frames, "voxel_m": RES, "chunk": CHUNK, "chunks_first_half": n_first, "chunks_second_half": n_second, "iters": a.iters, "merge": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        e.record()  # (creates the hipEvent_t the map records below)
    torch.cuda.synchronize()

    def fresh_destination():
        dst = Chisel((CHUNK,) * 3, RES, True, device_id=0, max_chunks=cap)
        dst.MergeMap(first, identity)
        return dst

    for name, pose in (("identity", identity), ("general_pose", general)):
        times, stats = [], None
        for it in range(a.warmup + a.iters):
            dst = fresh_destination()
            dst.record_event(ev[0].cuda_event)
            dst.MergeMap(second, pose, stats=False)
            dst.record_event(ev[1].cuda_event)
            ev[1].synchronize()
            if it >= a.warmup:
                times.append(ev[0].elapsed_time(ev[1]) * 1e3)
            if it == a.warmup + a.iters - 1:  # the figures of the case, from one more merge of the same maps into another fresh destination
                dst.close()
                dst = fresh_destination()
                stats = dst.MergeMap(second, pose)
            dst.close()
        bytes_ = 12 * V * (2 * stats["dst_chunks_updated"] + n_second)
        med = float(np.median(times))
        res["merge"][name] = dict(stats, call_us=round(med, 1), call_us_min=round(float(np.min(times)), 1), call_us_max=round(float(np.max(times)), 1),
                                  algorithmic_bytes=bytes_, share_of_8TBps=round(bytes_ / (med * 1e-6) / HBM_BYTES_PER_S, 4))

    # the route that exists without the entry point: chunk by chunk over the bus, the update on the host
    dst = fresh_destination()
    ids = [tuple(int(v) for v in cid) for cid in second.GetChunkIDs()]
    part = ids[:a.route_chunks]
    t0 = time.perf_counter()
    for cid in part:
        s, w, c = second.GetChunk(cid)
        if dst.HasChunk(cid):
            ds, dw, dc = dst.GetChunk(cid)
        else:
            ds, dw, dc = np.full(V, mr.DEFAULT_SDF), np.zeros(V, np.float32), np.zeros((V, 4), np.uint8)
        obs = w.astype(np.float64) > 1e-12
        if obs.any():
            ds[obs], dw[obs] = mr.dist_integrate(ds[obs], dw[obs], s[obs], w[obs])
            paint = obs & (c[:, 3] > 0)
            dc[paint] = mr.color_integrate(dc[paint], c[paint])[0]
            dst.AddChunk(cid, ds, dw, dc)
    route_s = time.perf_counter() - t0
    dst.close()
    res["route"] = {"chunks_timed": len(part), "wall_ms": round(route_s * 1e3, 1), "us_per_chunk": round(route_s * 1e6 / max(1, len(part)), 1),
                    "scaled_to_all_chunks_ms": round(route_s * 1e3 * len(ids) / max(1, len(part)), 1)}
    res["route_over_merge"] = round(res["route"]["scaled_to_all_chunks_ms"] * 1e3 / res["merge"]["identity"]["call_us"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
