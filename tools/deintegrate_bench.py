#!/usr/bin/env python3
"""Time chisel_hip_deintegrate_depth and chisel_hip_deintegrate_batch on the maps of bench.py's default stream (sphere_room, 640 x 480 depth + colour, 1 cm voxels, 16^3
chunks, InverseTruncator(1), carving 0.05 m): after frames 0-219 (the default window's map) and after frames 0-619 (the late window's,
three times larger), every depth image in HBM, after warm-up.

    python tools/deintegrate_bench.py [--frames 220,620 --iters 30 --warmup 3 --out profiles/deintegrate_bench.json]

Per map, medians and minima in microseconds (hipEvents on the map's stream around the call unless it says wall):
  deintegrate/device     one keyframe taken out (colour rules, as it went in), nothing waited for.  The keyframes rotate over the last
                         `iters` frames of the stream; each is integrated again, untimed, before the next one leaves, so that every
                         timed call meets the same map
  deintegrate/wall       the same call returning its stats and the emptied ids to the host
  deintegrate/device_again  the first line measured once more at the end of the map's lines: its run-to-run spread within one session
  deintegrate_batch/device  16 keyframes taken out by one chisel_hip_deintegrate_batch call (the 16 frames that end at the rotating
                         keyframe), nothing waited for; all 16 are integrated again, untimed, before the next call.  To be compared
                         with 16 x deintegrate/device of the same run; per_keyframe_us is the median over 16
  deintegrate_batch/wall the same call returning its stats and the emptied ids to the host
  list_only/device       the same call for a camera turned away from the map: the list kernel visits every committed slot, lists
                         (nearly) nothing, and the apply kernel's workgroups find an empty list -- the part of the call that grows with
                         the pool and not with the frame
  forward/device, /wall  one frame integrated per call on the same map (IntegrateDepthScanColor; wall: the caller waits after the call)
  reset_replay/wall      Reset() and every frame of the map integrated again, 10 per call: what a corrected keyframe cost before
First measurements of this kernel pair; nothing here is a threshold."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="220,620")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from cvids_amd import synth
    from cvids_amd.chisel import Chisel, ConstantWeighter, InverseTruncator, PinholeCamera, ProjectionIntegrator
    dev = torch.device("cuda:0")
    integ = ProjectionIntegrator(InverseTruncator(100 * RES), ConstantWeighter(1.0), 0.05, True)
    cam = PinholeCamera(*synth.intrinsics(W, H), W, H, NEAR, FAR)
    color = torch.from_numpy(synth.render_color(W, H, 3)).to(dev)
    counts = sorted(int(v) for v in a.frames.split(","))
    frames = [(torch.from_numpy(d).to(dev), p) for d, p in synth.stream("sphere_room", counts[-1], W, H)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        e.record()  # (creates the hipEvent_t the map records below)
    torch.cuda.synchronize()

    def stats(t):
        return {"us": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_p10": round(float(np.percentile(t, 10)), 1),
                "us_p90": round(float(np.percentile(t, 90)), 1)}

    res = {"voxel_m": RES, "chunk": CHUNK, "image": "%dx%d" % (W, H), "iters": a.iters, "maps": {}}
    for n in counts:
        gm = Chisel((CHUNK,) * 3, RES, True, device_id=0)

        def replay():
            for lo in range(0, n, 10):
                part = frames[lo:lo + 10]
                gm.IntegrateBatch(integ, [(d, p, cam) for d, p in part], [(color, p, cam) for _, p in part])
            gm.synchronize()

        replay()
        keys = list(range(max(0, n - a.iters), n))
        r = {"frames": n, "chunks": gm.NumChunks(), "committed_slots": gm.pool_info()["committed"]}

        def forward(k):
            gm.IntegrateDepthScanColor(integ, frames[k][0], frames[k][1], cam, color, frames[k][1], cam)

        def timed(call, undo=None, wall=False):
            t = []
            for i, k in enumerate(keys[:a.warmup] + keys):
                gm.synchronize()
                if wall:
                    t0 = time.perf_counter()
                    call(k)
                    gm.synchronize()
                    dt = (time.perf_counter() - t0) * 1e6
                else:
                    gm.record_event(ev[0].cuda_event)
                    call(k)
                    gm.record_event(ev[1].cuda_event)
                    ev[1].synchronize()
                    dt = ev[0].elapsed_time(ev[1]) * 1e3
                if i >= a.warmup:
                    t.append(dt)
                if undo:
                    undo(k)
            return stats(t)

        took = gm.DeintegrateDepthScan(integ, frames[keys[0]][0], frames[keys[0]][1], cam, color_rules=True)
        forward(keys[0])
        r["one_call"] = {k: v for k, v in took.items() if k != "emptied_ids"}
        r["deintegrate/device"] = timed(lambda k: gm.DeintegrateDepthScan(integ, frames[k][0], frames[k][1], cam, color_rules=True, stats=False), undo=forward)
        r["deintegrate/wall"] = timed(lambda k: gm.DeintegrateDepthScan(integ, frames[k][0], frames[k][1], cam, color_rules=True), undo=forward, wall=True)

        # ---- 16 keyframes per call
        def stretch(k):
            return list(range(max(0, k - 15), k + 1))

        def batch_out(k, **kw):
            return gm.DeintegrateDepthScans(integ, [(frames[j][0], frames[j][1], cam) for j in stretch(k)], color_rules=True, **kw)

        def batch_in(k):
            gm.IntegrateBatch(integ, [(frames[j][0], frames[j][1], cam) for j in stretch(k)], [(color, frames[j][1], cam) for j in stretch(k)])

        took = batch_out(keys[0])
        batch_in(keys[0])
        r["one_batch_call"] = dict({k: v for k, v in took.items() if k != "emptied_ids"}, keyframes=len(stretch(keys[0])))
        r["deintegrate_batch/device"] = timed(lambda k: batch_out(k, stats=False), undo=batch_in)
        r["deintegrate_batch/device"]["per_keyframe_us"] = round(r["deintegrate_batch/device"]["us"] / len(stretch(keys[0])), 2)
        r["deintegrate_batch/wall"] = timed(batch_out, undo=batch_in, wall=True)

        def away(k):
            p = np.array(frames[k][1], np.float32)
            p[:3, :3] = p[:3, :3] @ np.diag([1.0, -1.0, -1.0]).astype(np.float32)
            p[:3, 3] += 100.0  # (and far off: no chunk's sphere reaches into the pyramid)
            return gm.DeintegrateDepthScan(integ, frames[k][0], p, cam, color_rules=True, stats=False)

        r["list_only/device"] = timed(away)
        # (what the forward calls below add is taken out again, untimed, so that they too meet the same map)
        back = lambda k: gm.DeintegrateDepthScan(integ, frames[k][0], frames[k][1], cam, color_rules=True, stats=False)
        r["forward/device"] = timed(forward, undo=back)
        r["forward/wall"] = timed(forward, undo=back, wall=True)
        r["deintegrate/device_again"] = timed(lambda k: gm.DeintegrateDepthScan(integ, frames[k][0], frames[k][1], cam, color_rules=True, stats=False), undo=forward)
        t = []
        for _ in range(3):
            gm.synchronize()
            t0 = time.perf_counter()
            gm.Reset()
            replay()
            t.append((time.perf_counter() - t0) * 1e6)
        r["reset_replay/wall"] = stats(t)
        res["maps"][str(n)] = r
        gm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
