"""chisel_hip_deintegrate_batch restated (TEST INFRASTRUCTURE: DESIGN.md 3.10 "Many frames in one call" is the definition), and the frame
lists and reach predicates its CPU and GPU tests share.

The restated batch is a fold of deintegrate_restated.restated_deintegrate over the frames -- the definition itself: n single calls in
order, stats summed, emptied ids and touched chunks united.  It holds no logic of its own, so it cannot agree with the kernel by sharing
a mistake with it.  Everything here runs at 64 x 48, the restatement's W, H.
"""
import functools

import numpy as np

from tests import deintegrate_restated as dr

KMAX = 16  # frames per launch set (chisel_device.h)
OUT = slice(2, 19)  # the batch the cases take out of frames20: 17 frames, one full set and a set of one

# (sequence, chunk size, truncator, colour rules), all with carving on
CASES = [("tilt", 8, "inverse", False), ("hostile", 16, "constant", True), ("neg_aniso", 8, "quadratic", True)]


def restated_batch(field, frames, rules, N, res):
    """-> (new field, stats, detail): the fold.  detail: "emptied" (the union, sorted), "reports" (every id as the single calls report
    it, in order: a duplicate would show here), "touched" (the union of the touched chunks), "per_frame" (each single call's detail)"""
    stats = dict.fromkeys(dr.STAT_NAMES, 0)
    reports, touched, per_frame = [], set(), []
    for frame in frames:
        field, st, detail = dr.restated_deintegrate(field, frame, rules, N, res)
        for k in dr.STAT_NAMES:
            stats[k] += st[k]
        reports += detail["emptied"]
        touched |= {cid for cid, p in detail["chunks"].items() if p["touched"]}
        per_frame.append(detail)
    return field, stats, {"emptied": sorted(set(reports)), "reports": reports, "touched": touched, "per_frame": per_frame}


def batch_reach(detail):
    """dr.reach summed over the frames of a fold"""
    out = {}
    for d in detail["per_frame"]:
        out = dr.add_reach(out, dr.reach(d))
    return out


@functools.lru_cache(maxsize=None)
def frames20(seq):
    """-> (20 frames, camera): frame i is frame i % len of the sequence; in round r = i // len > 0 its pose is moved by 1.5 r cm and
    turned by 0.7 r degrees"""
    base, cam = dr.sequence(seq)
    out = []
    for i in range(20):
        d, pose, intr = base[i % len(base)]
        r = i // len(base)
        out.append((d, np.asarray(pose, np.float32) if r == 0 else dr.perturbed(pose, 0.015 * r, 0.7 * r), intr))
    return out, cam


def first_set_reach(ids, frames, rules, N, res):
    """what one launch set (`frames`, at most KMAX) reaches over the chunks `ids`, from dr.classify alone -> dict:
    shared_voxels: voxels selected by two or more of the frames; partial_masks: chunks in which some but not all of the
    frames select a voxel (a listed chunk whose exact mask is partial); single_frame: chunks in which exactly one does"""
    assert len(frames) <= KMAX
    shared = partial = single = 0
    for cid in ids:
        ks = [dr.classify(cid, N, res, f, rules) for f in frames]
        shared += int((np.sum([k["band"] for k in ks], axis=0) >= 2).sum())
        seen = sum(bool(k["band"].any()) for k in ks)
        partial += 0 < seen < len(frames)
        single += seen == 1
    return {"shared_voxels": shared, "partial_masks": partial, "single_frame": single}


@functools.lru_cache(maxsize=None)
def case(oracle_mod, seq, N, trunc, color_rules):
    """the 20 frames through the oracle with carving on, frames[2:19] folded out -> dict: frames, cam, rules, before, after, stats, detail"""
    frames, cam = frames20(seq)
    rules = dr.rules_of(trunc, color_rules, carving=True)
    before = dr.oracle_map(oracle_mod, N, dr.GRIDS[N], rules, frames, cam).fields()
    after, stats, detail = restated_batch(before, frames[OUT], rules, N, dr.GRIDS[N])
    return {"frames": frames, "cam": cam, "rules": rules, "before": before, "after": after, "stats": stats, "detail": detail}


# ---- the corrected stretch of trajectory ------------------------------------------------------------------------------------------------
REINTEGRATED = (1, 2)  # the frames of `tilt` that go in 2 cm / 1 degree off
# The largest |sdf difference| between a batch re-integration in the restatement and the oracle's map of the frames as they are, over
# 8^3 and 16^3 and the three truncators, by color_rules (test_reintegration_bound_is_the_measurement of
# tests/test_deintegrate_batch_cases.py prints them); the bound is four times that, since taking out more frames compounds the
# rounding.  Under the depth rules the weights are small integers and the round trip is exact: equality.  Metres.
REINTEGRATION_MEASURED = {False: 0.0, True: 5.9604644775390625e-08}  # 2^-24
REINTEGRATION_BOUND = {k: 4 * v for k, v in REINTEGRATION_MEASURED.items()}
REINTEGRATION_CASES = [(N, t) for N in (8, 16) for t in dr.TRUNCATORS]


def reintegration_frames():
    """-> (the four frames of `tilt` as they are, the same with frames 1 and 2 off, camera)"""
    frames, cam = dr.sequence("tilt")
    wrong = [(d, dr.perturbed(p), intr) if i in REINTEGRATED else (d, p, intr) for i, (d, p, intr) in enumerate(frames)]
    return list(frames), wrong, cam


@functools.lru_cache(maxsize=None)
def reintegration(oracle_mod, N, trunc, color_rules):
    """the oracle's map of the four frames with two of them off; those two restated out as a batch and in again at their own poses
    (all out, then all in) -> (restated field, the oracle's map of the four frames as they are)"""
    frames, wrong, cam = reintegration_frames()
    rules = dr.rules_of(trunc, color_rules)
    res = dr.GRIDS[N]
    right = dr.oracle_map(oracle_mod, N, res, rules, frames, cam).fields()
    field = {cid: (np.full(N ** 3, dr.DEFAULT_SDF), np.zeros(N ** 3, np.float32), None) for cid in right}
    field.update(dr.oracle_map(oracle_mod, N, res, rules, wrong, cam).fields())
    field, _, _ = restated_batch(field, [wrong[i] for i in REINTEGRATED], rules, N, res)
    for i in REINTEGRATED:
        field = dr.restated_integrate(field, frames[i], rules, N, res)
    return field, right
