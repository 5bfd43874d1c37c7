"""The restatement of chisel_hip_deintegrate_depth (tests/deintegrate_restated.py) on the CPU: its forward half against
the oracle bit for bit -- which pins the selection everything else rests on --, then what taking a frame out must give: nothing where
the frame was alone, the oracle's map of the other frames within a rounding bound measured here, the oracle's map of the corrected
frames after a re-integration, and every branch of the rule reached."""
import functools
import itertools

import numpy as np
import pytest

from tests import deintegrate_restated as dr
from tests import merge_restated as mr

# The largest |sdf difference| the round trips and the re-integrations below leave, measured with this file (test_measured_bounds_are_the_measurements prints them), and the
# bounds they are held to: four times that, since taking out more frames compounds the rounding.  Metres.
ROUND_TRIP_MEASURED = {False: 0.0, True: 8.940696716308594e-08}   # by color_rules; 3 * 2^-25
REINTEGRATION_MEASURED = {False: 0.0, True: 8.940696716308594e-08}
ROUND_TRIP_BOUND = {k: 4 * v for k, v in ROUND_TRIP_MEASURED.items()}
REINTEGRATION_BOUND = {k: 4 * v for k, v in REINTEGRATION_MEASURED.items()}


def empty_field(ids, N):
    return {cid: (np.full(N ** 3, dr.DEFAULT_SDF), np.zeros(N ** 3, np.float32), None) for cid in ids}


# ---- a. the forward restatement against the oracle -----------------------------------------------------------------------------------------
def _forward_cases():
    """every sequence, truncator, rule set and carving setting at 8^3 / 5 cm; at 16^3 / 2 cm every sequence and truncator with the rule set
    and the carving setting alternating"""
    out = [(s, 8, t, c, k) for s in dr.SEQUENCES for t in dr.TRUNCATORS for c in (False, True) for k in (False, True)]
    for i, (s, t) in enumerate(itertools.product(dr.SEQUENCES, dr.TRUNCATORS)):
        out += [(s, 16, t, bool(i % 2), True), (s, 16, t, not i % 2, False)]
    return out


@pytest.mark.parametrize("seq,N,trunc,color_rules,carving", _forward_cases(), ids=lambda v: str(v))
def test_forward_restatement_is_the_oracle(oracle_mod, seq, N, trunc, color_rules, carving):
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules, carving)
    want = dr.oracle_map(oracle_mod, N, dr.GRIDS[N], rules, frames, cam).fields()
    got = empty_field(want, N)
    for frame in frames:
        got = dr.restated_integrate(got, frame, rules, N, dr.GRIDS[N])
    assert len(want) > 50
    mr.assert_fields_bit_equal(dr.distances(want), dr.distances(got), False, "%s %d %s" % (seq, N, trunc))


# ---- b. a frame that was alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color_rules", [False, True])
@pytest.mark.parametrize("trunc", list(dr.TRUNCATORS))
@pytest.mark.parametrize("seq", list(dr.SEQUENCES))
def test_sole_frame_leaves_nothing(oracle_mod, seq, trunc, color_rules):
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules)
    N, res = 8, dr.GRIDS[8]
    before = dr.oracle_map(oracle_mod, N, res, rules, frames[:1], cam).fields()
    after, stats, detail = dr.restated_deintegrate(before, frames[0], rules, N, res)
    assert len(before) > 10
    for cid, (s, w, _) in after.items():
        assert (s == dr.DEFAULT_SDF).all() and mr.same_bits(w, np.zeros_like(w)), cid
    assert detail["emptied"] == sorted(before) and stats["chunks_emptied"] == stats["chunks_touched"] == len(before)
    assert stats["voxels_updated"] == 0 and stats["voxels_skipped"] == 0 and stats["voxels_cleared"] > 0


# ---- c. round trip and re-integration -------------------------------------------------------------------------------------------------------
SHARED = [(s, 8, t, c) for s in dr.SEQUENCES for t in dr.TRUNCATORS for c in (False, True)] + [("tilt", 16, "inverse", False), ("neg_aniso", 16, "quadratic", True)]


@functools.lru_cache(maxsize=None)
def round_trip(oracle_mod, seq, N, trunc, color_rules):
    """frames A, B of the sequence with carving off, B restated out -> (restated field, the oracle's map of A alone, stats, detail)"""
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules)
    res = dr.GRIDS[N]
    both = dr.oracle_map(oracle_mod, N, res, rules, frames[:2], cam).fields()
    alone = dr.oracle_map(oracle_mod, N, res, rules, frames[:1], cam).fields()
    got, stats, detail = dr.restated_deintegrate(both, frames[1], rules, N, res)
    return got, alone, stats, detail


@functools.lru_cache(maxsize=None)
def reintegration(oracle_mod, seq, N, trunc, color_rules):
    """three frames, the middle one integrated 2 cm and 1 degree off, restated out there and in again at its own pose -> (restated
    field, the oracle's map of the three frames as they are, detail)"""
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules)
    res = dr.GRIDS[N]
    d, pose, intr = frames[1]
    off = (d, dr.perturbed(pose), intr)
    wrong = dr.oracle_map(oracle_mod, N, res, rules, [frames[0], off, frames[2]], cam).fields()
    right = dr.oracle_map(oracle_mod, N, res, rules, frames[:3], cam).fields()
    field = empty_field(right, N)
    field.update(wrong)
    field, _, detail = dr.restated_deintegrate(field, off, rules, N, res)
    return dr.restated_integrate(field, frames[1], rules, N, res), right, detail


@pytest.mark.parametrize("seq,N,trunc,color_rules", SHARED, ids=lambda v: str(v))
def test_round_trip(oracle_mod, seq, N, trunc, color_rules):
    got, alone, stats, _ = round_trip(oracle_mod, seq, N, trunc, color_rules)
    worst, same_w = dr.max_sdf_difference(got, alone)
    print("round trip %s: max |d sdf| %.3e, weights bit-equal: %s, %s" % ((seq, N, trunc, color_rules), worst, same_w, stats))
    assert stats["voxels_cleared"] > 0  # (B alone somewhere; where A and B overlap: test_reach)
    if not color_rules:
        assert same_w  # (small integers)
    assert worst <= ROUND_TRIP_BOUND[color_rules], (worst, ROUND_TRIP_BOUND[color_rules])


@pytest.mark.parametrize("seq,N,trunc,color_rules", SHARED, ids=lambda v: str(v))
def test_reintegration(oracle_mod, seq, N, trunc, color_rules):
    got, right, _ = reintegration(oracle_mod, seq, N, trunc, color_rules)
    worst, same_w = dr.max_sdf_difference(got, right)
    print("re-integration %s: max |d sdf| %.3e, weights bit-equal: %s" % ((seq, N, trunc, color_rules), worst, same_w))
    if not color_rules:
        assert same_w
    assert worst <= REINTEGRATION_BOUND[color_rules], (worst, REINTEGRATION_BOUND[color_rules])


def test_measured_bounds_are_the_measurements(oracle_mod):
    """the constants above are what the shared cases give here: a bound that no longer belongs to its measurement fails"""
    for color_rules in (False, True):
        cases = [c for c in SHARED if c[3] == color_rules]
        rt = max(dr.max_sdf_difference(*round_trip(oracle_mod, *c)[:2])[0] for c in cases)
        ri = max(dr.max_sdf_difference(*reintegration(oracle_mod, *c)[:2])[0] for c in cases)
        print("color_rules %s: round trip %.9e, re-integration %.9e" % (color_rules, rt, ri))
        assert rt == ROUND_TRIP_MEASURED[color_rules] and ri == REINTEGRATION_MEASURED[color_rules], (rt, ri)


# ---- d. reach -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_built_case(oracle_mod, seq, N, trunc, color_rules):
    """the oracle's map of a sequence's first two frames with the weights under the second frame rewritten by class
    (deintegrate_restated.hand_built) -> (field, frame, rules)"""
    frames, cam = dr.sequence(seq)
    rules = dr.rules_of(trunc, color_rules)
    field = dr.oracle_map(oracle_mod, N, dr.GRIDS[N], rules, frames[:2], cam).fields()
    return dr.hand_built(field, frames[1], rules, N, dr.GRIDS[N]), frames[1], rules


HAND_BUILT = [("tilt", 8, "constant", False), ("neg_aniso", 8, "inverse", True), ("hostile", 16, "quadratic", False)]


def test_reach(oracle_mod):
    total = {}
    for case in SHARED:
        total = dr.add_reach(total, dr.reach(round_trip(oracle_mod, *case)[3]))
        total = dr.add_reach(total, dr.reach(reintegration(oracle_mod, *case)[2]))
    integrated = dict(total)
    for seq, N, trunc, color_rules in HAND_BUILT:
        field, frame, rules = hand_built_case(oracle_mod, seq, N, trunc, color_rules)
        r = dr.reach(dr.restated_deintegrate(field, frame, rules, N, dr.GRIDS[N])[2])
        for k in ("updated", "cleared_zero", "cleared_residue", "cleared_negative", "skipped"):  # no branch is left to chance
            assert r[k] > 0, (seq, k, r)
        total = dr.add_reach(total, r)
    print("integrated maps: %s\nwith the hand-built fields: %s" % (integrated, total))
    for k, v in total.items():
        assert v > 0, (k, total)
    for k in ("updated", "cleared_zero", "emptied", "touched_not_emptied", "listed_untouched"):
        assert integrated[k] > 0, (k, integrated)
