"""The cases of chisel_hip_deintegrate_batch (tests/deintegrate_batch_cases.py; DESIGN.md 3.10 "Many frames in one call") on the CPU, from
the oracle and the restatement alone: they reach what they are for -- voxels under several frames of a launch set, partial frame masks,
every kind of cleared voxel, emptied chunks, none reported twice --, the order of the frames matters, a corrected stretch of
trajectory comes back to the oracle's map within a bound measured here, and the library exports the entry its header declares."""
import os

import numpy as np
import pytest

from tests import deintegrate_batch_cases as bc
from tests import deintegrate_restated as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the construction gives (20 frames in with carving on, frames[2:19] out): resident chunks, then the reach of the fold
REACH = {
    "tilt": (187, {"updated": 97464, "cleared_zero": 18011, "cleared_residue": 0, "cleared_negative": 0, "skipped": 27242, "emptied": 80}),
    "hostile": (171, {"updated": 467161, "cleared_zero": 20602, "cleared_residue": 0, "cleared_negative": 11148, "skipped": 24745, "emptied": 32}),
    "neg_aniso": (245, {"updated": 208958, "cleared_zero": 4354, "cleared_residue": 1761, "cleared_negative": 8915, "skipped": 33068, "emptied": 19}),
}
FIRST_SET = {"tilt": (25477, 174, 6), "hostile": (134257, 163, 5), "neg_aniso": (43531, 209, 9)}


@pytest.mark.parametrize("seq,N,trunc,color_rules", bc.CASES, ids=lambda v: str(v))
def test_cases_reach_what_they_are_for(oracle_mod, seq, N, trunc, color_rules):
    k = bc.case(oracle_mod, seq, N, trunc, color_rules)
    r = bc.batch_reach(k["detail"])
    first = bc.first_set_reach(sorted(k["before"]), k["frames"][bc.OUT][:bc.KMAX], k["rules"], N, dr.GRIDS[N])
    print(seq, len(k["before"]), k["stats"], r, first)
    assert len(k["frames"][bc.OUT]) == 17
    chunks, want = REACH[seq]
    assert len(k["before"]) == chunks and k["stats"]["chunks_tested"] == 17 * chunks
    for name, n in want.items():
        assert (r[name] > 0) == (n > 0), (name, r[name], n)
    assert first["shared_voxels"] > 0 and first["partial_masks"] > 0 and first["single_frame"] > 0, first
    assert {name: r[name] for name in want} == want and tuple(first.values()) == FIRST_SET[seq]  # (the construction is the one written down)
    # a chunk without weight can only be skipped by later frames: the single calls report no id twice, and the batch's count is their sum
    reports = k["detail"]["reports"]
    assert len(reports) == len(set(reports)) == k["stats"]["chunks_emptied"] == len(k["detail"]["emptied"])
    assert set(k["detail"]["emptied"]) == set(k["detail"]["touched"]) - set(dr.holds_weight(k["after"]))


def test_order_matters(oracle_mod):
    """the rule depends on the voxel's state: two frames taken out in either order leave different distances"""
    k = bc.case(oracle_mod, *bc.CASES[2])
    f, N = k["frames"], 8
    a, _, _ = bc.restated_batch(k["before"], [f[2], f[3]], k["rules"], N, dr.GRIDS[N])
    b, _, _ = bc.restated_batch(k["before"], [f[3], f[2]], k["rules"], N, dr.GRIDS[N])
    differ = sum(int((np.asarray(a[cid][0]).view(np.uint32) != np.asarray(b[cid][0]).view(np.uint32)).sum()) for cid in a)
    print("voxels whose sdf bits depend on the order:", differ)
    assert differ == 1402


@pytest.mark.parametrize("color_rules", [False, True])
@pytest.mark.parametrize("N,trunc", bc.REINTEGRATION_CASES, ids=lambda v: str(v))
def test_batch_reintegration_against_the_oracle(oracle_mod, N, trunc, color_rules):
    got, right = bc.reintegration(oracle_mod, N, trunc, color_rules)
    worst, same_w = dr.max_sdf_difference(got, right)
    print("batch re-integration %s: max |d sdf| %.9e, weights bit-equal: %s" % ((N, trunc, color_rules), worst, same_w))
    assert len(right) > 50
    if not color_rules:
        assert same_w and worst == 0.0
    assert worst <= bc.REINTEGRATION_BOUND[color_rules], (worst, bc.REINTEGRATION_BOUND[color_rules])


def test_reintegration_bound_is_the_measurement(oracle_mod):
    for color_rules in (False, True):
        worst = max(dr.max_sdf_difference(*bc.reintegration(oracle_mod, N, t, color_rules))[0] for N, t in bc.REINTEGRATION_CASES)
        print("color_rules %s: %.17g" % (color_rules, worst))
        assert worst == bc.REINTEGRATION_MEASURED[color_rules]


def test_the_entry_is_declared_and_exported(hip_lib):
    from cvids_amd import capi
    with open(os.path.join(ROOT, "include", "chisel_hip.h")) as f:
        header = f.read()
    assert "int chisel_hip_deintegrate_batch(chisel_hip_map *map, int n, const chisel_hip_depth_frame *frames, int color_rules," in header
    assert "chisel_hip_deintegrate_batch" in capi.EXPORTS
    assert hasattr(hip_lib, "chisel_hip_deintegrate_batch")
