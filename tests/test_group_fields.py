"""What the group tests (tests/test_gpu_group_fields.py) run, established without a GPU on the oracle alone (tests/group_fields.py): every
sparse frame of every case changes exactly the chunks intended (a set written down per case and turn), the set to mesh is the 27-neighbourhood of what changed, the cases reach
what the GPU tests say they reach, and meshing on a rank's view is the right expectation for the field after the frame.  The counts
printed here stand in DESIGN.md 5.3."""
import numpy as np
import pytest

from tests import group_fields as gf
from tests import shard_views as sv

# (chunks changed, new chunks, job ids, of them resident before the frame) per dirty set in a fresh 4^3 block of 8^3 chunks at res 0.03
TABLE = {"one_inside": (3, 0, 45, 36), "corner": (3, 1, 45, 12), "line": (12, 0, 90, 48), "diagonal": (6, 2, 90, 24), "all": (93, 31, 288, 64)}


@pytest.mark.parametrize("family", ["dense", "thresholds"])
@pytest.mark.parametrize("base", [(0, 0, 0), (1000, -1000, 37), (-2, -2, -2)])
def test_table_of_the_dirty_sets(oracle_mod, family, base):
    """each dirty set into a fresh field: the same counts for both families and every base"""
    for name, want in TABLE.items():
        side = gf.OracleSide(oracle_mod, gf.Spec(family, 8, 4, 0.03, base))
        f = side.frame(name)
        got = (len(f.changed), len(f.new), len(f.jobs), len([j for j in f.jobs if j in f.field and j not in f.new]))
        print("%s base %s %s: %d chunks changed, %d new, %d job ids, %d resident" % ((family, base, name) + got))
        assert got == want, (name, got)


# (chunks changed, new chunks, job ids) per turn of every case, as the oracle gives them
_ALL = (93, 31, 288)
COUNTS = {"dense_origin": [_ALL], "dense_far_ids": [_ALL], "thresholds_origin": [_ALL], "thresholds_far_ids": [_ALL], "no_colour": [_ALL], "overflow": [_ALL],
          "turns": [(3, 1, 45), (93, 30, 288), (12, 0, 90), (3, 0, 45), (6, 0, 90)], "settles": [_ALL, (12, 0, 90), (3, 0, 45)],
          "chain": [_ALL, (12, 0, 90), (3, 0, 45), (6, 0, 90), (3, 0, 45)],
          "chunks_16": [(27, 0, 125)], "chunks_32": [(8, 0, 64)], "far_dense": [_ALL, (12, 0, 90)], "far_thresholds": [(88, 24, 290), (12, 0, 90)],
          "regrow": [(1, 0, 27), (62, 0, 216), (4, 0, 54)]}


@pytest.mark.parametrize("case", sorted(gf.CASES))
def test_reach_of_the_cases(oracle_mod, case):
    spec, turns, shardings = gf.CASES[case]
    side = gf.OracleSide(oracle_mod, spec)
    for t, name in enumerate(turns):
        f = side.frame(name)
        assert set(f.changed) == gf.intended(case, name), (case, name, len(f.changed))  # exactly the chunks intended
        assert (len(f.changed), len(f.new), len(f.jobs)) == COUNTS[case][t], (case, name, len(f.changed), len(f.new), len(f.jobs))
        assert name == "all" or len(f.whole) == len(f.targets), (case, name)  # (no patch of the smaller sets touches another)
        assert f.jobs == sv.job_ids(f.changed), (case, name)
        assert any(j not in f.field for j in f.jobs)  # a job that is not resident
        for world, block in shardings:
            owners, absent, idle = gf.reach(f.field, spec.N, f.jobs, world, block)
            assert owners >= min(2, world - 1), (case, name, world, block)  # some rank receives ghosts from two owners (from the other one of two)
            if case == "turns" and (world, block) == (8, 2) and name in ("corner", "one_inside"):
                assert idle, (case, name)  # a rank without jobs
            counts = sv.view_against_whole(oracle_mod, f.field, spec.N, spec.res, world, block, f.changed, color=spec.color)
            print("%s turn %d %s world %d block %d: %d changed, %d new, %d jobs (%d not resident), ghosts from up to %d owners, idle ranks %s, "
                  "%d vertices, %d far-reading" % (case, t + 1, name, world, block, len(f.changed), len(f.new), len(f.jobs), absent, owners, idle,
                                                   counts["vertices"], counts["far"]))
            assert counts["vertices"] > 0
            if case in gf.FAR_READING:
                assert counts["far"] > gf.FAR_READING[case][t], (case, name, counts)
            if case == "regrow":
                size = gf.largest_segment_voxels(f.field, spec.N, f.jobs, world, block) * 12 * world
                print("regrow turn %d: largest segment x world = %d bytes" % (t + 1, size))
                assert (size > 1 << 20) == (name == "all"), (name, size)  # the buffers start at 1 MiB: turn 2 outgrows them, turn 3 fits again


def test_collected_frame_overflows_a_list(oracle_mod):
    """the wide frame changes new chunks only; with all of them collected again the set to mesh is their 27-neighbourhoods, none of the
    field's chunks among them, and one of two shards lists more than the 4096 entries a group's lists start with"""
    spec, _, ((world, block),) = gf.CASES["overflow"]
    side = gf.OracleSide(oracle_mod, spec)
    side.frame("all")
    f = side.collected_frame()
    print("overflow: %d chunks changed and collected, %d job ids, %d entries in the longest list" % (len(f.changed), len(f.jobs), gf.most_entries(f, world, block)))
    assert f.jobs == sv.job_ids(f.collect) and not (f.jobs & set(side.initial))
    assert gf.most_entries(f, world, block) > 4096
    assert sorted(f.field) == sorted(gf.field_bits(side.om.fields())) and not (set(f.collect) & set(f.field))


def test_frame_beside_the_field(oracle_mod):
    """the last frame of a case creates at least 20 chunks and touches none of the field's"""
    for case in sorted(gf.CASES):
        spec = gf.CASES[case][0]
        side = gf.OracleSide(oracle_mod, spec)
        before = gf.field_bits(side.om.fields())
        depth, pose = side.rig.beside_frame()
        side.integrate(depth, pose)
        after = gf.field_bits(side.om.fields())
        print("%s: %d chunks created beside the field" % (case, len(after) - len(before)))
        assert len(after) - len(before) >= 20 and all(after[cid] == bits for cid, bits in before.items()), case


def test_routes_are_read_from_the_timing_lines():
    text = "\n".join(["## turn corner", "chisel_hip group recompute, host us: dirty lists 3 | x 4", "## turn all",
                      "chisel_hip group recompute (wait-free), host us: buffers 1 | y 2", "noise",
                      "chisel_hip group settle, host us: status 12 | commits 3 | status 4",
                      "chisel_hip group recompute (wait-free), host us: buffers 1 | y 2",
                      "chisel_hip group settle, host us: status 12 | commits 3 | status 0"])
    events = gf.routes(text)
    assert events == ["## turn corner", gf.BLOCKING, "## turn all", gf.WAIT_FREE, 4, gf.WAIT_FREE, 0]
    assert gf.sections(events) == [("", []), ("turn corner", [gf.BLOCKING]), ("turn all", [gf.WAIT_FREE, 4, gf.WAIT_FREE, 0])]
