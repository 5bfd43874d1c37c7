"""The contract of a sharded mesh recompute, established without a GPU (tests/shard_views.py): who owns a chunk, what is meshed, what a
rank's view holds -- against the product's pure host functions and the numpy restatement of its device plan -- and, on the oracle
alone, where meshing on a view differs from meshing the whole map: never in positions or grid entries, in normals and colours only
at far-reading vertices.  The counts printed here stand in DESIGN.md 5.3."""
import itertools

import numpy as np
import pytest

from tests import shard_views as sv
from tests import voxel_fields as vf

N = 8
BASES = ((0, 0, 0), (-2, -2, -2), (1000, -1000, 37))
SHARDINGS = ((2, 2), (2, 1), (3, 1), (3, 2), (8, 1), (8, 2))  # (world, shard block)
CASES = [(base, world, block, name) for base in BASES for world, block in SHARDINGS for name in sv.DIRTY_SETS]


def block_ids(base):
    return set(vf.block_ids(sv.B, base))


def test_owner_equals_the_product(hip_lib):
    from cvids_amd.chisel import chunk_owner
    near = list(itertools.product(range(-9, 10), repeat=3))
    far = [(1000 + x, -1000 + y, 37 + z) for x, y, z in itertools.product(range(-4, 5), repeat=3)]
    for world in (2, 3, 8):
        for block in (1, 2):
            for cid in near + far:
                assert sv.owner(cid, world, block) == chunk_owner(cid, world, block), (cid, world, block)


@pytest.mark.parametrize("world,block", SHARDINGS)
def test_job_set_equals_the_reference_plan(world, block):
    """the jobs of plan_shells_reference are job_ids split by owner; entries of both flags, resident or not"""
    from cvids_amd.sharded import plan_shells_reference
    for base in BASES:
        for name in sv.DIRTY_SETS:
            dirty = sv.dirty_set(name, base)
            extra = [(base[0] + 9, base[1] - 7, base[2] + 5), (base[0] + 1, base[1] + 1, base[2] + 2)]  # taken as they are
            entries = np.array([list(i) + [0] for i in dirty] + [list(i) + [1] for i in extra], np.int64)
            jobs = sv.job_ids(dirty + extra, [0] * len(dirty) + [1] * len(extra))
            assert extra[0] in jobs and (extra[0][0] + 1, extra[0][1], extra[0][2]) not in jobs
            seen = set()
            for rank in range(world):
                got = plan_shells_reference(entries, world, rank, lambda i: sv.owner(i, world, block))[0]
                assert got == sv.jobs_of(jobs, rank, world, block), (base, name, rank)
                seen.update(got)
            assert seen == jobs


_CODE_MASKS = {}


def _mask_of_codes(codes):
    """the voxels of the boxes `codes`, by the product's own shell_box_coords: (N, N, N) bool indexed [z, y, x]"""
    from cvids_amd.sharded import shell_box_coords
    m = np.zeros((N, N, N), bool)
    for code in codes:
        if code not in _CODE_MASKS:
            one = np.zeros((N, N, N), bool)
            for x, y, z in shell_box_coords(int(code), N):
                one[z, y, x] = True
            _CODE_MASKS[code] = one
        m |= _CODE_MASKS[code]
    return m


@pytest.mark.parametrize("world,block", SHARDINGS)
def test_covering_rule_ships_the_union_of_the_definition(hip_lib, world, block):
    """per rank and ghost id: the boxes of the items plan_shells_reference leaves (its covering rule drops an item whose box "is part of
    another item's") hold exactly the voxels the definition asks for, the union of box(d) over every (J, d); the host planner
    chisel_hip_mesh_shell_plan, which merges boxes per axis, holds at least those"""
    from cvids_amd.chisel import mesh_shell_plan
    from cvids_amd.sharded import plan_shells_reference
    own = lambda i: sv.owner(i, world, block)
    for base in BASES:
        for name in sv.DIRTY_SETS:
            dirty = sv.dirty_set(name, base)
            entries = np.array([list(i) + [0] for i in dirty], np.int32)
            jobs = sv.job_ids(dirty)
            for rank in range(world):
                want = sv.ghost_masks(jobs, rank, world, block, N)
                _, _, recv = plan_shells_reference(entries, world, rank, own)
                codes = {}
                for o, items in recv.items():
                    for x, y, z, code in items:
                        assert own((x, y, z)) == o != rank
                        codes.setdefault((x, y, z), []).append(code)
                assert set(codes) == set(want), (base, name, rank)
                for g, mask in want.items():
                    assert np.array_equal(_mask_of_codes(codes[g]), mask), (base, name, rank, g)
                merged = {}
                for o, x, y, z, code in mesh_shell_plan(entries, world, rank, block)[1].tolist():
                    merged.setdefault((x, y, z), []).append(code)
                assert set(merged) == set(want), (base, name, rank)
                for g, mask in want.items():
                    assert not (mask & ~_mask_of_codes(merged[g])).any(), (base, name, rank, g)


def _face_jobs(d, g):
    """the jobs whose box of g holds box(d): g - d', d' = d with some, not all, of its non-zero components zeroed"""
    nz = [a for a in range(3) if d[a]]
    out = []
    for keep in itertools.product((0, 1), repeat=len(nz)):
        if all(keep) or not any(keep):
            continue
        d2 = [0, 0, 0]
        for k, a in zip(keep, nz):
            d2[a] = d[a] if k else 0
        out.append((g[0] - d2[0], g[1] - d2[1], g[2] - d2[2]))
    return out


@pytest.mark.parametrize("base,world,block,name", CASES)
def test_reach_of_the_cases(base, world, block, name):
    """what the cases reach, on the plan of the definition.  Every dirty set smaller than the map has a request (J, d) for a RESIDENT
    neighbour whose face job g - d' is no job at all (the covering rule must not count on it); `corner` has job ids that are not
    resident and requests for neighbours that are not (found = 0); with 8 ranks every box code occurs.

    One exception, from the owner function itself: blocks that differ by +-(0, 1, 1) differ by 3 + 5 = 8 in bx + 3 by + 5 bz, so among
    8 ranks they share their owner, and with shard block 1 every chunk is its own block -- the two codes of d = +-(0, 1, 1) cannot
    occur with 8 ranks and shard block 1.  They occur with shard block 2 (below) and with 3 ranks and shard block 1 (the last test)."""
    resident = block_ids(base)
    jobs = sv.job_ids(sv.dirty_set(name, base))
    requests = [(rank, j, d, g) for rank in range(world) for j, d, g in sv.shell_requests(jobs, rank, world, block)]
    assert requests
    if name != "all":
        missing = [(j, d, g) for rank, j, d, g in requests if g in resident and any(f not in jobs for f in _face_jobs(d, g))]
        assert missing, (base, world, block, name)
        other_rank = [(j, d, g) for rank, j, d, g in requests
                      if any(f in jobs and sv.owner(f, world, block) != rank for f in _face_jobs(d, g))]
        assert other_rank, (base, world, block, name)
    if name == "corner":
        assert any(j not in resident for j in jobs)
        assert any(g not in resident for _, _, _, g in requests)
        assert any(j not in resident and g in resident for _, j, _, g in requests)  # a job that is not there still has its shells sent
    if world == 8:
        seen = {sv.box_code(d) for _, _, d, _ in requests}
        want = {sv.box_code(d) for d in sv.DIRECTIONS}
        if block == 1:
            want -= {sv.box_code((0, 1, 1)), sv.box_code((0, -1, -1))}
            assert not ({sv.box_code((0, 1, 1)), sv.box_code((0, -1, -1))} & seen)
        assert seen >= want, (base, block, name, sorted(want - seen))


def test_every_box_code_occurs_with_shard_block_1():
    seen = set()
    for world in (2, 3, 8):
        jobs = sv.job_ids(sv.dirty_set("one_inside"))
        seen |= {sv.box_code(d) for rank in range(world) for _, d, _ in sv.shell_requests(jobs, rank, world, 1)}
    assert seen == {sv.box_code(d) for d in sv.DIRECTIONS}


# ---- a view against the whole map, on the oracle alone -----------------------------------------------------------------------------
# (family, N, block edge, res, base, world, dirty set, far-reading vertices expected); shard block 1, seed 1
VIEW_ROWS = [
    ("dense", 8, 4, 0.03, (0, 0, 0), 8, "all", False),
    ("dense", 8, 4, 0.03, (0, 0, 0), 2, "all", False),
    ("dense", 8, 4, 0.03, (0, 0, 0), 3, "all", False),
    ("dense", 8, 4, 0.03, (0, 0, 0), 8, "one_inside", False),
    ("dense", 8, 4, 0.25, (-2, -2, -2), 8, "all", True),
    ("dense", 8, 4, 0.10, (-2, -2, -2), 8, "all", True),
    ("dense", 16, 3, 0.07, (0, 0, 0), 3, "all", True),
    ("dense", 32, 2, 0.05, (0, 0, 0), 2, "all", True),
    ("thresholds", 8, 4, 0.03, (0, 0, 0), 8, "all", True),
    ("thresholds", 8, 4, 0.03, (1000, -1000, 37), 8, "all", False),
    ("thresholds", 8, 4, 1.0, (-1, -1, -1), 8, "all", True),
]


@pytest.mark.parametrize("family,n,edge,res,base,world,name,far_expected", VIEW_ROWS)
def test_view_against_the_whole_map(oracle_mod, family, n, edge, res, base, world, name, far_expected):
    """every job of every rank meshed on its view and on the whole map: positions and grid entries equal everywhere, normals and colours
    equal except at far-reading vertices (asserted inside view_against_whole); far-reading vertices exist where the table of
    DESIGN.md 5.3 says so and nowhere else"""
    field = getattr(vf, family)(n, edge, 1, res=res, base=base)
    dirty = sv.dirty_set(name, base) if edge == sv.B else vf.block_ids(edge, base)
    counts = sv.view_against_whole(oracle_mod, field, n, res, world, 1, dirty)
    print("%s %d^3 x %d^3 res %g base %s world %d dirty %s: %d vertices, %d far-reading, %d normal rows differ, %d colour rows differ" % (
        family, n, edge, res, base, world, name, counts["vertices"], counts["far"], counts["normals"], counts["colors"]))
    assert counts["vertices"] > 0
    assert (counts["far"] > 0) == far_expected, counts
    assert counts["normals"] <= counts["far"] and counts["colors"] <= counts["far"]
