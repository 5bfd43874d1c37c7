"""tests/travel_restated.py against itself, on the CPU: the three forms of the cost (a numpy relaxation to the fixed point, a heapq
Dijkstra, scipy's Dijkstra on the explicit grid graph) agree exactly at every connectivity and cost set and under max_cost cuts; STEP
walks end at a seed with the summed move costs equal to the cost; the group table on hand rows; each shared case reaches what it is
for."""
import numpy as np
import pytest

from tests import frontier_restated as fr
from tests import travel_restated as tr

FORMS = (tr.relaxation, tr.heap, tr.scipy_form)


def small_walled():
    """the walled volume at a size the whole-volume relaxation takes a second for: 12 x 18 x 26 [z, y, x]"""
    v = tr.walled((12, 18, 26))
    assert (v == fr.OCCUPIED).any() and (v == fr.UNKNOWN).any()
    return v


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("step_cost", tr.COST_SETS)
def test_the_three_forms_agree(connectivity, step_cost):
    volume = small_walled()
    trav = volume == fr.FREE
    seeds = [(1, 1, 1), (24, 16, 10), (6, 3, 3)]  # the last on a wall: ignored
    costs = [form(trav, seeds, connectivity, step_cost) for form in FORMS]
    assert all(c.dtype == np.int32 and np.array_equal(c, costs[0]) for c in costs)
    assert (costs[0] == 0).sum() == 2 and (costs[0][trav] >= 0).all() and (costs[0][~trav] == -1).all()
    cut = int(np.median(costs[0][costs[0] >= 0]))
    for max_cost in (0, 1, cut, 500):
        cuts = [form(trav, seeds, connectivity, step_cost, max_cost) for form in FORMS]
        assert all(np.array_equal(c, cuts[0]) for c in cuts)
        assert np.array_equal(cuts[0], np.where((costs[0] >= 0) & (costs[0] <= max_cost), costs[0], -1))  # a cut only removes
    assert 0 < (tr.scipy_form(trav, seeds, connectivity, step_cost, cut) >= 0).sum() < trav.sum()


def test_the_forms_agree_on_the_full_walled_volume_with_a_cut():
    volume = tr.walled()
    trav = volume == fr.FREE
    for connectivity in (6, 26):
        a, b = tr.heap(trav, [(1, 1, 1)], connectivity, (10, 14, 17), 500), tr.scipy_form(trav, [(1, 1, 1)], connectivity, (10, 14, 17), 500)
        assert np.array_equal(a, b) and 0 < (a >= 0).sum() < trav.sum()


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_step_walks_end_at_a_seed_with_the_cost(connectivity):
    volume = small_walled()
    trav = volume == fr.FREE
    seeds = [(1, 1, 1), (24, 16, 10)]
    for step_cost in tr.COST_SETS:
        cost = tr.scipy_form(trav, seeds, connectivity, step_cost)
        step = tr.step_of(cost, connectivity, step_cost)
        assert step.dtype == np.uint8 and ((step == tr.SEED) == (cost == 0)).all() and ((step == tr.NONE) == (cost < 0)).all()
        codes = {tr.code(o) for o in tr.offsets(connectivity)}
        assert set(np.unique(step).tolist()) <= codes | {tr.SEED, tr.NONE}
        rng = np.random.default_rng(connectivity)
        z, y, x = np.nonzero(cost > 0)
        for k in rng.choice(len(x), 60, replace=False):
            path = tr.walk(step, (x[k], y[k], z[k]))
            assert tuple(path[-1]) in seeds and tr.walk_cost(path, step_cost) == cost[z[k], y[k], x[k]]
            along = cost[path[:, 2], path[:, 1], path[:, 0]]
            assert (np.diff(along) < 0).all()  # following steps strictly lowers the cost
    with pytest.raises(ValueError):
        tr.walk(step, (6, 3, 3))  # a wall: unreached


def test_the_smallest_code_wins_a_tie():
    cost = tr.scipy_form(np.ones((3, 3, 3), bool), [(0, 0, 0), (2, 0, 0)], 6, (1, 1, 1))
    step = tr.step_of(cost, 6, (1, 1, 1))
    assert cost[0, 0, 1] == 1 and step[0, 0, 1] == tr.code((0, 0, -1))  # -x and +x fit: -x has the smaller code
    assert cost[1, 1, 0] == 2 and step[1, 1, 0] == tr.code((-1, 0, 0))  # -z (4) and -y (10) fit


def test_the_group_table():
    cost = tr.scipy_form(np.ones((2, 3, 4), bool), [(0, 0, 0)], 6, (1, 1, 1))
    cost[1, 2, 3] = -1
    rows = [(1, 0, 0, 0), (0, 1, 0, 0), (2, 2, 1, 0), (3, 2, 1, 1), (4, 0, 0, 1), (0, 0, 0, 2), (0, 0, 0, -1)]
    table, reached, ignored = tr.table_of(cost, rows, 2)
    assert table.tolist() == [[3, 3, 1, 1], [1, 0, -1, -1]] and reached == 3 and ignored == 3


def test_each_shared_case_reaches_what_it_is_for():
    cases = tr.cases()
    for kind, level in (("face", 1), ("edge", 2), ("corner", 3)):
        volume, seeds = cases["seam_" + kind]
        free = list(zip(*np.nonzero(volume == fr.FREE)))
        assert len(free) == 2 and free[0] == (7, 15, 15) and seeds == [(15, 15, 7)]
        assert sum(a // t != b // t for a, b, t in zip(free[0], free[1], (8, 16, 16))) == level  # the move crosses that many tile borders
        for connectivity, has in ((6, 1), (18, 2), (26, 3)):
            assert (tr.scipy_form(volume == fr.FREE, seeds, connectivity) >= 0).sum() == (2 if has >= level else 1)
    for name in ("serpentine", "small_serpentine", "comb", "walled", "open_box"):
        volume, seeds = cases[name]
        trav = volume == fr.FREE
        cost = tr.scipy_form(trav, seeds, 6, (1, 1, 1))
        assert all(trav[z, y, x] for x, y, z in seeds) and ((cost >= 0) == trav).all(), name  # everything free is reached
        assert tr.tile_borders_crossed(volume, seeds) > 1, name
    corridor = int((cases["serpentine"][0] == fr.FREE).sum())
    assert tr.scipy_form(cases["serpentine"][0] == fr.FREE, cases["serpentine"][1], 6, (1, 1, 1)).max() == corridor - 1  # one long way
    box = tr.scipy_form(cases["open_box"][0] == fr.FREE, cases["open_box"][1], 26)
    assert abs(int(box[:, :, :20].max()) - int(box[:, :, 20:].max())) <= 17  # the two seeds' costs meet in the middle
    assert (tr.scipy_form(cases["small_serpentine"][0] == fr.FREE, cases["small_serpentine"][1], 6, (10, 14, 17), 1555) >= 0).sum() == 156
