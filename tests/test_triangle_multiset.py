"""tests.common.triangle_multiset (vectorised) against the plain loop it replaces, on triangles with ties (CPU only)."""
import numpy as np

from tests.common import triangle_multiset


def loop_form(vertices, decimals=5):
    """sorted list of triangles, each rotated to start at its lexicographically smallest vertex (the first of equals)"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3, 3).round(decimals) + 0.0
    out = []
    for tri in v:
        keys = [tuple(p) for p in tri]
        k = keys.index(min(keys))
        out.append(tuple(keys[k:] + keys[:k]))
    return sorted(out)


def test_equalities_are_those_of_the_loop_form():
    rng = np.random.default_rng(7)
    outcomes = {True: 0, False: 0}
    for trial in range(60):
        v = rng.integers(-2, 3, (40, 3, 3)).astype(np.float32) * np.float32(0.1)  # few distinct values: equal vertices, equal triangles
        v[rng.random(v.shape) < 0.1] = -0.0
        w = v.copy()
        kind = trial % 6
        if kind == 0:
            w = w[rng.permutation(len(w))]           # another order of the triangles: equal
        elif kind == 1:
            w[5] = w[5][[1, 2, 0]]                   # a triangle rotated: equal
        elif kind == 2:
            w[5] = w[5][[1, 0, 2]]                   # a triangle turned over: equal only if two of its vertices are
        elif kind == 3:
            w[7, 1, 2] += np.float32(0.1)            # a vertex moved
        elif kind == 4:
            w[7, 1, 2] += np.float32(1e-7)           # ... by less than the rounding: equal
        else:
            w[3] = w[4]                              # a triangle replaced by a copy of another
        want = loop_form(v.reshape(-1, 3)) == loop_form(w.reshape(-1, 3))
        assert (triangle_multiset(v.reshape(-1, 3)) == triangle_multiset(w.reshape(-1, 3))) == want, (trial, kind)
        outcomes[want] += 1
    assert outcomes[True] >= 20 and outcomes[False] >= 10, outcomes
    assert triangle_multiset(np.zeros((0, 3), np.float32)) == triangle_multiset(np.zeros((0, 3), np.float32))


def test_rotations_and_negative_zero():
    a, b, c = (0.0, 1.0, 2.0), (0.0, 1.0, 3.0), (-1.0, 5.0, 0.0)
    same = [np.array(t, np.float32) for t in ((a, b, c), (b, c, a), (c, a, b))]
    assert len({triangle_multiset(t) for t in same}) == 1
    assert triangle_multiset(np.array((a, c, b), np.float32)) != triangle_multiset(same[0])  # turned over
    assert triangle_multiset(np.array(((-0.0, 1.0, 2.0), b, c), np.float32)) == triangle_multiset(same[0])  # -0.0 is 0.0
    for t in same + [np.array((a, b, a), np.float32), np.array((b, a, a), np.float32)]:  # (two equal smallest vertices: the first starts)
        assert (triangle_multiset(t) == triangle_multiset(same[0])) == (loop_form(t) == loop_form(same[0]))
