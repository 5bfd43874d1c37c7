"""tests/hash_cases.py on the CPU: the restated hash against the oracle's, the key packing at the accepted extremes, the table model
against a dict, and the reach of the two crowded setups on the model."""
import numpy as np
import pytest

from tests import hash_cases as hc
from tests.common import make_frames, small_camera


def test_restated_hash_equals_the_oracles(oracle_mod):
    rng = np.random.default_rng(11)
    ids = np.concatenate([rng.integers(-1200, 1200, (3000, 3)), rng.integers(hc.ID_MIN, hc.ID_MAX + 1, (1000, 3)),
                          np.array([[0, 0, 0], [-1, -1, -1], [hc.ID_MIN] * 3, [hc.ID_MAX] * 3, [hc.ID_MIN, hc.ID_MAX, -1]])])
    assert (ids < 0).any(axis=1).sum() > 1000
    for x, y, z in ids.tolist():
        assert hc.chunk_hash(x, y, z) == oracle_mod.chunk_hash(x, y, z) & hc.MASK64, (x, y, z)


def test_pack_round_trip_at_the_accepted_extremes():
    ext = (hc.ID_MIN, hc.ID_MIN + 1, -1, 0, 1, hc.ID_MAX - 1, hc.ID_MAX)
    seen = set()
    for x in ext:
        for y in ext:
            for z in ext:
                k = hc.pack_id(x, y, z)
                assert hc.unpack_id(k) == (x, y, z)
                assert k not in (hc.KEY_EMPTY, hc.KEY_TOMB) and k < 1 << 63
                seen.add(k)
    assert len(seen) == len(ext) ** 3
    # the neighbours a kernel looks up around an accepted id still fit their 21 bits
    assert hc.unpack_id(hc.pack_id(hc.ID_MAX + 1, hc.ID_MIN - 1, 0)) == (hc.ID_MAX + 1, hc.ID_MIN - 1, 0)
    # ... and why the ids outside are refused: the fields carry into each other
    assert hc.pack_id(1 << 20, 0, 0) == hc.pack_id(-(1 << 20), 1, 0)


def test_far_ids_cover_every_bucket():
    for cap, need in ((1024, 12), (2048, 4)):
        by = hc._far_by_home(cap)
        assert min(len(by.get(h, [])) for h in range(cap)) >= need  # (12: the 32 colliding ids on 3 homes; 4: a run blocker and extras)
        for ids in by.values():
            for c in ids:
                assert all(600 <= abs(v) <= 1000 for v in c)
    allids = [c for ids in hc._far_by_home(1024).values() for c in ids]
    assert len(set(allids)) == 100 * 40 * 8
    for a in range(3):
        assert any(c[a] < 0 for c in allids) and any(c[a] > 0 for c in allids)
    ids = hc.colliding_ids(1024)
    assert len(set(ids)) == 32 and {hc.home_of(c, 1024) for c in ids} == {1023, 0, 517}


def test_model_against_a_dict():
    ids = hc.colliding_ids(1024)
    rng = np.random.default_rng(5)
    t, d = hc.TableModel(1024), set()
    wrapped = tombs = 0
    for step in range(5000):
        c = ids[int(rng.integers(len(ids)))]
        op = int(rng.integers(3))
        if op == 0:
            assert t.insert(c) >= 0
            d.add(c)
        elif op == 1:
            assert t.remove(c) == (c in d)
            d.discard(c)
        else:
            assert (t.find(c) >= 0) == (c in d)
        if step % 250 == 0:
            assert t.ids() == sorted(d)
            r = t.readout()
            wrapped += sum(hc.crosses_end(r, x) for x in d)
            tombs += sum(hc.tombstones_on_path(r, x) > 0 for x in d)
    assert t.ids() == sorted(d)
    assert wrapped > 20 and tombs > 20  # (the case is one: paths wrap and pass tombstones)


@pytest.fixture(scope="module")
def wall_order(oracle_mod):
    om = oracle_mod.OracleMap(8, 0.05, False)
    om.set_integrator(1, 2.0, 1.0, True, 0.05)
    return hc.scene_order(om, make_frames("wall", 2, 64, 48), small_camera(64, 48))


def test_reach_of_the_run_across_the_end_on_the_model(wall_order):
    """wall, 2 frames, 8^3, 5 cm, 64 x 48, capacity 1024: 90 chunks, 333 blockers, sequential inserts standing in for the frames.  On the
    model 74 chunks sit off their home, 32 have a probe length >= 8, 24 cross the end and 53 are behind a tombstone after the removal
    (the first figure depends on which far ids the extra blockers are; the other three follow from the full run alone)."""
    assert len(wall_order) == 90
    before, after, blockers, removed = hc.model_run_across_end(1024, wall_order)
    assert len(blockers) == 333 and len(set(blockers)) == 333 and len(blockers) + len(wall_order) == 423 <= 512
    assert len(removed) == 167
    r0, r1 = hc.reach(before, wall_order), hc.reach(after, wall_order)
    print("reach before the removal %s, after %s" % (r0, r1))
    assert r0["tomb"] == 0
    assert r0["off_home"] == 74
    assert r0["long"] == 32
    assert r0["cross"] == 24
    assert r1["tomb"] == 53
    assert (r1["off_home"], r1["long"], r1["cross"]) == (r0["off_home"], r0["long"], r0["cross"])  # (a removal moves nothing)


def test_saturation_takes_three_rounds_on_the_model():
    rounds = hc.saturation_rounds(1024, 400)
    assert [len(r) for r in rounds] == [400, 400, 224]
    t = hc.TableModel(1024)
    for r in rounds:
        for c in r:
            assert t.insert(c) == hc.home_of(c, 1024)
        for c in r:
            assert t.remove(c)
    assert hc.n_empty(t.readout()) == 0 and hc.n_tombstones(t.readout()) == 1024
    assert t.find((1, 2, 3)) == -1  # (a full scan, bounded by the capacity)
    assert t.insert((1, 2, 3)) == hc.home_of((1, 2, 3), 1024)


def test_invariants_catch_a_broken_table():
    """the checker itself: a consistent read-out passes, each broken one is named"""
    t = hc.TableModel(1024)
    ids = hc.colliding_ids(1024)[:6]
    for c in ids:
        t.insert(c)
    t.remove(ids[1])
    keys = np.array(t.keys, np.uint64)
    vals = np.zeros(1024, np.int32)
    slot_key = np.full(8, hc.KEY_EMPTY, np.uint64)
    live = [i for i, k in enumerate(t.keys) if k not in (hc.KEY_EMPTY, hc.KEY_TOMB)]
    for s, i in enumerate(live):
        vals[i] = s
        slot_key[s] = keys[i]
    good = {"capacity": 1024, "committed": 8, "free_top": 3, "hash_keys": keys, "hash_vals": vals, "slot_key": slot_key,
            "free_list": np.array([7, 6, 5], np.int32)}
    assert hc.check_invariants(good) == 5

    def broken(**kw):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, f in kw.items():
            b[k] = f(b[k])
        with pytest.raises(AssertionError):
            hc.check_invariants(b)

    def with_(i, v):
        def f(a):
            a[i] = v
            return a
        return f
    tomb = int(np.flatnonzero(keys == np.uint64(hc.KEY_TOMB))[0])
    broken(hash_keys=with_(tomb, np.uint64(hc.KEY_EMPTY)))          # an EMPTY cuts the later keys off from their home
    broken(hash_keys=with_(tomb, keys[live[0]]))                    # a key twice
    broken(hash_vals=with_(live[0], 1 if vals[live[0]] != 1 else 0))  # two keys share a slot / slot_key disagrees
    broken(hash_vals=with_(live[0], 9))                             # a slot outside the pool
    broken(free_list=lambda a: np.array([7, 6, 0], np.int32))       # a used slot on the free list
    broken(free_top=lambda v: 2, free_list=lambda a: a[:2])         # a slot neither used nor free
    broken(slot_key=with_(6, keys[live[0]]))                        # a free slot with a key
