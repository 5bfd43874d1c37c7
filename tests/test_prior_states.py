"""The hand-built states of tests/prior_states.py meet the rules they are meant for -- on the oracle alone (no GPU): a bit comparison over
them (tests/test_gpu_prior_states.py) says something about a comparison of the kernel only if voxels of that class reach that branch,
and only if the oracle's own answer there is the reference's.  The minimum counts are conditions, set before anything was counted; the
counts themselves are printed and recorded in DESIGN.md "What the prior-state tests cover"."""
import numpy as np
import pytest

from tests import prior_states as ps

F = np.float32
SIZES = (8, 16, 32)
DEFAULT = (F(99999.0), F(0.0))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class Touch:
    """flat arrays over the voxels of the block: the state in the uploaded field (s0, w0, c0), the state after the frame that first
    touches the voxel (s1, w1, c1; the uploaded one where no frame does), that frame (`first`) and its branches (`region`), the class"""

    def __init__(self, oracle_mod, N, path, family="finite", with_colours=False):
        self.reg = reg = ps.regions(oracle_mod, N, path, with_colours=with_colours)
        self.fld, self.states, self.counters, self.books = ps.run_oracle(oracle_mod, N, path, family, with_colours=with_colours)
        ids = reg.ids
        cat = lambda f, j: np.concatenate([f[cid][j] for cid in ids])
        self.s0, self.w0, self.c0 = (cat(self.fld, j) for j in range(3))
        self.first = np.concatenate([reg.first[cid] for cid in ids])
        self.region = np.concatenate([reg.region[cid] for cid in ids])
        self.cls = np.concatenate([ps.voxel_class(N, cid) for cid in ids])
        self.z = np.concatenate([(ps.voxel_coords(N, cid)[2] + 0.5) * ps.RES[N] for cid in ids])
        self.after = [tuple(cat(st, j) for j in range(3)) for st in self.states]
        sel = np.where(self.first < 0, 0, self.first + 1)
        rows = np.arange(len(sel))
        self.s1, self.w1, self.c1 = (np.stack([a[j] for a in self.after])[sel, rows] for j in range(3))
        self.band = (self.region & ps.BAND) != 0
        self.carve = (self.region & ps.CARVE) != 0

    def unchanged(self, m):
        return (bits(self.s1)[m] == bits(self.s0)[m]).all() and (bits(self.w1)[m] == bits(self.w0)[m]).all()

    def reset(self, m):
        return (bits(self.s1)[m] == bits(DEFAULT[0])).all() and (bits(self.w1)[m] == bits(DEFAULT[1])).all()


def carves(s):
    """`sdf < 1e-5` as the reference evaluates it, in double"""
    return s.astype(np.float64) < 1e-5


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
def test_tables():
    assert ps.WEIGHTS.dtype == ps.SDFS.dtype == F and len(ps.WEIGHTS) == 15 and len(ps.SDFS) == 14 and ps.NCLASS == 210
    assert len(set(bits(ps.WEIGHTS).tolist())) == 15 and len(set(bits(ps.SDFS).tolist())) == 14   # 0 and -0 are two states
    assert len({(int(a), int(b)) for a, b in zip(bits(ps.CLASS_W), bits(ps.CLASS_S))}) == 210
    assert float(ps.CARVE_SDF) < 1e-5 < float(ps.succ(ps.CARVE_SDF)) and ps.pred(ps.CARVE_SDF) < ps.CARVE_SDF
    assert ps.pred(5) < 5 < ps.succ(5) and F(ps.succ(5) - F(1)) != F(4.0) and 0 < ps.WEIGHTS[2] < 1.2e-38  # 1e-45: the smallest subnormal
    assert ps.WEIGHTS[2] == np.nextafter(F(0), F(1)) and 0 < abs(ps.SDFS[6]) < 1.2e-38
    assert np.signbit(ps.WEIGHTS[1]) and ps.WEIGHTS[1] == 0 and np.signbit(ps.SDFS[2]) and ps.SDFS[2] == 0
    assert F(ps.WEIGHTS[12] + F(1)) == ps.WEIGHTS[12] == 2.0 ** 24
    assert len(ps.TAME) == 180 and ps.COLOUR_WEIGHTS.tolist() == [0, 1, 6, 7, 8, 9, 127, 253, 254, 255]
    assert len(ps.NONFINITE) == 25 and not np.isfinite(ps.NONFINITE_S[:15]).any() and not np.isfinite(ps.NONFINITE_W[15:]).any()
    assert np.isfinite(ps.NONFINITE_W[:15]).all() and np.isfinite(ps.NONFINITE_S[15:]).all()


def test_the_class_of_a_voxel_hangs_on_its_world_coordinates_alone():
    """the same world voxel through chunks of 8^3 and of 16^3 voxels; both sides of a comparison therefore hold the same field"""
    for cid16 in ((0, 0, 1), (-1, -1, 2)):
        k16 = ps.voxel_class(16, cid16).reshape(16, 16, 16)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    cid8 = (2 * cid16[0] + dx, 2 * cid16[1] + dy, 2 * cid16[2] + dz)
                    k8 = ps.voxel_class(8, cid8).reshape(8, 8, 8)
                    assert np.array_equal(k8, k16[8 * dz:8 * dz + 8, 8 * dy:8 * dy + 8, 8 * dx:8 * dx + 8])
    for family in ("finite", "tame", "nonfinite"):
        a, b = ps.field(8, family), ps.field(8, family, partial=True)
        assert len(a) == 24 and len(b) == 12 and all((sum(cid) % 2 == 0) for cid in b)
        for cid in b:
            for x, y in zip(a[cid], b[cid]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    s, w, c = (np.concatenate([v[j] for v in ps.field(8, "finite").values()]) for j in range(3))
    assert len({(int(x), int(y)) for x, y in zip(bits(s), bits(w))}) == 210
    assert set(c[:, 3].tolist()) == set(ps.COLOUR_WEIGHTS.tolist()) and set(c[:, :3].ravel().tolist()) == set(ps.CHANNELS.tolist())
    s, w, _ = (np.concatenate([v[j] for v in ps.field(8, "tame").values()]) for j in range(3))
    assert ((np.abs(s) <= 0.5) | (s == 99999)).all() and len({(int(x), int(y)) for x, y in zip(bits(s), bits(w))}) == 180
    s, w, _ = (np.concatenate([v[j] for v in ps.field(8, "nonfinite").values()]) for j in range(3))
    bad = ~np.isfinite(s) | ~np.isfinite(w)
    assert abs(bad.mean() - 0.5) < 0.01
    seen = {(int(x), int(y)) for x, y in zip(bits(s[bad]), bits(w[bad]))}
    assert seen == {(int(x), int(y)) for x, y in zip(bits(ps.NONFINITE_S), bits(ps.NONFINITE_W))}
    assert len(ps.block(8, "tilt")) >= 12 and len(ps.block(8)) == 24 and len(ps.block(16)) == 20 and len(ps.block(32)) == 12


# ---- coverage --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_every_class_reaches_every_branch(oracle_mod, N):
    """per entry path: every (weight, distance) class is first touched in the band, and first touched by a carve test, at 8 voxels at least;
    every colour weight meets an in-band voxel 8 times at least; a cloud (few voxels per ray) meets every weight in both regions at 2"""
    row = [N]
    for path in ("depth", "colour"):
        reg = ps.regions(oracle_mod, N, path)
        band, carve = ps.class_counts(reg, N, ps.voxel_class, ps.NCLASS)
        print("coverage %2d^3 %-6s: in band, min per class %5d; carve, min per class %5d" % (N, path, band.min(), carve.min()))
        assert band.min() >= 8 and carve.min() >= 8, (path, band.min(), carve.min())
        row += [int(band.min()), int(carve.min())]
    cw_index = lambda N, cid: np.searchsorted(ps.COLOUR_WEIGHTS, ps.colours(N, cid)[:, 3])
    cband, _ = ps.class_counts(ps.regions(oracle_mod, N, "colour"), N, cw_index, len(ps.COLOUR_WEIGHTS))
    print("coverage %2d^3 colour weights in band, min per weight %5d" % (N, cband.min()))
    assert cband.min() >= 8
    for with_colours in (False, True):
        reg = ps.regions(oracle_mod, N, "cloud", with_colours=with_colours)
        band, carve = ps.class_counts(reg, N, lambda N, cid: ps.voxel_class(N, cid) % ps.NW, ps.NW)
        every, _ = ps.class_counts(reg, N, ps.voxel_class, ps.NCLASS)
        print("coverage %2d^3 cloud%s: in band, min per weight %5d (per class %3d); carve, min per weight %4d" % (
            N, " + colours" if with_colours else "          ", band.min(), every.min(), carve.min()))
        assert band.min() >= 2 and carve.min() >= 2, (with_colours, band.min(), carve.min())
        if with_colours:
            cband, _ = ps.class_counts(reg, N, cw_index, len(ps.COLOUR_WEIGHTS))
            print("coverage %2d^3 cloud + colours: colour weights in band, min per weight %5d" % (N, cband.min()))
            assert cband.min() >= 8


@pytest.mark.parametrize("path,with_colours", [("depth", False), ("colour", False), ("cloud", False), ("cloud", True)])
@pytest.mark.parametrize("N", SIZES)
def test_no_nan_where_bits_are_compared(oracle_mod, N, path, with_colours):
    """`finite` and `tame`: no distance or weight of the oracle's map is a NaN after any frame (infinities occur: 1e30 x 1e30)"""
    for family in ("finite", "tame"):
        books = ps.run_oracle(oracle_mod, N, path, family, with_colours=with_colours)[3]
        assert [b[2] for b in books] == [0] * 6, (family, [b[2] for b in books])


@pytest.mark.parametrize("path,with_colours", [("depth", False), ("colour", False), ("cloud", False), ("cloud", True)])
@pytest.mark.parametrize("N", SIZES)
def test_a_voxel_keeps_its_state_until_a_frame_touches_it(oracle_mod, N, path, with_colours):
    """what the witness calls untouched the other field leaves alone, bit for bit: the regions do not hang on the state"""
    t = Touch(oracle_mod, N, path, with_colours=with_colours)
    for k, (s, w, c) in enumerate(t.after):
        still = (t.first < 0) | (t.first >= k)
        assert (bits(s)[still] == bits(t.s0)[still]).all() and (bits(w)[still] == bits(t.w0)[still]).all()
        assert path == "depth" or (c[still] == t.c0[still]).all()  # (the depth path runs on a map without colour voxels)
    assert (t.first >= 0).sum() > 100


# ---- the edges are live ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_depth_path_edges(oracle_mod, N):
    t = Touch(oracle_mod, N, "depth")
    live = t.carve & (t.w0 > 0)
    m = live & (bits(t.s0) == bits(ps.CARVE_SDF))
    assert m.sum() >= 8 * 12 and t.reset(m)                          # 1e-5f < 1e-5: always reset
    m = live & (bits(t.s0) == bits(ps.succ(ps.CARVE_SDF)))
    assert m.sum() >= 8 * 12 and t.unchanged(m)                      # its successor: never
    m = t.carve & (bits(t.w0) == bits(ps.WEIGHTS[2])) & carves(t.s0)
    assert m.sum() >= 8 * 9 and t.reset(m)                           # weight 1e-45 is a weight
    m = live & carves(t.s0)
    assert t.reset(m) and t.unchanged(live & ~carves(t.s0))
    for w in (ps.WEIGHTS[0], ps.WEIGHTS[1], ps.WEIGHTS[14]):         # 0, -0.0, -0.25 are not, whatever the distance
        m = t.carve & (bits(t.w0) == bits(w))
        assert m.sum() >= 8 * 14 and t.unchanged(m)
    m = t.band & (t.w0 == F(2.0 ** 24))
    assert m.sum() >= 8 * 14 and (t.w1[m] == F(2.0 ** 24)).all()      # 2^24 + 1 rounds back
    assert t.counters[0]["probe"] > 0 and t.counters[0]["carved"] > 0
    assert t.counters[2]["carved"] > 0                                # the first far wall carves behind the near ones


@pytest.mark.parametrize("N", SIZES)
def test_colour_path_edges(oracle_mod, N):
    t = Touch(oracle_mod, N, "colour")
    live = t.carve & carves(t.s0)
    m = live & (bits(t.w0) == bits(ps.pred(5)))
    assert m.sum() >= 8 * 9 and t.reset(m)
    for w in (F(5), ps.succ(5), F(6), F(100), F(2.0 ** 24), F(1e30)):
        m = live & (t.w0 == w)
        assert m.sum() >= 8 * 9
        assert (bits(t.w1)[m] == bits(F(w - F(1)))).all() and (bits(t.s1)[m] == bits(t.s0)[m]).all(), w   # one off, the distance kept
    for w in (ps.WEIGHTS[2], ps.WEIGHTS[3], F(0.5), F(1), F(2.5)):
        m = live & (bits(t.w0) == bits(w))
        assert m.sum() >= 8 * 9 and t.reset(m)
    assert t.unchanged(t.carve & ~((t.w0 > 0) & carves(t.s0)))
    # weight 6 in front of every wall (their nearest point is 1.15 m, the band 0.12 m + 2 sqrt(3) voxels): 6 -> 5 -> 4 -> reset
    m = live & (t.w0 == F(6)) & (t.first == 0) & (t.z < 0.8)
    assert m.sum() >= 8
    assert (t.after[1][1][m] == F(5)).all() and (t.after[2][1][m] == F(4)).all()
    assert (bits(t.after[2][0])[m] == bits(t.s0)[m]).all()
    assert (bits(t.after[3][0])[m] == bits(DEFAULT[0])).all() and (bits(t.after[3][1])[m] == bits(DEFAULT[1])).all()
    # the colour sample: only below weight 8
    cw0, cw1 = t.c0[:, 3], t.c1[:, 3]
    m = t.band & (cw0 == 7)
    assert m.sum() >= 8 and (cw1[m] == 8).all()
    for cw in (0, 1, 6):
        assert (cw1[t.band & (cw0 == cw)] == cw + 1).all()
    m = t.band & (cw0 >= 8)
    assert m.sum() >= 8 * 6 and (t.c1[m] == t.c0[m]).all()
    assert (t.c1[~t.band] == t.c0[~t.band]).all()
    sat0 = int(((t.first == 0) & t.band & (cw0 >= 8)).sum())         # chunks outside the block start at colour weight 0
    assert t.counters[0]["col_sat"] == sat0 > 0 and t.counters[0]["col"] > 0


@pytest.mark.parametrize("N", SIZES)
def test_cloud_path_edges(oracle_mod, N):
    t = Touch(oracle_mod, N, "cloud", with_colours=True)
    cw0, cw1 = t.c0[:, 3], t.c1[:, 3]
    m = t.band & (cw0 == 253)
    assert m.sum() >= 8 and (cw1[m] == 254).all()                    # one sample, then the early return
    m = t.band & (cw0 >= 254)
    assert m.sum() >= 16 and (t.c1[m] == t.c0[m]).all()
    m = t.band & (cw0 == 9)
    assert m.sum() >= 8 and (cw1[m] > 9).all()                       # no limit at 8 on this path
    only_carve = t.region == ps.CARVE
    for w in (ps.WEIGHTS[0], ps.WEIGHTS[1], ps.WEIGHTS[14]):
        m = only_carve & (bits(t.w0) == bits(w))
        assert m.sum() >= 2 and t.unchanged(m)
    m = only_carve & (bits(t.w0) == bits(ps.WEIGHTS[2]))
    assert m.sum() >= 2 and (t.w1[m] >= 5).all() and (t.w1[m] % 5 == 0).all()       # Integrate(1e-5, 5) from weight 1e-45 on
    m = only_carve & (t.w0 > 0)
    assert (t.w1[m] > t.w0[m]).sum() > 0 and (t.w1[m] >= t.w0[m]).all()
    assert t.counters[0]["carved"] > 0 and t.counters[0]["sdf"] > 0


# ---- residency ---------------------------------------------------------------------------------------------------------------------------------
def _carve_only_chunks(reg):
    """chunks of the block in which frame 0 makes carve tests and nothing else"""
    return [cid for cid in reg.ids if reg.carve[0][cid].any() and not reg.band[0][cid].any()]


@pytest.mark.parametrize("path", ps.PATHS)
def test_resident_but_empty_chunks(oracle_mod, path):
    """a chunk of default voxels in a carve-only region: the frame tests its voxels (the probe counter of the image paths counts the tests
    on resident chunks only), changes nothing, and the chunk stays; an absent chunk there stays absent"""
    N = 8
    reg = ps.regions(oracle_mod, N, path)
    only = _carve_only_chunks(reg)
    if path == "cloud":  # a ray is walked through its band only: the few carve tests at its near end fall into chunks that it also updates
        assert not only
    else:
        assert len(only) >= 4 and any(ps.is_uploaded(cid, True) for cid in only) and not all(ps.is_uploaded(cid, True) for cid in only)
    fld, states, counters, books = ps.run_oracle(oracle_mod, N, path, "default", full=True)
    before, after = states[0], states[1]
    changed = 0
    for cid in after:
        same = cid in before and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before[cid], after[cid]))
        changed += not same
        if cid in only:
            assert same
    assert all(cid in after for cid in only)
    assert counters[0]["updated_chunks"] == changed
    if path == "cloud":  # (a later ray of the same cloud can carve what an earlier one gave a weight)
        assert counters[0]["visited"] == reg.counters[0]["visited"] > 0
    else:  # every test on the witness carves, and on the witness as here the tests on chunks made by this frame are not counted
        assert counters[0]["probe"] == reg.counters[0]["probe"] == reg.counters[0]["carved"] > 0 and counters[0]["carved"] == 0
    _, pstates, pcounters, pbooks = ps.run_oracle(oracle_mod, N, path, "default", partial=True, full=True)
    for cid in only:
        assert (cid in pstates[1]) == ps.is_uploaded(cid, True), cid
    if path != "cloud":
        assert 0 < pcounters[0]["probe"] < counters[0]["probe"]
