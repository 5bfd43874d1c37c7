"""The restatement of chisel_hip_merge_map (tests/merge_restated.py) against the reference's own GetSDF and voxel updates, what its cases
reach, and the declaration of the entry point.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import merge_restated as mr
from tests import voxel_fields as vf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mr.case_names()
_id = lambda c: "%d-%s-%s" % c


@pytest.fixture(scope="module")
def source_oracles(oracle_mod):
    """the source field of every chunk size in an OracleMap, built once"""
    maps = {}
    for N in (8, 16, 32):
        src = mr.case(N, "identity", "empty")[0]
        om = oracle_mod.OracleMap(N, mr.RES[N], True)
        for cid, (s, w, c) in src.items():
            om.put_chunk(cid, s, w, c)
        maps[N] = om
    return maps


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "empty"], ids=_id)
def test_source_voxel_is_the_one_getsdf_reads(source_oracles, case):
    """rule 3 tied to the reference: at every destination voxel the restatement visits (every chunk of the moved source's bounding box
    plus a margin), ChunkManager::GetSDF at the same float32 position finds what the restatement picks"""
    N, name, _ = case
    detail = mr.merged(*case)[2]
    om = source_oracles[N]
    total = found_total = 0
    for cid, d in detail.items():
        found, sdf, _ = om.query_points(d["p"], gradient=False)
        got = (found & 1).astype(bool)
        assert np.array_equal(got, d["observed"]), "chunk %s: found differs at %d positions" % (cid, int((got != d["observed"]).sum()))
        assert np.array_equal(sdf[got], d["sdf"][got].astype(np.float64)), "chunk %s: another voxel was picked" % (cid,)
        total += len(got)
        found_total += int(got.sum())
    assert found_total > 1000 and total > 10 * found_total // 4, (total, found_total)


def test_voxel_updates_are_the_reference_s(oracle_mod):
    """the float32 formulas of the restatement against the reference's DistVoxel::Integrate / ColorVoxel::Integrate on values drawn from
    the cases' own fields (both branches of the colour-saturation test among them)"""
    src, dst, _, _ = mr.case(8, "identity", "dense")
    s = np.concatenate([v[0] for v in src.values()])[:400]
    w = np.concatenate([v[1] for v in src.values()])[:400]
    ds = np.concatenate([v[0] for v in dst.values()])[:400]
    dw = np.concatenate([v[1] for v in dst.values()])[:400]
    ns, nw = mr.dist_integrate(ds, dw, s, w)
    for i in range(400):
        a, b = oracle_mod.dist_integrate(ds[i], dw[i], s[i], w[i])
        assert np.float32(a).tobytes() == ns[i].tobytes() and np.float32(b).tobytes() == nw[i].tobytes(), i
    c = np.concatenate([v[2] for v in src.values()])[:600]
    dc = np.concatenate([v[2] for v in dst.values()])[:600]
    dc[:8, 3] = (0, 1, 254, 255, 0, 128, 127, 200)
    c[:8, 3] = (255, 254, 1, 1, 1, 127, 127, 55)
    new, early = mr.color_integrate(dc, c)
    assert early.any() and (~early).any()
    for i in range(600):
        want = oracle_mod.color_integrate(tuple(int(v) for v in dc[i]), int(c[i, 0]), int(c[i, 1]), int(c[i, 2]), int(c[i, 3]))
        assert tuple(int(v) for v in new[i]) == tuple(want), (i, dc[i], c[i], new[i], want)


@pytest.mark.parametrize("N", [8, 16, 32])
def test_identity_into_an_empty_map(N):
    """the source's chunk set, its weights exactly (0 + w) where observed, and sdf = dist_integrate(99999, 0, s, w)"""
    src = mr.case(N, "identity", "empty")[0]
    out, stats, _ = mr.merged(N, "identity", "empty")
    assert sorted(out) == sorted(src) and stats["dst_chunks_created"] == len(src) == stats["src_chunks"]
    for cid, (s, w, c) in src.items():
        obs = w.astype(np.float64) > 1e-12
        gs, gw, gc = out[cid]
        assert mr.same_bits(gw[obs], w[obs]) and not gw[~obs].any() and (gs[~obs] == mr.DEFAULT_SDF).all()
        want = mr.dist_integrate(np.full(int(obs.sum()), mr.DEFAULT_SDF), np.zeros(int(obs.sum()), np.float32), s[obs], w[obs])[0]
        assert mr.same_bits(gs[obs], want)
        assert not gc[~obs].any()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cases_reach_what_they_are_built_for(case):
    """counted from the restatement alone.  The one exception is stated here: a single source chunk (N = 16, 32) merged at identity into the
    dense chunk of the same id can create nothing -- that case is there for the larger chunk's updates of an existing chunk."""
    N, name, kind = case
    r = mr.reach(*case)
    print(case, r)
    if not (kind == "dense" and name == "identity" and N > 8):
        assert r["created"] >= 1
    if name in mr.ROTATED:
        assert r["candidates_not_created"] >= 1
    if kind == "dense":
        assert r["updated_in_existing"] >= 1
    assert r["weight_edge_below"] >= 1 and r["weight_edge_above"] >= 1
    assert r["color_early"] >= 1 and r["color_applied"] >= 1 and r["color_weight_zero"] >= 1
    src, dst = mr.case(*case)[:2]
    classes = vf.weight_classes(src)
    assert float(vf.W_EDGE) in classes and float(vf.W_EDGE_NEXT) in classes


def test_colour_only_on_one_side_leaves_the_destination_s_colours():
    src, dst, _, _ = mr.case(8, "rpy_neg", "dense")
    for dc, sc in ((True, False), (False, True)):
        out, stats, _ = mr.merged(8, "rpy_neg", "dense", dc, sc)
        assert stats["col"] == 0 and stats["voxels_updated"] > 0
        for cid, v in out.items():
            assert mr.same_bits(v[2], dst[cid][2] if cid in dst else np.zeros((8 ** 3, 4), np.uint8))


def test_header_and_mirror_declare_the_entry_point():
    from cvids_amd import capi
    txt = open(os.path.join(ROOT, "include", "chisel_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+chisel_hip_merge_map\s*\(\s*chisel_hip_map\s*\*\s*dst\s*,\s*chisel_hip_map\s*\*\s*src\s*,\s*const\s+float\s+src_to_dst\[12\]", code)
    assert re.search(r"int64_t\s+src_chunks\s*,\s*dst_chunks_created\s*,\s*dst_chunks_updated\s*,\s*voxels_updated\s*;\s*}\s*chisel_hip_merge_stats", code)
    assert "chisel_hip_merge_map" in capi.EXPORTS
    assert ctypes.sizeof(capi.MergeStats) == 32
    assert [n for n, _ in capi.MergeStats._fields_] == ["src_chunks", "dst_chunks_created", "dst_chunks_updated", "voxels_updated"]
