"""What the GPU tests of chisel_hip_deintegrate_depth and chisel_hip_deintegrate_batch share (TEST INFRASTRUCTURE): maps, integrators and
cameras of the restatement's cases (tests/deintegrate_restated.py), and take_out, one frame de-integrated on the GPU and in the
restatement with everything of the contract compared."""
from tests import deintegrate_restated as dr
from tests import merge_restated as mr
from tests.common import fields_of

MAX_CHUNKS = {8: 4096, 16: 4096, 32: 1024}
W, H = dr.W, dr.H


def integrator(rules):
    from cvids_amd import chisel as ch
    cls = {0: ch.ConstantTruncator, 1: ch.InverseTruncator, 2: ch.QuadraticTruncator}[rules.kind]
    return ch.ProjectionIntegrator(cls(float(rules.param)), ch.ConstantWeighter(float(rules.weight)), float(rules.carving_dist), rules.carving)


def pinhole(cam):
    from cvids_amd.chisel import PinholeCamera
    return PinholeCamera(cam[0], cam[1], cam[2], cam[3], W, H, cam[4], cam[5])


def new_map(N, color, **kw):
    from cvids_amd import chisel as ch
    return ch.Chisel((N, N, N), dr.GRIDS[N], color, max_chunks=kw.pop("max_chunks", MAX_CHUNKS[N]), **kw)


def integrate(gm, rules, frames, cam):
    integ, camera = integrator(rules), pinhole(cam)
    for depth, pose, _ in frames:
        if rules.color_rules:
            gm.IntegrateDepthScanColor(integ, depth, pose, camera, dr.color_image(), pose, camera)
        else:
            gm.IntegrateDepthScan(integ, depth, pose, camera)


def dirty(gm):
    return set(map(tuple, gm.GetMeshesToUpdate().tolist()))


def neighbourhoods(ids):
    return {(x + dx, y + dy, z + dz) for x, y, z in ids for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)}


def take_out(gm, frame, rules, cam, N, **kw):
    """the frame de-integrated on the GPU and in the restatement, from the fields the map holds now; everything of the contract
    compared -> (restated field, restated stats, restated detail, what the call returned)"""
    before, listed = fields_of(gm, N), dirty(gm)
    counters = gm.counters()
    want, wstats, detail = dr.restated_deintegrate(before, frame, rules, N, dr.GRIDS[N])
    got = gm.DeintegrateDepthScan(integrator(rules), frame[0], frame[1], pinhole(cam), color_rules=rules.color_rules, **kw)
    print(wstats, dr.reach(detail))
    assert {k: got[k] for k in dr.STAT_NAMES} == wstats, (got, wstats)
    assert sorted(map(tuple, got["emptied_ids"].tolist())) == detail["emptied"]
    after = fields_of(gm, N)
    if kw.get("collect"):
        want = {cid: v for cid, v in want.items() if cid not in set(detail["emptied"])}
    mr.assert_fields_bit_equal(want, after, True, "after the de-integration")  # (sdf, weight, and rgbw as it was)
    assert gm.counters() == counters  # CHISEL_HIP_CNT_* count forward executions
    touched = {cid for cid, p in detail["chunks"].items() if p["touched"]}
    if not kw.get("collect"):
        assert dirty(gm) == listed | (neighbourhoods(touched) if touched else set())
    return want, wstats, detail, got
