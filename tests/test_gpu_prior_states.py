"""GPU parity of integrate_kernel and cloud_integrate_kernel on voxel states they did not make themselves (tests/prior_states.py): the same
hand-built field goes into the oracle (put_chunk) and into the map (AddChunk), the same frames go over both, and after every frame -- or
every launch set -- the counters, the chunk id sets, every bit of every voxel and the sets of meshes_to_update are compared.  Distances and
weights are compared as uint32, so the sign of a zero and every infinity count.  tests/test_prior_states.py shows on the oracle alone that
every class of state reaches every branch, and that the oracle's answers at the edges are the reference's."""
import numpy as np
import pytest

from cvids_amd import synth
from tests import prior_states as ps
from tests.common import compare_meshes, fields_of, same_bits, upload
from tests.merge_restated import assert_fields_bit_equal
from tests.test_gpu_configs import _color_rig
from tests.test_gpu_parity import _mk

pytestmark = pytest.mark.gpu
COUNTERS = ("sdf", "col", "col_sat", "probe", "carved", "updated_chunks")
CLOUD_PAIRS = (("sdf", "sdf"), ("carved", "carved"), ("visited", "probe"), ("candidates", "work_chunks"), ("updated_chunks", "updated_chunks"))
MAX_CHUNKS = {8: 8192, 16: 8192, 32: 2048}
SIZES = (8, 16, 32)


def _oracle_fields(om):
    N = om.chunk_size[0]
    return {cid: (s, w, c if c is not None else np.zeros((N ** 3, 4), np.uint8)) for cid, (s, w, c) in om.fields().items()}


def _same_maps(om, gm, what, nan_ok=False):
    """chunk id sets, every voxel bit for bit (with `nan_ok`: NaN in the same places, the bits everywhere else), meshes_to_update"""
    N = om.chunk_size[0]
    want, got = _oracle_fields(om), fields_of(gm, N)
    assert om.num_chunks() == gm.NumChunks() == len(got), what
    if nan_ok:
        assert sorted(want) == sorted(got), "%s: chunk ids differ" % what
        for cid in sorted(want):
            same_bits(got[cid][0], want[cid][0], "%s chunk %s sdf" % (what, cid))
            same_bits(got[cid][1], want[cid][1], "%s chunk %s weight" % (what, cid))
            assert np.array_equal(got[cid][2], want[cid][2]), "%s chunk %s: colours differ" % (what, cid)
    else:
        assert_fields_bit_equal(want, got, True, what)
    assert ps.dirty(om) == sorted(map(tuple, gm.GetMeshesToUpdate().tolist())), "%s: meshes_to_update differ" % what
    return want


class Case:
    """one field under one path: the oracle and the map side by side"""

    def __init__(self, oracle_mod, N, path, family, pose="front", partial=False, use_color=None, weight=1.0, trunc=("constant", ps.TRUNCATION),
                 channels=3, rig=False, with_colours=False, nan_ok=False):
        self.N, self.path, self.pose, self.with_colours, self.nan_ok = N, path, pose, with_colours, nan_ok
        color = path != "depth" if use_color is None else use_color
        self.om, self.gm, self.integ = _mk(oracle_mod, N, ps.RES[N], color, trunc=trunc, weight=weight, carving=True, carving_dist=0.0,
                                           max_chunks=MAX_CHUNKS[N])
        self.cam = ps.camera()
        self.intr = (self.cam.fx, self.cam.fy, self.cam.cx, self.cam.cy)
        self.color_img = ps.colour_image(channels) if path == "colour" else None
        self.ccam, self.offset = (self.cam, None)
        if rig:  # a colour camera of its own, beside the depth camera
            self.ccam, self.offset = _color_rig(ps.W, ps.H, 80, 60)
            self.color_img = synth.render_color(80, 60, channels)
        self.field = ps.field(N, family, pose, partial)
        ps.put(self.om, self.field)
        upload(self.gm, self.field)
        self.gm.counters(reset=True)
        self.frames = ps.clouds(pose, with_colours) if path == "cloud" else ps.depth_frames(pose)
        _same_maps(self.om, self.gm, "after the upload", nan_ok)
        assert len(self.gm.GetMeshesToUpdate()) == 0

    def _cpose(self, p):
        return p if self.offset is None else (np.asarray(p, np.float64) @ self.offset).astype(np.float32)

    def _oracle_frame(self, t):
        om = self.om
        if self.path == "cloud":
            pts, col, p = self.frames[t]
            om.integrate_pointcloud(pts, p, col, ps.TRUNCATION, ps.MAX_DIST)
        elif self.path == "depth":
            d, p = self.frames[t]
            om.integrate_depth(d, p, self.intr, self.cam.near_plane, self.cam.far_plane)
        else:
            d, p = self.frames[t]
            cc = self.ccam
            om.integrate_depth_color(d, p, self.intr, self.color_img, color_pose=self._cpose(p), color_intr=(cc.fx, cc.fy, cc.cx, cc.cy),
                                     near=self.cam.near_plane, far=self.cam.far_plane)
        return om.counters()

    def run(self, batch=1):
        """all frames, `batch` per launch set (the oracle frame by frame), everything compared after every launch set -> counter totals"""
        gm, total = self.gm, {}
        for lo in range(0, len(self.frames), batch):
            ts = list(range(lo, min(lo + batch, len(self.frames))))
            oc = {}
            for t in ts:
                for k, v in self._oracle_frame(t).items():
                    oc[k] = oc.get(k, 0) + v
            if self.path == "cloud":
                assert batch == 1
                pts, col, p = self.frames[lo]
                gm.IntegratePointCloud(self.integ, (pts, col), p, ps.TRUNCATION, ps.MAX_DIST)
            elif batch == 1 and self.path == "depth":
                gm.IntegrateDepthScan(self.integ, self.frames[lo][0], self.frames[lo][1], self.cam)
            elif batch == 1:
                d, p = self.frames[lo]
                gm.IntegrateDepthScanColor(self.integ, d, p, self.cam, self.color_img, self._cpose(p), self.ccam)
            else:
                part = [self.frames[t] for t in ts]
                gm.IntegrateBatch(self.integ, [(d, p, self.cam) for d, p in part],
                                  None if self.path == "depth" else [(self.color_img, self._cpose(p), self.ccam) for _, p in part])
            gc = gm.counters(reset=True)
            what = "%s %d^3 frames %d..%d" % (self.path, self.N, ts[0], ts[-1])
            pairs = CLOUD_PAIRS if self.path == "cloud" else tuple((k, k) for k in COUNTERS)
            for a, b in pairs:
                assert oc[a] == gc[b], "%s counter %s: oracle %d gpu %d" % (what, a, oc[a], gc[b])
            assert oc["created"] - oc["collected"] == gc["new_chunks"], "%s: chunks made %d - %d, gpu %d" % (what, oc["created"], oc["collected"], gc["new_chunks"])
            self.last = _same_maps(self.om, gm, what, self.nan_ok)
            for k, v in oc.items():
                total[k] = total.get(k, 0) + v
        return total

    def meshes(self):
        self.om.update_meshes(force=True)
        self.gm.UpdateMeshes(force=True)
        n, nv = compare_meshes(self.om, self.gm, self.om.use_color)
        assert len(self.gm.GetMeshesToUpdate()) == 0 and len(self.om.meshes_to_update()) == 0
        return n, nv


# ---- a. depth only ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_depth_frames_over_every_state(oracle_mod, N):
    tot = Case(oracle_mod, N, "depth", "finite").run()
    assert tot["sdf"] > 1000 and tot["carved"] > 100 and tot["probe"] > tot["carved"]


@pytest.mark.parametrize("variant", ["partial", "tilt", "nonfinite", "colour_voxels"])
def test_depth_frames_variants(oracle_mod, variant):
    """every second chunk absent; a tilted pose with a block of its own; NaN and infinite distances and weights; a map that keeps colour
    voxels, which a depth frame must hand back untouched"""
    c = Case(oracle_mod, 8, "depth", "nonfinite" if variant == "nonfinite" else "finite", pose="tilt" if variant == "tilt" else "front",
             partial=variant == "partial", use_color=variant == "colour_voxels", nan_ok=variant == "nonfinite")
    tot = c.run()
    assert tot["sdf"] > 1000 and tot["carved"] > 50
    if variant == "colour_voxels":
        got = c.gm.fields()
        for cid, (_, _, rgbw) in c.field.items():
            assert np.array_equal(got[cid][2], rgbw), cid


# ---- b. depth and colour -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [1.0, 2.0])
@pytest.mark.parametrize("N", SIZES)
def test_colour_frames_over_every_state(oracle_mod, N, weight):
    """weighter 1.0: the short reciprocal of the weight update (WI_FASTWU); 2.0: the IEEE division"""
    tot = Case(oracle_mod, N, "colour", "finite", weight=weight).run()
    assert tot["sdf"] > 1000 and tot["carved"] > 100 and tot["col"] > 1000 and tot["col_sat"] > 100


@pytest.mark.parametrize("variant", ["mono", "rgba", "colour_camera", "partial", "nonfinite", "inverse"])
def test_colour_frames_variants(oracle_mod, variant):
    kw = {"mono": dict(channels=1), "rgba": dict(channels=4), "colour_camera": dict(rig=True), "partial": dict(partial=True),
          "nonfinite": dict(nan_ok=True), "inverse": dict(trunc=("inverse", 2.0))}[variant]
    tot = Case(oracle_mod, 8, "colour", "nonfinite" if variant == "nonfinite" else "finite", **kw).run()
    assert tot["sdf"] > 1000 and tot["carved"] > 50 and tot["col"] > 500 and tot["col_sat"] > 50


# ---- c. launch sets --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 5])
@pytest.mark.parametrize("path", ["depth", "colour"])
def test_launch_sets_over_every_state(oracle_mod, path, batch):
    """a voxel's state stays in registers from frame to frame of a set: integrate, then carve; a weight of 6 that goes 5, 4, reset"""
    tot = Case(oracle_mod, 8, path, "finite").run(batch=batch)
    assert tot["sdf"] > 1000 and tot["carved"] > 100


# ---- d. schedules ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["vpl2", "vpl4", "uncertain", "pipeline"])
@pytest.mark.parametrize("N", SIZES)
def test_schedules_over_every_state(oracle_mod, N, mode, monkeypatch):
    """both granularities, and the two forms in which the kernel looks a chunk up itself and so decides itself whether a unit starts from
    the chunk's voxels or from default registers; every second chunk of the block is absent"""
    name, value = {"vpl2": ("CHISEL_HIP_VPL", "2"), "vpl4": ("CHISEL_HIP_VPL", "4"), "uncertain": ("CHISEL_HIP_FORCE_UNCERTAIN", "1"),
                   "pipeline": ("CHISEL_HIP_FORCE_PIPELINE", "1")}[mode]
    monkeypatch.setenv(name, value)
    tot = Case(oracle_mod, N, "colour", "finite", partial=True).run(batch=2 if mode in ("uncertain", "pipeline") else 1)
    assert tot["sdf"] > 1000 and tot["carved"] > 50


# ---- e. clouds -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_colours", [False, True])
@pytest.mark.parametrize("N", SIZES)
def test_clouds_over_every_state(oracle_mod, N, with_colours):
    tot = Case(oracle_mod, N, "cloud", "finite", with_colours=with_colours).run()
    assert tot["sdf"] > 1000 and tot["carved"] > 50


@pytest.mark.parametrize("with_colours", [False, True])
@pytest.mark.parametrize("variant", ["partial", "nonfinite"])
def test_clouds_variants(oracle_mod, variant, with_colours):
    tot = Case(oracle_mod, 8, "cloud", "nonfinite" if variant == "nonfinite" else "finite", partial=variant == "partial",
               with_colours=with_colours, nan_ok=variant == "nonfinite").run()
    assert tot["sdf"] > 1000 and tot["carved"] > 20


# ---- f. resident but empty ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partial", [False, True])
@pytest.mark.parametrize("path", ps.PATHS)
def test_resident_chunks_of_default_voxels(oracle_mod, path, partial):
    """a resident chunk that holds nothing, where the frame can only carve: its carve tests count (`probe`), it is not updated and it
    stays, bit for bit; where the chunk is absent nothing is made"""
    reg = ps.regions(oracle_mod, 8, path)
    only = [cid for cid in reg.ids if reg.carve[0][cid].any() and not reg.band[0][cid].any()]
    c = Case(oracle_mod, 8, path, "default", partial=partial)
    c.frames = c.frames[:1]
    tot = c.run()
    got = fields_of(c.gm, 8)
    for cid in only:
        assert (cid in got) == ps.is_uploaded(cid, partial), cid
        if cid in got:
            assert (got[cid][0] == np.float32(99999.0)).all() and not got[cid][1].view(np.uint32).any() and not got[cid][2].any()
    if path != "cloud":
        assert len(only) >= 4 and tot["probe"] > 0 and tot["carved"] == 0
        assert partial or tot["probe"] == reg.counters[0]["probe"]
    c.frames = ps.depth_frames()[1:] if path != "cloud" else ps.clouds()[1:]
    c.run()


# ---- g. the mesher afterwards ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,with_colours", [("depth", False), ("colour", False), ("cloud", True)])
@pytest.mark.parametrize("N", SIZES)
def test_meshes_of_uploaded_chunks_that_frames_changed(oracle_mod, N, path, with_colours):
    """the dirty flags, the 27-neighbourhood listing and the sign summary of an uploaded chunk that integration then changes: a recompute
    after two frames and one at the end, every mesh array bit for bit"""
    c = Case(oracle_mod, N, path, "tame", with_colours=with_colours)
    frames = c.frames
    c.frames = frames[:2]
    c.run()
    n, nv = c.meshes()
    assert n > 4 and nv > 100
    c.frames = frames[2:]
    c.run()
    n, nv = c.meshes()
    assert n > 4 and nv > 100
