"""GPU tests of the stereo matcher's raw-image path at the sizes and point sets test_gpu_stereo_prep.py does not reach: the
minimum work size 9 x 9, work sizes with partial 16 x 16 tiles in both directions, every route of the two resizes (copy, exact
halving, upscale, non-integer downscale), point counts around the rasteriser's chunk of 256, hundreds of points piled on one
pixel across two chunks, positions that fit no int and depths of 0, NaN and inf.  Every prepared input and both depth maps are
compared bit for bit with tests/stereo_prep_restated.py chained into the vectorised restatement."""
import ctypes as C

import numpy as np
import pytest

import stereo_cases as sc
import stereo_prep_restated as pr
import stereo_restated as sr
from test_gpu_stereo_prep import GpuRaw, camera, random_image, random_pose, run_raw_sequence

pytestmark = pytest.mark.gpu
f32 = np.float32


def restated(W, H):
    return pr.RawStereo(sr.VectorisedStereo(W, H), W, H)


def assert_same_states(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for i, ((name, g), (_, w)) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, name)
        if not sr.same_bits(g, w):
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            idx = tuple(np.argwhere(bad)[0])
            pytest.fail("state %d (%s): %d entries differ, first at %s: gpu %r cpu %r" % (i, name, bad.sum(), idx, g[idx], w[idx]))


# work size, camera size, points per frame (the counts of stereo_cases.COUNTS, one per geometry)
GEOMETRY = [
    (9, 9, 9, 9, 1),            # set_camera's minimum: the Sobel's reflected apron inside one tile; both resizes copy
    (37, 29, 74, 58, 255),      # partial tiles in x and y; the 8-bit frame halves exactly (INTER_AREA), the depth doubles
    (37, 29, 37, 29, 256),      # the copy routes of both resizes
    (64, 48, 32, 24, 257),      # the camera half the work size: the 8-bit frame is upscaled, the depth halves exactly
    (40, 30, 31, 23, 0),        # a camera smaller by an odd ratio: 8-bit upscale, non-integer downscale of the depth
    (161, 121, 200, 150, 513),  # one above a tested size: W % 16 = 1, H % 16 = 9
]
assert sorted(g[4] for g in GEOMETRY) == sorted(sc.COUNTS)


@pytest.mark.parametrize("W,H,real_w,real_h,n", GEOMETRY)
def test_raw_path_matches_the_restatement_at_odd_sizes(hip_lib, W, H, real_w, real_h, n):
    want = run_raw_sequence(restated(W, H), W, H, real_w, real_h, 5, n)
    got = run_raw_sequence(GpuRaw(W, H), W, H, real_w, real_h, 5, n)
    assert {"ref", "p2w", "mask_x", "mask_y", "match", "sparse_depth", "sparse_dist", "depth", "depth_real"} <= {k for k, _ in want}
    assert_same_states(got, want)
    if n >= 255:
        assert (dict(want)["sparse_depth"] > 0).sum() > 50


def run_point_sets(obj, W, H, real_w, real_h, seed):
    """one reference and one match frame, then every point set of stereo_cases.point_sets (built on the object's own gradient
    masks) bound and put out in turn -> ([(name, array)], {set name: (depths, points)})"""
    rng = np.random.default_rng(seed)
    K, D = camera(real_w, real_h)
    obj.set_camera(real_w, real_h, K, D, K, D)
    ref_pose = random_pose(rng)
    obj.set_reference_image(random_image(rng, real_w, real_h))
    obj.update_image(random_image(rng, real_w, real_h), ref_pose, random_pose(rng))
    mask_x, mask_y = np.array(obj.mask_x, copy=True), np.array(obj.mask_y, copy=True)
    out, sets = [("mask_x", mask_x), ("mask_y", mask_y)], {}
    for name, d, p in sc.point_sets(mask_x, mask_y, W, H, real_w, real_h):
        obj.bind_sparse_points(d, p)
        obj.output_image()
        out += [(name + ":" + k, np.array(getattr(obj, k), copy=True)) for k in ("sparse_depth", "sparse_dist", "depth", "depth_real")]
        sets[name] = (d, p)
    return out, sets


@pytest.mark.parametrize("W,H,real_w,real_h", [(37, 29, 74, 58), (64, 48, 32, 24), (80, 60, 94, 60)])
def test_raw_path_matches_the_restatement_on_the_point_sets(hip_lib, W, H, real_w, real_h):
    want, sets = run_point_sets(restated(W, H), W, H, real_w, real_h, 9)
    got, _ = run_point_sets(GpuRaw(W, H), W, H, real_w, real_h, 9)
    assert_same_states(got, want)
    named = dict(want)
    # the restatement's own maps show what the sets reach: the pile's pixel ends on the last point, of the second chunk
    d, p, (cx, cy) = sc.pile(sc.quiet_pixel(named["mask_x"], named["mask_y"]), W, H, real_w, real_h)
    assert np.array_equal(d, sets["pile"][0]) and len(d) > sc.CHUNK
    assert named["pile:sparse_depth"][cy, cx] == f32(d[-1])
    assert (named["unfit:sparse_depth"] > 0).sum() > 50
    odd = named["odd-depths:sparse_depth"][named["odd-depths:sparse_dist"] > 0]
    assert np.isnan(odd).any() and np.isinf(odd).any() and (odd == 0).any() and (odd < 0).any()


def test_raw_path_is_deterministic_at_an_odd_size(hip_lib):
    a = run_raw_sequence(GpuRaw(37, 29), 37, 29, 74, 58, 21, 300)
    b = run_raw_sequence(GpuRaw(37, 29), 37, 29, 74, 58, 21, 300)
    assert len(a) == len(b) > 0
    for (_, x), (_, y) in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_set_camera_work_size_limit(hip_lib):
    """the raw path needs a work size of at least 9 x 9 (the 9-tap Sobel's border): 8 x 9 and 9 x 8 are refused, 9 x 9 is taken"""
    from cvids_amd.chisel import StereoMapper
    K4, D5 = (C.c_double * 4)(60.0, 60.0, 40.0, 30.0), (C.c_double * 5)()
    for W, H, rc in [(8, 9, 1), (9, 8, 1), (9, 9, 0)]:
        m = StereoMapper(W, H)
        assert hip_lib.chisel_hip_stereo_set_camera(m.h, 80, 60, K4, D5, K4, D5) == rc, (W, H)
