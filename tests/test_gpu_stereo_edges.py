"""GPU tests of the stereo matcher at the shapes, parameters and values the parity tests of test_gpu_stereo.py do not reach: work
sizes with tails in every kernel (scanlines that are no multiple of the SGM ring, line and pixel counts that leave idle waves,
an odd pixel count, scanlines shorter than the ring), and the cases of tests/stereo_cases.py -- WTA ties, the variance rejection,
non-default SGM penalties on a smooth reference, denominators that are negative or exactly zero, the sparse prior's edge values,
twelve measurements.  Every comparison is bit for bit with the vectorised CPU restatement; tests/test_stereo_cases.py shows on the
CPU that each case reaches its branch."""
import numpy as np
import pytest

import stereo_cases as sc
import stereo_restated as sr
from test_gpu_stereo import GpuStereo
from test_stereo_restated import run_sequence

pytestmark = pytest.mark.gpu


class GpuStereoWith(GpuStereo):
    """GpuStereo created with StereoParams: the restatement's keyword parameters over the library's defaults"""

    def __init__(self, W, H, **params):
        from cvids_amd.chisel import StereoMapper, stereo_default_params
        p = stereo_default_params()
        for k, v in params.items():
            assert hasattr(p, k), k
            setattr(p, k, float(v))
        self.m = StereoMapper(W, H, params=p)


def assert_same_states(got, want):
    assert [n for n, _ in got] == [n for n, _ in want]
    for k, ((name, g), (_, w)) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (k, name)
        if not sr.same_bits(g, w):
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            idx = tuple(np.argwhere(bad)[0])
            pytest.fail("state %d (%s): %d entries differ, first at %s: gpu %r cpu %r" % (k, name, bad.sum(), idx, g[idx], w[idx]))


# work size -> seeds.  2 x 2 is create's minimum; 5 x 12 and 12 x 5 have scanlines shorter than the SGM ring of 8 in one direction
# and 5 x 3 in both; 37 x 29 is odd in both dimensions with an odd pixel count; 161 x 121 sits one above a tested size with
# W % 8 = 1 and H % 4 = 1; 515 x 3 and 3 x 515 are one long scanline direction against one of three steps.
SHAPES = [(2, 2, (7, 8)), (5, 3, (7, 8)), (5, 12, (7, 8)), (12, 5, (7, 8)), (37, 29, (7, 8)), (515, 3, (7, 8)), (3, 515, (7, 8)), (161, 121, (7,))]
ACCEPTING = {(37, 29): 0.2, (161, 121): 0.2}     # the restatement's share of accepted depths in its last output (none at the tiny sizes)


@pytest.mark.parametrize("W,H,seed", [(W, H, s) for W, H, seeds in SHAPES for s in seeds])
def test_stereo_matches_the_restatement_at_odd_shapes(hip_lib, W, H, seed):
    want = run_sequence(sr.VectorisedStereo, W, H, seed)
    got = run_sequence(GpuStereo, W, H, seed)
    assert_same_states(got, want)
    if (W, H) in ACCEPTING:
        assert (sc.last(want, "depth") != 1000).mean() > ACCEPTING[(W, H)]


SIZES = [(48, 32), (45, 27)]     # every dimension a multiple of 8; every dimension and the pixel count odd
CASES = [c for W, H in SIZES for c in sc.float_cases(W, H)]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_stereo_case_matches_the_restatement(hip_lib, case):
    """the cost after every update, and the fused cost, the SGM volume and the depth after the output"""
    want = sc.run_case(sr.VectorisedStereo, case)
    got = sc.run_case(GpuStereoWith, case)
    assert {"cost", "sgm", "depth"} <= {n for n, _ in want}
    assert_same_states(got, want)


def test_stereo_params_reach_the_kernels(hip_lib):
    """a parameter set that the binding dropped would give the default volume: the restatement's two volumes differ, and the
    library's follows the non-default one"""
    case = sc.smooth(45, 27, sc.SGM_SETS[0])
    plain = sc.Case("plain", 45, 27, {}, case.steps)
    got, base = sc.run_case(GpuStereoWith, case), sc.run_case(GpuStereoWith, plain)
    assert not sr.same_bits(sc.last(got, "sgm"), sc.last(base, "sgm"))
    assert_same_states(base, sc.run_case(sr.VectorisedStereo, plain))


def test_odd_size_runs_are_deterministic(hip_lib):
    a = run_sequence(GpuStereo, 37, 29, 11)
    b = run_sequence(GpuStereo, 37, 29, 11)
    assert len(a) == len(b) > 0
    for (_, x), (_, y) in zip(a, b):
        assert x.tobytes() == y.tobytes()
