"""The numpy restatement of chisel_hip_distance_field (tests/distance_restated.py) against itself, on the CPU: the definition as written
(`brute`) equals the three passes (`separable`) exactly, the sparse maps contain what the GPU tests claim they reach, a window's answer
does not depend on where the window lies, and the host-only header (cvids_amd/csrc/distance_checks.h) holds in a stand-alone program
under the address and undefined-behaviour sanitizers."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import distance_restated as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.0625
BASE = (-2, -1, -3)  # the negative octant: floor division of negative voxel indices


@functools.lru_cache(maxsize=None)
def sparse(N):
    return dr.sparse(N, 3, 7, RES, base=BASE)


@pytest.mark.parametrize("N", [8, 16])
@pytest.mark.parametrize("R", [1, 2, 5])
def test_brute_equals_separable(N, R):
    origin, dims = dr.block_window(N, 3, BASE)
    seen = set()
    for offset in (0.0, RES / 2, -RES / 2):
        st = dr.states(sparse(N), N, origin, dims, R, offset)
        for flag in (False, True):
            a, b = dr.brute(st, R, flag), dr.separable(st, R, flag)
            assert a.shape == (dims[2], dims[1], dims[0]) and a.dtype == b.dtype == np.int32
            assert np.array_equal(a, b), (N, R, offset, flag, int((a != b).sum()))
            assert a.max() <= R * R and a.min() >= -1
            obs = dr.window_of(dr.obstacles(st, flag), R)
            assert np.array_equal(a == 0, obs)  # (an obstacle is its own nearest one)
            seen.add((offset, flag, int((a >= 0).sum())))
    assert len({s[2] for s in seen}) >= 4  # (offset and flag change the answer)


def test_states_by_hand():
    """one chunk at (-1, 0, 2), N = 8: a voxel of every kind at a known global index, the chunk's neighbours unknown"""
    N = 8
    sdf = np.full(N ** 3, 0.01, np.float32)
    w = np.ones(N ** 3, np.float32)
    at = lambda x, y, z: (z * N + y) * N + x
    sdf[at(0, 0, 0)] = -0.01
    sdf[at(7, 7, 7)] = -0.0
    sdf[at(1, 0, 0)] = np.float32(-1e-42)
    sdf[at(2, 0, 0)] = np.nan
    w[at(3, 0, 0)] = 1e-12
    w[at(4, 0, 0)] = np.nextafter(np.float32(1e-12), np.float32(1))
    sdf[at(4, 0, 0)] = -1.0
    fields = {(-1, 0, 2): (sdf, w, None)}
    st = dr.states(fields, N, (-8, 0, 16), (8, 8, 8), 1, 0.0)
    assert st.shape == (10, 10, 10)
    inner = dr.window_of(st, 1)
    assert inner[0, 0, 0] == 2 and inner[7, 7, 7] == 1 and inner[0, 0, 1] == 2 and inner[0, 0, 2] == 1 and inner[0, 0, 3] == 0 and inner[0, 0, 4] == 2
    shell = st.copy()
    shell[1:-1, 1:-1, 1:-1] = 0
    assert not shell.any() and (inner != 0).sum() == N ** 3 - 1
    assert dr.window_of(dr.states(fields, N, (-8, 0, 16), (8, 8, 8), 1, -0.0), 1)[7, 7, 7] == 1  # -0.0 < -0.0 is false too
    assert dr.window_of(dr.states(fields, N, (-8, 0, 16), (8, 8, 8), 1, 0.02), 1)[0, 0, 2] == 1   # NaN is never occupied
    d2 = dr.brute(st, 1)
    assert d2[0, 0, 0] == 0 and d2[0, 1, 0] == 1 and d2[1, 1, 0] == -1 and d2[7, 7, 7] == -1
    assert np.array_equal(dr.distance(np.array([-1, 0, 1, 2, 25], np.int32), RES),
                          np.array([np.inf, 0, RES, np.float32(np.sqrt(2.0) * RES), 5 * RES], np.float32))


@pytest.mark.parametrize("N", [8, 16, 32])
def test_reach_of_the_sparse_maps(N):
    """what tests/test_gpu_distance.py asserts of the device's own output holds on the restatement"""
    origin, dims = dr.block_window(N, 3, BASE)
    for R in (1, 5, 13):
        st = dr.states(sparse(N), N, origin, dims, R, 0.0)
        r = dr.check_reach(dr.window_of(st, R), dr.separable(st, R), R)
        print(N, R, {k: (len(v) if k == "values" else round(v, 4)) for k, v in r.items()})
    assert len(sparse(N)) == 25


def test_a_window_cut_into_eight_answers_as_the_whole():
    """dist2 at a voxel depends on the map, R, the flag and the offset, not on the window: eight sub-windows, cut at an odd place,
    each from states of its own"""
    N, R = 8, 5
    origin, dims = dr.block_window(N, 3, BASE)
    for flag in (False, True):
        whole = dr.separable(dr.states(sparse(N), N, origin, dims, R, 0.0), R, flag)
        cut = (13, 20, 7)
        for k in range(8):
            lo = [0 if not (k >> a) & 1 else cut[a] for a in range(3)]
            hi = [cut[a] if not (k >> a) & 1 else dims[a] for a in range(3)]
            sub_origin = tuple(origin[a] + lo[a] for a in range(3))
            sub_dims = tuple(hi[a] - lo[a] for a in range(3))
            part = dr.separable(dr.states(sparse(N), N, sub_origin, sub_dims, R, 0.0), R, flag)
            assert np.array_equal(part, whole[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]), (flag, k)


def test_window_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "distance_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), os.path.join(ROOT, "tests", "distance_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)
