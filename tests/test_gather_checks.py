"""The host-only part of chisel_hip_gather_meshes (cvids_amd/csrc/gather_checks.h: gather_request_refusal, gather_plan) in a stand-alone
program under the address and undefined-behaviour sanitizers, on the CPU: every refusal that needs no device, the segment tables of 0
meshes, one empty mesh and meshes in three arenas with and without colour, the totals at the 2^31 - 1 limit and one past it, a
capacity one short, the prefix and the tile count against a naive loop."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gather_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "gather_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_tile_constant_is_one_number():
    """the header's macro, the host-only header's constant and the Python mirror's"""
    import re
    from cvids_amd import capi
    header = open(os.path.join(ROOT, "include", "chisel_hip.h")).read()
    checks = open(os.path.join(ROOT, "cvids_amd", "csrc", "gather_checks.h")).read()
    a = int(re.search(r"#define\s+CHISEL_HIP_GATHER_TILE_FLOATS\s+(\d+)", header).group(1))
    b = int(re.search(r"GATHER_TILE_FLOATS\s*=\s*(\d+)", checks).group(1))
    assert a == b == capi.GATHER_TILE_FLOATS and a & (a - 1) == 0
    import ctypes
    assert ctypes.sizeof(capi.MeshRequest) == 56 and ctypes.sizeof(capi.MeshTotals) == 48
