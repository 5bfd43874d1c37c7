"""The host-only part of chisel_hip_coarse_mesh (cvids_amd/csrc/coarse_checks.h) in a stand-alone program under the address and
undefined-behaviour sanitizers, on the CPU: every refusal that needs no device in the header's order, the stride rule for every chunk
edge and every stride from 0 to N + 1, the float arithmetic at and beside 2^31 - 1."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_coarse_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "coarse_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "coarse_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_coarse_checks_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "coarse_checks.h")).read()
    assert not re.search(r"#include\s*[<\"](hip|chisel)", text)


def test_coarse_mirrors_are_the_headers_size():
    from cvids_amd import capi
    assert ctypes.sizeof(capi.CoarseRequest) == 56 and ctypes.sizeof(capi.CoarseTotals) == 32
    assert "chisel_hip_coarse_mesh" in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "chisel_hip.h")).read()
    assert re.search(r"int\s+chisel_hip_coarse_mesh\s*\(", header)
