"""The host-only part of chisel_hip_frontiers (cvids_amd/csrc/frontier_checks.h) in a stand-alone program under the address and
undefined-behaviour sanitizers, on the CPU: every refusal in the order of the header, the tile grid and the scratch sizes against
brute force for small windows, the arithmetic at the limits."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frontier_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frontier_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), os.path.join(ROOT, "tests", "frontier_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_frontier_checks_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "frontier_checks.h")).read()
    assert not re.search(r"#include\s*[<\"](hip|chisel)", text)
