"""The host-only part of chisel_hip_mesh_components and chisel_hip_filter_mesh (cvids_amd/csrc/components_checks.h) in a stand-alone
program under the address and undefined-behaviour sanitizers, on the CPU: every refusal that needs no device, the capacities against
the totals, the size, tile and key arithmetic at and beside 2^31 - 1."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_components_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "components_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "components_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_components_checks_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "components_checks.h")).read()
    assert not re.search(r"#include\s*[<\"](hip|chisel)", text)
