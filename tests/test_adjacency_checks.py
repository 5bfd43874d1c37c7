"""The host-only part of chisel_hip_mesh_adjacency, chisel_hip_mesh_vertex_normals and chisel_hip_smooth_mesh
(cvids_amd/csrc/adjacency_checks.h) in a stand-alone program under the address and undefined-behaviour sanitizers, on the CPU: every
refusal that needs no device, the valence limit and the capacities against the totals, the order of the smoothing passes, the size and
scratch arithmetic at and beside 2^31 - 1."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adjacency_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "adjacency_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "adjacency_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_adjacency_checks_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "adjacency_checks.h")).read()
    assert not re.search(r"#include\s*[<\"](hip|chisel)", text)
