"""The host-only part of chisel_hip_travel_field and chisel_hip_travel_path (cvids_amd/csrc/travel_checks.h) in a stand-alone program
under the address and undefined-behaviour sanitizers, on the CPU: every refusal in the order of the header, the seed check, the tile
grid against brute force, the arithmetic at 2^26 voxels and at +-2^30, the walk on hand step volumes."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_travel_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "travel_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), os.path.join(ROOT, "tests", "travel_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_travel_checks_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "travel_checks.h")).read()
    assert not re.search(r"#include\s*[<\"](hip|chisel)", text)


def test_the_constants_python_exports_are_the_header_s():
    from cvids_amd import capi
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "travel_checks.h")).read()
    assert int(re.search(r"TRAVEL_ROUNDS_PER_WAIT = (\d+);", text).group(1)) == capi.TRAVEL_ROUNDS_PER_WAIT
    assert capi.TRAVEL_ROUNDS_PER_WAIT in (8, 16, 32, 64)
    assert len(capi.TRAVEL_TOTALS) == 12 and len(capi.TRAVEL_TABLE_COLUMNS) == 4
