"""The host-side pieces of the side entries that call nothing of HIP (cvids_amd/csrc/host_checks.h: the image check of the alignment
entries and of de-integration, de-integration's refusals and the planes its list kernel rejects chunks by) in a stand-alone program
under the address and undefined-behaviour sanitizers, on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planes_and_refusals_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), os.path.join(ROOT, "tests", "host_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)
