"""The argument check of chisel_hip_deintegrate_batch (cvids_amd/csrc/host_checks.h: deintegrate_batch_refusal) in a stand-alone
program under the address and undefined-behaviour sanitizers, on the CPU: n < 0, null frames, a bad frame first, in the middle and
last with its index named, ids without stats, n == 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_refusals_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_checks_batch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_checks_batch_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)
