"""The host-only part of chisel_hip_indexed_mesh (cvids_amd/csrc/indexed_checks.h) in a stand-alone program under the address and
undefined-behaviour sanitizers, on the CPU: every refusal that needs no device, duplicates, the extras of lists and boxes against a
brute-force set, the row, id and index arithmetic at and beside 2^31 - 1."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_indexed_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "indexed_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "indexed_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_indexed_checks_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "indexed_checks.h")).read()
    assert not re.search(r"#include\s*[<\"](hip|chisel)", text)


def test_indexed_mirrors_are_the_headers_size():
    from cvids_amd import capi
    assert ctypes.sizeof(capi.IndexedTotals) == 40
    assert "chisel_hip_indexed_mesh" in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "chisel_hip.h")).read()
    assert re.search(r"int\s+chisel_hip_indexed_mesh\s*\(", header)
    assert [n for n, _ in capi.IndexedTotals._fields_] == re.search(r"typedef struct \{ int64_t ([a-z_, ]+); \} chisel_hip_indexed_totals;", header).group(1).split(", ")
