"""The host-only part of chisel_hip_gather_chunks and chisel_hip_scatter_chunks (cvids_amd/csrc/chunk_checks.h) in a stand-alone program
under the address and undefined-behaviour sanitizers, on the CPU: every refusal that needs no device in the header's order, duplicate
detection, the box filter and the ascending order of the "all" selection, the 64-bit byte and grid arithmetic at its limits."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chunk_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", os.path.join(ROOT, "cvids_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "chunk_checks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.stdout, run.stderr)


def test_chunk_checks_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "chunk_checks.h")).read()
    assert not re.search(r"#include\s*[<\"](hip|chisel)", text)


def test_chunk_request_mirror_is_the_headers_size():
    from cvids_amd import capi
    assert ctypes.sizeof(capi.ChunkRequest) == 48
    assert "chisel_hip_gather_chunks" in capi.EXPORTS and "chisel_hip_scatter_chunks" in capi.EXPORTS


def test_tile_constant_is_one_number():
    """the host-only header's constants and the Python mirror's"""
    from cvids_amd import capi
    text = open(os.path.join(ROOT, "cvids_amd", "csrc", "chunk_checks.h")).read()
    threads = int(re.search(r"CHUNK_COPY_THREADS\s*=\s*(\d+)", text).group(1))
    depth = int(re.search(r"CHUNK_COPY_DEPTH\s*=\s*(\d+)", text).group(1))
    assert threads * depth * 16 == capi.CHUNK_TILE_BYTES
