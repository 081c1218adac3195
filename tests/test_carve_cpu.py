"""csrc/dfe_carve.h, the carver every launcher lays its scratch out with, as a host program of its own (tests/carve_check.cpp) under
AddressSanitizer and UndefinedBehaviorSanitizer: the sizing pass and the carving pass agree, every buffer starts 256 bytes-aligned in the
block, a take of nothing returns no pointer and uses no space, and buffers of float, double, float2-sized and int64 elements at 1, 63, 64
and 65 elements neither overlap nor leave the block.  The program's own binary is run; nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depth-estimation_amd", "csrc")


def test_carver_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler found (g++, c++ or clang++)")
    exe = str(tmp_path / "carve_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                            "-I", CSRC, os.path.join(ROOT, "tests", "carve_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr   # (a sanitizer report ends the program with another status)
