"""csrc/dfe_contig_pool.h, the books of the process's physically contiguous device blocks, as a host program of its own
(tests/contig_pool_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer: a released block is reused, a request may get a larger
block and is told its size, the smallest idle block that fits is taken, a device sees its own blocks only, a second release is refused and
hands the block out once, and trim takes idle blocks largest first down to its bound.  The program's own binary is run; nothing is loaded
into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depth-estimation_amd", "csrc")


def test_contig_pool_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler found (g++, c++ or clang++)")
    exe = str(tmp_path / "contig_pool_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                            "-I", CSRC, os.path.join(ROOT, "tests", "contig_pool_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr   # (a sanitizer report ends the program with another status)
