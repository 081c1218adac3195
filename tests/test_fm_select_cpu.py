"""csrc/fm_select.h, the one function that chooses the kernel for a pair of feature maps, as a host program of its own
(tests/fm_select_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer.  The program's own binary is run; nothing is loaded
into this process.
  * every case of tests/golden/fm_select_cases.json -- recorded on a GPU from the public entries, before the choice moved into
    fm_select.h (tests/test_gpu_fm_select.py) -- gets the recorded kernel, the entry's own fall-backs (a contiguous copy of a strided in1,
    the volume behind the arg-min / soft-max forms) followed as the entries follow them;
  * option fm_split shows in S, which the kernel's name does not carry;
  * with no input the program sweeps the shapes around every guard and checks what must hold for every pick (the budgets, the forms)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depth-estimation_amd", "csrc")
FORMS = {"volume": 0, "strided": 0, "argmin": 1, "soft": 2, "mean": 3}
BASE = 1 << 20   # where the test's tensors start: the allocator's blocks are at least 256-byte aligned


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler found (g++, c++ or clang++)")
    path = str(tmp_path_factory.mktemp("fm_select") / "fm_select_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                            "-I", CSRC, os.path.join(ROOT, "tests", "fm_select_check.cpp"), "-o", path], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return path


def _lines(c):
    """the entry's own job, then the volume of contiguous maps it falls back to"""
    K, H1, W1, mh, mw = c["K"], c["H1"], c["W1"], c["maxh"], c["maxw"]
    H2, W2 = H1 + mh - 1, W1 + mw - 1
    o = c["opts"]
    env = [c["cv"], o.get("fm_flat", -1), o.get("fm64", -1), o.get("fm_rows", -1), o.get("fm_mfma", -1), o.get("fm_split", -1)]
    pitch, plane, in1, soft = W1, H1 * W1, BASE, [0, 0, 0]
    if c["entry"] == "strided":
        pitch = W1 + c["view"]
        plane = H1 * pitch + (3 if c["view"] else 0)
    elif c["entry"] in ("soft", "mean"):   # in1: prepareInput's narrow of the whole map
        pitch, plane, in1, soft = W2, H2 * W2, BASE + 4 * (((mh + 1) // 2 - 1) * W2 + (mw + 1) // 2 - 1), [1, H2, W2]
    out = BASE + c["out_off"]
    first = env + [FORMS[c["entry"]], K, H1, W1, mh, mw, pitch, plane, in1, BASE, out] + soft
    second = env + [0, K, H1, W1, mh, mw, W1, H1 * W1, BASE, BASE, out, 0, 0, 0]
    return [" ".join(str(v) for v in first), " ".join(str(v) for v in second)]


def test_choice_equals_the_recorded_one(exe):
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "fm_select_cases.json")))
    assert len(cases) >= 40
    run = subprocess.run([exe], input="\n".join(l for c in cases for l in _lines(c)) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    got = run.stdout.split("\n")[:-1]
    assert len(got) == 2 * len(cases)
    bad = []
    for i, c in enumerate(cases):
        own, back = got[2 * i].split(), got[2 * i + 1].split()
        assert back[0] != "none", c                       # the volume of contiguous maps always has a kernel
        name = own[0] if own[0] != "none" else back[0]
        if name != c["kernel"]:
            bad.append("%s: %s, recorded %s" % (c, name, c["kernel"]))
        if "fm_split" in c["opts"] and own[0] == "feat_matching_flat_kernel":
            S, nd = int(own[1]), int(own[2])
            assert S == {0: 1, 2: 2, 4: 4}[c["opts"]["fm_split"]] and S * nd == c["maxh"], (c, own)
    assert not bad, "\n".join(bad)
    assert sum(1 for c in cases if "fm_split" in c["opts"]) >= 3


def test_sweep_around_every_guard(exe):
    run = subprocess.run([exe], input="", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr   # (a sanitizer report ends the program with another status)
    print(run.stdout)
