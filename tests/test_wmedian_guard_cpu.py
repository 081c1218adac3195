"""The weighted-median kernel (csrc/wmedian.hip) inside the register file: no scratch and no SGPR spill in any of its 36 forms (C = 1 .. 4
times Cg = 0, and Cg = 1 .. 4 with and without the weight table; 81 VGPRs at most when this was written -- left to itself the compiler
interleaved the C = 1 window loop eight-fold and spilled SGPRs, which is what the loop pragmas there are for).  And the argument checks
of weightedMedian and flowDepthPair(median=...) that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wmedian_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "wmedian.hip"), "wmedian_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"wmedian_kernel<(\d), (\d), (true|false)>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)
    want = sorted((c, g, t) for c in range(1, 5) for g in range(5) for t in ("false", "true") if g or t == "false")
    assert len(want) == 36 and sorted((int(r[0]), int(r[1]), r[2]) for r in rows) == want, out
    for c, g, table, vgpr, scratch, spill in rows:
        form = "wmedian_kernel<%s, %s, %s>: %s VGPRs, %s B scratch, %s SGPR spills" % (c, g, table, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, form
        assert int(vgpr) <= 128, form + ": below 4 waves a SIMD"


def test_weighted_median_argument_checks_need_no_device():
    import depth_estimation_amd as d

    v, w, g = torch.zeros((2, 6, 8)), torch.ones((6, 8)), torch.zeros((3, 6, 8))
    with pytest.raises(TypeError):
        d.weightedMedian(v, w, g)                   # CPU tensors
    with pytest.raises(TypeError):
        d.weightedMedian(v)
    with pytest.raises(TypeError):
        d.weightedMedian(v.double())
    for bad in (dict(values=torch.zeros((5, 6, 8))), dict(values=torch.zeros((0, 6, 8))), dict(values=torch.zeros((6, 8))), dict(weight=torch.ones((6, 7))),
                dict(weight=torch.ones((1, 6, 8))), dict(guide=torch.zeros((6, 8))), dict(guide=torch.zeros((5, 6, 8))), dict(guide=torch.zeros((0, 6, 8))),
                dict(guide=torch.zeros((3, 6, 9))), dict(k=0), dict(k=4), dict(k=17), dict(k=-3), dict(k=3.0), dict(k=True)):
        with pytest.raises(ValueError):
            d.weightedMedian(**{**dict(values=v, weight=w, guide=g, k=3), **bad})


def test_flow_depth_pair_median_argument_checks_need_no_device():
    import depth_estimation_amd as d

    a = torch.zeros((3, 40, 40))
    for bad in (0, 2, 17, -1, True, 5.0, (4, 1.0), (5,), (5, 1.0, 2), "7", (7.0, 3.0)):
        with pytest.raises(ValueError):
            d.flowDepthPair(a, a, 5, 9, 9, (20, 20), median=bad)
    for good in (7, (7, 12.5), [3, 0], None, False):
        with pytest.raises(TypeError):              # the value is accepted; the CPU frames are not
            d.flowDepthPair(a, a, 5, 9, 9, (20, 20), median=good)
