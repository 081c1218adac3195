"""The hole-filling kernels (csrc/fill.hip) inside the register file: no scratch and no SGPR spill in any of them (36 VGPRs at most when
this was written; per-cell kernels of four taps have no reason to spill).  And the argument checks of fillHoles that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fill_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "fill.hip"), "fill_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"(fill_\w+)(<[^>]*>)\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)
    # push from level 0 and from a level, pull into a level and into the caller's planes, the apex: each for C = 1 .. 4
    want = {"fill_push_kernel": 8, "fill_pull_kernel": 4, "fill_pull0_kernel": 4, "fill_apex_kernel": 4}
    assert {k: sum(r[0] == k for r in rows) for k in want} == want and len(rows) == 20, out
    for name, targs, vgpr, scratch, spill in rows:
        assert int(scratch) == 0 and int(spill) == 0, "%s%s: %s VGPRs, %s B scratch, %s SGPR spills" % (name, targs, vgpr, scratch, spill)


def test_fill_holes_argument_checks_need_no_device():
    import depth_estimation_amd as d

    v, w = torch.zeros((2, 6, 8)), torch.ones((6, 8))
    with pytest.raises(TypeError):
        d.fillHoles(v, w)                       # CPU tensors
    with pytest.raises(TypeError):
        d.fillHoles(v.double(), w.double())
    for bad_v, bad_w in ((torch.zeros((5, 6, 8)), w), (torch.zeros((0, 6, 8)), w), (torch.zeros((6, 8)), w), (v, torch.ones((6, 7))), (v, torch.ones((1, 6, 8)))):
        with pytest.raises(ValueError):
            d.fillHoles(bad_v, bad_w)
    with pytest.raises(TypeError):
        d.flowDepthPair(torch.zeros((3, 40, 40)), torch.zeros((3, 40, 40)), 5, 9, 9, (20, 20), fill=True)
