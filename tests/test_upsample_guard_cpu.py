"""The guided-upsampling kernel (csrc/upsample.hip) inside the register file: all 20 forms (C = 1 .. 4 times Cg = 0 .. 4) present, no
scratch and no SGPR spill (48 VGPRs at most when this was written).  And the argument checks of guidedUpsample that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_upsample_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "upsample.hip"), "guided_upsample_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"guided_upsample_kernel<(\d), (\d)>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)
    want = sorted((c, g) for c in range(1, 5) for g in range(5))
    assert len(want) == 20 and sorted((int(r[0]), int(r[1])) for r in rows) == want, out
    for c, g, vgpr, scratch, spill in rows:
        form = "guided_upsample_kernel<%s, %s>: %s VGPRs, %s B scratch, %s SGPR spills" % (c, g, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, form
        assert int(vgpr) <= 128, form + ": below 4 waves a SIMD"


def test_guided_upsample_argument_checks_need_no_device():
    import depth_estimation_amd as d

    v, w, g, gl = torch.zeros((2, 6, 8)), torch.ones((6, 8)), torch.zeros((3, 12, 16)), torch.zeros((3, 6, 8))
    good = dict(values=v, size=(12, 16), weight=w, guide=g, guide_lo=gl, r=2, sigma=1.0, gain=(2.0, 2.0))
    for ok in (dict(), dict(size=None), dict(guide=None, guide_lo=None), dict(gain="flow"), dict(gain=None), dict(weight=None), dict(guide=g[0], guide_lo=gl[0]),
               dict(size=(6, 8), guide=None, guide_lo=None), dict(size=[12, 16])):
        with pytest.raises(TypeError):              # the values are accepted; the CPU tensors are not
            d.guidedUpsample(**{**good, **ok})
    with pytest.raises(TypeError):
        d.guidedUpsample(v.double(), (12, 16))
    for bad in (dict(values=torch.zeros((5, 6, 8))), dict(values=torch.zeros((0, 6, 8))), dict(values=torch.zeros((6, 8))), dict(weight=torch.ones((6, 7))),
                dict(weight=torch.ones((1, 6, 8))), dict(guide=torch.zeros((5, 12, 16))), dict(guide=torch.zeros((0, 12, 16))), dict(guide=torch.zeros((3, 12, 17))),
                dict(guide=torch.zeros((1, 3, 12, 16))), dict(guide_lo=torch.zeros((3, 6, 9))), dict(guide_lo=torch.zeros((2, 6, 8))), dict(guide=None),
                dict(guide=None, guide_lo=None, size=None), dict(size=(5, 16)), dict(size=(12, 7)), dict(size=(12, 32769)), dict(size=(12,)), dict(size=12),
                dict(size=(12.0, 16)), dict(size=(True, 16), guide=None, guide_lo=None), dict(r=0), dict(r=5), dict(r=-1), dict(r=2.0), dict(r=True),
                dict(gain=(1.0,)), dict(gain=(1.0, 2.0, 3.0)), dict(gain=(1.0, float("nan"))), dict(gain=(float("inf"), 1.0)), dict(gain=2.0), dict(gain="depth"),
                dict(gain="flow", values=torch.zeros((3, 6, 8)))):
        with pytest.raises(ValueError):
            d.guidedUpsample(**{**good, **bad})
