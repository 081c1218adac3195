"""The temporal filter's kernels (csrc/temporal.hip) inside the register file: no scratch and no SGPR spill in any of them (25 VGPRs at
most when this was written; per-pixel kernels of one gather have no reason to spill).  And the argument checks of forwardWarp,
temporalFuse, temporalStep and TemporalFilter.push that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_temporal_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "temporal.hip"), "temporal_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"(temporal_\w+)(<[^>]*>)\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)
    # the splat, the resolve, the fusion alone and the fused resolve: each for C = 1 .. 4
    want = {"temporal_splat_kernel": 4, "temporal_resolve_kernel": 4, "temporal_fuse_kernel": 4, "temporal_step_kernel": 4}
    assert {k: sum(r[0] == k for r in rows) for k in want} == want and len(rows) == 16, out
    for name, targs, vgpr, scratch, spill in rows:
        assert int(scratch) == 0 and int(spill) == 0, "%s%s: %s VGPRs, %s B scratch, %s SGPR spills" % (name, targs, vgpr, scratch, spill)


def test_temporal_argument_checks_need_no_device():
    import depth_estimation_amd as d

    v, w, f = torch.zeros((2, 6, 8)), torch.ones((6, 8)), torch.zeros((2, 6, 8))
    calls = {
        "forwardWarp": lambda v=v, w=w, f=f, **kw: d.forwardWarp(v, w, f, **kw),
        "temporalFuse": lambda v=v, w=w, f=f, m=None, wm=None, **kw: d.temporalFuse(v, w, v if m is None else m, w if wm is None else wm, kw.pop("tol", 1.0), **kw),
        "temporalStep": lambda v=v, w=w, f=f, m=None, wm=None, **kw: d.temporalStep(v, w, f, v if m is None else m, w if wm is None else wm, kw.pop("tol", 1.0), **kw),
        "push": lambda v=v, w=w, f=f, **kw: d.TemporalFilter(1.0).push(v, w, f, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(TypeError):
            call()                                  # CPU tensors
        with pytest.raises(TypeError):
            call(v=v.double(), w=w.double(), f=f.double())
        for bad_v, bad_w in ((torch.zeros((5, 6, 8)), w), (torch.zeros((0, 6, 8)), w), (torch.zeros((6, 8)), w), (v, torch.ones((6, 7))), (v, torch.ones((1, 6, 8)))):
            with pytest.raises(ValueError):
                call(v=bad_v, w=bad_w)
    for name in ("forwardWarp", "temporalStep", "push"):
        for bad_f in (torch.zeros((6, 8)), torch.zeros((3, 6, 8)), torch.zeros((2, 6, 7))):
            with pytest.raises(ValueError):
                calls[name](f=bad_f)
    for name in ("forwardWarp", "temporalStep"):
        for kw in (dict(key=torch.zeros((6, 7))), dict(key=torch.zeros((1, 6, 8))), dict(gain=(1.0,)), dict(gain=(1.0, float("nan"))), dict(bias=(0.0, float("inf"))),
                   dict(bias=3.0), dict(decay=0.0), dict(decay=1.5), dict(decay=float("nan"))):
            with pytest.raises(ValueError):
                calls[name](**kw)
    for name in ("temporalFuse", "temporalStep"):
        for kw in (dict(tol=-1.0), dict(tol=float("nan")), dict(wmax=0.0), dict(wmax=float("inf")), dict(wmax=float("nan")), dict(m=torch.zeros((1, 6, 8))),
                   dict(wm=torch.ones((6, 9)))):
            with pytest.raises(ValueError):
                calls[name](**kw)
    with pytest.raises(ValueError):
        d.TemporalFilter(1.0, key_channel=4)
    with pytest.raises(ValueError):
        d.TemporalFilter(1.0, key_channel=2).push(v, w, f)          # two channels
