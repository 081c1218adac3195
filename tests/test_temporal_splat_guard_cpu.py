"""The four-tap splat's kernels (csrc/temporal_splat.hip) inside the register file: no scratch and no SGPR spill in any of them (49
VGPRs at most when this was written, the LDS form of the accumulate pass for C = 4: four 64-bit products per tap).  And the argument checks
of forwardSplat, temporalStep(splat="bilinear") and TemporalFilter(splat="bilinear") that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_temporal_splat_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "temporal_splat.hip"), "splat4_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"(splat4_\w+)(<[^>]*>)?\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)
    # the clear; the two forms of the front and of the accumulate pass, the resolve and the fused resolve: each for C = 1 .. 4
    want = {"splat4_clear_kernel": 1, "splat4_front_kernel": 4, "splat4_front_lds_kernel": 4, "splat4_accum_kernel": 4, "splat4_accum_lds_kernel": 4,
            "splat4_resolve_kernel": 4, "splat4_step_kernel": 4}
    assert {k: sum(r[0] == k for r in rows) for k in want} == want and len(rows) == 25, out
    for name, targs, vgpr, scratch, spill in rows:
        assert int(scratch) == 0 and int(spill) == 0, "%s%s: %s VGPRs, %s B scratch, %s SGPR spills" % (name, targs, vgpr, scratch, spill)


def test_temporal_splat_argument_checks_need_no_device():
    import depth_estimation_amd as d

    v, w, f = torch.zeros((2, 6, 8)), torch.ones((6, 8)), torch.zeros((2, 6, 8))
    calls = {
        "forwardSplat": lambda v=v, w=w, f=f, **kw: d.forwardSplat(v, w, f, **kw),
        "temporalStep": lambda v=v, w=w, f=f, **kw: d.temporalStep(v, w, f, v, w, 1.0, splat="bilinear", **kw),
        "push": lambda v=v, w=w, f=f, **kw: d.TemporalFilter(1.0, splat="bilinear").push(v, w, f, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(TypeError):
            call()                                  # CPU tensors
        for bad_v, bad_w in ((torch.zeros((5, 6, 8)), w), (torch.zeros((6, 8)), w), (v, torch.ones((6, 7)))):
            with pytest.raises(ValueError):
                call(v=bad_v, w=bad_w)
        for bad_f in (torch.zeros((6, 8)), torch.zeros((2, 6, 7))):
            with pytest.raises(ValueError):
                call(f=bad_f)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(ztol=-1.0), dict(ztol=nan), dict(ztol=inf), dict(quant=0.0), dict(quant=-2.0), dict(quant=inf), dict(quant=nan), dict(min_cover=-0.5),
               dict(min_cover=1.5), dict(min_cover=nan)):
        for name in ("forwardSplat", "temporalStep"):
            with pytest.raises(ValueError):
                calls[name](**kw)
        with pytest.raises(ValueError):
            d.TemporalFilter(1.0, splat="bilinear", **kw)
    for kw in (dict(key=torch.zeros((6, 7))), dict(gain=(1.0,)), dict(bias=(0.0, inf)), dict(decay=0.0), dict(decay=nan)):
        for name in ("forwardSplat", "temporalStep"):
            with pytest.raises(ValueError):
                calls[name](**kw)
    with pytest.raises(ValueError):
        d.temporalStep(v, w, f, v, w, 1.0, splat="cubic")
    with pytest.raises(ValueError):
        d.TemporalFilter(1.0, splat="cubic")
    with pytest.raises(ValueError):
        d.TemporalFilter(-1.0, splat="bilinear")    # ztol = None takes tol
    flt = d.TemporalFilter(1.5, splat="bilinear")
    assert (flt.splat, flt.ztol, flt.quant, flt.min_cover) == ("bilinear", 1.5, 1024.0, 0.25)
    assert d.TemporalFilter(1.5).splat == "nearest" and d.TemporalFilter(1.5, splat="bilinear", ztol=0.25).ztol == 0.25
