"""The radial census kernels (csrc/census_radial.hip) inside the register file: the staged volume kernel, the
score kernel and the twelve forms of the fused matcher (agg 1 / 3 / 5 by 1 .. 4 channels), 0 bytes of scratch and 0 SGPR spills -- a
lane's frame-0 signatures, its column of Hamming distances and its labels' costs are arrays indexed by unrolled constants, and a form that
indexed them at run time would move them to scratch.  And the argument checks of the Python wrappers, which need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_radial_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "census_radial.hip"),
                          "census_radial_"], capture_output=True, text=True).stdout
    rows = re.findall(r"^(census_radial_\w+)(?:<([^>]*)>)?\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out, flags=re.M)
    want = sorted([("census_radial_flow_kernel", "%d, %d" % (a, c)) for a in (1, 3, 5) for c in (1, 2, 3, 4)]
                  + [("census_radial_volume_kernel", ""), ("census_radial_score_kernel", "")])
    assert sorted(r[:2] for r in rows) == want and len(rows) == len(re.findall(r"^census_radial_", out, flags=re.M)), out
    for name, form, vgpr, scratch, spill in rows:
        text = "%s<%s>: %s VGPRs, %s B scratch, %s SGPR spills" % (name, form, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, text
        assert int(vgpr) <= 168, text + ": below 3 waves a SIMD"


def test_census_radial_argument_checks_need_no_device():
    import depth_estimation_amd as d

    img = torch.zeros((3, 60, 80))
    sig = torch.zeros((3, 42, 64), dtype=torch.int64)
    e2 = (41.3, 27.6)
    depth = lambda *a, **k: d.censusRadialFlowDepth(img, img, e2, 48, 64, *a, **k)
    # the values are accepted; the CPU tensor is not
    for call in (lambda: d.censusRadialCostVolume(sig, sig, 5), lambda: d.censusRadialCostVolume(sig, sig, 32, agg=5),
                 lambda: d.censusRadialFlow(sig, sig, 48, 8), lambda: d.censusRadialFlow(sig, sig, 26, 15, agg=1, subpixel=True, want_volume=True),
                 lambda: depth(8), lambda: depth(16, k=(3, 9), agg=5, one_call=False), lambda: depth(12, sgm=(4, 32), subpixel=True),
                 lambda: depth(8, sgm=dict(P1=1, P2=2, paths=0xff, ring=0))):
        with pytest.raises(TypeError):
            call()
    # a wrong dtype
    for call in (lambda: d.censusRadialCostVolume(sig.int(), sig.int(), 8), lambda: d.censusRadialFlow(sig.float(), sig.float(), 48, 8),
                 lambda: d.censusRadialFlowDepth(img.double(), img.double(), e2, 48, 64, 8), lambda: d.censusRadialFlowDepth(img, img.to(torch.uint8), e2, 48, 64, 8)):
        with pytest.raises(TypeError):
            call()
    # agg outside {1, 3, 5}, or wider than the ring
    for agg in (0, 2, 4, 7, 3.0, True):
        for call in (lambda: d.censusRadialCostVolume(sig, sig, 8, agg), lambda: d.censusRadialFlow(sig, sig, 48, 8, agg), lambda: depth(8, agg=agg)):
            with pytest.raises(ValueError):
                call()
    for call in (lambda: d.censusRadialCostVolume(sig[:, :, :4], sig[:, :, :4], 8, 5), lambda: d.censusRadialFlow(sig[:, :, :2], sig[:, :, :2], 48, 8, 3),
                 lambda: d.censusRadialFlowDepth(img, img, e2, 48, 4, 8, agg=5)):
        with pytest.raises(ValueError):
            call()
    # a window the fused matcher has no instantiation for (the staged volume takes any), a window of no cells
    for hWin in (1, 5, 9, 17, 32):
        with pytest.raises(ValueError):
            d.censusRadialFlow(sig, sig, 48, hWin)
        with pytest.raises(ValueError):
            depth(hWin)
    for hWin in (0, -8, 8.0, True):
        for call in (lambda: d.censusRadialCostVolume(sig, sig, hWin), lambda: d.censusRadialFlow(sig, sig, 48, hWin), lambda: depth(hWin)):
            with pytest.raises(ValueError):
                call()
    # more than 4 channels, shapes that differ, no row left, nbits out of range
    big, bigsig = torch.zeros((5, 60, 80)), torch.zeros((5, 42, 64), dtype=torch.int64)
    for call in (lambda: d.censusRadialCostVolume(bigsig, bigsig, 8), lambda: d.censusRadialFlow(bigsig, bigsig, 48, 8),
                 lambda: d.censusRadialFlowDepth(big, big, e2, 48, 64, 8), lambda: d.censusRadialFlow(sig, sig[:, 1:], 48, 8),
                 lambda: d.censusRadialFlowDepth(img, img[:, 1:], e2, 48, 64, 8), lambda: d.censusRadialCostVolume(sig, sig, 43, 1),
                 lambda: d.censusRadialCostVolume(sig, sig, 41, 3), lambda: d.censusRadialFlow(sig[:, :17], sig[:, :17], 48, 16, 3),
                 lambda: d.censusRadialFlowDepth(img, img, e2, 23, 64, 16, agg=3), lambda: d.censusRadialFlowDepth(img, img, e2, 6, 64, 8),
                 lambda: d.censusRadialFlow(sig, sig, 0, 8), lambda: d.censusRadialFlow(sig, sig, 64, 8), lambda: d.censusRadialFlow(sig, sig, 48.0, 8)):
        with pytest.raises(ValueError):
            call()
    # the patch, the polar grid's constants, the sgm argument
    for k in (6, 9, 1, (7, 8), (9, 9), (3, 23), 7.0, True):
        with pytest.raises(ValueError):
            depth(8, k=k)
    for bad in (dict(alpha_polar=0.0), dict(kinfty=-1.0), dict(sgm=(1.0,)), dict(sgm=(2.0, 1.0)), dict(sgm=dict(P1=1.0, P2=2.0, paths=0)),
                dict(sgm=dict(P1=1.0, P2=2.0, ring=65)), dict(sgm=dict(P1=1.0, P2=float("nan"))), dict(sgm="ab")):
        for oc in (True, False):
            with pytest.raises(ValueError):
                depth(8, one_call=oc, **bad)
