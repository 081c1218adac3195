"""The census kernels (csrc/census.hip) inside the register file: both transforms, the staged volume kernel and the
twelve forms of the fused sweep (agg 1 / 3 / 5 by 1 .. 4 channels), 0 bytes of scratch and 0 SGPR spills -- a lane's frame-0 signatures,
its row sums and its running keys are arrays indexed by unrolled constants, and a form that indexed them at run time would move them to
scratch.  And the argument checks of the Python wrappers, which need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "census.hip"), "census_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"^(census_\w+)(?:<([^>]*)>)?\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out, flags=re.M)
    want = sorted([("census_sweep_kernel", "%d, %d" % (a, c)) for a in (1, 3, 5) for c in (1, 2, 3, 4)]
                  + [("census_transform_kernel", t) for t in ("float", "unsigned char")] + [("census_volume_kernel", "")])
    assert sorted(r[:2] for r in rows) == want and len(rows) == len(re.findall(r"^census_", out, flags=re.M)), out
    for name, form, vgpr, scratch, spill in rows:
        text = "%s<%s>: %s VGPRs, %s B scratch, %s SGPR spills" % (name, form, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, text
        assert int(vgpr) <= 168, text + ": below 3 waves a SIMD"


def test_census_argument_checks_need_no_device():
    import depth_estimation_amd as d

    img = torch.zeros((3, 40, 60))
    sig = torch.zeros((3, 34, 54), dtype=torch.int64)
    foe = (30.0, 20.0)
    # the values are accepted; the CPU tensor is not
    for call in (lambda: d.censusTransform(img, 7), lambda: d.censusTransform(img.to(torch.uint8), (9, 7)), lambda: d.censusCostVolume(sig, sig, 9, 9),
                 lambda: d.censusFlow(sig, sig, 48, 9, 9, agg=5), lambda: d.censusFlowDepthPair(img, img, 7, 9, 9, foe),
                 lambda: d.censusFlowDepthPair(img.to(torch.uint8), img.to(torch.uint8), 7, 9, 9, foe, agg=1, median=5)):
        with pytest.raises(TypeError):
            call()
    # a wrong dtype
    for call in (lambda: d.censusTransform(img.double(), 7), lambda: d.censusCostVolume(sig.int(), sig.int(), 9, 9), lambda: d.censusFlow(sig.float(), sig.float(), 48, 9, 9),
                 lambda: d.censusFlowDepthPair(img.double(), img.double(), 7, 9, 9, foe), lambda: d.censusFlowDepthPair(img, img.to(torch.uint8), 7, 9, 9, foe)):
        with pytest.raises(TypeError):
            call()
    # even or too large k
    for k in (6, 9, 1, (7, 8), (9, 9), (3, 23), 7.0, True):
        with pytest.raises(ValueError):
            d.censusTransform(img, k)
    for k in (6, 9, 1, (7, 7), 7.0):
        with pytest.raises(ValueError):
            d.censusFlowDepthPair(img, img, k, 9, 9, foe)
    # agg outside {1, 3, 5}
    for agg in (0, 2, 4, 7, 3.0, True):
        for call in (lambda: d.censusCostVolume(sig, sig, 9, 9, agg), lambda: d.censusFlow(sig, sig, 48, 9, 9, agg), lambda: d.censusFlowDepthPair(img, img, 7, 9, 9, foe, agg=agg)):
            with pytest.raises(ValueError):
                call()
    # more than 4 channels
    big, bigsig = torch.zeros((5, 40, 60)), torch.zeros((5, 34, 54), dtype=torch.int64)
    for call in (lambda: d.censusTransform(big), lambda: d.censusCostVolume(bigsig, bigsig, 9, 9), lambda: d.censusFlow(bigsig, bigsig, 48, 9, 9),
                 lambda: d.censusFlowDepthPair(big, big, 7, 9, 9, foe)):
        with pytest.raises(ValueError):
            call()
    # an empty region, a window of more than 1096 cells, a frame below the patch, nbits out of range, shapes that differ
    for call in (lambda: d.censusCostVolume(sig, sig, 33, 9), lambda: d.censusFlow(sig, sig, 48, 9, 53, agg=3), lambda: d.censusFlowDepthPair(img, img, 7, 33, 33, foe),
                 lambda: d.censusFlowDepthPair(img[:, :5], img[:, :5], 7, 1, 1, foe, agg=1), lambda: d.censusCostVolume(sig, sig, 34, 33), lambda: d.censusTransform(img[:, :5], 7),
                 lambda: d.censusFlow(sig, sig, 0, 9, 9), lambda: d.censusFlow(sig, sig, 64, 9, 9), lambda: d.censusFlow(sig, sig[:, 1:], 48, 9, 9),
                 lambda: d.censusFlowDepthPair(img, img[:, 1:], 7, 9, 9, foe), lambda: d.censusFlowDepthPair(img, img, 7, 9, 9, foe, scale=0.0),
                 lambda: d.censusFlowDepthPair(img, img, 7, 9, 9, foe, median=4)):
        with pytest.raises(ValueError):
            call()
