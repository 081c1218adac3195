"""The pick kernel (csrc/sgm_pick.hip) inside the register file: both forms of sgpk_pick_kernel with 0 bytes of
scratch and 0 SGPR spills, within the registers of three waves a SIMD -- the bound the widest path form of sgm_plane.hip meets, so the
pick never holds fewer waves than the launch in front of it.  And the argument checks of semiGlobalPick and of the sgm= keywords of
flowDepthPair and censusFlowDepthPair that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [("sgpk_pick_kernel", "false"), ("sgpk_pick_kernel", "true")]


def test_sgpk_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "sgm_pick.hip"), "sgpk_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"^(sgpk_\w+)<([^>]*)>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out, flags=re.M)
    assert sorted(r[:2] for r in rows) == sorted(FORMS) and len(rows) == len(re.findall(r"^sgpk_", out, flags=re.M)), out
    for name, form, vgpr, scratch, spill in rows:
        text = "%s<%s>: %s VGPRs, %s B scratch, %s SGPR spills" % (name, form, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, text
        assert int(vgpr) <= 168, text + ": below 3 waves a SIMD"


def test_the_pick_adds_no_kernel_to_the_aggregation_file():
    src = open(os.path.join(ROOT, "depth-estimation_amd", "csrc", "sgm_pick.hip")).read()
    assert not re.search(r"__global__[^;{]*\bsgmp_", src), "kernels of this file carry the sgpk_ prefix"
    assert "sgm_pick.hip" in open(os.path.join(ROOT, "depth-estimation_amd", "csrc", "Makefile")).read()


def test_semiGlobalPick_argument_checks_need_no_device():
    import depth_estimation_amd as d

    vol = torch.zeros((5, 7, 3, 4))
    for good in (dict(), dict(paths=0xff, P1=1.0, P2=2.0, subpixel=True, min_unique=0.2, want_volume=True), dict(min_unique=1), dict(min_unique=0)):
        with pytest.raises(TypeError):              # the values are accepted; the CPU tensor is not
            d.semiGlobalPick(vol, **good)
    with pytest.raises(TypeError):
        d.semiGlobalPick(vol.double())
    for bad in (dict(paths=-1), dict(paths=256), dict(paths=3.0), dict(paths=True), dict(P1=-1.0), dict(P1=3.0, P2=2.0), dict(P2=float("inf")), dict(P1="a"),
                dict(paths=0, P1=3.0, P2=2.0), dict(paths=0, P1=float("nan")),                 # ignored without paths, checked all the same
                dict(min_unique=-0.1), dict(min_unique=1.5), dict(min_unique=float("nan")), dict(min_unique="a"), dict(min_unique=True),
                dict(volume=vol[0]), dict(volume=torch.zeros((5, 7, 33, 34))), dict(volume=torch.zeros((5, 0, 3, 3))), dict(volume=None)):
        with pytest.raises(ValueError):
            d.semiGlobalPick(**{**dict(volume=vol), **bad})


def test_the_sgm_keyword_of_flowDepthPair_is_checked_before_the_device():
    import depth_estimation_amd as d

    f = torch.zeros((1, 40, 60), dtype=torch.uint8)
    for good in ((1.0, 2.0), [1, 2], dict(P1=1.0, P2=2.0), dict(P1=0, P2=0, paths=0xff), dict(P1=1, P2=2, min_unique=0.2), dict(P1=1, P2=2, paths=1, min_unique=1)):
        with pytest.raises(TypeError):              # the values are accepted; the CPU frames are not
            d.flowDepthPair(f, f, 7, 9, 9, (30.0, 20.0), sgm=good, subpixel=True)
    for bad in ((1.0,), (1.0, 2.0, 3), 5.0, "ab", (3.0, 2.0), (-1.0, 2.0), (1.0, float("nan")), dict(P1=1.0), dict(P1=1.0, P2=2.0, ring=3),
                dict(P1=1.0, P2=2.0, paths=0), dict(P1=1.0, P2=2.0, paths=256), dict(P1=1.0, P2=2.0, paths=1.0), dict(P1=1.0, P2=2.0, min_unique=2),
                dict(P1=1.0, P2=2.0, min_unique=-1), dict(P1=1.0, P2=2.0, min_unique="x"), dict(P2=2.0, min_unique=0.5), dict(P1=1, P2=2, min_unique=0.5, ring=1)):
        with pytest.raises(ValueError):
            d.flowDepthPair(f, f, 7, 9, 9, (30.0, 20.0), sgm=bad)
    with pytest.raises(ValueError, match="consistency"):
        d.flowDepthPair(f, f, 7, 9, 9, (30.0, 20.0), sgm=(1.0, 2.0), consistency=1.0)


def test_the_new_keywords_of_censusFlowDepthPair_are_checked_before_the_device():
    import depth_estimation_amd as d

    f = torch.zeros((1, 40, 60), dtype=torch.uint8)
    for good in (dict(sgm=(1.0, 2.0), subpixel=True), dict(sgm=dict(P1=1.0, P2=2.0, min_unique=0.2)), dict(sgm=dict(P1=1, P2=2, paths=0xff, min_unique=0), subpixel=True)):
        with pytest.raises(TypeError):              # the values are accepted; the CPU frames are not
            d.censusFlowDepthPair(f, f, 7, 9, 9, (30.0, 20.0), **good)
    for bad in (dict(subpixel=True), dict(sgm=dict(P1=1.0, P2=2.0, min_unique=1.5)), dict(sgm=dict(P1=1.0, P2=2.0, min_unique=None)),
                dict(sgm=dict(P1=3.0, P2=2.0, min_unique=0.5)), dict(sgm=dict(P1=1.0, min_unique=0.5)), dict(sgm=dict(P1=1.0, P2=2.0, paths=0, min_unique=0.5))):
        with pytest.raises(ValueError):
            d.censusFlowDepthPair(f, f, 7, 9, 9, (30.0, 20.0), **bad)
