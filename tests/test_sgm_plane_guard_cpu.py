"""The kernels of the aggregation on the two-dimensional label plane (csrc/sgm_plane.hip) inside the register
file: the five forms of sgmp_path_kernel (cells a lane, steps whose loads are in flight) and the two of sgmp_sum_kernel, 0 bytes of
scratch and 0 SGPR spills -- a lane's cells and the load pipeline's slots are arrays indexed by unrolled constants, and a form that
indexed them at run time would move them to scratch -- and the widest form within the registers of three waves a SIMD.  And the argument
checks of semiGlobalAggregatePlane and of censusFlowDepthPair's sgm= keyword that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [("sgmp_path_kernel", "1, 8"), ("sgmp_path_kernel", "2, 8"), ("sgmp_path_kernel", "5, 4"), ("sgmp_path_kernel", "9, 4"), ("sgmp_path_kernel", "18, 2"),
         ("sgmp_sum_kernel", "false"), ("sgmp_sum_kernel", "true")]


def test_sgmp_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "sgm_plane.hip"), "sgmp_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"^(sgmp_\w+)<([^>]*)>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out, flags=re.M)
    assert sorted(r[:2] for r in rows) == sorted(FORMS) and len(rows) == len(re.findall(r"^sgmp_", out, flags=re.M)), out
    for name, form, vgpr, scratch, spill in rows:
        text = "%s<%s>: %s VGPRs, %s B scratch, %s SGPR spills" % (name, form, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, text
        # 18 cells a lane keep 18 L, 18 LDS offsets, 18 clamped classes and 2 x 18 loads in flight: 168 registers = 3 waves a SIMD
        assert int(vgpr) <= 168, text + ": below 3 waves a SIMD"
        if form not in ("9, 4", "18, 2"):
            assert int(vgpr) <= 64, text + ": below 8 waves a SIMD"


def test_semiGlobalAggregatePlane_argument_checks_need_no_device():
    import depth_estimation_amd as d

    vol = torch.zeros((5, 7, 3, 4))
    with pytest.raises(TypeError):                  # the values are accepted; the CPU tensor is not
        d.semiGlobalAggregatePlane(vol, 1.0, 2.0, paths=0xff, want_volume=False)
    with pytest.raises(TypeError):
        d.semiGlobalAggregatePlane(vol.double(), 1.0, 2.0)
    for bad in (dict(paths=0), dict(paths=256), dict(paths=3.0), dict(paths=True), dict(P1=-1.0), dict(P1=3.0), dict(P2=float("inf")), dict(P1="a"),
                dict(volume=vol[0]), dict(volume=torch.zeros((5, 7, 33, 34))), dict(volume=torch.zeros((5, 0, 3, 3))), dict(volume=None)):
        with pytest.raises(ValueError):
            d.semiGlobalAggregatePlane(**{**dict(volume=vol, P1=1.0, P2=2.0), **bad})


def test_the_sgm_keyword_of_censusFlowDepthPair_is_checked_without_a_device():
    import depth_estimation_amd as d

    f = torch.zeros((1, 40, 60), dtype=torch.uint8)
    for good in ((1.0, 2.0), [1, 2], dict(P1=1.0, P2=2.0), dict(P1=0, P2=0, paths=0xff)):
        with pytest.raises(TypeError):              # the values are accepted; the CPU frames are not
            d.censusFlowDepthPair(f, f, 7, 9, 9, (30.0, 20.0), sgm=good)
    for bad in ((1.0,), (1.0, 2.0, 3), 5.0, "ab", (3.0, 2.0), (-1.0, 2.0), (1.0, float("nan")), dict(P1=1.0), dict(P1=1.0, P2=2.0, ring=3),
                dict(P1=1.0, P2=2.0, paths=0), dict(P1=1.0, P2=2.0, paths=256), dict(P1=1.0, P2=2.0, paths=1.0)):
        with pytest.raises(ValueError):
            d.censusFlowDepthPair(f, f, 7, 9, 9, (30.0, 20.0), sgm=bad)
