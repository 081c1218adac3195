"""The semi-global aggregation kernels (csrc/sgm.hip) inside the register file: sgm_path_kernel with one and with
two labels a lane and the four forms of sgm_sum_kernel, 0 bytes of scratch and 0 SGPR spills -- the load pipeline's slots are arrays indexed
by unrolled constants, and a form that indexed them at run time would move them to scratch.  And the argument checks of
semiGlobalAggregate that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgm_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "sgm.hip"), "sgm_"],
                         capture_output=True, text=True).stdout
    rows = re.findall(r"^(sgm_\w+)<([^>]*)>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out, flags=re.M)
    want = sorted([("sgm_path_kernel", l) for l in "12"] + [("sgm_sum_kernel", "%s, %s" % (l, f)) for l in "12" for f in ("false", "true")])
    assert sorted(r[:2] for r in rows) == want and len(rows) == len(re.findall(r"^sgm_", out, flags=re.M)), out
    for name, form, vgpr, scratch, spill in rows:
        text = "%s<%s>: %s VGPRs, %s B scratch, %s SGPR spills" % (name, form, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, text
        assert int(vgpr) <= 64, text + ": below 8 waves a SIMD"


def test_semiGlobalAggregate_argument_checks_need_no_device():
    import depth_estimation_amd as d

    vol = torch.zeros((5, 7, 12))
    with pytest.raises(TypeError):                  # the values are accepted; the CPU tensor is not
        d.semiGlobalAggregate(vol, 1.0, 2.0, paths=0xff, ring=7, want_volume=False)
    with pytest.raises(TypeError):
        d.semiGlobalAggregate(vol.double(), 1.0, 2.0)
    for bad in (dict(paths=0), dict(paths=256), dict(paths=3.0), dict(ring=-1), dict(ring=8), dict(P1=-1.0), dict(P1=3.0), dict(P2=float("inf")),
                dict(volume=vol[0]), dict(volume=torch.zeros((5, 7, 33))), dict(volume=torch.zeros((5, 0, 3)))):
        with pytest.raises(ValueError):
            d.semiGlobalAggregate(**{**dict(volume=vol, P1=1.0, P2=2.0), **bad})
