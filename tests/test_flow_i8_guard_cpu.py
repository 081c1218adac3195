"""The int8 flow sweep (csrc/ssd_flow_i8.hip) and the gated float sweep behind it inside the register file, and the identity the int8 kernel
rests on: on bytes, |a|^2 + |b|^2 - 2 a.b with a' = a - 128, b' = b - 128 in integers IS the sum of squared differences, bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depth-estimation_amd", "csrc")

# VGPRs of ssd_flow_i8_kernel<R> as built when the kernel was written (three waves per SIMD); more means a spill is near or occupancy drops
I8_VGPR = {"1": 167, "2": 166}


def _kres(src, pat):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(CSRC, src), pat], capture_output=True, text=True).stdout


def test_int8_sweep_stays_inside_the_register_file():
    out = _kres("ssd_flow_i8.hip", "ssd_flow_i8_kernel")
    rows = dict((r, (int(v), int(s))) for r, v, s in re.findall(r"ssd_flow_i8_kernel<(\d)>\s+VGPR (\d+) scratch (\d+)", out))
    assert sorted(rows) == ["1", "2"], out
    for r, (vgpr, scratch) in rows.items():
        assert scratch == 0 and vgpr <= I8_VGPR[r], "ssd_flow_i8_kernel<%s>: %d VGPRs, %d B scratch" % (r, vgpr, scratch)


def test_gated_float_sweep_stays_inside_the_register_file():
    out = _kres("ssd_cost_volume.hip", "rowimg_flow_gated")
    rows = re.findall(r"ssd_cv_rowimg_flow_gated_kernel<3, 7, 8>\s+VGPR (\d+) scratch (\d+)", out)
    assert len(rows) == 1, out
    vgpr, scratch = (int(x) for x in rows[0])
    assert vgpr <= 128 and scratch <= 8, "gated float sweep: %d VGPRs, %d B scratch" % (vgpr, scratch)


def test_shifted_byte_algebra_equals_the_oracle_cost_volume(oracle):
    K, WIN, Ho, Wo = 7, 33, 2, 3
    H, W = Ho + K + WIN - 2, Wo + K + WIN - 2
    rng = np.random.default_rng(3)
    f0 = rng.integers(0, 256, (3, H, W)).astype(np.float32)
    f1 = rng.integers(0, 256, (3, H, W)).astype(np.float32)
    f1[:, :8, :8] = 0      # the extremes meet somewhere: 255 against 0
    f0[:, 16:24, 16:24] = 255
    ref = oracle.ssd_cost_volume(f0, f1, K, K, WIN, WIN).reshape(Ho, Wo, WIN, WIN)
    a, b = f0.astype(np.int64) - 128, f1.astype(np.int64) - 128
    assert a.min() >= -128 and a.max() <= 127 and b.min() >= -128 and b.max() <= 127   # int8 operands

    def patch(x, y0, x0):
        return x[:, y0 : y0 + K, x0 : x0 + K].ravel()

    got = np.empty((Ho, Wo, WIN, WIN), np.float32)
    for y in range(Ho):
        for x in range(Wo):
            pa = patch(a, y + 16, x + 16)
            s0 = int(pa @ pa)
            for dy in range(WIN):
                for dx in range(WIN):
                    pb = patch(b, y + dy, x + dx)
                    e = 2 * int(pa @ pb) - int(pb @ pb)          # what the kernel maximises: fits 24 bits signed
                    assert -(1 << 23) <= e < (1 << 23)
                    got[y, x, dy, dx] = np.float32(s0 - e)       # < 2^24: exact as a float
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(ref, np.float32).view(np.uint8))
