"""The 'mean' extraction of the one-call single-scale model (dfe_flow_pair_filtered_mean_f32), checked without a GPU:
  * its three matcher forms (feat_matching_flat_mean_kernel<MW, EXTRA>: 16 wide, 17 wide, 17 x 17 with the extra row task) compile
    inside the register file -- no scratch, at most 128 VGPRs (the 1024-thread launch bound);
  * the rule its epilogue applies for the confidence: extractOutput(m, scores, 0.11, imaxs) on a window's row marginals into zeroed
    scores, then scores > 0, is "some m_r, compared as a double, exceeds 0.11" -- checked against the oracle's extract_output."""
import os
import re
import subprocess
import sys

import numpy as np

from tests import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mean_matcher_forms_stay_inside_the_register_file():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "feat_matching_flat.hip"),
                          "flat_mean"], capture_output=True, text=True).stdout
    rows = {m[0]: tuple(int(x) for x in m[1:]) for m in re.findall(r"feat_matching_flat_mean_kernel<([^>]*)>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)}
    assert sorted(rows) == ["16, false", "17, false", "17, true"], out
    for form, (vgpr, scratch, _) in rows.items():
        assert scratch == 0 and vgpr <= 128, "feat_matching_flat_mean_kernel<%s>: %d VGPRs, %d B scratch" % (form, vgpr, scratch)


def test_mean_confidence_is_some_row_marginal_above_0_11():
    rng = np.random.default_rng(5)
    P, A = 4000, 17
    m = rng.uniform(0.0, 0.13, (P, A)).astype(np.float32)
    m[rng.uniform(size=(P, A)) < 0.85] *= np.float32(0.5)          # most rows well below, a spread of pixels with 0 .. several hits
    edge = np.float32(0.11)                                         # 0.11 rounds to a float BELOW 0.11: equal to it is not above it
    near = np.nextafter(edge, np.float32(1))
    m[0, :] = edge
    m[1, :] = 0.0
    m[1, 16] = near
    m[2, :] = 1.0 / 16
    m[3, :9] = 1.0                                                  # more than extractOutput's 8 kept values
    scores = np.zeros(P, np.float32)
    imaxs = np.zeros(P, np.int64)
    orc.extract_output(m.reshape(P, 1, A), 0.11, imaxs, scores)
    conf = scores > 0
    rule = (m.astype(np.float64) > 0.11).any(axis=1)
    assert np.array_equal(conf, rule)
    assert not conf[0] and conf[1] and not conf[2] and conf[3]
    assert 0.2 < conf.mean() < 0.8
