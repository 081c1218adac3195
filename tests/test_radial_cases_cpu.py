"""The conditions under which tests/test_gpu_radial_edges.py says something, checked on the oracle alone (no GPU): the cases of
tests/radial_cases.py have few near-ties between their two best costs, a polar flow that uses the window, next to no P2C pixel on the
angle seam, finite outputs -- and at least three of them tell a float scaled radius in getP2CMask's `ky` from a double one."""
import numpy as np
import pytest

from tests import oracle as orc
from tests import radial_cases as rc


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_case_is_not_vacuous(name):
    C, hIn, wIn, hWin, layers, alpha, e2 = rc.CASES[name]
    ref, g = rc.reference(name), rc.geometry(name)
    out, pf = ref["output"], ref["polar_flow"]
    assert out.shape == (g["hm"], wIn, hWin) and ref["flow"].shape == (g["hOut"], g["wOut"]) and g["hm"] >= 1
    for k, v in ref.items():
        assert np.isfinite(v).all(), k
    # geometry()'s constants are the oracle path's: its P2C grid and its flow2depth reproduce the oracle's flow, depth and confidences
    assert np.array_equal(orc.warp_bilinear(pf[None], rc.p2c_grid(name))[0], ref["flow"])
    depth, confs = orc.flow_to_depth_radial(ref["flow"], g["cx"], g["cy"], g["infty"])
    assert np.array_equal(depth, ref["depth"]) and np.array_equal(confs, ref["confs"])
    gap = rc.cost_gap(out)
    near, exact = float(((gap > 0) & (gap <= rc.TIE_REL * np.abs(out).max())).mean()), float((gap == 0).mean())
    seam = float(rc.seam_set(name).mean())
    values = np.unique(pf)
    print("case %s: inexact near-ties %.2f %%, exact ties %.2f %% (taps clamped to the frame border; not excluded anywhere), %d flow values, "
          "%.1f %% of the flow > 0, angle seam %.3f %%" % (name, 100 * near, 100 * exact, len(values), 100 * float((pf > 0).mean()), 100 * seam))
    assert near <= rc.TIE_CAP
    assert len(values) >= 3 and float((pf > 0).mean()) > 0.4
    if name in rc.FULL_WINDOW:
        assert np.array_equal(values, np.arange(hWin))
    assert seam <= rc.SEAM_CAP
    # the geometry the case is in the table for
    kW, hf = layers[0][2], ref["feat2"].shape[1]                              # hf: rows of a full polar frame's features
    assert hf == hIn - 16 and ref["feat2"].shape[2] == wIn >= (kW - 1) // 2
    assert {"A": hIn % 2 == 1 and hf % 4 == 3 and C == 1, "B": wIn == 257 and e2 == (0.0, 0.0), "C": C > 4 and alpha == 0.8,
            "D": kW != 17 and hf % 4 == 1, "E": layers[0][3] == 6 and alpha == 1.25, "F": g["hm"] == 1 and wIn == (kW - 1) // 2,
            "G": g["hm"] == 64 and wIn + 16 == 288, "H": wIn == 256 and layers[-1][3] == 7 and hIn % 2 == 1}[name]


def test_enough_cases_tell_the_two_ky_conventions_apart():
    differ = [n for n in sorted(rc.CASES) if rc.ky_pair(n)[0] != rc.ky_pair(n)[1]]
    print("ky with a float scaled radius differs from the double one in", differ)
    assert len(differ) >= 3
    for n in differ:
        f, d = rc.ky_pair(n)
        assert abs(float(f) - float(d)) <= 2 * np.spacing(np.float32(f))      # (one ulp: the two are roundings of nearly the same double)
