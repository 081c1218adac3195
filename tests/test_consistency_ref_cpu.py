"""The float64 restatement of the forward-backward consistency definition (tests/consistency_ref64.py; include/dfe.h) pinned to hand-worked
cases, and what the check is for: on a scene with a known covered band, the oracle's SSD flows in both directions plus the reference mask
flag the band and leave the un-occluded interior alone.  No GPU."""
import numpy as np

from tests import refpath as rp
from tests.consistency_ref64 import consistency_ref, occlusion_scene

INF = np.inf


def _const(H, W, dy, dx):
    f = np.empty((2, H, W), np.float32)
    f[0], f[1] = dy, dx
    return f


def test_one_by_one_region():
    fw, bw = _const(5, 7, 0, 0), _const(5, 7, 0, 0)
    m, e = consistency_ref(fw, bw, (2, 3, 1, 1), 0.0)
    want = np.zeros((5, 7))
    want[2, 3] = 1
    assert np.array_equal(m, want) and not e.any()
    fw[1, 2, 3] = 0.5      # any step leaves a one-pixel region
    m, e = consistency_ref(fw, bw, (2, 3, 1, 1), 10.0)
    assert not m.any() and e[2, 3] == INF and np.count_nonzero(e) == 1


def test_constant_integer_flow_and_the_strip_that_leaves():
    H, W, R = 12, 16, (1, 2, 9, 11)
    fw, bw = _const(H, W, 2, -3), _const(H, W, -2, 3)
    m, e = consistency_ref(fw, bw, R, 0.0)
    want = np.zeros((H, W))
    want[1 : 10 - 2, 2 + 3 : 13] = 1      # q = p + (2, -3) stays inside rows 1..9, columns 2..12
    assert np.array_equal(m, want)
    inR = np.zeros((H, W), bool)
    inR[1:10, 2:13] = True
    assert (e[inR & (want == 0)] == INF).all() and not e[~inR].any() and not e[want == 1].any()


def test_last_row_is_inside_a_fraction_beyond_is_not():
    H, W, R = 10, 8, (2, 1, 6, 5)          # rows 2..7, columns 1..5
    fw, bw = _const(H, W, 0, 0), _const(H, W, 0, 0)
    fw[0, 5, 3] = 2.0                      # q.y = 7: R's last row
    fw[0, 5, 4] = 2.25                     # q.y = 7.25: ceil = 8 is outside
    fw[1, 4, 2] = 3.0                      # q.x = 5: R's last column
    fw[1, 4, 3] = 2.25                     # q.x = 5.25
    fw[0, 3, 2] = -1.0                     # q.y = 2: first row
    fw[0, 3, 3] = -1.25                    # q.y = 1.75
    m, e = consistency_ref(fw, bw, R, 4.0)
    assert m[5, 3] == 1 and e[5, 3] == 2.0 and m[4, 2] == 1 and e[4, 2] == 3.0 and m[3, 2] == 1 and e[3, 2] == 1.0
    for p in ((5, 4), (4, 3), (3, 3)):
        assert m[p] == 0 and e[p] == INF


def test_non_finite_forward_flow():
    fw, bw = _const(6, 6, 0, 0), _const(6, 6, 0, 0)
    fw[0, 2, 2] = np.nan
    fw[1, 3, 3] = np.inf
    fw[1, 4, 4] = -np.inf
    m, e = consistency_ref(fw, bw, (0, 0, 6, 6), 1.0)
    for p in ((2, 2), (3, 3), (4, 4)):
        assert m[p] == 0 and e[p] == INF
    assert m.sum() == 33 and np.count_nonzero(e) == 3


def test_nan_neighbour_of_the_backward_flow_counts_only_with_weight():
    fw, bw = _const(6, 6, 0, 0), _const(6, 6, 0, 0)
    fw[:, 2, 2] = (1.0, 1.0)               # integral q = (3, 3): one tap, the NaNs around it carry weight 0
    bw[:, 3, 3] = (-1.0, -1.0)
    bw[:, 3, 4] = np.nan
    bw[:, 4, 3] = np.nan
    bw[:, 4, 4] = np.nan
    fw[:, 1, 1] = (0.0, 0.5)               # q = (1, 1.5): taps (1, 1), (1, 2) with weight 1/2 each, row 2 with weight 0
    bw[:, 2, 1] = np.nan
    bw[:, 2, 2] = np.inf
    bw[1, 1, 1], bw[1, 1, 2] = -0.25, -0.75
    m, e = consistency_ref(fw, bw, (0, 0, 6, 6), 0.0)
    assert m[2, 2] == 1 and e[2, 2] == 0 and m[1, 1] == 1 and e[1, 1] == 0
    fw[:, 0, 2] = (2.5, 1.0)               # q = (2.5, 3): taps (2, 3) and (3, 3); then (2, 3) is made NaN
    m, e = consistency_ref(fw, bw, (0, 0, 6, 6), 5.0)
    assert m[0, 2] == 1 and np.isfinite(e[0, 2])
    bw[0, 2, 3] = np.nan
    m, e = consistency_ref(fw, bw, (0, 0, 6, 6), 5.0)
    assert m[0, 2] == 0 and e[0, 2] == INF
    assert m[2, 2] == 1 and m[1, 1] == 1
    # the pixels whose own q lands on a NaN are flagged too
    assert m[3, 4] == 0 and e[3, 4] == INF


def test_even_window_plus_eight_has_no_backward_counterpart():
    """A 16-wide window decodes displacements -7 .. +8: a true forward motion of +8 can be found, the matching -8 cannot, so the backward
    arg-min is some other cell and the check rejects the pixel; +7 / -7 passes."""
    H, W = 4, 40
    for d, back, want in ((8, -7, 0), (7, -7, 1)):
        fw, bw = _const(H, W, 0, d), _const(H, W, 0, back)
        m, e = consistency_ref(fw, bw, (0, 0, H, W), 0.5)
        assert (m[:, : W - d] == want).all() and (e[:, : W - d] == abs(d + back)).all()
        assert not m[:, W - d :].any() and (e[:, W - d :] == INF).all()


def test_tolerance_is_compared_as_the_fp32_square():
    fw, bw = _const(8, 8, 0, 0), _const(8, 8, 0, 0)
    fw[:, 0, 0] = (3, 4)                                 # |e| = 5 exactly
    assert consistency_ref(fw, bw, (0, 0, 8, 8), 5.0)[0][0, 0] == 1
    assert consistency_ref(fw, bw, (0, 0, 8, 8), np.nextafter(np.float32(5), np.float32(0)))[0][0, 0] == 0


# ---- what the feature is for ---------------------------------------------------------------------------------------------------------
SCENE = dict(H=64, W=96, k=5, win=9, bg=(1, -2), fg=(-2, 3), rect=(18, 28, 28, 36))
COVERED_FLAGGED = (0.815, 0.798, 0.798)   # seeds 0, 1, 2
COVERED_MARGIN = 0.017                    # their spread


def scene_shares(seed, flows):
    """(share of the covered band flagged, share of the interior flagged) with `flows(f0, f1)` -> flow [2][H][W] of the pair step."""
    s = SCENE
    H, W, k, win = s["H"], s["W"], s["k"], s["win"]
    Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
    R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo)
    reach = (win - 1) // 2 + (k - 1) // 2
    f0, f1, covered, interior = occlusion_scene(H, W, s["bg"], s["fg"], s["rect"], reach, R, seed=seed)
    assert covered.sum() == 233 and interior.sum() == 1007
    m, _ = consistency_ref(flows(f0, f1), flows(f1, f0), R, 1.0)
    return 1.0 - float(m[covered].mean()), 1.0 - float(m[interior].mean())


def test_covered_band_is_flagged_and_interior_is_not():
    """64 x 96 frames, k = 5, a 9 x 9 window, background moving by (1, -2), a 28 x 36 rectangle by (-2, 3): 233 background pixels are
    covered in frame 1, 1007 pixels are farther than the window's reach (4 + 2) from every motion boundary and from R's edge.  With
    the oracle's SSD flow in both directions and the reference mask at tol = 1, the covered band is flagged to 0.815 / 0.798 / 0.798
    (seeds 0 / 1 / 2; the rest found some patch that matches back) and the interior to 0.000 on every seed.  Each seed is asserted
    against the three seeds' mean within their spread; the interior share has no spread, so it is asserted to be 0."""
    mean = sum(COVERED_FLAGGED) / 3
    for seed in (0, 1, 2):
        cov, inter = scene_shares(seed, lambda a, b: rp.dense_flow_oracle(a, b, SCENE["win"], SCENE["win"], SCENE["k"], SCENE["k"])["flowp"][:2])
        print("seed %d: covered band flagged %.3f, interior flagged %.4f" % (seed, cov, inter))
        assert abs(cov - mean) <= COVERED_MARGIN, (seed, cov)
        assert inter == 0.0, (seed, inter)
