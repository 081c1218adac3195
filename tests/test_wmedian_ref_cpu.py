"""The numpy restatement of the guided weighted median (tests/wmedian_ref.py; include/dfe.h: dfe_weighted_median_f32, DESIGN section
4.27) against the consequences its definition states, and the two-motion scene: what the guide buys.  No device."""
import numpy as np
import pytest

from tests.wmedian_ref import SCENE, scene_scores, two_motion_scene, weighted_median_ref, wmedian_pixel

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def test_k1_is_the_identity_on_valid_pixels():
    rng = np.random.default_rng(0)
    v = rng.uniform(-4, 4, size=(3, 9, 13)).astype(F)
    w = np.where(rng.random((9, 13)) < 0.6, 1, 0).astype(F)
    v[1, 2, 3] = np.nan                    # a non-finite channel: the pixel is not a sample
    w[2, 3] = 1
    out, filtered = weighted_median_ref(v, w, k=1)
    ok = (w > 0) & np.isfinite(v).all(axis=0)
    assert np.array_equal(filtered, ok.astype(F))
    assert np.array_equal(_bits(out[:, ok]), _bits(v[:, ok])) and not out[:, ~ok].any()
    out1, f1 = weighted_median_ref(v, None, k=1, region=(1, 2, 5, 7))
    inR = np.zeros((9, 13), bool)
    inR[1:6, 2:9] = True
    keep = inR & np.isfinite(v).all(axis=0)
    assert np.array_equal(_bits(out1[:, keep]), _bits(v[:, keep])) and not out1[:, ~keep].any() and np.array_equal(f1, keep.astype(F))


@pytest.mark.parametrize("k", [3, 5, 7])
def test_unit_weights_give_the_plain_median_on_full_windows(k):
    rng = np.random.default_rng(k)
    v = rng.uniform(-9, 9, size=(2, 17, 21)).astype(F)
    out, filtered = weighted_median_ref(v, None, k=k)
    h = k // 2
    assert filtered.all()
    for c in range(2):
        win = np.lib.stride_tricks.sliding_window_view(v[c], (k, k)).reshape(17 - k + 1, 21 - k + 1, k * k)
        assert np.array_equal(out[c, h : 17 - h, h : 21 - h], np.median(win, axis=-1).astype(F))


def test_a_clipped_even_window_gives_the_lower_median():
    v = np.arange(12, dtype=F).reshape(1, 3, 4)
    out, _ = weighted_median_ref(v, None, k=3)
    # corner (0, 0): the window is {0, 1, 4, 5}: the lower of the two middle values
    assert out[0, 0, 0] == 1 and out[0, 2, 3] == 7
    # an edge pixel: 2 x 3 = {0, 1, 2, 4, 5, 6} -> 2
    assert out[0, 0, 1] == 2
    # inside a region the window is clipped to the REGION, not to the frame
    out, filtered = weighted_median_ref(v, None, k=3, region=(1, 1, 2, 2))
    assert out[0, 1, 1] == 6 and filtered.sum() == 4 and not out[0, 0].any()          # {5, 6, 9, 10} -> 6
    # weights move it: {0 (w 1), 1 (w 0.25), 4 (w 0.25), 5 (w 1)}: T = 10240, 2 S(0) = 8192, 2 S(1) = 10240 >= T -> 1
    w = np.ones((3, 4), F)
    w[0, 1] = w[1, 0] = 0.25
    assert weighted_median_ref(v, w, k=3)[0][0, 0, 0] == 1
    w[0, 0] = 0.5                                                                      # T = 8192, 2 S(0) = 4096, 2 S(1) = 6144, 2 S(4) = 8192 -> 4
    assert weighted_median_ref(v, w, k=3)[0][0, 0, 0] == 4


def test_planted_specials_behave_as_defined():
    rng = np.random.default_rng(4)
    v = rng.uniform(-3, 3, size=(2, 8, 10)).astype(F)
    w = np.ones((8, 10), F)
    holes = [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (2, 4)]
    v[0, 1, 1], v[1, 1, 2], v[0, 1, 3] = np.nan, np.inf, -np.inf            # values that are not finite, under w = 1
    w[2, 1], w[2, 2], w[2, 3], w[2, 4] = np.nan, np.inf, -0.5, 5e-7          # weights that make a hole
    w[5, 5], w[5, 6] = 7.0, 1e30                                             # above 1: as 1
    w[6, 6] = 1e-6                                                           # the smallest valid weight: wt = (uint32)(0.004096 + 0.5) = 0
    out, filtered = weighted_median_ref(v, w, k=1)
    for y, x in holes + [(6, 6)]:
        assert filtered[y, x] == 0 and not out[:, y, x].any(), (y, x)
    assert np.array_equal(_bits(out[:, 5, 5:7]), _bits(v[:, 5, 5:7])) and filtered[5, 5] == filtered[5, 6] == 1
    out, filtered = weighted_median_ref(v, w, k=5)
    assert np.isfinite(out).all() and filtered.all()
    # the same answer as with the holes' values replaced by anything finite: what is under a = 0 is never read
    v2 = v.copy()
    for y, x in holes:
        v2[:, y, x] = 100.0
    w2 = w.copy()
    for y, x in holes:
        w2[y, x] = 0
    out2, _ = weighted_median_ref(v2, w2, k=5)
    assert np.array_equal(_bits(out), _bits(out2))
    # a weight above 1 counts as 1
    w3 = w.copy()
    w3[5, 5] = w3[5, 6] = 1
    assert np.array_equal(_bits(weighted_median_ref(v, w3, k=5)[0]), _bits(out))


def test_guide_range_term():
    rng = np.random.default_rng(5)
    v = rng.uniform(-3, 3, size=(1, 7, 9)).astype(F)
    g = rng.uniform(0, 4, size=(2, 7, 9)).astype(F)
    # sigma <= 0, NaN, no guide, Cg = 0: no range term
    base = weighted_median_ref(v, None, k=3)[0]
    for kw in (dict(guide=g, sigma=0.0), dict(guide=g, sigma=-1.0), dict(guide=g, sigma=float("nan")), dict(guide=None, sigma=3.0), dict(guide=g[:0], sigma=3.0)):
        assert np.array_equal(_bits(weighted_median_ref(v, None, k=3, **kw)[0]), _bits(base))
    # a sigma so small that only samples of the pixel's own guide value count: the pixel itself
    out, filtered = weighted_median_ref(v, None, g, 1e-3, 5)
    assert np.array_equal(_bits(out), _bits(v)) and filtered.all()
    # a NaN in the guide at p: every r is NaN, T = 0; its neighbours lose that one sample only
    g2 = g.copy()
    g2[1, 3, 4] = np.nan
    out, filtered = weighted_median_ref(v, None, g2, 100.0, 3)
    assert filtered[3, 4] == 0 and out[0, 3, 4] == 0 and filtered.sum() == 7 * 9 - 1 and np.isfinite(out).all()
    # a sigma whose square overflows: inv_s2 = 0, r = 1 everywhere; one whose square underflows: inv_s2 = Inf, 0 * Inf = NaN at p itself, T = 0
    assert np.array_equal(_bits(weighted_median_ref(v, None, g, 1e30, 3)[0]), _bits(base))
    out, filtered = weighted_median_ref(v, None, g, 1e-30, 3)
    assert not filtered.any() and not out.any()


def test_negative_zero_sorts_below_positive_zero():
    v = np.array([[[0.0, -0.0]]], F)
    out, _ = weighted_median_ref(v, None, k=3)             # both windows are {+0, -0}: the lower one is -0
    assert np.array_equal(_bits(out), _bits(np.array([[[-0.0, -0.0]]], F)))
    v = np.array([[[0.0, -0.0, 0.0]]], F)
    out, _ = weighted_median_ref(v, None, k=3)             # the middle: {+0, -0, +0} -> +0
    assert _bits(out)[0, 0, 1] == 0
    v = np.array([[[-1.0, -2.0, 3.0, -0.0, 1e-40]]], F)     # negatives in order, a denormal above -0
    out, _ = weighted_median_ref(v, None, k=5)
    assert out[0, 0, 2] == 0 and np.signbit(out[0, 0, 2]) and out[0, 0, 0] == -1.0        # {-2, -1, -0, 1e-40, 3}; {-2, -1, 3} clipped


@pytest.mark.parametrize("Cg,sigma", [(0, 0.0), (1, 3.0), (3, 0.7)])
def test_the_stacked_form_is_the_literal_definition(Cg, sigma):
    rng = np.random.default_rng(7 + Cg)
    v = rng.integers(-3, 4, size=(2, 12, 15)).astype(F)     # many ties
    w = np.where(rng.random((12, 15)) < 0.5, rng.choice(np.array([1, 0.5, 1e-3], F), size=(12, 15)), 0).astype(F)
    g = rng.uniform(0, 2, size=(Cg, 12, 15)).astype(F) if Cg else None
    R = (1, 2, 10, 12)
    for k in (3, 7):
        out, filtered = weighted_median_ref(v, w, g, sigma, k, R)
        for y in range(R[0], R[0] + R[2]):
            for x in range(R[1], R[1] + R[3]):
                o, f = wmedian_pixel(v, w, g, sigma, k, R, y, x)
                assert np.array_equal(_bits(o), _bits(out[:, y, x])) and f == filtered[y, x], (k, y, x)
        assert 0 < filtered.sum() and not out[:, 0].any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_guide_moves_the_band_to_its_own_side(seed):
    """DESIGN section 4.27's table: 64 x 96, k = 11, a one-channel guide, sigma = 40.  Guided: every band pixel away from the corners
    takes the rectangle's motion and no non-band pixel is left off by 0.5 px; unguided: none of the band, and about 1 % of the rest."""
    sc = two_motion_scene(seed)
    assert sc["band"].sum() == 144
    before = scene_scores(sc["flow"], sc)
    assert before[0] == 0.0 and 0.07 < before[1] < 0.13
    guided = scene_scores(weighted_median_ref(sc["flow"], None, sc["guide"], SCENE["sigma"], SCENE["k"])[0], sc)
    plain = scene_scores(weighted_median_ref(sc["flow"], None, None, 0.0, SCENE["k"])[0], sc)
    print("seed %d: band fixed %.3f guided, %.3f unguided; non-band off by >= 0.5 px: %.4f guided, %.4f unguided (%.4f before)"
          % (seed, guided[0], plain[0], guided[1], plain[1], before[1]))
    assert guided[0] >= 0.95 and plain[0] <= 0.05 and guided[1] < plain[1]
