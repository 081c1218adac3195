"""The numpy restatement of the sub-pixel rule on the raw census cost (tests/census_subpixel_ref.py; include/dfe.h)
on its own, no device: hand-made costs whose refined flow can be worked out on paper, the class decode against the pyramid's codec, and
the quality table -- the vee fit against the integer flow and the SSD paths' parabola on a scene moved by a fraction of a pixel.

The table as measured on this reference (median end-point error over the region, seeds 0 - 2, 56 x 72, k = 7, 9 x 9 window):
    C  agg  move             integer  parabola       vee
    1  3    (2.3, -2.6)      0.500    0.244 - 0.268  0.168 - 0.186
    1  3    (1.5, -0.5)      0.707    0.367 - 0.412  0.258 - 0.308
    1  3    (-1.25, 2.75)    0.354    0.179 - 0.185  0.144 - 0.155
    1  5    (2.3, -2.6)      0.500    0.180 - 0.208  0.107 - 0.132
    1  5    (1.5, -0.5)      0.707    0.268 - 0.327  0.171 - 0.217
    1  5    (-1.25, 2.75)    0.354    0.154 - 0.157  0.098 - 0.110
    3  3    (2.3, -2.6)      0.500    0.146 - 0.151  0.083 - 0.094
    3  3    (1.5, -0.5)      0.707    0.208 - 0.221  0.124 - 0.134
    3  3    (-1.25, 2.75)    0.354    0.136 - 0.141  0.077 - 0.079
    3  5    (2.3, -2.6)      0.500    0.118 - 0.133  0.058 - 0.066
    3  5    (1.5, -0.5)      0.707    0.154 - 0.164  0.088 - 0.094
    3  5    (-1.25, 2.75)    0.354    0.133 - 0.138  0.055 - 0.057
  recorded, nothing asserted (agg = 1: with one channel and no box 48 bits a pixel are too few to refine on):
    1  1    (2.3, -2.6)      0.671    0.503 - 0.517  0.500 - 0.525
    1  1    (1.5, -0.5)      0.707    0.586 - 0.606  0.572 - 0.614
    1  1    (-1.25, 2.75)    0.354    0.381 - 0.395  0.415 - 0.425     <- worse than the integer flow
    3  1    (2.3, -2.6)      0.500    0.285 - 0.301  0.221 - 0.235
    3  1    (1.5, -0.5)      0.707    0.373 - 0.389  0.271 - 0.286
    3  1    (-1.25, 2.75)    0.354    0.222 - 0.228  0.211 - 0.215
  the pyramid (96 x 128, C = 3, k = 7, 8 x 8, ratios 1, 2, 4, agg 3, move (2.3, -2.6), 16 pixels of border left out; the finest scale wins
  all but some 100 of 12288 pixels): integer 0.500, parabola 0.408 - 0.411, vee 0.404.  The x component, -2.6, lies on the border of the
  8 x 8 window (cells -3 .. 4), where no fit is made: the vee's gain there is the y axis' alone."""
import numpy as np
import pytest

from tests import census_ref as cr
from tests import census_subpixel_ref as sr

F = np.float32


def _vol(h, w, fill=50):
    return np.full((1, 1, h, w), fill, np.int64)


def _one(cost, idx, **kw):
    fy, fx = sr.refine(cost, np.array([[idx]], np.int64), **kw)
    return float(fy[0, 0]), float(fx[0, 0])


def test_hand_made_triples():
    # a strict minimum at (r, s) = (4, 4) of a 9 x 9 window, the centre: x (10, 4, 7) -> 3 / 12, y (6, 4, 12) -> -6 / 16
    c = _vol(9, 9)
    c[0, 0, 4, 4], c[0, 0, 4, 3], c[0, 0, 4, 5], c[0, 0, 3, 4], c[0, 0, 5, 4] = 4, 10, 7, 6, 12
    idx, _ = cr.arg_best(c)
    assert idx[0, 0] == 4 * 9 + 4 + 1
    assert _one(c, idx[0, 0]) == (float(F(-6) / F(16)), float(F(3) / F(12)))
    # off the centre the integer part comes with it: the same costs around (2, 6)
    c = _vol(9, 9)
    c[0, 0, 2, 6], c[0, 0, 2, 5], c[0, 0, 2, 7], c[0, 0, 1, 6], c[0, 0, 3, 6] = 4, 10, 7, 6, 12
    assert _one(c, cr.arg_best(c)[0][0, 0]) == (-2 + float(F(-6) / F(16)), 2 + float(F(3) / F(12)))
    # equal minima left and right: the point between them
    for left, want in ((True, -0.5), (False, 0.5)):
        c = _vol(9, 9)
        c[0, 0, 4, 4] = 4
        c[0, 0, 4, 3 if left else 5] = 4
        assert _one(c, 4 * 9 + 4 + 1) == (0.0, want)
        c = _vol(9, 9)
        c[0, 0, 4, 4] = 4
        c[0, 0, 3 if left else 5, 4] = 4
        assert _one(c, 4 * 9 + 4 + 1) == (want, 0.0)
    # a flat triple
    assert _one(_vol(9, 9), 4 * 9 + 4 + 1) == (0.0, 0.0)
    assert _one(_vol(9, 9), 2 * 9 + 7 + 1) == (-2.0, 3.0)


def test_window_edges_and_thin_windows():
    # a winner on each edge of the window: that axis keeps its integer, the other is fitted
    for r, s in ((0, 4), (8, 4), (4, 0), (4, 8), (0, 0), (8, 8)):
        c = _vol(9, 9)
        c[0, 0, r, s] = 4
        for rr, ss, v in ((r, s - 1, 10), (r, s + 1, 7), (r - 1, s, 6), (r + 1, s, 12)):
            if 0 <= rr < 9 and 0 <= ss < 9:
                c[0, 0, rr, ss] = v
        idx = cr.arg_best(c)[0][0, 0]
        assert idx == r * 9 + s + 1
        fy, fx = _one(c, idx)
        assert fy == r - 4 + (0.0 if r in (0, 8) else float(F(-6) / F(16)))
        assert fx == s - 4 + (0.0 if s in (0, 8) else float(F(3) / F(12)))
    # 1 x 9 and 9 x 1 windows: one axis has no neighbours at all
    c = _vol(1, 9)
    c[0, 0, 0, 6], c[0, 0, 0, 5], c[0, 0, 0, 7] = 4, 10, 7
    assert _one(c, 7) == (0.0, 2 + float(F(3) / F(12)))
    c = _vol(9, 1)
    c[0, 0, 6, 0], c[0, 0, 5, 0], c[0, 0, 7, 0] = 4, 6, 12
    assert _one(c, 7) == (2 + float(F(-6) / F(16)), 0.0)
    # a 2 x 2 window: nothing is refined, whichever cell wins (offsets floor((2 - 1) / 2) = 0)
    for n in range(4):
        c = _vol(2, 2)
        c[0, 0, n // 2, n % 2] = 4
        assert _one(c, n + 1) == (float(n // 2), float(n % 2))


def test_even_window_centre_tie_and_foreign_idx():
    # 8 x 8: the centre class is cell (3, 3) (getMiddleIndex 28); an equal minimum before it in class order loses to it, and the fit sees
    # the loser beside the winner: the point between them
    c = _vol(8, 8)
    c[0, 0, 3, 3] = c[0, 0, 3, 2] = 4
    idx = cr.arg_best(c)[0][0, 0]
    assert idx == cr.middle_index(8, 8) == 28
    assert _one(c, idx) == (0.0, -0.5)
    c = _vol(8, 8)
    c[0, 0, 3, 3] = c[0, 0, 0, 0] = 4
    assert cr.arg_best(c)[0][0, 0] == 28 and _one(c, 28) == (0.0, 0.0)
    # every cost equal: the centre, offset 0 (constant frames)
    z = np.zeros((1, 1, 8, 8), np.int64)
    assert cr.arg_best(z)[0][0, 0] == 28 and _one(z, 28) == (0.0, 0.0)
    # a class map from another producer, c0 not the minimum: the clamp (x: (0, 5, 6) -> m = 1, -6 / 2 -> -0.5; y: (9, 5, 0) -> +0.5) ...
    c = _vol(9, 9)
    c[0, 0, 4, 4], c[0, 0, 4, 3], c[0, 0, 4, 5], c[0, 0, 3, 4], c[0, 0, 5, 4] = 5, 0, 6, 9, 0
    assert _one(c, 4 * 9 + 4 + 1) == (0.5, -0.5)
    # ... and m <= 0 (both neighbours at or below c0): 0
    c[0, 0, 4, 3], c[0, 0, 4, 5], c[0, 0, 3, 4], c[0, 0, 5, 4] = 3, 4, 5, 5
    assert _one(c, 4 * 9 + 4 + 1) == (0.0, 0.0)
    # no class at all: the planes keep what they held
    for bad in (0, 82, -3):
        assert _one(c, bad, fy=np.full((1, 1), -7, F), fx=np.full((1, 1), -7, F)) == (-7.0, -7.0)


def test_offsets_stay_within_half_a_cell_where_c0_is_the_minimum():
    rng = np.random.RandomState(0)
    cm, c0, cp = rng.randint(0, 4726, size=(3, 20000))
    c0 = np.minimum(c0, np.minimum(cm, cp))
    m = np.maximum(cm - c0, cp - c0)
    raw = np.divide((cm - cp).astype(F), (2 * m).astype(F), out=np.zeros(cm.shape, F), where=m > 0)
    assert np.abs(raw).max() <= 0.5 and np.array_equal(sr.vee(cm, c0, cp, np.ones(cm.shape, bool)), raw)


def test_class_table_is_the_pyramids_codec(oracle):
    for maxh, maxw, ratios in ((8, 8, [1, 2, 4]), (8, 8, [1, 2]), (6, 6, [1, 3]), (16, 4, [1, 2, 4]), (4, 8, [1, 2]), (5, 7, [1])):
        tab = sr.class_table(maxh, maxw, ratios)
        assert len(tab) == oracle.multi_nclasses(maxh, maxw, ratios)
        for i, (s, a, b) in enumerate(tab):
            rc, y, x = oracle.x2yx_multi_number(maxh, maxw, ratios, i + 1)
            assert rc == 0 and (y, x) == ((a - (maxh - 1) // 2) * ratios[s], (b - (maxw - 1) // 2) * ratios[s]), (maxh, maxw, ratios, i)


def _row(C, agg, move):
    """(integer, parabola, vee) median end-point errors of the scene, one triple per seed"""
    k, win = sr.SCENE["k"], sr.SCENE["win"]
    out = []
    for seed in sr.SEEDS:
        f0, f1 = sr.scene(seed, move, C)
        cost = cr.cost_volume(cr.signature(f0, k, k), cr.signature(f1, k, k), win, win, agg)
        idx, _ = cr.arg_best(cost)
        iy, ix = cr.decode(idx, win, win)
        vy, vx = sr.refine(cost, idx)
        py, px = sr.refine(cost, idx, fit=sr.parabola)
        assert np.array_equal(np.round(vy - iy), np.zeros_like(vy)) and np.abs(vy - iy).max() <= 0.5 and np.abs(vx - ix).max() <= 0.5
        out.append((sr.median_epe(iy, ix, move), sr.median_epe(py, px, move), sr.median_epe(vy, vx, move)))
    return out


@pytest.mark.parametrize("C, agg", [(1, 3), (1, 5), (3, 3), (3, 5)])
def test_quality_table_vee_beats_integer_and_parabola(C, agg):
    for move in sr.MOVES:
        for seed, (e_int, e_par, e_vee) in zip(sr.SEEDS, _row(C, agg, move)):
            print("C=%d agg=%d move=%s seed=%d: integer %.3f parabola %.3f vee %.3f" % (C, agg, move, seed, e_int, e_par, e_vee))
            assert e_vee < e_int, (C, agg, move, seed, e_int, e_vee)
            assert e_vee <= e_par, (C, agg, move, seed, e_par, e_vee)


@pytest.mark.parametrize("C", [1, 3])
def test_quality_table_without_a_box_is_recorded(C):
    """agg = 1: the numbers of the docstring's last rows; nothing is asserted about them -- with one channel the refined flow can be
    worse than the integer one, which is why the documents name agg >= 3 or several channels as the refinement's ground"""
    for move in sr.MOVES:
        for seed, (e_int, e_par, e_vee) in zip(sr.SEEDS, _row(C, 1, move)):
            print("C=%d agg=1 move=%s seed=%d: integer %.3f parabola %.3f vee %.3f" % (C, move, seed, e_int, e_par, e_vee))
            assert np.isfinite([e_int, e_par, e_vee]).all()


def test_quality_table_pyramid():
    from tests import census_pyramid_ref as cp

    s = cp.SCENE
    move, ratios = (2.3, -2.6), list(s["ratios"])
    for seed in sr.SEEDS:
        f0, f1 = sr.scene(seed, move, s["C"], s["H"], s["W"], s["margin"])
        f0, f1 = f0.astype(F), f1.astype(F)
        ch = cp.chain(f0, f1, s["k"], s["win"], s["win"], ratios, s["a"], cp.default_beta(s["C"], s["a"]))
        vols = [cp.scale_volume(f0, f1, r, s["k"], s["win"], s["win"], s["a"], 1.0) for r in ratios]
        flow, scale = sr.pyramid_refine(vols, ch["idx"], s["win"], s["win"], ratios)
        par, _ = sr.pyramid_refine(vols, ch["idx"], s["win"], s["win"], ratios, fit=sr.parabola)
        assert (scale >= 0).all() and (scale == 0).mean() > 0.9                        # the finest scale wins
        rho = np.array(ratios)[scale]
        assert (np.abs(flow[0] - ch["y"]) <= rho / 2).all() and (np.abs(flow[1] - ch["x"]) <= rho / 2).all()
        b = s["border"]
        e_int, e_par, e_vee = sr.median_epe(ch["y"], ch["x"], move, b), sr.median_epe(par[0], par[1], move, b), sr.median_epe(flow[0], flow[1], move, b)
        print("pyramid seed=%d: integer %.3f parabola %.3f vee %.3f" % (seed, e_int, e_par, e_vee))
        assert e_vee < e_int, (seed, e_int, e_vee)
