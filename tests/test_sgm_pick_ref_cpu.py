"""The numpy restatement of dfe_sgm_plane_pick_f32 (tests/sgm_pick_ref.py) on hand-made one-pixel volumes whose
answers can be read off the definition, and the quality claims of the section on the reference alone: the wide band scene, k = 7, 9 x 9,
SSD, seeds 0 .. 2.  No device."""
import numpy as np
import pytest

from tests import census_ref as cr
from tests import sgm_pick_ref as kr
from tests import sgm_plane_ref as pr

F = np.float32
INF = F(np.inf)


def _one(cells, **kw):
    p = kr.pick(np.asarray(cells, F)[None, None], **kw)
    return {k: v[0, 0] for k, v in p.items()}


def test_a_window_with_no_far_cell():
    for shape in ((1, 1), (3, 3), (2, 3), (1, 3)):
        cells = np.arange(1, shape[0] * shape[1] + 1, dtype=F).reshape(shape)
        cells[(shape[0] - 1) // 2, (shape[1] - 1) // 2] = 0.5          # the winner in the middle: every cell is within its 3 x 3
        p = _one(cells, subpixel=True)
        assert p["second"] == INF and p["unique"] == 0 and p["best"] == F(0.5), shape
    p = _one([[1, 5, 7, 3]])                                           # 1 x 4, the winner at the left end: cells 2 and 3 are far
    assert p["idx"] == 1 and p["second"] == 3 and p["unique"] == F(F(2) / F(3))
    p = _one([[9, 1, 5, 7]])                                           # the winner at cell 1: only cell 3 is far
    assert p["idx"] == 2 and p["second"] == 7 and p["unique"] == F(F(6) / F(7))


def test_a_winner_on_the_window_edge_moves_along_the_edge_only():
    cells = np.full((5, 5), 20, F)
    cells[0, 1:4] = (8, 2, 5)                                          # top edge: no row above
    p = _one(cells, subpixel=True)
    assert p["idx"] == 3 and p["flow_y"] == -2                         # off_y = 0
    den = F(F(8 - 2) + F(5 - 2))
    assert p["flow_x"] == F(F(0) + F(F(8 - 5) / F(2 * den))) and 0 < p["flow_x"] < 0.5
    cells = np.full((5, 5), 20, F)
    cells[1:4, 4] = (3, 1, 9)                                          # right edge: no column beyond
    p = _one(cells, subpixel=True)
    assert p["idx"] == 15 and p["flow_x"] == 2
    den = F(F(3 - 1) + F(9 - 1))
    assert p["flow_y"] == F(F(0) + F(F(3 - 9) / F(2 * den))) and -0.5 < p["flow_y"] < 0
    cells = np.full((5, 5), 20, F)
    cells[4, 0] = 1                                                    # a corner: neither axis moves
    p = _one(cells, subpixel=True)
    assert p["idx"] == 21 and p["flow_y"] == 2 and p["flow_x"] == -2
    assert _one(cells)["flow_y"] == 2 and p["second"] == 20 and p["unique"] == F(F(19) / F(20))


def test_a_flat_parabola_and_the_clamp():
    cells = np.full((3, 5), 7, F)
    cells[1, 3] = 7                                                    # every cell equal: the centre wins, den = 0 on both axes
    p = _one(cells, subpixel=True)
    assert p["idx"] == cr.middle_index(3, 5) and p["flow_y"] == 0 and p["flow_x"] == 0
    assert p["second"] == 7 and p["unique"] == 0                       # (7 - 7) / 7
    cells = np.full((3, 5), 9, F)
    cells[1, 1:4] = (4, 4, 9)                                          # a tie of the winner with its left neighbour: den = 5, off = -0.5 exactly
    p = _one(cells, subpixel=True)
    assert p["idx"] == 8 and p["flow_x"] == F(-0.5)                    # the centre class (8) wins the tie with class 7
    cells[1, 1:4] = (3, 4, 9)                                          # first minimum left of the centre
    cells[1, 0] = 3
    p = _one(cells, subpixel=True)                                     # winner class 6 (the first of two 3s), on the left edge
    assert p["idx"] == 6 and p["flow_x"] == -2


def test_second_not_above_zero_gives_no_uniqueness():
    cells = np.full((1, 5), 0, F)
    cells[0, 0] = -3
    p = _one(cells)
    assert p["idx"] == 1 and p["second"] == 0 and p["unique"] == 0     # second == 0
    cells[0, 2:] = -1
    p = _one(cells)
    assert p["second"] == -1 and p["unique"] == 0                      # second < 0
    cells[0, 2:] = 2
    p = _one(cells)
    assert p["second"] == 2 and p["unique"] == F(2.5)                  # (2 - -3) / 2: not clamped


def test_an_exact_tie_with_the_centre_and_the_gate():
    cells = np.full((5, 5), 9, F)
    cells[0, 0] = cells[2, 2] = 1                                      # class 1 ties with the centre class 13: the centre wins
    p = _one(cells, subpixel=True)
    assert p["idx"] == 13 and p["flow_y"] == 0 and p["flow_x"] == 0
    assert p["second"] == 1 and p["unique"] == 0                       # the other minimum is far: nothing unique about the winner
    cells[0, 0] = 4
    for mu, want in ((0.0, F(0.75)), (0.75, F(0.75)), (0.76, F(0)), (1.0, F(0))):
        assert _one(cells, min_unique=mu)["unique"] == want, mu
    assert _one(cells, min_unique=1.0)["idx"] == 13                    # the gate touches neither idx nor the flow


def test_pick_without_subpixel_is_arg_best():
    vol = np.random.default_rng(5).uniform(-3, 9, size=(4, 6, 5, 7)).astype(F)
    p = kr.pick(vol)
    idx, fy, fx = pr.arg_best(vol)
    assert np.array_equal(p["idx"], idx) and np.array_equal(p["flow_y"], fy) and np.array_equal(p["flow_x"], fx)
    assert np.array_equal(p["best"], vol.reshape(4, 6, -1).min(-1))
    q = kr.pick(vol, subpixel=True)
    assert np.abs(q["flow_y"] - fy).max() <= 0.5 and np.abs(q["flow_x"] - fx).max() <= 0.5 and not np.array_equal(q["flow_x"], fx)


# ---- the quality claims of DESIGN.md section 4.32, on the reference alone ----
# measured on this reference, seeds 0, 1, 2 (shares of the 58 x 90 output pixels)
WTA_WRONG = (0.166475, 0.168199, 0.163602)        # SSD winner-takes-all
SGM_WRONG = (0.057663, 0.031609, 0.056705)        # the 8-path aggregate at (P1, P2) = (400, 3200)
RIGHT_KEPT = (0.993795, 0.993551, 0.992671)       # of the right WTA vectors, those with uniqueness >= 0.2 on the raw volume
WRONG_KEPT = (0.064442, 0.075171, 0.040984)       # of the wrong ones
# a bound sits a quarter of the gap between the two quantities it separates away from the measured one
GAP_WRONG = min(WTA_WRONG) - max(SGM_WRONG)
GAP_KEPT = min(RIGHT_KEPT) - max(WRONG_KEPT)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_aggregate_repairs_the_band(seed):
    wta, sgm = float(kr.wrong(kr.wide_pick(seed, 0)).mean()), float(kr.wrong(kr.wide_pick(seed, 0xff)).mean())
    print("seed %d: wrong vectors WTA %.6f, 8 paths %.6f" % (seed, wta, sgm))
    assert wta >= min(WTA_WRONG) - GAP_WRONG / 4, "the scene is easier than the one that was measured"
    assert sgm <= max(SGM_WRONG) + GAP_WRONG / 4


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_uniqueness_separates_right_from_wrong_vectors(seed):
    p = kr.wide_pick(seed, 0)
    bad, kept = kr.wrong(p), p["unique"] > 0
    right_kept, wrong_kept = float(kept[~bad].mean()), float(kept[bad].mean())
    print("seed %d: kept at min_unique 0.2: %.6f of the right vectors, %.6f of the wrong ones" % (seed, right_kept, wrong_kept))
    assert right_kept >= min(RIGHT_KEPT) - GAP_KEPT / 4
    assert wrong_kept <= max(WRONG_KEPT) + GAP_KEPT / 4


def test_the_wide_band_scene_is_what_it_says():
    f0, f1 = kr.wide_band_scene(0)
    assert f0.shape == f1.shape == (1, 72, 104) and f0.dtype == np.uint8
    assert abs(float(f0[0, 28:44].mean()) - 127.5) < 0.5 and float(f0[0, 28:44].std()) < 2.5     # the band: 128 + N(0, 2), floored
    assert float(f0[0, :28].std()) > 10 and float(f0[0, 44:].std()) > 10                           # texture above and below
    assert kr.wide_volume(0).shape == (58, 90, 9, 9)
