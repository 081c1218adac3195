"""The numpy restatement of the radial census cost (tests/census_radial_ref.py) against the properties its
definition implies, and the quality figures of the polar exposure scene -- the figures the device has to reproduce exactly
(tests/test_gpu_census_radial.py)."""
import functools

import numpy as np
import pytest

from tests import census_radial_ref as rr
from tests.census_ref import popcount

K, HWIN = rr.SCENE["k"], rr.SCENE["hWin"]


def _frames(seed, C=2, H=30, W=23):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(C, H, W)).astype(np.uint8), rng.randint(0, 256, size=(C, H, W)).astype(np.uint8)


@pytest.mark.parametrize("a", [1, 3, 5])
def test_rolling_the_frames_columns_rolls_the_costs_columns(a):
    f0, f1 = _frames(a)
    cost = rr.cost_volume(rr.signatures(f0, 5, 7), rr.signatures(f1, 5, 7), 6, a)
    for s in (1, 9, 22):
        g0, g1 = np.roll(f0, s, 2), np.roll(f1, s, 2)
        assert np.array_equal(rr.cost_volume(rr.signatures(g0, 5, 7), rr.signatures(g1, 5, 7), 6, a), np.roll(cost, s, 1)), (a, s)


def test_a_box_of_one_is_the_hamming_distance():
    f0, f1 = _frames(7)
    S0, S1 = rr.signatures(f0, 7, 3), rr.signatures(f1, 7, 3)
    cost = rr.cost_volume(S0, S1, 5, 1)
    assert cost.shape == (30 - 6 - 4, 23, 5)
    for y, x, d in ((0, 0, 0), (3, 22, 4), (19, 11, 2)):
        assert cost[y, x, d] == sum(int(popcount(S0[c, y, x] ^ S1[c, y + d, x]).sum()) for c in range(2))
    # a box of three by hand at a column whose box wraps
    c3 = rr.cost_volume(S0, S1, 5, 3)
    assert c3.shape == (18, 23, 5)
    assert c3[2, 0, 1] == sum(cost[2 + u, (0 + v - 1) % 23, 1] for u in range(3) for v in range(3))
    assert c3[5, 22, 4] == sum(cost[5 + u, (22 + v - 1) % 23, 4] for u in range(3) for v in range(3))


@pytest.mark.parametrize("a", [1, 3, 5])
def test_equal_frames_cost_nothing_at_no_motion(a):
    f0, _ = _frames(11)
    S = rr.signatures(f0, 3, 5)
    r = rr.flow(S, S, 14, 8, a, sub=True)
    assert not r["output"][:, :, 0].any() and not r["flow"].any() and not r["best"].any() and (r["match"] == 1).all()


def test_the_sub_pixel_rule_moves_by_half_a_label_at_the_most_and_not_at_the_edge():
    f0, f1 = _frames(5, C=1)
    S0, S1 = rr.signatures(f0, 3, 3), rr.signatures(f1, 3, 3)
    plain, sub = rr.flow(S0, S1, 8, 8, 3), rr.flow(S0, S1, 8, 8, 3, sub=True, zero_last_row=True)
    d = sub["flow"][:-1] - plain["flow"][:-1]
    assert np.abs(d).max() <= 0.5 and (d != 0).any() and not sub["flow"][-1].any()
    edge = (plain["flow"][:-1] == 0) | (plain["flow"][:-1] == 7)
    assert edge.any() and not d[edge].any()


@functools.lru_cache(maxsize=None)
def scene_shares(seed):
    """(census wrong share at a = 1, 3, 5; SSD wrong share at a = 3) of the polar exposure scene"""
    f0, f1 = rr.scene(seed)
    S0, S1 = rr.signatures(f0, K, K), rr.signatures(f1, K, K)
    census = tuple(rr.share_wrong(rr.flow(S0, S1, K * K - 1, HWIN, a)["flow"]) for a in (1, 3, 5))
    return census, rr.share_wrong(rr.ssd_flow(f0, f1, K, K, HWIN, 3))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scene_figures(seed):
    """measured: census 0.84 - 1.29 % wrong at a = 1 and none at a = 3 and 5; float64 SSD over the a = 3 support 3.1 - 13.1 %"""
    (c1, c3, c5), ssd3 = scene_shares(seed)
    print("seed %d: census wrong share %.4f / %.4f / %.4f at a = 1 / 3 / 5, SSD at a = 3 %.4f" % (seed, c1, c3, c5, ssd3))
    assert c3 == 0 and c5 == 0
    assert c1 <= 0.02
    assert ssd3 >= 0.02
