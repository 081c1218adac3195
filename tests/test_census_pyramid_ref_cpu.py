"""The numpy restatement of the census pyramid (tests/census_pyramid_ref.py) with no device: the fitness of its
case table -- a row whose own tie share came near the 2 % that the device may differ on would test nothing, and a scale that wins no
pixels moves no class id -- and the quality statement of the exposure scene, census against the SSD oracle chain.  Every threshold here
comes from the references, none from the device."""
import functools

import numpy as np
import pytest

from tests import census_pyramid_ref as cp
from tests import pyramid_cases as pc
from tests.census_ref import cost_volume, signature


@pytest.mark.parametrize("c", cp.FIT, ids=lambda c: c.id)
def test_row_is_fit_on_the_reference(c, oracle):
    ref = cp.reference(c.no)
    ties = float(pc.tie_mask(ref).mean())
    wins = np.bincount(pc.scale_of(ref["idx"], c.ratios, c.mh, c.mw).ravel(), minlength=len(c.ratios)).tolist()
    print("row %d: tie share %.4f (table %.4f), wins per scale %s (table %s)" % (c.no, ties, c.ties, wins, c.wins))
    assert ties <= cp.FIT_TIE_CAP
    assert min(wins) >= pc.MIN_WINS
    assert abs(ties - c.ties) < 5e-5 and wins == c.wins, "the table's figures are not this reference's: write the measured ones into it"


def test_scale_volume_is_the_census_volume_of_the_padded_scale(oracle):
    """the box ends up centred on the pixel: with equal frames the centre class costs nothing, and one cell by hand"""
    c = cp.BY_NO[8]
    f0, f1 = cp.frames(c)
    k, a, mh, mw = c.k, c.a, c.mh, c.mw
    v = cp.scale_volume(f0, f0, 1, k, mh, mw, a, 1.0)
    assert v.shape == (c.H, c.W, mh, mw) and v.dtype == np.float32
    assert not v[:, :, (mh - 1) // 2, (mw - 1) // 2].any()
    hp, wp = mh - 1 + k - 1 + a - 1, mw - 1 + k - 1 + a - 1
    pad = lambda f: np.pad(f, ((0, 0), (hp // 2, hp - hp // 2), (wp // 2, wp - wp // 2)))
    S0, S1 = signature(pad(f0), k, k), signature(pad(f1), k, k)
    v = cp.scale_volume(f0, f1, 1, k, mh, mw, a, 0.125)
    y, x, dy, dx = 7, 11, 4, 1
    by_hand = sum(bin(int(S0[ch, y + (mh - 1) // 2 + u, x + (mw - 1) // 2 + w]) ^ int(S1[ch, y + dy + u, x + dx + w])).count("1")
                  for ch in range(c.C) for u in range(a) for w in range(a))
    assert v[y, x, dy, dx] == np.float32(by_hand) * np.float32(0.125)
    assert np.array_equal(v, cost_volume(S0, S1, mh, mw, a).astype(np.float32) * np.float32(0.125))


@functools.lru_cache(maxsize=None)
def scene_shares(seed, move, tol):
    census, ssd = cp.scene_census(seed, move), cp.scene_ssd(seed, move)
    return cp.share_wrong(census["y"], census["x"], move, tol), cp.share_wrong(ssd["y"], ssd["x"], move, tol)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("move,tol", cp.MOVES, ids=lambda v: str(v).replace(" ", ""))
def test_scene_figures(seed, move, tol, oracle):
    """measured, seeds 1 - 3: census wrong on 0 % at (2, -3) and (5, -6) and on 0.23 - 1.92 % at (9, -11); the SSD oracle chain on
    24.4 - 33.7 %, 71.6 - 74.6 % and 100 %"""
    census, ssd = scene_shares(seed, move, tol)
    print("seed %d move %s tolerance %d px: census wrong share %.4f, SSD oracle chain %.4f" % (seed, move, tol, census, ssd))
    assert census <= 0.05
    assert ssd >= 0.20
