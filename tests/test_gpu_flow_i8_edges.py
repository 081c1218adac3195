"""The int8 flow sweep (csrc/ssd_flow_i8.hip) at the places its loop structure singles out, against the float sweep (cv_i8 = 0) bit for bit on
all ten outputs of both entry points: the two diagonals of the lane masks (dx = -16 and +16) and the columns one outside them, the first,
centre and last displacement rows (the peeled steps of one-row and two-row items, the shifted last pair of an odd height), the centre cell
tied with an earlier minimum, and the pack kernel's tiles (whole tiles, one row or column into the next, and the gate at a tile's last pixel,
at the next tile's first and at one that a tile reads only as its neighbour's halo)."""
import numpy as np
import pytest

from tests.test_gpu_flow_i8 import PAD, _check, _float_ref, _pair, _run, _same

CENTRE = 16 * 33 + 16 + 1
ONE_ROW_ITEMS = 1 << 20   # i8_slots so large that no round of two-row items is full: one-row items alone


def _random(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, H, W)).astype(np.float32)


def _shifted(f1, dy, dx):
    """frame 0 whose patch at (y + 16, x + 16) is frame 1's at (y + dy, x + dx): window cell (dy, dx), index dy * 33 + dx + 1"""
    return np.ascontiguousarray(np.roll(f1, (16 - dy, 16 - dx), axis=(1, 2)))


def _check_slots(dfe, cuda, key, f0, f1, foe, thr, slots):
    if slots is None:
        return _check(dfe, cuda, key, f0, f1, foe, thr)
    ctx = dfe.get_ctx(0)
    ref = _float_ref(dfe, cuda, key, f0, f1, foe, thr)
    ctx.set_option("i8_slots", slots)
    try:
        new, tp, tf = _run(dfe, cuda, f0, f1, foe, thr, 1)
    finally:
        ctx.set_option("i8_slots", None)
    assert tp and tf
    _same(new, ref)
    return new


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", [(3, 48), (1, 16)])
@pytest.mark.parametrize("dx", [0, 32], ids=["dx-16", "dx+16"])
def test_minimum_on_the_mask_diagonals(dfe, cuda, Ho, Wo, dx):
    """dx = -16 is candidate q = n of the first tile, dx = +16 is q = n + 32 of the third: lane m = n, the last one each mask keeps"""
    H, W = Ho + PAD, Wo + PAD
    f1 = _random(H, W, 31)
    new = _check(dfe, cuda, ("edge-x", Ho, Wo, dx), _shifted(f1, 16, dx), f1, (W / 2, H / 2), 0.21)
    assert (new["best"] == 0).all() and (new["idx"] == 16 * 33 + dx + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", [(3, 48), (1, 16)])
@pytest.mark.parametrize("dx", [-1, 33], ids=["dx-17", "dx+17"])
def test_match_one_column_outside_the_window_is_dropped(dfe, cuda, Ho, Wo, dx):
    """the zero-cost match lies at q = n - 1 (first tile) or q = n + 33 (third tile): computed by the MFMA, dropped by the masks"""
    H, W = Ho + PAD, Wo + PAD
    f1 = _random(H, W, 31)
    new = _check(dfe, cuda, ("edge-x", Ho, Wo, dx), _shifted(f1, 16, dx), f1, (W / 2, H / 2), 0.21)
    assert (new["best"] > 0).all()
    assert (new["idx"] >= 1).all() and (new["idx"] <= 33 * 33).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [None, 1, ONE_ROW_ITEMS], ids=["auto", "two-row", "one-row"])
@pytest.mark.parametrize("Ho", [1, 2, 3])
@pytest.mark.parametrize("dy", [0, 16, 32], ids=["dy-16", "dy0", "dy+16"])
def test_minimum_in_the_first_centre_and_last_displacement_row(dfe, cuda, dy, Ho, slots):
    """the displacement rows of the peeled steps: 0 (the lead cells' step; in a two-row item the second row's comes one step later), 16 (the
    centre cell's) and 32 (the step past the last whole round; in a two-row item the first row has left the window in the step after it)"""
    Wo = 24
    H, W = Ho + PAD, Wo + PAD
    f1 = _random(H, W, 37)
    new = _check_slots(dfe, cuda, ("edge-y", Ho, dy), _shifted(f1, dy, 16), f1, (W / 2, H / 2), 0.21, slots)
    assert (new["best"] == 0).all() and (new["idx"] == dy * 33 + 16 + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_centre_cell_tied_with_an_earlier_minimum(dfe, cuda, thr):
    """rows of period 5, columns random, both frames the same: cost 0 in the centre column of the displacement rows 1, 6, 11, 16 (the centre), 21, ...;
    the centre wins against the earlier rows 1, 6, 11, and the lead cells (displacement row 0) all cost more than the threshold"""
    Ho, Wo = 5, 40
    H, W = Ho + PAD, Wo + PAD
    rows = _random(5, W, 41)
    f = np.ascontiguousarray(rows[:, np.arange(H) % 5, :])
    new = _check(dfe, cuda, ("tie-centre-rows", thr), f, f.copy(), (W / 2, H / 2), thr)
    assert (new["best"] == 0).all() and (new["idx"] == CENTRE).all()
    assert (new["scores2"] > 0).mean() > 0.5


# the pack kernel's tiles are 32 x 32 (kPackW, kPackH); until the loads were issued ahead of their use they were 64 x 16
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(48, 64), (49, 65), (48, 65), (64, 64), (65, 65), (65, 64)])
def test_pack_tiles_whole_and_one_into_the_next(dfe, cuda, H, W):
    f0, f1, foe = _pair(H - PAD, W - PAD, seed=13)
    assert f0.shape == (3, H, W)
    new = _check(dfe, cuda, ("pack", H, W), f0, f1, foe, 0.21)
    assert (new["scores2"] > 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("frame,ch", [(0, 0), (1, 2)])
@pytest.mark.parametrize("y,x", [(31, 31), (32, 32), (37, 37), (15, 63), (16, 64), (21, 64)],
                         ids=["last-of-32x32", "first-of-next-32x32", "halo-of-32x32", "last-of-64x16", "first-of-next-64x16", "halo-of-64x16"])
def test_gate_at_the_tile_borders(dfe, cuda, y, x, frame, ch):
    """one 100.5 at a tile's last row and column, at the first pixel of the tile diagonally after it, and at the last pixel that the first
    tile reads only as its halo (six rows and columns into the neighbour), for the tiling shipped and for the one before it"""
    H, W = 65, 65
    f0, f1, foe = _pair(H - PAD, W - PAD, seed=13)
    g = [f0.copy(), f1.copy()]
    g[frame][ch, y, x] = 100.5
    _check(dfe, cuda, ("pack-gate", y, x, frame, ch), g[0], g[1], foe, 0.21, expect_i8=False)
    # the untouched pair on the same context: no stale verdict
    _check(dfe, cuda, ("pack", H, W), f0, f1, foe, 0.21, expect_i8=True)
