"""The int8 flow sweep's wave items (csrc/flow_i8_items.h: two-row items, then one-row items) and its absolute tie-break term, against the
float sweep (cv_i8 = 0) bit for bit on all ten outputs of both entry points.  Option "i8_slots" stands in for the number of waves the device
holds at once, so that at small shapes the boundary between the two kinds of item falls at a strip's first row, inside a strip, on the last
strip and on the odd last row, and so that every shape also runs as two-row items alone (i8_slots = 1) and as one-row items alone."""
import numpy as np
import pytest

from tests.test_gpu_flow_i8 import PAD, _float_ref, _pair, _run, _same, _texture

ONE_ROW_COST = 0.6   # kI8OneRowCost


def _plan(Ho, nstrips, slots):
    """flow_i8_item_plan: (two-row items, first row of the one-row items as (strip, row), one-row items)"""
    nrp = (Ho + 1) // 2
    total2, rows = nstrips * nrp, nstrips * Ho
    full = total2 // slots * slots
    r0 = full // nrp * Ho + 2 * (full % nrp)
    n1 = rows - r0
    if Ho >= 2 and n1 > 0 and full // slots + ONE_ROW_COST * -(-n1 // slots) < -(-total2 // slots):
        return full, divmod(r0, Ho), n1
    return (0, (0, 0), rows) if Ho < 2 else (total2, None, 0)


def _check_slots(dfe, cuda, key, f0, f1, foe, thr, slots):
    ctx = dfe.get_ctx(0)
    ref = _float_ref(dfe, cuda, key, f0, f1, foe, thr)
    ctx.set_option("i8_slots", slots)
    try:
        new, tp, tf = _run(dfe, cuda, f0, f1, foe, thr, 1)
    finally:
        ctx.set_option("i8_slots", None)
    assert tp and tf   # dfe_flow_last_path: the int8 kernel did the step
    _same(new, ref)
    return new


# (Ho, Wo, i8_slots) -> where the one-row items begin: (two-row items, (strip, row), one-row items)
BOUNDARIES = {
    (2, 16, 1): (1, None, 0),           # two-row items alone
    (2, 16, 4): (0, (0, 0), 2),         # one-row items alone: the boundary at the first strip's first row
    (3, 16, 1): (2, None, 0),           # ... with the shifted last pair
    (3, 16, 4): (0, (0, 0), 3),
    (4, 33, 1): (6, None, 0),
    (4, 33, 4): (4, (2, 0), 4),         # at the last strip's first row
    (4, 33, 5): (5, (2, 2), 2),         # inside the last strip
    (7, 40, 1): (12, None, 0),
    (7, 40, 5): (10, (2, 4), 3),        # inside a strip, the odd last row among the one-row items
    (7, 40, 8): (8, (2, 0), 7),
    (7, 40, 11): (11, (2, 6), 1),       # the odd last row alone: a one-row item in place of the shifted pair
    (7, 40, 7): (12, None, 0),          # (eight rows left for seven slots: two rounds of one-row items would be slower; two-row items kept)
    (11, 17, 1): (12, None, 0),
    (11, 17, 5): (10, (1, 8), 3),
    (11, 17, 8): (8, (1, 4), 7),        # inside the last strip, which is one pixel wide
    (11, 17, 11): (11, (1, 10), 1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo,slots", sorted(BOUNDARIES))
def test_mixed_items_equal_the_float_sweep(dfe, cuda, Ho, Wo, slots):
    assert _plan(Ho, -(-Wo // 16), slots) == BOUNDARIES[(Ho, Wo, slots)]
    f0, f1, foe = _pair(Ho, Wo, seed=9)
    new = _check_slots(dfe, cuda, ("sched", Ho, Wo), f0, f1, foe, 0.21, slots)
    assert (new["idx"] >= 1).all() and (new["idx"] <= 33 * 33).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [1, 40, 4096])
def test_ties_over_fifty_rows(dfe, cuda, slots):
    """the plane's order term falls by 6 per row: over 50 output rows + 32 displacement rows it spans more than 256, the weight of one unit of
    cost, between the first and the last row; the first minimum in index order must still win in every row"""
    Ho, Wo = 50, 24
    assert _plan(Ho, 2, slots) == {1: (50, None, 0), 40: (40, (1, 30), 20), 4096: (0, (0, 0), 100)}[slots]
    assert 6 * (Ho - 1 + 32) > 256
    H, W = Ho + PAD, Wo + PAD
    t = _texture(H, W)
    f0 = np.ascontiguousarray(np.roll(t, (3, -5), axis=(1, 2)))
    new = _check_slots(dfe, cuda, "sched-ties", f0, t, (W / 2, H / 2), 0.21, slots)
    assert (new["best"] == 0).all() and (new["idx"] == 1 * 33 + 5 + 1).all()   # (as tests/test_gpu_flow_i8.py derives it)


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [1, 4096])
@pytest.mark.parametrize("dy,dx", [(0, 0), (0, 32), (32, 0), (32, 32)])
def test_unique_minimum_at_the_band_corners(dfe, cuda, dy, dx, slots):
    """dx = 0 is candidate q = n of the first tile (lane m = n, the mask's diagonal), dx = 32 is q = n + 32 of the third tile (again m = n)"""
    Ho, Wo = 9, 48
    H, W = Ho + PAD, Wo + PAD
    f1 = np.random.default_rng(23).integers(0, 256, (3, H, W)).astype(np.float32)
    f0 = np.ascontiguousarray(np.roll(f1, (16 - dy, 16 - dx), axis=(1, 2)))   # frame 0's patch at (y + 16, x + 16) is frame 1's at (y + dy, x + dx)
    new = _check_slots(dfe, cuda, ("sched-corner", dy, dx), f0, f1, (W / 2, H / 2), 0.21, slots)
    assert (new["best"] == 0).all() and (new["idx"] == dy * 33 + dx + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [1, 250, 4096])
def test_flat_block_fallback_inside_one_row_items(dfe, cuda, slots):
    assert _plan(82, 8, slots) == {1: (328, None, 0), 250: (250, (6, 8), 156), 4096: (0, (0, 0), 656)}[slots]
    f0, f1, foe = _pair(82, 122)
    f0, f1 = f0.copy(), f1.copy()
    v = f1[:, 20, 20].copy()
    f0[:, 30:90, 40:100] = v[:, None, None]
    f1[:, 30:90, 40:100] = v[:, None, None]
    new = _check_slots(dfe, cuda, "sched-flat", f0, f1, foe, 0.21, slots)
    assert (new["scores2"][30:52, 40:62] == -7).all() and new["scores2"][60, 50] > 0   # (as tests/test_gpu_flow_i8.py derives it)
