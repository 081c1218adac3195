"""The int8 flow sweep's window masks live in the MFMA accumulators (csrc/ssd_flow_i8.hip: a candidate outside 0 <= q - n <= 32 starts its dot
product from a penalty, and nothing selects afterwards) and its key has a 7-bit order field with four running keys per lane.  Against the
float sweep (cv_i8 = 0) bit for bit on all ten outputs of both entry points, every case as two-row items alone (i8_slots = 1) and as
one-row items alone (4096): a perfect match just outside the window, which a leaking mask would take; the minimum on the window's own edge
columns, the diagonal cells of the first and third tile; ties across tiles, where the first index must win; and the flat block whose
fall-back sweep decodes the plane a second time."""
import numpy as np
import pytest

from tests.test_gpu_flow_i8 import PAD, _float_ref, _pair, _run, _same

SHAPES = [(2, 16), (3, 16), (4, 33), (9, 48)]   # (3, 16): the shifted last pair; (4, 33): a strip one pixel wide; (9, 48): both
SLOTS = [1, 4096]                               # two-row items alone, one-row items alone
DYS = [0, 16, 32]


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


def _shifted(big, Ho, Wo, dy, dx, m):
    """frame 1 = big at offset (m, m), frame 0 the same field displaced so that frame 0's patch at (y + 16, x + 16) is frame 1's at
    (y + dy, x + dx) wherever that lies in the frame -- no wrap-around"""
    H, W = Ho + PAD, Wo + PAD
    f1 = big[:, m : m + H, m : m + W]
    f0 = big[:, m - 16 + dy : m - 16 + dy + H, m - 16 + dx : m - 16 + dx + W]
    return np.ascontiguousarray(f0), np.ascontiguousarray(f1), (W / 2, H / 2)


def _random_field(Ho, Wo, m, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, Ho + PAD + 2 * m, Wo + PAD + 2 * m)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("dy", DYS)
@pytest.mark.parametrize("dx", [-1, -15, 33, 47])
@pytest.mark.parametrize("Ho,Wo", SHAPES)
def test_perfect_match_just_outside_the_window_is_not_taken(dfe, cuda, Ho, Wo, dx, dy, slots):
    """the cost-0 candidate sits in a masked cell of the first (dx < 0) or third (dx > 32) tile, in the first, the centre and the last
    displacement row"""
    f0, f1, foe = _shifted(_random_field(Ho, Wo, 48, seed=51), Ho, Wo, dy, dx, 48)
    new = _check_slots(dfe, cuda, ("wm-outside", Ho, Wo, dy, dx), f0, f1, foe, 0.21, slots)
    assert (new["best"] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("dy", DYS)
@pytest.mark.parametrize("dx", [0, 32])
@pytest.mark.parametrize("Ho,Wo", SHAPES)
def test_minimum_on_the_windows_edge_columns_is_kept(dfe, cuda, Ho, Wo, dx, dy, slots):
    """q = n (first tile) and q = n + 32 (third tile): the diagonal cells, valid in both masks"""
    f0, f1, foe = _shifted(_random_field(Ho, Wo, 48, seed=53), Ho, Wo, dy, dx, 48)
    new = _check_slots(dfe, cuda, ("wm-edge", Ho, Wo, dy, dx), f0, f1, foe, 0.21, slots)
    assert (new["best"] == 0).all() and (new["idx"] == dy * 33 + dx + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("period,dy,dx", [(8, 5, 3), (8, 0, 0), (8, 32, 7), (2, 21, 1)])
@pytest.mark.parametrize("Ho,Wo", SHAPES)
def test_ties_across_tiles_first_index_wins(dfe, cuda, Ho, Wo, period, dy, dx, slots):
    """a texture of period `period` in x and none in y, displaced off the centre row: cost 0 at dx, dx + period, ... of displacement row
    dy alone -- in all three tiles, in several lane groups and, with period 2, in two of a lane's four running keys"""
    m = 48
    rows = Ho + PAD + 2 * m
    cell = np.random.default_rng(57).integers(0, 256, (3, rows, period)).astype(np.float32)
    big = np.tile(cell, (1, 1, (Wo + PAD + 2 * m) // period + 1))
    f0, f1, foe = _shifted(big, Ho, Wo, dy, dx, m)
    new = _check_slots(dfe, cuda, ("wm-ties", Ho, Wo, period, dy, dx), f0, f1, foe, 0.21, slots)
    assert (new["best"] == 0).all() and (new["idx"] == dy * 33 + dx + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
def test_flat_block_fallback_decodes_the_plane(dfe, cuda, slots):
    """as tests/test_gpu_flow_i8_shared_rows.py builds it: the second sweep forms its costs from the same plane cells, without the penalty"""
    f0, f1, foe = _pair(82, 122)
    f0, f1 = f0.copy(), f1.copy()
    v = f1[:, 20, 20].copy()
    f0[:, 30:90, 40:100] = v[:, None, None]
    f1[:, 30:90, 40:100] = v[:, None, None]
    new = _check_slots(dfe, cuda, "wm-flat", f0, f1, foe, 0.21, slots)
    assert (new["scores2"][30:52, 40:62] == -7).all() and new["scores2"][60, 50] > 0
