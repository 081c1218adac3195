"""The int8 flow sweep's two-row step shares the products of six image rows between the two output rows of an item (csrc/ssd_flow_i8.hip:
C, carried from step s - 1 to step s; row y0 adds its patch row 0, row y0 + 1 its patch row 6).  Against the float sweep (cv_i8 = 0) bit for
bit on all ten outputs of both entry points, every case as two-row items alone (i8_slots = 1) and as one-row items alone (4096), on frames
that put the minimum on the steps where the second row's result is absent, first present, last fed by a fresh C and alone, and on pairs
that differ in ONE frame-1 image row, so that a single patch row of a single output row carries the whole cost."""
import numpy as np
import pytest

from tests.test_gpu_flow_i8 import PAD, _float_ref, _pair, _run, _same, _texture

SHAPES = [(2, 16), (3, 16), (4, 33), (9, 48)]   # (3, 16): the shifted last pair; (4, 33): a strip one pixel wide; (9, 48): both
SLOTS = [1, 4096]                               # two-row items alone, one-row items alone


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


def _rolled(Ho, Wo, dy, dx, seed):
    """frame 0's patch at (y + 16, x + 16) is frame 1's at (y + dy, x + dx): the one candidate of cost 0"""
    H, W = Ho + PAD, Wo + PAD
    f1 = np.random.default_rng(seed).integers(0, 256, (3, H, W)).astype(np.float32)
    return np.ascontiguousarray(np.roll(f1, (16 - dy, 16 - dx), axis=(1, 2))), f1, (W / 2, H / 2)


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("dy", [0, 1, 31, 32])
@pytest.mark.parametrize("Ho,Wo", SHAPES)
def test_unique_minimum_at_the_edge_steps(dfe, cuda, Ho, Wo, dy, slots):
    """row y0 + 1 meets displacement row dy at step dy + 1: step 1 is its first, step 32 the last that forms a C, step 33 its own"""
    f0, f1, foe = _rolled(Ho, Wo, dy, 7, seed=31)
    new = _check_slots(dfe, cuda, ("shared-edge", Ho, Wo, dy), f0, f1, foe, 0.21, slots)
    assert (new["best"] == 0).all() and (new["idx"] == dy * 33 + 7 + 1).all()


def _targets():
    """(Ho, Wo, output row): rows 0 and 1 (the first item's two rows) and the last row (the second row of the last, or shifted last, pair)"""
    return [(Ho, Wo, y) for Ho, Wo in SHAPES for y in sorted({0, 1, Ho - 1})]


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("dy", [0, 13, 32])
@pytest.mark.parametrize("p", [0, 6])
@pytest.mark.parametrize("Ho,Wo,y", _targets())
def test_one_changed_frame1_row_on_one_patch_row(dfe, cuda, Ho, Wo, y, p, dy, slots):
    """The pair of _rolled, cost 0 at displacement row dy, with frame-1 image row y + dy + p replaced: at output row y that row is patch
    row p of the candidates of displacement row dy and of no other patch row there, so the minimum's cost is that patch row's alone (21
    taps against 126 unchanged ones elsewhere: it stays the minimum).  A wrong operand for the row's own patch row (0 or 6), or a C from
    the wrong step, changes it."""
    f0, f1, foe = _rolled(Ho, Wo, dy, 7, seed=37)
    f1 = f1.copy()
    f1[:, y + dy + p, :] = np.random.default_rng(43).integers(0, 256, (3, f1.shape[2])).astype(np.float32)
    new = _check_slots(dfe, cuda, ("shared-one-row", Ho, Wo, y, p, dy), f0, f1, foe, 0.21, slots)
    assert (new["best"][y] > 0).all() and (new["idx"][y] == dy * 33 + 7 + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("Ho,Wo", SHAPES)
def test_identical_frames_centre_and_lead_cells(dfe, cuda, Ho, Wo, slots):
    """a periodic texture against itself: cost 0 at many candidates, so the centre override decides, in both rows of an item (steps 16 and
    17); the lead cells (steps 0 and 1) go into `scores`"""
    H, W = Ho + PAD, Wo + PAD
    t = _texture(H, W)
    new = _check_slots(dfe, cuda, ("shared-same", Ho, Wo), t, t.copy(), (W / 2, H / 2), 0.21, slots)
    assert (new["best"] == 0).all() and (new["idx"] == 16 * 33 + 16 + 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
def test_flat_block_fallback_follows_a_two_row_item(dfe, cuda, slots):
    f0, f1, foe = _pair(82, 122)
    f0, f1 = f0.copy(), f1.copy()
    v = f1[:, 20, 20].copy()
    f0[:, 30:90, 40:100] = v[:, None, None]
    f1[:, 30:90, 40:100] = v[:, None, None]
    new = _check_slots(dfe, cuda, "shared-flat", f0, f1, foe, 0.21, slots)
    assert (new["scores2"][30:52, 40:62] == -7).all() and new["scores2"][60, 50] > 0   # (as tests/test_gpu_flow_i8.py derives it)
