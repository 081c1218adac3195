"""The int8 flow sweep reads the S1 key plane through a per-wave ring of four plane rows in LDS (csrc/ssd_flow_i8.hip: slot s & 3 holds plane
row y0 + s, refilled with row y0 + s + 4 behind the step's reads).  Against the float sweep of the same entry (cv_i8 = 0), bit for bit on
every output (flow, scores, depth, confidence and the flow call's six), on random byte-valued frames: every cost of a displacement row
carries that row's plane cells, so a slot mix-up, a row staged too late or a refill too early changes the costs of a whole row.

Every frame here is Ho + 38 rows high, so the last output row is the frame's last possible one: the last plane row a sweep consumes
(y0 + 32 of a one-row item, y0 + 33 of a two-row item) is row H - 7 of a plane of H + 1 rows, and a prefetch that ran further would fetch
rows the step never needs.  i8_slots = 1 makes two-row items alone, 4096 one-row items alone (tests/test_gpu_flow_i8_shared_rows.py);
Ho = 9, Wo = 40 with i8_slots = 6 is flow_i8_item_plan's mixed plan: 15 two-row items in whole rounds of 6 are 12, the rows behind them
(strip 2, rows 4..8) five one-row items, so the boundary lies inside a strip and 17 items fill five blocks of four waves."""
import numpy as np
import pytest

from tests.test_gpu_flow_i8 import K, PAD, _float_ref, _run, _same

THR = 0.21


def _random_pair(Ho, Wo, seed=101):
    H, W = Ho + PAD, Wo + PAD
    rng = np.random.default_rng(seed)
    f0 = rng.integers(0, 256, (3, H, W)).astype(np.float32)
    f1 = rng.integers(0, 256, (3, H, W)).astype(np.float32)
    return f0, f1, (W / 2, H / 2)


def _check_slots(dfe, cuda, key, f0, f1, foe, thr, slots, expect_i8=True):
    ctx = dfe.get_ctx(0)
    ref = _float_ref(dfe, cuda, key, f0, f1, foe, thr)
    ctx.set_option("i8_slots", slots)
    try:
        new, tp, tf = _run(dfe, cuda, f0, f1, foe, thr, 1)
    finally:
        ctx.set_option("i8_slots", None)
    if expect_i8:
        assert tp and tf   # dfe_flow_last_path: the int8 kernel did the step
    _same(new, ref)
    return new


# Ho = 1: the one-row kernel; 2: one two-row item, all 34 steps and the steps past the last prefetch; 3: the shifted last pair.
# Wo = 8: less than a strip (handled or declined: equal both ways); 16: a full strip; 17: a second strip one pixel wide, whose staged cells
# reach x0 + 63 and whose reads reach x0 + 47; 40: three strips
def _shape_cases():
    out = []
    for Ho in (1, 2, 3):
        for Wo in (8, 16, 17, 40):
            for slots in ((4096,) if Ho == 1 else (1, 4096)):
                out.append((Ho, Wo, slots))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo,slots", _shape_cases())
def test_ring_on_random_bytes_at_the_strip_and_row_edges(dfe, cuda, Ho, Wo, slots):
    f0, f1, foe = _random_pair(Ho, Wo)
    new = _check_slots(dfe, cuda, ("ring", Ho, Wo, THR), f0, f1, foe, THR, slots, expect_i8=Wo != 8)
    assert (new["best"] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [1, 6, 4096])
def test_ring_of_every_wave_and_block_is_its_own(dfe, cuda, slots):
    """Ho = 9, Wo = 40: 15 two-row items (slots = 1), 27 one-row items (4096), or 12 + 5 with the boundary inside strip 2 (6): several
    waves of a block and several blocks, each wave with a ring of its own"""
    f0, f1, foe = _random_pair(9, 40, seed=103)
    new = _check_slots(dfe, cuda, ("ring", 9, 40, THR), f0, f1, foe, THR, slots)
    assert (new["best"] > 0).all()


def _lead_hits(f0, f1, thr):
    """per output pixel, how many of the eight lead cells (displacement row 0, dx = 0..7) cost more than thr"""
    H, W = f0.shape[1:]
    Ho, Wo = H - PAD, W - PAD
    n = np.zeros((Ho, Wo), np.int64)
    for y in range(Ho):
        for x in range(Wo):
            a = f0[:, y + 16 : y + 16 + K, x + 16 : x + 16 + K].astype(np.int64)
            for dx in range(8):
                b = f1[:, y : y + K, x + dx : x + dx + K].astype(np.int64)
                n[y, x] += int(((a - b) ** 2).sum()) > thr
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo,slots", [(3, 17, 1), (3, 17, 4096), (9, 40, 6)])
def test_fallback_sweep_between_uses_of_the_ring(dfe, cuda, Ho, Wo, slots):
    """A threshold at the costs' mean (147 taps of mean 2 (256^2 - 1) / 12 = 1.6e6; M = 4 above 0.2): a fifth of the pixels and more have fewer than
    four lead cells above it (counted below) and take the fall-back sweep, which keeps its global loads, inside the wave that has just swept through its
    ring and, in a two-row item, before the finalize of the second row"""
    thr = 1.6e6
    f0, f1, foe = _random_pair(Ho, Wo, seed=107)
    hits = _lead_hits(f0, f1, thr)
    assert (hits < 4).any() and (hits >= 4).any()   # flagged pixels and others, whatever the split
    for y in range(0, Ho - 1, 2):
        assert (hits[y : y + 2] < 4).any()          # in every row pair
    _check_slots(dfe, cuda, ("ring-fb", Ho, Wo, thr), f0, f1, foe, thr, slots)


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,slots", [(1, 4096), (2, 1), (2, 4096), (3, 1), (3, 4096)])
def test_minimum_on_the_last_plane_row_of_the_frame(dfe, cuda, Ho, slots):
    """frame 0's patch at (y + 16, x + 16) is frame 1's at (y + 32, x + 7): the one candidate of cost 0 lies in displacement row 32, whose
    plane row for the last output row is the last one any step reads, the last that is staged"""
    H, W = Ho + PAD, 17 + PAD
    f1 = np.random.default_rng(109).integers(0, 256, (3, H, W)).astype(np.float32)
    f0 = np.ascontiguousarray(np.roll(f1, (16 - 32, 16 - 7), axis=(1, 2)))
    new = _check_slots(dfe, cuda, ("ring-last", Ho), f0, f1, (W / 2, H / 2), THR, slots)
    assert (new["best"] == 0).all() and (new["idx"] == 32 * 33 + 7 + 1).all()
