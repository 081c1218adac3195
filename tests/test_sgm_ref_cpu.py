"""The numpy restatement of semi-global aggregation (tests/sgm_ref.py; include/dfe.h: dfe_sgm_aggregate_f32) against
what its definition implies -- the sum's order, the mirror symmetries of single paths, the ring's shift invariance -- and the quality scene:
what the aggregation buys over winner-takes-all.  No device."""
import numpy as np
import pytest

from tests.sgm_ref import SCENE, off_by_more_than_one, quality_scene, sgm_aggregate, sgm_path

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _volume(H, W, D, seed):
    return np.random.default_rng(seed).uniform(-3, 9, size=(H, W, D)).astype(F)


@pytest.mark.parametrize("ring", [0, 5, 11])
def test_zero_penalties_leave_the_sum_of_the_costs_in_the_definitions_order(ring):
    # P1 = P2 = 0: t = m for every label, so L_r = C + 0 = C, and agg is C added to itself in the chain's association
    C = _volume(9, 11, 7, 0)
    agg, flow = sgm_aggregate(C, 0.0, 0.0, 0x0f, ring)
    assert np.array_equal(_bits(agg), _bits(((C + C) + C) + C))
    agg8, _ = sgm_aggregate(C, 0.0, 0.0, 0xff, ring)
    want = C
    for _ in range(7):
        want = (want + C).astype(F)
    assert np.array_equal(_bits(agg8), _bits(want))
    assert np.array_equal(flow, np.argmin(agg, axis=-1).astype(F))


@pytest.mark.parametrize("ring", [0, 4, 10])
def test_a_single_path_on_a_flipped_volume_is_the_flipped_mirror_path(ring):
    C = _volume(8, 10, 6, 1)
    flip_x = {0: 1, 1: 0, 2: 2, 3: 3, 4: 6, 6: 4, 5: 7, 7: 5}      # (dy, dx) -> (dy, -dx)
    flip_y = {0: 0, 1: 1, 2: 3, 3: 2, 4: 7, 7: 4, 5: 6, 6: 5}      # (dy, dx) -> (-dy, dx)
    for r in range(8):
        a = sgm_path(C[:, ::-1], r, 1.5, 6.0, ring)
        assert np.array_equal(_bits(a), _bits(sgm_path(C, flip_x[r], 1.5, 6.0, ring)[:, ::-1])), "x, path %d" % r
        a = sgm_path(C[::-1], r, 1.5, 6.0, ring)
        assert np.array_equal(_bits(a), _bits(sgm_path(C, flip_y[r], 1.5, 6.0, ring)[::-1])), "y, path %d" % r


def test_on_a_full_ring_the_vertical_paths_move_with_the_columns():
    C = _volume(7, 12, 5, 2)
    for k in (1, 5, 11):
        for r in (2, 3, 4, 5, 6, 7):     # the diagonals too: with the columns a ring nothing marks a column
            assert np.array_equal(_bits(sgm_path(np.roll(C, k, axis=1), r, 0.5, 4.0, 12)), _bits(np.roll(sgm_path(C, r, 0.5, 4.0, 12), k, axis=1))), (k, r)


def test_a_path_starts_where_its_predecessor_is_outside_and_penalises_label_changes():
    # two pixels in a row, D = 3: L_0 of the second pixel by hand
    C = np.array([[[5, 1, 7], [2, 9, 0]]], F)
    L = sgm_path(C, 0, 1.0, 3.0)
    assert np.array_equal(L[0, 0], C[0, 0])
    # m = 1; t = min(5, 1 + 1, inf, 4) = 2 | min(1, 5 + 1, 7 + 1, 4) = 1 | min(7, 1 + 1, inf, 4) = 2
    assert np.array_equal(L[0, 1], np.array([2 + 1, 9 + 0, 0 + 1], F))
    # ring = 1: column 1 is the warm-up column, column 0 follows it, then column 1 follows column 0 again
    R = sgm_path(C, 0, 1.0, 3.0, ring=1)
    l0 = np.array([5 + 2, 1 + 1, 7 + 0], F)      # from (2, 9, 0): m = 0; t = min(2, inf, 9+1, 3) = 2 | min(9, 3, 1, 3) = 1 | min(0, 10, inf, 3) = 0
    assert np.array_equal(R[0, 0], l0)
    m = l0.min()
    t = np.minimum(np.minimum(np.minimum(l0, np.array([np.inf, l0[0] + 1, l0[1] + 1], F)), np.array([l0[1] + 1, l0[2] + 1, np.inf], F)), m + 3)
    assert np.array_equal(R[0, 1], C[0, 1] + (t - m))


@pytest.mark.parametrize("seed", SCENE["seeds"])
def test_aggregation_at_least_halves_the_pixels_off_by_more_than_one(seed):
    vol, truth = quality_scene(seed)
    wta = off_by_more_than_one(np.argmin(vol, axis=-1).astype(F), truth)
    assert wta > 0.1, "the scene must be hard for winner-takes-all (%.3f)" % wta
    for paths in (0x0f, 0xff):
        _, flow = sgm_aggregate(vol, SCENE["P1"], SCENE["P2"], paths, SCENE["ring"])
        got = off_by_more_than_one(flow, truth)
        print("seed %d paths 0x%02x: winner-takes-all %.4f, aggregated %.4f" % (seed, paths, wta, got))
        assert got <= 0.5 * wta, "seed %d paths 0x%02x: %.4f against winner-takes-all's %.4f" % (seed, paths, got, wta)
