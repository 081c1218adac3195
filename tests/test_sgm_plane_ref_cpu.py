"""The numpy restatement of the aggregation on a two-dimensional label plane (tests/sgm_plane_ref.py) against what
the definition implies on its own: no penalty and a single label leave the volume as it is, a window of one row or one column is the
one-dimensional rule of tests/sgm_ref.py bit for bit, a case computed by hand, ties; and the quality conditions of the band scene, on
the reference alone."""
import numpy as np
import pytest

from tests import census_ref as cr
from tests import sgm_plane_ref as pr
from tests import sgm_ref

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _volume(shape, seed):
    return np.random.default_rng(seed).uniform(-3, 9, size=shape).astype(F)


@pytest.mark.parametrize("r", range(8))
def test_no_penalty_and_a_single_label_leave_the_volume(r):
    vol = _volume((5, 7, 3, 4), r)
    assert np.array_equal(_bits(pr.plane_path(vol, r, 0.0, 0.0)), _bits(vol))          # t = m, so L = C + (m - m)
    one = _volume((6, 5, 1, 1), 10 + r)
    assert np.array_equal(_bits(pr.plane_path(one, r, 0.5, 4.0)), _bits(one))


@pytest.mark.parametrize("r", range(8))
def test_a_window_of_one_row_or_one_column_is_the_one_dimensional_rule(r):
    vol = _volume((9, 11, 7), 20 + r)
    for P1, P2 in ((0.5, 4.0), (2.0, 16.0), (3.0, 3.0)):
        want = sgm_ref.sgm_path(vol, r, P1, P2, ring=0)
        assert np.array_equal(_bits(pr.plane_path(vol[:, :, None, :], r, P1, P2)[:, :, 0, :]), _bits(want)), "1 x 7"
        assert np.array_equal(_bits(pr.plane_path(vol[:, :, :, None], r, P1, P2)[:, :, :, 0]), _bits(want)), "7 x 1"


def test_a_case_computed_by_hand():
    # 1 x 3 pixels, 1 x 3 labels, P1 = 1, P2 = 3
    vol = np.array([[[1, 5, 2], [4, 0, 6], [3, 3, 0]]], F)[:, :, None, :]
    # direction 0: x = 0 starts; x = 1: m = 1, t = (min(1, 5+1, 1+3), min(5, 1+1, 2+1, 4), min(2, 5+1, 4)) = (1, 2, 2), L = C + t - 1;
    # x = 2: m = 1, t = (min(4, 1+1, 4), min(1, 4+1, 7+1, 4), min(7, 1+1, 4)) = (2, 1, 2)
    L0 = np.array([[[1, 5, 2], [4, 1, 7], [4, 3, 1]]], F)
    # direction 1: x = 2 starts; x = 1: m = 0, t = (min(3, 3+1, 3), min(3, 3+1, 0+1, 3), min(0, 3+1, 3)) = (3, 1, 0);
    # x = 0: m = 1, t = (min(7, 1+1, 4), min(1, 7+1, 6+1, 4), min(6, 1+1, 4)) = (2, 1, 2)
    L1 = np.array([[[2, 5, 3], [7, 1, 6], [3, 3, 0]]], F)
    assert np.array_equal(pr.plane_path(vol, 0, 1.0, 3.0)[:, :, 0], L0)
    assert np.array_equal(pr.plane_path(vol, 1, 1.0, 3.0)[:, :, 0], L1)
    res = pr.plane_aggregate(vol, 1.0, 3.0, 0x03)
    assert np.array_equal(res["agg"][:, :, 0], L0 + L1)
    assert res["idx"].tolist() == [[1, 2, 3]] and res["flow_x"].tolist() == [[-1.0, 0.0, 1.0]] and not res["flow_y"].any()
    # the same labels down a column: the neighbours are (dy -+ 1, dx)
    col = pr.plane_aggregate(np.ascontiguousarray(vol.transpose(0, 1, 3, 2)), 1.0, 3.0, 0x03)
    assert np.array_equal(col["agg"][:, :, :, 0], L0 + L1) and col["flow_y"].tolist() == [[-1.0, 0.0, 1.0]] and not col["flow_x"].any()
    # a vertical path over one row of pixels starts everywhere
    assert np.array_equal(pr.plane_path(vol, 2, 1.0, 3.0), vol) and np.array_equal(pr.plane_path(vol, 7, 1.0, 3.0), vol)


def test_a_flat_volume_takes_the_centre_class_everywhere():
    for hWin, wWin in ((3, 3), (4, 6), (1, 5), (9, 9)):
        res = pr.plane_aggregate(np.full((4, 5, hWin, wWin), 3.0, F), 1.0, 2.0, 0xff)
        assert (res["idx"] == cr.middle_index(hWin, wWin)).all()
        assert (res["flow_y"] == (hWin + 1) // 2 - 1 - (hWin - 1) // 2).all() and (res["flow_x"] == (wWin + 1) // 2 - 1 - (wWin - 1) // 2).all()
    vol = _volume((4, 5, 3, 3), 3)
    vol[1:3] = 2.0                                                 # flat pixels among others, no penalty: they stay flat
    assert (pr.plane_aggregate(vol, 0.0, 0.0, 0x0f)["idx"][1:3] == 5).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quality_on_the_band_scene(seed):
    wta, four, eight = (pr.band_share_wrong(seed, paths) for paths in (0, 0x0f, 0xff))
    print("band scene seed %d: winner-takes-all %.4f, 4 paths %.4f, 8 paths %.4f" % (seed, wta, four, eight))
    assert wta > 0.04
    assert eight < 0.01
    assert four < 0.5 * wta
