"""The case table of tests/pyramid_cases.py is fit for purpose -- checked on the oracle alone, without a device.

The device suite (tests/test_gpu_pyramid_shapes.py) excuses a pixel only where the oracle's two best classes lie within 1e-5, and at most
2 % of them.  A row whose own tie share came near that cap would let a wrong kernel through, and a row whose winners all sit in one scale
would never decode a class of the others.  Both are pinned here, per row, on the inputs the device suite uses."""
import numpy as np
import pytest

from tests import oracle as orc
from tests import pyramid_cases as pc


@pytest.mark.parametrize("c", pc.CASES + [pc.SWITCH_ORACLE], ids=[c.id for c in pc.CASES + [pc.SWITCH_ORACLE]])
def test_row_has_few_ties_and_reaches_its_scales(c):
    assert all(c.H % r == 0 and c.W % r == 0 for r in c.ratios)
    bases, ncls = pc.class_bases(c.ratios, c.mh, c.mw)
    assert ncls == orc.multi_nclasses(c.mh, c.mw, c.ratios)
    ref = pc.reference(c.no)
    assert ref["idx"].shape == (c.H, c.W) and ref["idx"].min() >= 1 and ref["idx"].max() <= ncls
    share = float(pc.tie_mask(ref).mean())
    wins = np.bincount(pc.scale_of(ref["idx"], c.ratios, c.mh, c.mw).ravel(), minlength=len(c.ratios)).tolist()
    print("row %d: tie share %.4f (table %.4f), winners per scale %s (table %s)" % (c.no, share, c.ties, wins, c.wins))
    assert share <= pc.TIE_CAP
    if c.wins is not None:
        for s, w in enumerate(c.wins):
            if w >= pc.MIN_WINS:
                assert wins[s] >= pc.MIN_WINS, "scale %d wins %d pixels only (%d when the table was made)" % (s, wins[s], w)


def test_switch_row_is_what_the_switch_suite_needs():
    """row 21: the fp16 oracle chain has few fp32-rule ties too, the share of pixels the fp16 rule may excuse is the measured one (the rule
    itself caps the pixels that differ at 2 %), every scale wins pixels, and the coarsest scale is one tile of 5 row groups high"""
    c = pc.SWITCH_ORACLE
    ref = pc.reference(c.no, 1.0)
    top2 = ref["top2"]
    share16 = float((top2[..., 1] - top2[..., 0] <= 2e-3 * np.maximum(top2[..., 1], 1e-6) + 1e-5).mean())
    print("row %d, fp16 chain: fp32-rule tie share %.4f, fp16-rule share %.4f (table %.4f)" % (c.no, float(pc.tie_mask(ref).mean()), share16, c.ties16))
    assert float(pc.tie_mask(ref).mean()) <= pc.TIE_CAP and abs(share16 - c.ties16) <= 0.005
    assert all(w >= pc.MIN_WINS for w in c.wins)
    assert c.H // c.ratios[-1] == 6 * 5 - 6 and (c.W // 8) % 4 == 1 and (c.W // c.ratios[-1]) % 32 == 2
    assert (c.mh, c.mw, c.k, c.C) == (8, 8, 7, 3)


def test_prep_tiles_oracle_row_has_few_ties():
    """1032 x 1480, C = 1, ratios 1, 2, 4, 8: the frame the device suite takes through prep_tiles_kernel and compares with the oracle"""
    c = pc.PREP_ORACLE
    ref = pc.reference(0)
    share = float(pc.tie_mask(ref).mean())
    wins = np.bincount(pc.scale_of(ref["idx"], c.ratios, c.mh, c.mw).ravel(), minlength=len(c.ratios)).tolist()
    print("prep row: tie share %.4f, winners per scale %s" % (share, wins))
    assert share <= pc.TIE_CAP


def test_the_table_reaches_what_it_says():
    """the geometry each row is there for, restated from its numbers"""
    by = pc.BY_NO
    d = {n: pc.ring_widths(c.ratios, c.mw) for n, c in by.items()}
    assert by[1].mh == 2 * d[1][1] and by[1].mh * by[1].mw == 32
    assert by[2].k % 2 == 0 and by[2].mh > by[2].mw
    assert by[3].ratios == [1, 3] and by[3].W % 2 == 1 and by[3].mh != by[3].mw
    assert by[5].mh == by[5].mw == 8 and d[5][1] == 3
    assert by[6].mh * by[6].mw == 64 and by[6].mh != 8
    assert by[7].mh * by[7].mw == 96 and by[8].mh * by[8].mw == 144 and by[8].ratios == [1, 2, 6]
    assert len(by[9].ratios) == 6 and by[9].mh * by[9].mw == 64
    assert by[10].W % 8 == 6 and by[10].k == 9 and by[10].C == 4
    assert by[11].W % 8 == 2 and (by[11].H // 2) % 2 == 1 and (by[11].k, by[11].C) == (7, 3) and d[11][1] == 2
    assert by[12].ratios == [1] and by[12].mh % 2 == 1 and by[12].mw % 2 == 1
    assert (by[13].mh, by[13].mw, d[13][1]) == (8, 8, 2) and (by[13].k, by[13].C) != (7, 3)
    for ratios, mh, mw, s in pc.BAD_RINGS:
        assert mh < 2 * pc.ring_widths(ratios, mw)[s]
    for ratios, mh, mw in pc.EDGE_RINGS:
        assert mh == 2 * pc.ring_widths(ratios, mw)[1]
    for H, W, C, ratios, _ in pc.PREP_CASES:
        assert H * W >= 1500000 and all(H % r == 0 and W % r == 0 for r in ratios) and set(ratios) <= {1, 2, 4, 8, 16}
    H, W = pc.PREP_CASES[0][:2]
    assert H % 64 == 8 and W % 64 == 8
