"""The numpy definition of the census matching cost (tests/census_ref.py) against properties that follow from include/dfe.h, and the
quality claim of DESIGN.md section 4.30 on the exposure scene: where the second frame is darker, offset and noisy, the SSD's arg-min points
at the wrong cell on a quarter of the pixels or more, and the census cost summed over 3 x 3 on none or nearly none.  Reference only: no
device, no library."""
import numpy as np
import pytest

from tests import census_ref as cr


def _frames(seed, C=2, H=21, W=30):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 100, size=(C, H, W)).astype(np.float32), rng.randint(0, 100, size=(C, H, W)).astype(np.float32)


@pytest.mark.parametrize("kh,kw", [(3, 3), (7, 7), (9, 7), (3, 21)])
def test_signature_is_unchanged_by_gain_and_offset(kh, kw):
    a, _ = _frames(0, H=25, W=33)
    s = cr.signature(a, kh, kw)
    assert np.array_equal(s, cr.signature(2 * a + 3, kh, kw))
    assert np.array_equal(s, cr.signature(a.astype(np.uint8), kh, kw))          # the bytes themselves give the same bits
    assert s.dtype == np.uint64 and s.shape == (2, 25 - kh + 1, 33 - kw + 1)
    assert int(s.max()) < 2 ** (kh * kw - 1) and s.any()                          # the unused high bits are 0


def test_constant_frame_has_signature_zero_and_nan_compares_false():
    assert not cr.signature(np.full((1, 9, 11), 7.0, dtype=np.float32), 5, 5).any()
    a = np.arange(25, dtype=np.float32).reshape(1, 5, 5)
    assert int(cr.signature(a, 5, 5)[0, 0, 0]) == 2 ** 12 - 1                    # the 12 cells in front of the centre are below it
    b = a.copy()
    b[0, 0, 1] = np.nan                                                          # a NaN cell: its bit (1) is 0
    assert int(cr.signature(b, 5, 5)[0, 0, 0]) == 2 ** 12 - 1 - 2
    b = a.copy()
    b[0, 2, 2] = np.nan                                                          # a NaN centre: every bit is 0
    assert int(cr.signature(b, 5, 5)[0, 0, 0]) == 0


def test_bit_order_is_row_major_without_the_centre():
    a = np.full((1, 3, 5), 9.0, dtype=np.float32)
    for n, (i, j) in enumerate([(0, 0), (0, 4), (1, 1), (1, 3), (2, 4)]):
        b = a.copy()
        b[0, i, j] = 1.0
        cell = i * 5 + j
        assert int(cr.signature(b, 3, 5)[0, 0, 0]) == 1 << (cell if cell < 7 else cell - 1)


@pytest.mark.parametrize("hWin,wWin", [(5, 5), (4, 6)])
def test_cost_of_a_frame_against_itself_is_zero_at_the_centre(hWin, wWin):
    a, _ = _frames(1)
    s = cr.signature(a, 5, 5)
    c = cr.cost_volume(s, s, hWin, wWin, 1)
    mid = cr.middle_index(hWin, wWin) - 1
    assert not c.reshape(c.shape[:2] + (-1,))[:, :, mid].any()
    r = cr.flow(s, s, 24, hWin, wWin, 1)
    assert (r["idx"] == mid + 1).all() and not r["best"].any() and (r["match"] == 1).all()
    assert not r["flow_y"].any() and not r["flow_x"].any()


@pytest.mark.parametrize("a", [3, 5])
def test_aggregated_cost_is_the_box_sum_of_the_plain_one(a):
    f0, f1 = _frames(2)
    s0, s1 = cr.signature(f0, 7, 7), cr.signature(f1, 7, 7)
    h = cr.cost_volume(s0, s1, 4, 5, 1)
    c = cr.cost_volume(s0, s1, 4, 5, a)
    assert c.shape == (h.shape[0] - a + 1, h.shape[1] - a + 1, 4, 5)
    for y, x in [(0, 0), (c.shape[0] - 1, c.shape[1] - 1), (3, 7)]:
        assert np.array_equal(c[y, x], h[y:y + a, x:x + a].sum((0, 1)))
    assert c.max() <= 63 * 2 * a * a


def test_centre_wins_a_tie_and_the_first_minimum_wins_otherwise():
    cost = np.full((1, 3, 3, 3), 5, dtype=np.int64)
    cost[0, 1, 0, 2] = cost[0, 1, 2, 0] = 4          # pixel 1: two minima below the centre: the first one
    cost[0, 2, 2, 2] = 5                             # pixel 2: everything ties, the centre among them
    idx, best = cr.arg_best(cost)
    assert idx.tolist() == [[5, 3, 5]] and best.tolist() == [[5, 4, 5]]
    fy, fx = cr.decode(idx, 3, 3)
    assert fy.tolist() == [[0, -1, 0]] and fx.tolist() == [[0, 1, 0]]


def _ssd_flow(f0, f1, k, win):
    """float64 SSD over k x k patches, the first minimum over the win x win window in class order: the single-scale matcher's cost
    without its tie rule"""
    a, b = f0.astype(np.float64), f1.astype(np.float64)
    C, H, W = a.shape
    Hp, Wp = H - k + 1, W - k + 1
    Ho, Wo = Hp - win + 1, Wp - win + 1
    o = (win - 1) // 2
    cost = np.empty((Ho, Wo, win * win))
    for dy in range(win):
        for dx in range(win):
            d2 = ((a[:, o:o + Ho + k - 1, o:o + Wo + k - 1] - b[:, dy:dy + Ho + k - 1, dx:dx + Wo + k - 1]) ** 2).sum(0)
            s = np.zeros((Ho, Wo))
            for i in range(k):
                for j in range(k):
                    s += d2[i:i + Ho, j:j + Wo]
            cost[:, :, dy * win + dx] = s
    idx = cost.argmin(-1)
    return idx // win - o, idx % win - o


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exposure_scene_ssd_fails_and_census_does_not(seed):
    f0, f1 = cr.scene(seed)
    k, win = cr.SCENE["k"], cr.SCENE["win"]
    ssd = cr.share_wrong(*_ssd_flow(f0, f1, k, win))
    s0, s1 = cr.signature(f0, k, k), cr.signature(f1, k, k)
    r = cr.flow(s0, s1, k * k - 1, win, win, 3)
    census = cr.share_wrong(r["flow_y"], r["flow_x"])
    print("seed %d: SSD wrong on %.3f of the pixels, census agg 3 on %.3f" % (seed, ssd, census))
    assert ssd >= 0.25
    assert census <= 0.01 and census <= ssd / 10
