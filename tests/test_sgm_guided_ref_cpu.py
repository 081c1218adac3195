"""The numpy restatement of the edge-aware semi-global aggregation (tests/sgm_guided_ref.py; include/dfe.h) against the
existing references where the guide says nothing, against a hand-computed case where it does, the Python keywords' checks (which need
no device), and the bar scene's conditions.  The device is compared with this reference bit for bit in tests/test_gpu_sgm_guided.py."""
import numpy as np
import pytest
import torch

from tests import sgm_guided_ref as gr
from tests import sgm_plane_ref as pr
from tests import sgm_ref as sr

F = np.float32
INF = F(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _volume(shape, seed):
    return np.random.default_rng(seed).uniform(-3, 9, size=shape).astype(F)


UNGUIDED = (dict(), dict(guide="ramp", sigma=0.0), dict(guide="ramp", sigma=float("nan")), dict(guide="ramp", sigma=-2.0), dict(guide="flat", sigma=3.0),
            dict(guide=None, sigma=3.0))


def _guide(kind, H, W):
    if kind is None:
        return None
    g = np.full((2, H, W), 7.25, F)
    if kind == "ramp":
        g[0] += np.arange(W, dtype=F)[None, :] * F(1.5)
        g[1] += np.arange(H, dtype=F)[:, None] * F(0.75)
    return g


@pytest.mark.parametrize("kw", UNGUIDED, ids=lambda kw: "%s-%s" % (kw.get("guide"), kw.get("sigma")))
def test_without_a_say_of_the_guide_both_families_are_the_existing_references(kw):
    H, W = 5, 7
    kw = dict(kw, P2_edge=0.75)
    if "guide" in kw:
        kw["guide"] = _guide(kw["guide"], H, W)
    vol = _volume((H, W, 6), 1)
    for ring in (0, 3, W):
        for r in range(8):
            assert np.array_equal(_bits(gr.sgm_path(vol, r, 0.5, 4.0, ring, **kw)), _bits(sr.sgm_path(vol, r, 0.5, 4.0, ring))), (ring, r)
        got, want = gr.sgm_aggregate(vol, 0.5, 4.0, 0xff, ring, **kw), sr.sgm_aggregate(vol, 0.5, 4.0, 0xff, ring)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    vol = _volume((H, W, 3, 4), 2)
    for r in range(8):
        assert np.array_equal(_bits(gr.plane_path(vol, r, 0.5, 4.0, **kw)), _bits(pr.plane_path(vol, r, 0.5, 4.0))), r
    assert np.array_equal(_bits(gr.plane_sum(vol, 0.5, 4.0, 0xff, **kw)), _bits(pr.plane_sum(vol, 0.5, 4.0, 0xff)))


# ---- the hand-computed case: 1 x 3 pixels, direction 0 (the predecessor is the pixel on the left) ----
P1 = F(0.25)
P2 = F(3) + F(2.0 ** -22)            # an odd significand in [2, 4) ...
P2_EDGE = F(0.5) + F(2.0 ** -23)     # ... and half a unit of it: P2 - P2_edge is a tie and rounds to 2.5, P2_edge + 2.5 is a tie and rounds to 3
SIGMA = 4.0                          # 1 / sigma^2 = 0.0625 exactly


def _hand_step(prev, c, pen):
    """the step on a label plane (lists of rows of float32 scalars), label by label"""
    hW, wW = len(prev), len(prev[0])
    m = min(v for row in prev for v in row)
    at = lambda y, x: prev[y][x] if 0 <= y < hW and 0 <= x < wW else INF
    out = []
    for y in range(hW):
        out.append([])
        for x in range(wW):
            t = prev[y][x]
            for ny, nx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                t = min(t, F(at(ny, nx) + P1))
            t = min(t, F(m + pen))
            out[-1].append(F(c[y][x] + F(t - m)))
    return out


def _hand_line(vol, pens):
    """L_0 of a 1 x 3 volume [1][3][hW][wW] under the two steps' penalties"""
    rows = lambda a: [[F(v) for v in row] for row in a]
    L = [rows(vol[0, 0])]
    for x in (1, 2):
        L.append(_hand_step(L[-1], rows(vol[0, x]), pens[x - 1]))
    return np.asarray(L, F)[None]


@pytest.mark.parametrize("guide,pens", [
    ((10.0, 10.0, 13.0), (P2, F(P2_EDGE + F(F(P2 - P2_EDGE) * F(0.4375))))),      # w = 1: P2 itself; d = 3: w = 1 - 9 / 16
    ((10.0, 30.0, 33.0), (P2_EDGE, F(P2_EDGE + F(F(P2 - P2_EDGE) * F(0.4375))))),  # d = 20: 1 - 25 < 0, w = 0: P2_edge + span 0
], ids=["flat-then-ramp", "step-then-ramp"])
def test_hand_computed_line_of_three_pixels(guide, pens):
    assert F(P2_EDGE + F(P2 - P2_EDGE)) != P2, "the constants are chosen so that the w == 1 rule shows"
    assert P2_EDGE < pens[1] < P2
    g = np.asarray(guide, F).reshape(1, 1, 3)
    # the penalties themselves, then the lines of both families (the radial labels are a 1 x D plane: its cells have two neighbours)
    got = gr.penalty(g, np.zeros(2, int), np.array([1, 2]), np.zeros(2, int), np.array([0, 1]), SIGMA, P2, P2_EDGE)
    assert np.array_equal(_bits(got), _bits(np.asarray(pens, F)))
    vol = _volume((1, 3, 1, 5), 3)
    want = _hand_line(vol, pens)
    assert np.array_equal(_bits(gr.sgm_path(vol[:, :, 0], 0, P1, P2, 0, g, SIGMA, P2_EDGE)), _bits(want[:, :, 0]))
    assert np.array_equal(_bits(gr.plane_path(vol, 0, P1, P2, g, SIGMA, P2_EDGE)), _bits(want))
    vol = _volume((1, 3, 3, 3), 4)
    assert np.array_equal(_bits(gr.plane_path(vol, 0, P1, P2, g, SIGMA, P2_EDGE)), _bits(_hand_line(vol, pens)))
    # the penalty matters: with P2 everywhere the second pixel's line differs
    assert not np.array_equal(_bits(pr.plane_path(vol, 0, P1, P2)), _bits(_hand_line(vol, pens)))
    # direction 1 walks the same pairs from the other end: the same two numbers
    back = gr.penalty(g, np.zeros(2, int), np.array([0, 1]), np.zeros(2, int), np.array([1, 2]), SIGMA, P2, P2_EDGE)
    assert np.array_equal(_bits(back), _bits(got))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_guide_sample_that_is_not_finite_gives_P2_edge_on_both_steps_that_touch_it(bad):
    g = np.full((2, 1, 5), 3.0, F)
    g[1, 0, 2] = bad
    xs = np.arange(1, 5)
    pen = gr.penalty(g, np.zeros(4, int), xs, np.zeros(4, int), xs - 1, 2.0, 9.0, 1.5)
    assert np.array_equal(_bits(pen), _bits(np.asarray([9.0, 1.5, 1.5, 9.0], F)))
    g2 = np.repeat(g, 4, axis=1)
    for r in range(8):
        assert np.isfinite(gr.plane_path(_volume((4, 5, 3, 3), 5), r, 0.5, 9.0, g2, 2.0, 1.5)).all()
        assert np.isfinite(gr.sgm_path(_volume((4, 5, 6), 6), r, 0.5, 9.0, 5, g2, 2.0, 1.5)).all()


def test_direction_r_at_p_and_minus_r_at_its_predecessor_share_the_penalty_bits():
    rng = np.random.default_rng(7)
    g = rng.uniform(0, 9, size=(3, 6, 8)).astype(F)
    ys, xs = (a.ravel() for a in np.mgrid[1:5, 1:7])
    for dy, dx in gr.DIRS:
        a = gr.penalty(g, ys, xs, ys - dy, xs - dx, 12.0, 9.0, 1.5)                     # direction r at p, predecessor q = p - r
        b = gr.penalty(g, ys - dy, xs - dx, ys, xs, 12.0, 9.0, 1.5)                     # direction -r at q, predecessor q + r = p
        assert np.array_equal(_bits(a), _bits(b)) and len(set(_bits(a).tolist())) > 8


def test_the_wrappers_check_the_new_keywords_before_any_device_work():
    import depth_estimation_amd as d

    vol = torch.zeros((6, 9, 5))
    pvol = torch.zeros((6, 9, 3, 3))
    g = torch.zeros((2, 6, 9))
    img = torch.zeros((3, 40, 60))
    foe = (30.0, 20.0)
    ops = (lambda **kw: d.semiGlobalAggregate(vol, 1.0, 4.0, **kw), lambda **kw: d.semiGlobalAggregatePlane(pvol, 1.0, 4.0, **kw),
           lambda **kw: d.semiGlobalPick(pvol, 1.0, 4.0, paths=0x0f, **kw))
    for op in ops:
        # the values are accepted; the CPU volume is not
        for kw in (dict(), dict(guide=g, sigma=2.0), dict(guide=g, sigma=2.0, P2_edge=1.0), dict(guide=g, sigma=2.0, P2_edge=4.0), dict(guide=g),
                   dict(P2_edge=2.0), dict(guide=g[:1], sigma=float("inf"))):
            with pytest.raises(TypeError, match="CUDA"):
                op(**kw)
        with pytest.raises(ValueError, match="needs a guide"):
            op(sigma=2.0)
        for pe in (0.5, 4.5, float("nan"), "2", True):
            with pytest.raises(ValueError, match="P2_edge"):
                op(guide=g, sigma=2.0, P2_edge=pe)
        for sg in ("2", None, True):
            with pytest.raises(ValueError, match="sigma"):
                op(guide=g, sigma=sg)
        for bad in (g[0], g[:, :5], g[:, :, :8], torch.zeros((0, 6, 9)), torch.zeros((2, 9, 6))):
            with pytest.raises(ValueError, match="guide"):
                op(guide=bad, sigma=2.0)
        for bad in (g.double(), g.to(torch.uint8), g.numpy()):
            with pytest.raises(TypeError, match="guide"):
                op(guide=bad, sigma=2.0)
    pairs = (lambda sgm: d.flowDepthPair(img, img, 7, 9, 9, foe, sgm=sgm), lambda sgm: d.censusFlowDepthPair(img, img, 7, 9, 9, foe, sgm=sgm),
             lambda sgm: d.censusFlowDepthPair(img.to(torch.uint8), img.to(torch.uint8), 7, 9, 9, foe, sgm=sgm, consistency=1.0, subpixel=True))
    for pair in pairs:
        for sgm in (dict(P1=1.0, P2=4.0, sigma=2.0), dict(P1=1.0, P2=4.0, sigma=2.0, P2_edge=3.0, paths=0xff, min_unique=0.2), dict(P1=1.0, P2=4.0, P2_edge=1.0)):
            with pytest.raises(TypeError):                  # accepted up to the device check
                pair(sgm)
        for sgm in (dict(P1=1.0, P2=4.0, sigma=2.0, P2_edge=0.5), dict(P1=1.0, P2=4.0, sigma=2.0, P2_edge=5.0), dict(P1=1.0, P2=4.0, sigma="2"),
                    dict(P1=1.0, P2=4.0, sigma=2.0, guide=img), dict(P1=1.0, P2=4.0, Sigma=2.0), dict(P2=4.0, sigma=2.0)):
            with pytest.raises(ValueError):
                pair(sgm)


# ---- the bar scene: conditions, not measured values ----
@pytest.mark.parametrize("k", [7, 5])
def test_bar_scene_adaptive_penalties_keep_the_thin_object(k):
    seeds = gr.BAR["seeds"] if k == gr.BAR["k"] else gr.BAR_K5["seeds"]
    assert len(seeds) >= 3
    for seed in seeds:
        for paths in (0x0f, 0xff):
            wta, fixed, adaptive = (gr.bar_shares(seed, paths, mode, k) for mode in ("wta", "fixed", "adaptive"))
            print("k %d seed %d paths 0x%02x  bar: wta %.3f fixed %.3f adaptive %.3f   far: wta %.4f fixed %.4f adaptive %.4f"
                  % (k, seed, paths, wta[0], fixed[0], adaptive[0], wta[1], fixed[1], adaptive[1]))
            assert adaptive[0] <= 0.5 * fixed[0], (k, seed, paths, fixed, adaptive)
            assert adaptive[1] <= fixed[1] + 0.01, (k, seed, paths, fixed, adaptive)
        assert fixed[0] > 0, "8 paths at fixed penalties lose part of the bar: the scene shows the effect"
