"""The numpy definitions of tests/postfilter_ref.py against the compiled oracle on every case of tests/postfilter_cases.py -- bit for
bit where the definition is fp32, within the stated bounds where it is float64 -- and the case lists against the edges they claim."""
import numpy as np
import pytest

from tests import oracle as orc
from tests import postfilter_cases as pc
from tests import postfilter_ref as pr

F = np.float32


def same_bits(a, b):
    return np.array_equal(pr.bits(a), pr.bits(b))


@pytest.mark.parametrize("name,H,W,centre", pc.RADIAL_FRAMES, ids=[c[0] for c in pc.RADIAL_FRAMES])
def test_radial_depth(name, H, W, centre):
    f = pc.radial_flow(H, W)
    d, c = pr.flow_to_depth_radial(f, centre[0], centre[1], pc.RADIAL_INFTY)
    ed, ec = orc.flow_to_depth_radial(f, centre[0], centre[1], pc.RADIAL_INFTY)
    assert same_bits(d, ed) and same_bits(c, ec)


@pytest.mark.parametrize("fix_dot", [False, True])
def test_cartesian_depth(fix_dot):
    f = pc.cart_flow()
    d, c = pr.flow_to_depth_cartesian(f, pc.CART_FOE[0], pc.CART_FOE[1], fix_dot)
    ed, ec = orc.flow_to_depth_cartesian(f, pc.CART_FOE[0], pc.CART_FOE[1], fix_dot)
    assert same_bits(d, ed) and same_bits(c, ec)
    assert c.min() == 0 and c.max() == 1 and (d == F(pc.CART_FRAME[1] / 2)).any() and (d < F(pc.CART_FRAME[1] / 2)).any()


@pytest.mark.parametrize("name,H,W", pc.ARDRONE_FRAMES, ids=[c[0] for c in pc.ARDRONE_FRAMES])
def test_ardrone_depth(name, H, W):
    xflow, mask = pc.ardrone_case(H, W)
    d, c = pr.flow_to_depth_ardrone(xflow, mask, pc.ARDRONE_M)
    ed, ec = orc.flow_to_depth_ardrone(xflow, mask, pc.ARDRONE_M)
    assert same_bits(d, ed) and same_bits(c, ec)
    if W == 1:
        assert not c.any() and not d.any()   # every pixel is the middle column


def test_c_round():
    assert pr.c_round(np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999997, -8.4, -8.5, 11.4, 11.5], F)).tolist() == [1, -1, 2, -2, 3, 0, -8, -9, 11, 12]


@pytest.mark.parametrize("name,C,H,W", pc.WARP_CASES, ids=[c[0] for c in pc.WARP_CASES])
def test_warp(name, C, H, W):
    img, mask = pc.warp_case(C, H, W)
    ref32 = pr.warp_bilinear(img, mask, F)
    assert ref32.dtype == F and same_bits(ref32, orc.warp_bilinear(img, mask))
    ref64 = pr.warp_bilinear(img, mask)
    assert np.abs(ref32 - ref64).max() <= pr.warp_bound(img)
    # exact integer coordinates gather pixels; NaN samples row / column 0
    assert np.array_equal(ref32[:, :H, :W], img)
    assert np.array_equal(ref32[:, -1, :W], img[:, 0, :]) and np.array_equal(ref32[:, :H, -1], img[:, :, 0])


def test_warp_one_pixel():
    img, mask = pc.warp_one_pixel()
    assert same_bits(pr.warp_bilinear(img, mask, F), orc.warp_bilinear(img, mask))


@pytest.mark.parametrize("alpha", pc.GRID_ALPHAS)
def test_polar_grids(alpha):
    g = pc.C2P_GRID
    ref = pr.polar_grid_c2p(g["wdst"], g["hdst"], g["xc"], g["yc"], 2, 3, g["rmax"], alpha)
    o = orc.polar_grid_c2p(g["wsrc"], g["hsrc"], g["wdst"], g["hdst"], g["xc"], g["yc"], 2, 3, g["rmax"], alpha)
    assert o.shape == ref.shape and (np.abs(o - ref) <= pr.one_ulp(ref)).all()
    for g in (pc.P2C_GRID, pc.P2C_GRID_OFF):
        ref = pr.polar_grid_p2c(g["wsrc"], g["hsrc"], g["wdst"], g["hdst"], g["xc"], g["yc"], g["rmax"], alpha)
        o = orc.polar_grid_p2c(g["wsrc"], g["hsrc"], g["wdst"], g["hdst"], g["xc"], g["yc"], g["rmax"], alpha)
        assert (np.abs(o - ref) <= pr.one_ulp(ref)).all()
    assert ref.shape == (2, 29, 41) and pr.polar_grid_p2c(**dict(pc.P2C_GRID, alpha=alpha))[:, 11, 17].tolist() == [0, 0]


@pytest.mark.parametrize("lpad,rpad", pc.C2P_PADS)
def test_c2p_padding(lpad, rpad):
    wdst, hdst = pc.C2P_PAD_GRID
    o = orc.polar_grid_c2p(64, 48, wdst, hdst, 30.3, 20.7, lpad, rpad, 25.0, 1.0)
    core = o[:, :, lpad : lpad + wdst]
    assert np.array_equal(o[:, :, :lpad], core[:, :, wdst - lpad :]) and np.array_equal(o[:, :, lpad + wdst :], core[:, :, :rpad])
    ref = pr.polar_grid_c2p(wdst, hdst, 30.3, 20.7, lpad, rpad, 25.0, 1.0)
    assert (np.abs(o - ref) <= pr.one_ulp(ref)).all()


def _filter_cases(k, kind):
    if kind == "max":
        return pc.mode_cases(k) + ([("tie",) + pc.mode_tie_case()] if k == 3 else [])
    return [("frame",) + pc.median_case(k)]


@pytest.mark.parametrize("k", pc.MODE_KS)
def test_mode_filter(k):
    for name, flow, mask in _filter_cases(k, "max"):
        rc, o = orc.postprocess_image(flow, mask, k, "max")
        ref = pr.postprocess_mode(flow, mask, k)
        assert rc == 0 and np.array_equal(o, ref), name
        lo, _ = pr.rounded_span(flow)
        if name == "H==k":
            assert (o == lo).all()            # no window: the lifted border only
        if name != "tie":
            rc, _ = orc.postprocess_image(pc.span16(flow), mask, k, "max")
            assert rc == -1 and pr.postprocess_mode(pc.span16(flow), mask, k) is None, name
    if k == 3:
        _, flow, mask = _filter_cases(k, "max")[-1]
        assert pr.postprocess_mode(flow, mask, 3)[:, 1, 1].tolist() == [0, 5]   # the lower of the two codes


@pytest.mark.parametrize("k", pc.MEDIAN_KS)
def test_median_filter(k):
    flow, mask = pc.median_case(k)
    rc, o = orc.postprocess_image(flow, mask, k, "med")
    assert rc == 0 and np.array_equal(o, pr.postprocess_median(flow, mask, k))
    assert o[0, k // 2, k // 2] == pc.INF and o[1, k // 2, k // 2] == -pc.INF


@pytest.mark.parametrize("H,W", pc.ENLARGE_SIZES)
def test_enlarge_mask(H, W):
    for name, mask in pc.enlarge_masks(H, W):
        for ix, iy in pc.ENLARGE_WIDTHS:
            ref = pr.enlarge_mask(mask, ix, iy)
            assert np.array_equal(orc.enlarge_mask(mask, ix, iy), ref), (name, ix, iy)
            if ix == 0 and iy == 0:
                assert np.array_equal(ref, mask)


@pytest.mark.parametrize("maxh,maxw", pc.EXTRACTOR_WINDOWS)
def test_output_extractor(maxh, maxw):
    N = maxh * maxw
    for P in pc.EXTRACTOR_PS:
        p = pc.probabilities(P, N)
        x, y, sx, sy = pr.output_extractor(p, maxh, maxw)
        ex, ey = orc.output_extractor(p, maxh, maxw)
        # the oracle adds N products one after the other: N roundings of the running sum and one of each product
        assert (np.abs(ex - x) <= (N + 1) * pr.U * sx).all() and (np.abs(ey - y) <= (N + 1) * pr.U * sy).all()


@pytest.mark.parametrize("B", pc.MARGINAL_BS)
def test_marginal_sum(B):
    x = pc.marginal_input(5, 3, B)
    assert same_bits(orc.marginal_sum(x, 3, B), pr.marginal_sum(x, 3, B))


def test_the_cases_reach_every_edge():
    # off-grid radial centres: a fused a*a + b*b differs from the separately rounded one somewhere, in the sum and in the distance
    for name, H, W, centre in pc.RADIAL_FRAMES[:2]:
        a, b = pr.radial_offsets(H, W, *centre)
        plain = (a * a + b * b).astype(F)
        for fused in pr.fused_sq_sums(a, b):
            assert (fused != plain).any(), name
            assert (np.sqrt(fused.astype(np.float64)).astype(F) != np.sqrt(plain.astype(np.float64)).astype(F)).any(), name
    # ... which the on-grid centres of the first-generation tests never show
    a, b = pr.radial_offsets(60, 80, 33.0, 27.0)
    assert all((fused == (a * a + b * b).astype(F)).all() for fused in pr.fused_sq_sums(a, b))
    # sub-pixel flows: the same for the flow norm and the focus distance of the cartesian depth
    f = pc.cart_flow()
    assert any((fused != (f[1] * f[1] + f[0] * f[0]).astype(F)).any() for fused in pr.fused_sq_sums(f[1], f[0]))
    px, py = pr.radial_offsets(*pc.CART_FRAME, *pc.CART_FOE)
    assert any((fused != (px * px + py * py).astype(F)).any() for fused in pr.fused_sq_sums(px, py))
    dn = pr.flow_norm(f)
    assert (dn < F(0.2)).any() and (dn == F(0.2)).any() and ((dn > F(0.2)) & (dn < F(0.21))).any()
    # radial: d == 10 exactly (confidence 0) beside d^2 = 101 (confidence 1); every special flow value outside the centre disc
    name, H, W, centre = pc.RADIAL_FRAMES[-1]
    d = pr.radial_distance(H, W, *centre)
    _, conf = pr.flow_to_depth_radial(pc.radial_flow(H, W), centre[0], centre[1], pc.RADIAL_INFTY)
    assert d[0, 0] == 10 and conf[0, 0] == 0 and d[9, 16] == F(np.sqrt(101.0)) and conf[9, 16] == 1
    assert pc.BELOW_01 < float(F(0.1)) and F(pc.BELOW_01) == np.nextafter(F(0.1), F(0))
    for name, H, W, centre in pc.RADIAL_FRAMES:
        f, far = pc.radial_flow(H, W), pr.radial_distance(H, W, *centre) > 10
        if name == "9x13":   # the whole frame lies inside the disc d <= 10: no depth, no confidence anywhere
            assert not far.any()
            continue
        assert far.any() and (name in ("outside", "H1", "W1") or not far.all()), name
        for v in pc.RADIAL_SPECIALS:
            assert ((f == F(v)) & far).any(), (name, v)
    # ardrone: halves, both end bins, dropped samples, a tie of the two fullest bins, |mode| 1 and 2 with a confidence, mask 0.3
    seen = dict(tie=False, one=False, two=False, weak=False, end_bins=False)
    for name, H, W in pc.ARDRONE_FRAMES:
        xflow, mask = pc.ardrone_case(H, W)
        hist = pr.ardrone_histograms(xflow, mask)
        top = np.sort(hist, 0)
        _, conf = pr.flow_to_depth_ardrone(xflow, mask, pc.ARDRONE_M)
        mode = np.where(hist.max(0) > 0, hist.argmax(0) - 8, 0)
        seen["tie"] |= bool(((top[-1] == top[-2]) & (top[-1] > 0) & (mask != 0)).any())
        seen["one"] |= bool(((np.abs(mode) == 1) & (conf == 1)).any())
        seen["two"] |= bool(((np.abs(mode) == 2) & (conf == 1)).any())
        seen["weak"] |= bool(((mask == F(0.3)) & (hist.sum(0) > 0)).any())
        seen["end_bins"] |= bool(hist[0].any() and hist[19].any())
    assert all(seen.values()), seen
    r = pr.c_round(np.array(pc.ARDRONE_VALUES, F))
    assert {-9, -8, 11, 12, 1, -1, 2, -2} <= set(r.tolist())
    # mode filter: a span of exactly 15 with a negative minimum, an empty window, a tie between two codes
    tie = empty = False
    for k in pc.MODE_KS:
        for name, flow, mask in _filter_cases(k, "max"):
            lo, hi = pr.rounded_span(flow)
            if name != "tie":
                assert hi - lo == 15 and lo < 0, (k, name)
                lo16, hi16 = pr.rounded_span(pc.span16(flow))
                assert hi16 - lo16 == 16
            for i in range(flow.shape[1] - k):
                for j in range(flow.shape[2] - k):
                    cnt = np.sort(np.bincount(pr.window_codes(flow, mask, k, i, j), minlength=256))
                    empty |= cnt[-1] == 0
                    tie |= cnt[-1] > 0 and cnt[-1] == cnt[-2]
        assert not pc.mode_cases(k)[1][1].shape[1] - k and pc.mode_cases(k)[2][1].shape[1] - k == 1
    flow, mask = pc.mode_tie_case()
    cnt = np.bincount(pr.window_codes(flow, mask, 3, 0, 0), minlength=256)
    assert tie and empty and cnt[5] == 4 and cnt[18] == 4 and cnt.sum() == 9
    # median filter: a window with an even number of valid samples, an empty one, duplicates, both infinities, no zero
    for k in pc.MEDIAN_KS:
        flow, mask = pc.median_case(k)
        counts = [len(pr.window_values(flow, mask, k, i, j)[0]) for i in range(flow.shape[1] - k) for j in range(flow.shape[2] - k)]
        assert 0 in counts and (k == 1 or any(n and n % 2 == 0 for n in counts)), k
        assert not (flow == 0).any() and (flow == pc.INF).any() and (flow == -pc.INF).any() and np.unique(flow).size < flow.size / 2
    # enlargeMask: values of exactly 0.5 and of 0.75; a row whose only set pixel is the last column
    for H, W in pc.ENLARGE_SIZES:
        masks = dict(pc.enlarge_masks(H, W))
        assert (masks["halves"] == F(0.5)).any() and (masks["halves"] == F(0.75)).any()
        assert (masks["last-column"][:, -1] == 1).all() and masks["last-column"][:, :-1].sum() == 0
    assert any(ix >= W for ix, _ in pc.ENLARGE_WIDTHS for _, W in pc.ENLARGE_SIZES)
    # sizes above the caps of a single launch
    assert pc.BIG[0] * pc.BIG[1] > 8192 * 256 and pc.EXTRACTOR_OVER_CAP[0] > 8192 * 4 and pc.MARGINAL_OVER_CAP[0] > 8192 * 256
