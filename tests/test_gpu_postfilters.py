"""GPU suite of the kernels that turn a flow field into depth, confidence and mask -- polar.hip, postfilters.hip, the cartesian depth of
postops.hip and cv_records.h -- on the cases of tests/postfilter_cases.py: centres and flows off the float grid, one-pixel-wide frames,
every size at which a kernel takes another path, and one frame above the 1-D grid cap, where the grid-stride step runs.

Bars.  The depth kernels, the filters, the mask erosion and the marginal sum equal the oracle bit for bit (fp32 operations rounded one
by one on both sides; division and the sqrt of a double are correctly rounded).  The warp stays within 7 * 2^-24 * max|img| of the
float64 definition, the polar grids within one float ulp, the extractor within (ceil(N / 64) + 7) * 2^-24 * sum p_k coord_k
(tests/postfilter_ref.py derives each)."""
import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import postfilter_cases as pc
from tests import postfilter_ref as pr

pytestmark = pytest.mark.gpu
F = np.float32
DFE_OK, DFE_E_ARG = 0, -1   # include/dfe.h


def T(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)   # (a copy: the cases are read-only arrays)


def assert_bits(got, ref, what):
    g, r = pr.bits(got), pr.bits(ref)
    assert g.shape == r.shape
    n = int(np.count_nonzero(g != r))
    assert n == 0, "%s: %d of %d values differ from the oracle" % (what, n, g.size)


def radial(dfe, cuda, f, centre, infty):
    ctx = dfe.get_ctx(0)
    H, W = f.shape
    t = T(f, cuda)
    d, c = (torch.full((H, W), -7.0, device=cuda) for _ in range(2))
    ctx.check(dfe.lib().dfe_flow_to_depth_radial(ctx.handle, t.data_ptr(), H, W, centre[0], centre[1], infty, d.data_ptr(), c.data_ptr()))
    return d.cpu().numpy(), c.cpu().numpy()


# ---- depth kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H,W,centre", pc.RADIAL_FRAMES, ids=[c[0] for c in pc.RADIAL_FRAMES])
def test_radial_depth_bits(dfe, cuda, name, H, W, centre):
    f = pc.radial_flow(H, W)
    d, c = radial(dfe, cuda, f, centre, pc.RADIAL_INFTY)
    ed, ec = orc.flow_to_depth_radial(f, centre[0], centre[1], pc.RADIAL_INFTY)
    assert_bits(d, ed, "depth")
    assert_bits(c, ec, "confidence")
    if name == "d10":
        assert c[0, 0] == 0 and d[0, 0] == 0 and c[9, 16] == 1   # d == 10 exactly is inside, d^2 = 101 outside
    if name == "60x80":   # the same through the module function (its own infty)
        gd, gc = dfe.flow2depth(dict(hImg=H, wImg=W), T(f, cuda), centre, 0.65)
        ed, ec = orc.flow_to_depth_radial(f, centre[0], centre[1], dfe.getRMax(H, W, centre) * 0.65)
        assert_bits(gd.cpu().numpy(), ed, "flow2depth depth")
        assert_bits(gc.cpu().numpy(), ec, "flow2depth confidence")


def cartesian(dfe, cuda, f, foe, fix_dot):
    ctx = dfe.get_ctx(0)
    _, H, W = f.shape
    t = T(f, cuda)
    d, c = (torch.full((H, W), -7.0, device=cuda) for _ in range(2))
    ctx.check(dfe.lib().dfe_flow_to_depth_cartesian(ctx.handle, t.data_ptr(), H, W, foe[0], foe[1], int(fix_dot), d.data_ptr(), c.data_ptr()))
    return d.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("fix_dot", [False, True])
def test_cartesian_depth_bits(dfe, cuda, fix_dot):
    f = pc.cart_flow()
    d, c = cartesian(dfe, cuda, f, pc.CART_FOE, fix_dot)
    ed, ec = orc.flow_to_depth_cartesian(f, pc.CART_FOE[0], pc.CART_FOE[1], fix_dot)
    assert_bits(d, ed, "depth")
    assert_bits(c, ec, "confidence")


def test_pair_step_depth_equals_the_oracle_formula(dfe, cuda):
    """The sub-pixel pair step's own depth epilogue (pair_depth_px) on its sub-pixel flow and a focus off the float grid, against the
    oracle's formula on the returned flow -- not against the device's stand-alone depth kernel."""
    from tests.test_gpu_subpixel import pair, translation, warped_pair

    H, W, k, hWin, wWin = pc.PAIR_STEP
    f0, f1 = warped_pair(H, W, translation(1.7, -2.2), seed=4)
    flow, _, dd, cc = pair(dfe, cuda, f0, f1, k, hWin, wWin, pc.CART_FOE, subpixel=True)
    assert np.count_nonzero(flow != np.round(flow)) > 0.3 * flow.size / 2, "hardly any sub-pixel flow"
    ed, ec = orc.flow_to_depth_cartesian(flow, pc.CART_FOE[0], pc.CART_FOE[1])
    assert_bits(dd, ed, "pair depth")
    assert_bits(cc, ec, "pair confidence")


@pytest.mark.parametrize("name,H,W", pc.ARDRONE_FRAMES, ids=[c[0] for c in pc.ARDRONE_FRAMES])
def test_ardrone_depth_bits(dfe, cuda, name, H, W):
    xflow, mask = pc.ardrone_case(H, W)
    d, c = dfe.computeDepthMapFromFlow(T(xflow, cuda), T(mask, cuda), pc.ARDRONE_M)
    ed, ec = orc.flow_to_depth_ardrone(xflow, mask, pc.ARDRONE_M)
    assert_bits(d.cpu().numpy(), ed, "depth")
    assert_bits(c.cpu().numpy(), ec, "confidence")


# ---- warp --------------------------------------------------------------------------------------------------------------------------
def _check_warp(dfe, cuda, img, mask):
    g = dfe.cartesian2polar(T(img, cuda), T(mask, cuda)).cpu().numpy()
    ref = pr.warp_bilinear(img, mask)
    err = float(np.abs(g - ref).max())
    assert err <= pr.warp_bound(img), "warp: %g off the float64 definition, bound %g" % (err, pr.warp_bound(img))
    return g


@pytest.mark.parametrize("name,C,H,W", pc.WARP_CASES, ids=[c[0] for c in pc.WARP_CASES])
def test_warp_edges(dfe, cuda, name, C, H, W):
    img, mask = pc.warp_case(C, H, W)
    g = _check_warp(dfe, cuda, img, mask)
    assert np.array_equal(g[:, :H, :W], img), "integer coordinates must gather the pixels"
    assert np.array_equal(g[:, H, :W], img[:, H - 1]) and np.array_equal(g[:, :H, W], img[:, :, W - 1])             # exactly H - 1 / W - 1
    assert np.array_equal(g[:, H + 1, :W], img[:, 0]) and np.array_equal(g[:, H + 2, :W], img[:, H - 1])            # -3.5, H + 10
    assert np.array_equal(g[:, H + 3, :W], img[:, H - 1]) and np.array_equal(g[:, H + 4, :W], img[:, 0])            # +inf, -inf
    assert np.array_equal(g[:, :H, W + 3], img[:, :, W - 1]) and np.array_equal(g[:, :H, W + 4], img[:, :, 0])
    assert np.array_equal(g[:, -1, :W], img[:, 0]) and np.array_equal(g[:, :H, -1], img[:, :, 0])                   # NaN: row / column 0
    assert np.allclose(g, orc.warp_bilinear(img, mask), rtol=0, atol=1e-6)


def test_warp_one_pixel(dfe, cuda):
    img, mask = pc.warp_one_pixel()
    g = _check_warp(dfe, cuda, img, mask)
    assert g.shape == (3, 1, 1)
    g2 = dfe.cartesian2polar(T(img[0], cuda), T(mask, cuda)).cpu().numpy()   # a 2-D image
    assert g2.shape == (1, 1) and g2[0, 0] == g[0, 0, 0]


# ---- polar grids -------------------------------------------------------------------------------------------------------------------
def _within_one_ulp(g, ref, what):
    bad = np.abs(g.astype(np.float64) - ref) > pr.one_ulp(ref)
    assert not bad.any(), "%s: %d of %d values off by more than one ulp, worst %g" % (what, bad.sum(), bad.size, np.abs(g - ref).max())


@pytest.mark.parametrize("lpad,rpad", pc.C2P_PADS)
def test_c2p_padding(dfe, cuda, lpad, rpad):
    wdst, hdst = pc.C2P_PAD_GRID
    m = dfe.getC2PMask(64, 48, wdst, hdst, 30.3, 20.7, lpad, rpad, 25.0).cpu().numpy()
    assert m.shape == (2, hdst, wdst + lpad + rpad)
    core = m[:, :, lpad : lpad + wdst]
    assert np.array_equal(m[:, :, :lpad], core[:, :, wdst - lpad :]), "left pad = the last lpad core columns"
    assert np.array_equal(m[:, :, lpad + wdst :], core[:, :, :rpad]), "right pad = the first rpad core columns"
    _within_one_ulp(m, pr.polar_grid_c2p(wdst, hdst, 30.3, 20.7, lpad, rpad, 25.0), "c2p")


@pytest.mark.parametrize("alpha", pc.GRID_ALPHAS)
def test_polar_grids_one_ulp(dfe, cuda, alpha):
    g = pc.C2P_GRID
    m = dfe.getC2PMask(g["wsrc"], g["hsrc"], g["wdst"], g["hdst"], g["xc"], g["yc"], 2, 3, g["rmax"], alpha).cpu().numpy()
    _within_one_ulp(m, pr.polar_grid_c2p(g["wdst"], g["hdst"], g["xc"], g["yc"], 2, 3, g["rmax"], alpha), "c2p")
    for g in (pc.P2C_GRID, pc.P2C_GRID_OFF):
        m = dfe.getP2CMask(g["wsrc"], g["hsrc"], g["wdst"], g["hdst"], g["xc"], g["yc"], g["rmax"], alpha).cpu().numpy()
        _within_one_ulp(m, pr.polar_grid_p2c(alpha=alpha, **g), "p2c")
        if g is pc.P2C_GRID:
            assert m[:, 11, 17].tolist() == [0, 0]   # the centre pixel: pow(0, .) = 0, atan2(0, 0) = 0


def test_c2p_refuses_what_makes_nan_coordinates(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    m = torch.full((2, 5, 12), -7.0, device=cuda)
    for rmax, alpha in ((25.0, 0.0), (25.0, -1.0), (0.0, 1.0), (-3.0, 1.0), (float("nan"), 1.0), (25.0, float("nan"))):
        assert lib.dfe_polar_grid_c2p_f32(ctx.handle, 64, 48, 12, 5, 30.0, 20.0, 0, 0, rmax, alpha, m.data_ptr()) == DFE_E_ARG
    torch.cuda.synchronize()
    assert bool((m == -7.0).all()), "a refused call wrote its grid"
    with pytest.raises(dfe.DfeError):
        dfe.getC2PMask(64, 48, 12, 5, 30.0, 20.0, 0, 0, 25.0, -0.5)


# ---- postProcessImage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", pc.MODE_KS)
def test_mode_filter_edges(dfe, cuda, k):
    cases = pc.mode_cases(k) + ([("tie",) + pc.mode_tie_case()] if k == 3 else [])
    for name, flow, mask in cases:
        rc, ref = orc.postprocess_image(flow, mask, k, "max")
        assert rc == 0
        out = dfe.postProcessImage(T(flow, cuda), T(mask, cuda), k, "max").cpu().numpy()
        assert np.array_equal(out, ref), "%s: %d values differ" % (name, np.count_nonzero(out != ref))
        if name == "H==k":
            assert (out == pr.rounded_span(flow)[0]).all()   # no window: the lifted border only
        if name == "tie":
            assert out[:, 1, 1].tolist() == [0, 5]           # two codes four times each: the lower one
        else:
            with pytest.raises(dfe.DfeError):                # one value more: a span of 16
                dfe.postProcessImage(T(pc.span16(flow), cuda), T(mask, cuda), k, "max")


@pytest.mark.parametrize("k", pc.MEDIAN_KS)
def test_median_filter_edges(dfe, cuda, k):
    flow, mask = pc.median_case(k)
    rc, ref = orc.postprocess_image(flow, mask, k, "med")
    assert rc == 0
    out = dfe.postProcessImage(T(flow, cuda), T(mask, cuda), k, "med").cpu().numpy()
    assert np.array_equal(out, ref), "%d values differ" % np.count_nonzero(out != ref)
    assert out[0, k // 2, k // 2] == pc.INF and out[1, k // 2, k // 2] == -pc.INF


@pytest.mark.parametrize("H,W", pc.ENLARGE_SIZES)
def test_enlarge_mask_edges(dfe, cuda, H, W):
    for name, mask in pc.enlarge_masks(H, W):
        for ix, iy in pc.ENLARGE_WIDTHS:
            t = T(mask, cuda)
            assert dfe.enlargeMask(t, ix, iy) is t
            assert np.array_equal(t.cpu().numpy(), orc.enlarge_mask(mask, ix, iy)), (name, ix, iy)


# ---- OutputExtractor / marginal sum ------------------------------------------------------------------------------------------------
def _check_extractor(dfe, cuda, P, maxh, maxw):
    N = maxh * maxw
    p = pc.probabilities(P, N)
    x, y, sx, sy = pr.output_extractor(p, maxh, maxw)
    ctx = dfe.get_ctx(0)
    t = T(p, cuda)
    gx, gy = (torch.full((P,), -7.0, device=cuda) for _ in range(2))
    ctx.check(dfe.lib().dfe_output_extractor_f32(ctx.handle, t.data_ptr(), P, maxh, maxw, gx.data_ptr(), gy.data_ptr()))
    ex, ey = np.abs(gx.cpu().numpy() - x), np.abs(gy.cpu().numpy() - y)
    assert (ex <= pr.extractor_bound(N, sx)).all() and (ey <= pr.extractor_bound(N, sy)).all(), (P, float((ex / sx).max()), float((ey / sy).max()))


@pytest.mark.parametrize("maxh,maxw", pc.EXTRACTOR_WINDOWS)
def test_output_extractor_windows(dfe, cuda, maxh, maxw):
    for P in pc.EXTRACTOR_PS:
        _check_extractor(dfe, cuda, P, maxh, maxw)


def test_output_extractor_above_the_grid_cap(dfe, cuda):
    _check_extractor(dfe, cuda, *pc.EXTRACTOR_OVER_CAP)


def _check_marginal(dfe, cuda, P, A, B):
    x = pc.marginal_input(P, A, B)
    ctx = dfe.get_ctx(0)
    t = T(x, cuda)
    out = torch.full((P, A), -7.0, device=cuda)
    ctx.check(dfe.lib().dfe_marginal_sum_f32(ctx.handle, t.data_ptr(), P, A, B, out.data_ptr()))
    assert_bits(out.cpu().numpy(), orc.marginal_sum(x, A, B), "marginal sum")


@pytest.mark.parametrize("B", pc.MARGINAL_BS)
def test_marginal_sum_bits(dfe, cuda, B):
    _check_marginal(dfe, cuda, 5, 3, B)


def test_marginal_sum_above_the_grid_cap(dfe, cuda):
    _check_marginal(dfe, cuda, *pc.MARGINAL_OVER_CAP)


# ---- one frame above the 1-D grid cap: the grid-stride step of every kernel --------------------------------------------------------
def test_big_frame_warp(dfe, cuda):
    img, mask = pc.warp_big()
    g = _check_warp(dfe, cuda, img, mask)
    assert np.allclose(g, orc.warp_bilinear(img, mask), rtol=0, atol=1e-6)


def test_big_frame_depths(dfe, cuda):
    H, W = pc.BIG
    f = pc.radial_flow(H, W, seed=3)
    d, c = radial(dfe, cuda, f, pc.BIG_CENTRE, 650.5)
    ed, ec = orc.flow_to_depth_radial(f, pc.BIG_CENTRE[0], pc.BIG_CENTRE[1], 650.5)
    assert_bits(d, ed, "radial depth")
    assert_bits(c, ec, "radial confidence")
    xflow, mask = pc.ardrone_big()
    d, c = dfe.computeDepthMapFromFlow(T(xflow, cuda), T(mask, cuda), pc.ARDRONE_M)
    ed, ec = orc.flow_to_depth_ardrone(xflow, mask, pc.ARDRONE_M)
    assert_bits(d.cpu().numpy(), ed, "ardrone depth")
    assert_bits(c.cpu().numpy(), ec, "ardrone confidence")


@pytest.mark.parametrize("method", ["max", "med"])
def test_big_frame_filters(dfe, cuda, method):
    flow, mask = pc.filter_big()
    rc, ref = orc.postprocess_image(flow, mask, 3, method)
    assert rc == 0
    out = dfe.postProcessImage(T(flow, cuda), T(mask, cuda), 3, method).cpu().numpy()
    assert np.array_equal(out, ref), "%d values differ" % np.count_nonzero(out != ref)


def test_big_polar_grids(dfe, cuda):
    g = pc.BIG_GRID
    m = dfe.getC2PMask(2560, 1440, g["wdst"], g["hdst"], g["xc"], g["yc"], 3, 4, g["rmax"], 1.25).cpu().numpy()
    _within_one_ulp(m, orc.polar_grid_c2p(2560, 1440, g["wdst"], g["hdst"], g["xc"], g["yc"], 3, 4, g["rmax"], 1.25), "c2p")
    m = dfe.getP2CMask(1280, 720, g["wdst"], g["hdst"], g["xc"], g["yc"], g["rmax"], 1.25).cpu().numpy()
    _within_one_ulp(m, orc.polar_grid_p2c(1280, 720, g["wdst"], g["hdst"], g["xc"], g["yc"], g["rmax"], 1.25), "p2c")


# ---- empty inputs ------------------------------------------------------------------------------------------------------------------
def test_empty_inputs_need_no_tensors(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    h = ctx.handle
    for H, W in ((0, 5), (5, 0), (0, 0)):
        assert lib.dfe_flow_to_depth_radial(h, None, H, W, 1.5, 2.5, 10.0, None, None) == DFE_OK
        assert lib.dfe_flow_to_depth_cartesian(h, None, H, W, 1.5, 2.5, 0, None, None) == DFE_OK
        assert lib.dfe_flow_to_depth_ardrone(h, None, None, H, W, 0.37, None, None) == DFE_OK
        assert lib.dfe_enlarge_mask_f32(h, None, H, W, 2, 2) == DFE_OK
        assert lib.dfe_warp_bilinear_f32(h, None, 3, 4, 5, None, H, W, None) == DFE_OK
    assert lib.dfe_output_extractor_f32(h, None, 0, 8, 8, None, None) == DFE_OK
    assert lib.dfe_marginal_sum_f32(h, None, 0, 8, 8, None) == DFE_OK
    torch.cuda.synchronize()
