"""GPU suite of the sub-pixel radial flow: dfe_radial_match_subpixel_f32, dfe_radial_refine_subpixel_f32,
dfe_radial_flow_depth_pair_subpixel_f32 and radialFlowDepth(subpixel=True).

The reference of the bit-for-bit tests is numpy in float32 with the kernel's own operation order: the matcher volume
`vol[:, :, d] = vol[:, :, d] + t * t`, `t = in1[k] - in2[k, d:d+H1]`, k ascending; its first minimum bi; and the rule of include/dfe.h,
off = (cm - cp) / (2 ((cm - c0) + (cp - c0))) clamped to [-0.5, 0.5] where bi is inside the window and the denominator positive, else 0;
flow = bi + off.  Every numpy operation on float32 arrays is one separately rounded IEEE operation, as in the kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import refpath as rp

pytestmark = pytest.mark.gpu
DFE_E_ARG, DFE_E_SHAPE, DFE_E_UNSUPPORTED = -1, -2, -5


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def np_volume(in1, in2, H1, hWin):
    K, _, W = in1.shape
    vol = np.zeros((H1, W, hWin), np.float32)
    for k in range(K):
        for d in range(hWin):
            t = in1[k, :H1] - in2[k, d:d + H1]
            vol[:, :, d] = vol[:, :, d] + t * t
    return vol


def np_rule(vol):
    """(bi, bi + off) of include/dfe.h for a volume [...][hWin], float32 throughout."""
    vol = np.asarray(vol, np.float32)
    hW = vol.shape[-1]
    bi = vol.argmin(-1)                                   # numpy: the first minimum

    def cell(k):
        return np.take_along_axis(vol, np.clip(k, 0, hW - 1)[..., None], -1)[..., 0]

    c0, cm, cp = cell(bi), cell(bi - 1), cell(bi + 1)
    den = (cm - c0) + (cp - c0)
    ok = (bi >= 1) & (bi + 1 < hW) & (den > 0)
    with np.errstate(all="ignore"):
        off = (cm - cp) / (np.float32(2) * den)
    off = np.minimum(np.maximum(off, np.float32(-0.5)), np.float32(0.5))
    off = np.where(ok, off, np.float32(0)).astype(np.float32)
    assert off.dtype == np.float32 and den.dtype == np.float32
    return bi, bi.astype(np.float32) + off


def run_match(dfe, cuda, name, in1, in2, H1, hWin, want_volume, zero_last):
    K, rows, W = in1.shape
    ctx = dfe.get_ctx(0)
    t1, t2 = T(in1, cuda), T(in2, cuda)
    vol = torch.full((H1, W, hWin), float("nan"), device=cuda) if want_volume else None
    flow = torch.full((H1, W), float("nan"), device=cuda)
    ctx.check(getattr(dfe.lib(), name)(ctx.handle, t1.data_ptr(), rows, t2.data_ptr(), K, H1, W, hWin, vol.data_ptr() if want_volume else None,
                                       flow.data_ptr(), zero_last))
    torch.cuda.synchronize()
    return flow.cpu().numpy(), (vol.cpu().numpy() if want_volume else None)


def match_inputs(hWin, K, H1, W, extra, integer, seed=0):
    rng = np.random.default_rng(seed)
    if integer:
        in1 = rng.integers(-3, 4, size=(K, H1 + extra, W)).astype(np.float32)      # exact ties, zero denominators
        in2 = rng.integers(-3, 4, size=(K, H1 + hWin - 1, W)).astype(np.float32)
    else:
        in1 = rng.standard_normal((K, H1 + extra, W)).astype(np.float32)           # planes taller than H1: only the first H1 rows are read
        in2 = rng.standard_normal((K, H1 + hWin - 1, W)).astype(np.float32)
        if W > 5 and H1 >= 5:
            in2[:, 3:8, 5] = in1[:, 0:5, 5]                                        # exact zeros -> exact ties at some cells
    return in1, in2


# hWin, K, H1, W, rows of in1 beyond H1, zero_last_row, volume given, integer-valued features
MATCH_CASES = [
    (15, 10, 37, 100, 5, 0, True, False),
    (15, 10, 37, 100, 5, 1, False, False),
    (12, 7, 20, 64, 0, 1, True, False),
    (8, 3, 9, 130, 2, 0, False, False),
    (16, 12, 33, 65, 0, 0, True, False),
    (15, 4, 64, 128, 0, 1, True, False),
    (15, 5, 41, 70, 3, 0, True, True),
    (16, 6, 70, 200, 1, 1, False, True),
    (8, 2, 1, 3, 0, 0, True, False),
]


@pytest.mark.parametrize("hWin,K,H1,W,extra,zero_last,want_volume,integer", MATCH_CASES)
def test_matcher_subpixel_equals_numpy_bitwise(dfe, cuda, hWin, K, H1, W, extra, zero_last, want_volume, integer):
    in1, in2 = match_inputs(hWin, K, H1, W, extra, integer)
    ref_vol = np_volume(in1, in2, H1, hWin)
    bi, ref = np_rule(ref_vol)
    if zero_last:
        ref[-1] = 0
    flow, vol = run_match(dfe, cuda, "dfe_radial_match_subpixel_f32", in1, in2, H1, hWin, want_volume, zero_last)
    if want_volume:
        assert np.array_equal(vol, ref_vol)
    assert np.array_equal(flow, ref)
    plain, pvol = run_match(dfe, cuda, "dfe_radial_match_argmin_f32", in1, in2, H1, hWin, want_volume, zero_last)
    if want_volume:
        assert np.array_equal(pvol, ref_vol)
    assert np.abs(flow - plain).max() <= 0.5
    edge = (bi == 0) | (bi == hWin - 1)
    assert np.array_equal(flow[edge], plain[edge])
    if H1 * W > 100 and not integer:
        assert (flow != plain).mean() > 0.3               # the refinement does something


@pytest.mark.parametrize("hWin,K,H1,W,extra,zero_last,want_volume,integer", MATCH_CASES)
def test_standalone_refine_equals_fused_bitwise(dfe, cuda, hWin, K, H1, W, extra, zero_last, want_volume, integer):
    in1, in2 = match_inputs(hWin, K, H1, W, extra, integer)
    fused, vol = run_match(dfe, cuda, "dfe_radial_match_subpixel_f32", in1, in2, H1, hWin, True, 0)
    plain, _ = run_match(dfe, cuda, "dfe_radial_match_argmin_f32", in1, in2, H1, hWin, False, 0)
    out = dfe.refineRadialFlowSubpixel(T(vol, cuda), T(plain, cuda))
    assert np.array_equal(out.cpu().numpy(), fused)
    ctx = dfe.get_ctx(0)
    tv, tf = T(vol, cuda), T(plain, cuda)                 # in place
    ctx.check(dfe.lib().dfe_radial_refine_subpixel_f32(ctx.handle, tv.data_ptr(), tf.data_ptr(), H1 * W, hWin, tf.data_ptr()))
    assert np.array_equal(tf.cpu().numpy(), fused)


@pytest.mark.parametrize("hWin", [1, 2, 5, 17])
def test_standalone_refine_any_window_equals_numpy(dfe, cuda, hWin):
    rng = np.random.default_rng(hWin)
    P = 3001
    vol = rng.standard_normal((P, hWin)).astype(np.float32) ** 2
    vol[::7] = np.round(vol[::7] * 2)                     # ties and flat neighbourhoods
    bi, ref = np_rule(vol)
    flow = bi.astype(np.float32)
    out = dfe.refineRadialFlowSubpixel(T(vol, cuda), T(flow, cuda))
    assert tuple(out.shape) == (P,)
    assert np.array_equal(out.cpu().numpy(), ref)
    if hWin <= 2:
        assert np.array_equal(out.cpu().numpy(), flow)
    else:
        assert (ref != flow).mean() > 0.3
    ctx = dfe.get_ctx(0)
    tv, tf = T(vol, cuda), T(flow, cuda)
    ctx.check(dfe.lib().dfe_radial_refine_subpixel_f32(ctx.handle, tv.data_ptr(), tf.data_ptr(), P, hWin, tf.data_ptr()))
    assert torch.equal(tf, out)
    # a flow that is no index of the window stays as it is
    odd = np.array([-1, hWin, 1e9, -0.0], np.float32)
    o2 = dfe.refineRadialFlowSubpixel(T(vol[:4], cuda), T(odd, cuda))
    assert np.array_equal(o2.cpu().numpy(), odd)


# ------------------------------------------------------------------ the one-call path (the configurations of tests/test_gpu_multiscale_radial.py)
def _radial_setup(dfe, cuda, hImg, wImg, hIn, wIn, layers, hWin=15, seed=0):
    networkp = dict(hImg=hImg, wImg=wImg, hInput=hIn, wInput=wIn, hWin=hWin, layers=layers)
    g = torch.Generator().manual_seed(seed)
    net = dfe.getTesterNetwork(networkp, device=cuda, generator=g)
    f0, f1, _, (cx, cy) = rp.synth_pair(hImg, wImg, C=3, seed=seed, max_flow=6, noise_sigma=0)
    return networkp, net, f0 / np.float32(255), f1 / np.float32(255), (cx, cy)


@pytest.mark.parametrize("hImg,wImg,hIn,wIn,layers,seed", [
    (720, 1280, 720, 1280, [[3, 1, 17, 5], [5, 17, 1, 10]], 3),          # the `720p-radial` bench workload
    (180, 320, 200, 200, [[3, 1, 17, 5], [5, 17, 1, 10]], 0),            # the reference's defaults (train_radial:27-33)
    (180, 320, 120, 136, [[3, 1, 17, 5], "tanh", [5, 17, 1, 10]], 0),
    (180, 320, 96, 100, [[3, 1, 9, 4], [4, 11, 1, 6]], 0),               # generic convolutions inside the one call
])
@pytest.mark.parametrize("zero_last", [False, True])
def test_one_call_subpixel_equals_staged_and_numpy(dfe, cuda, hImg, wImg, hIn, wIn, layers, seed, zero_last):
    networkp, net, f0, f1, e2 = _radial_setup(dfe, cuda, hImg, wImg, hIn, wIn, layers, seed=seed)
    a, b = T(f0, cuda), T(f1, cuda)
    one = dfe.radialFlowDepth(networkp, net, a, b, e2, one_call=True, want_volume=True, zero_last_row=zero_last, subpixel=True)
    stg = dfe.radialFlowDepth(networkp, net, a, b, e2, one_call=False, want_volume=True, zero_last_row=zero_last, subpixel=True)
    hm, hOut, wOut = dfe.radial_out_shape(networkp)
    assert tuple(one["polar_flow"].shape) == (hm, wIn) and tuple(one["depth"].shape) == (hOut, wOut)
    for k in ("output", "polar_flow", "flow", "depth", "confs"):
        assert torch.equal(one[k], stg[k]), k
    bi, ref = np_rule(one["output"].cpu().numpy())
    if zero_last:
        ref[-1] = 0
    pf = one["polar_flow"].cpu().numpy()
    assert np.array_equal(pf, ref)
    assert (pf != np.round(pf)).mean() > 0.2              # fractional flows reach the depth stage
    # subpixel=False is the entry as it was: the wrapper and a direct call of dfe_radial_flow_depth_pair_f32 agree bit for bit, and
    # its polar flow is the integer the sub-pixel flow was refined from
    plain = dfe.radialFlowDepth(networkp, net, a, b, e2, one_call=True, want_volume=True, zero_last_row=zero_last, subpixel=False)
    dflt = dfe.radialFlowDepth(networkp, net, a, b, e2, one_call=True, want_volume=True, zero_last_row=zero_last)
    plain_stg = dfe.radialFlowDepth(networkp, net, a, b, e2, one_call=False, want_volume=True, zero_last_row=zero_last, subpixel=False)
    for k in ("output", "polar_flow", "flow", "depth", "confs"):
        assert torch.equal(plain[k], dflt[k]) and torch.equal(plain[k], plain_stg[k]), k
    assert torch.equal(plain["output"], one["output"])
    refi = bi.astype(np.float32)
    if zero_last:
        refi[-1] = 0
    assert np.array_equal(plain["polar_flow"].cpu().numpy(), refi)
    from depth_estimation_amd._lib import RadialParams
    from depth_estimation_amd.radial import _separable_weights

    w1, b1, w2, b2, th = _separable_weights(net, networkp)
    prm = RadialParams(3, hImg, wImg, hIn, wIn, 15, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), 1.0, 0.65, 1 if zero_last else 0)
    outs = {k: torch.empty_like(plain[k]) for k in ("output", "polar_flow", "flow", "depth", "confs")}
    ctx = dfe.get_ctx(0)
    ctx.check(dfe.lib().dfe_radial_flow_depth_pair_f32(ctx.handle, C.byref(prm), a.data_ptr(), b.data_ptr(), float(e2[0]), float(e2[1]), w1.data_ptr(),
                                                       b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), outs["output"].data_ptr(),
                                                       outs["polar_flow"].data_ptr(), outs["flow"].data_ptr(), outs["depth"].data_ptr(),
                                                       outs["confs"].data_ptr()))
    for k in outs:
        assert torch.equal(outs[k], plain[k]), k


def test_errors(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    K, H1, W = 2, 8, 16
    i1 = torch.zeros((K, H1, W), device=cuda)
    i2 = torch.zeros((K, H1 + 15, W), device=cuda)
    fl = torch.zeros((H1, W), device=cuda)
    vol = torch.zeros((H1, W, 16), device=cuda)
    p1, p2, pf, pv = i1.data_ptr(), i2.data_ptr(), fl.data_ptr(), vol.data_ptr()
    fn = lib.dfe_radial_match_subpixel_f32
    assert fn(ctx.handle, p1, 0, p2, K, H1, W, 9, None, pf, 0) == DFE_E_UNSUPPORTED
    assert fn(ctx.handle, None, 0, p2, K, H1, W, 15, None, pf, 0) == DFE_E_ARG
    assert fn(ctx.handle, p1, 0, None, K, H1, W, 15, None, pf, 0) == DFE_E_ARG
    assert fn(ctx.handle, p1, 0, p2, K, H1, W, 15, pv, None, 0) == DFE_E_ARG
    assert fn(None, p1, 0, p2, K, H1, W, 15, None, pf, 0) == DFE_E_ARG
    assert fn(ctx.handle, p1, 0, p2, 0, H1, W, 15, None, pf, 0) == DFE_E_SHAPE
    assert fn(ctx.handle, p1, 0, p2, K, 0, W, 15, None, pf, 0) == DFE_E_SHAPE
    assert fn(ctx.handle, p1, 0, p2, K, H1, -1, 15, None, pf, 0) == DFE_E_SHAPE
    assert fn(ctx.handle, p1, 0, p2, K, H1, W, 0, None, pf, 0) == DFE_E_SHAPE
    assert fn(ctx.handle, p1, H1 - 1, p2, K, H1, W, 15, None, pf, 0) == DFE_E_SHAPE
    assert fn(ctx.handle, p1, 0, p2, K, H1, W, 16, pv, pf, 0) == 0
    fn = lib.dfe_radial_refine_subpixel_f32
    assert fn(ctx.handle, None, pf, H1 * W, 16, pf) == DFE_E_ARG
    assert fn(ctx.handle, pv, None, H1 * W, 16, pf) == DFE_E_ARG
    assert fn(ctx.handle, pv, pf, H1 * W, 16, None) == DFE_E_ARG
    assert fn(None, pv, pf, H1 * W, 16, pf) == DFE_E_ARG
    assert fn(ctx.handle, pv, pf, 0, 16, pf) == DFE_E_SHAPE
    assert fn(ctx.handle, pv, pf, H1 * W, 0, pf) == DFE_E_SHAPE
    assert fn(ctx.handle, pv, pf, H1 * W, 16, pf) == 0
    from depth_estimation_amd._lib import RadialParams

    prm = RadialParams(3, 60, 80, 64, 64, 15, 5, 17, 10, 17, 0, 1.0, 0.65, 0)
    fr = torch.zeros((3, 60, 80), device=cuda)
    w1, w2 = torch.zeros((5, 3, 1, 17), device=cuda), torch.zeros((10, 5, 17, 1), device=cuda)
    fn = lib.dfe_radial_flow_depth_pair_subpixel_f32
    args = lambda p, f0, wa: (ctx.handle, C.byref(p) if p is not None else None, f0, fr.data_ptr(), 40.0, 30.0, wa, None, w2.data_ptr(), None, None, None,
                              None, None, None)
    assert fn(*args(prm, fr.data_ptr(), w1.data_ptr())) == 0
    assert fn(*args(None, fr.data_ptr(), w1.data_ptr())) == DFE_E_ARG
    assert fn(*args(prm, None, w1.data_ptr())) == DFE_E_ARG
    assert fn(*args(prm, fr.data_ptr(), None)) == DFE_E_ARG
    small = RadialParams(3, 60, 80, 30, 64, 15, 5, 17, 10, 17, 0, 1.0, 0.65, 0)   # 30 polar rows < kernel 17 + window 15 - 1
    assert fn(*args(small, fr.data_ptr(), w1.data_ptr())) == DFE_E_SHAPE
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        dfe.refineRadialFlowSubpixel(vol, fl[:4])


# ------------------------------------------------------------------ accuracy at the matcher
def _shifted_features(s, noise, K=10, H1=96, W=192, hWin=15):
    """in2 = box-smoothed (5 rows) standard-normal planes, in1[y] = their linear interpolation at row y + s: the true flow is s."""
    rng = np.random.default_rng(1)
    raw = rng.standard_normal((K, H1 + hWin - 1 + 12, W)).astype(np.float32)
    n = raw.shape[1] - 4
    base = (raw[:, 0:n] + raw[:, 1:n + 1] + raw[:, 2:n + 2] + raw[:, 3:n + 3] + raw[:, 4:n + 4]) / np.float32(5)
    in2 = np.ascontiguousarray(base[:, 4:4 + H1 + hWin - 1])
    pos = 4 + np.arange(H1, dtype=np.float32) + np.float32(s)
    i0 = np.floor(pos).astype(int)
    w = (pos - i0).astype(np.float32)[None, :, None]
    in1 = ((1 - w) * base[:, i0] + w * base[:, i0 + 1]).astype(np.float32)
    if noise:
        in1 = (in1 + rng.normal(0, noise, in1.shape)).astype(np.float32)
    return np.ascontiguousarray(in1), in2


@pytest.mark.parametrize("noise", [0.0, 0.05])
@pytest.mark.parametrize("s", [3.3, 2.75, 9.4])
def test_matcher_accuracy_inside_the_window(dfe, cuda, s, noise):
    """The refined flow's median |flow - s| is at most half the integer flow's (CPU prototype in float32: 0.098 / 0.104 / 0.068
    against 0.300 / 0.250 / 0.400 without noise, 0.106 / 0.112 / 0.085 with N(0, 0.05) noise)."""
    in1, in2 = _shifted_features(s, noise)
    sub, _ = run_match(dfe, cuda, "dfe_radial_match_subpixel_f32", in1, in2, 96, 15, False, 0)
    plain, _ = run_match(dfe, cuda, "dfe_radial_match_argmin_f32", in1, in2, 96, 15, False, 0)
    e_sub, e_int = float(np.median(np.abs(sub - np.float32(s)))), float(np.median(np.abs(plain - np.float32(s))))
    print("s=%.2f noise=%.2f: median |flow - s| integer %.4f refined %.4f ratio %.3f" % (s, noise, e_int, e_sub, e_sub / e_int))
    assert e_sub <= 0.5 * e_int


@pytest.mark.parametrize("s", [0.4, 13.6])
def test_matcher_accuracy_at_the_window_edge_is_the_integer(dfe, cuda, s):
    """A true flow within half a row of the window's edge: the minimum sits on the edge cell in nearly every pixel, where the rule
    gives off = 0 (a neighbour lies outside the window)."""
    in1, in2 = _shifted_features(s, 0.0)
    sub, _ = run_match(dfe, cuda, "dfe_radial_match_subpixel_f32", in1, in2, 96, 15, False, 0)
    plain, _ = run_match(dfe, cuda, "dfe_radial_match_argmin_f32", in1, in2, 96, 15, False, 0)
    edge = (plain == 0) | (plain == 14)
    print("s=%.1f: minimum on the window's edge in %.1f %% of the pixels" % (s, 100 * edge.mean()))
    assert edge.mean() > 0.94
    assert np.array_equal(sub[edge], plain[edge])


# ------------------------------------------------------------------ end to end: a planted zoom about the epipole
def _zoom_pair(H, W, a, seed, sm=5, C=3):
    """frame1(c + (1 + a)(p - c)) = frame0(p): frame0 a box-smoothed byte texture, frame1 its bilinear resampling rounded to bytes."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(C, H + sm - 1, W + sm - 1)).astype(np.float64)
    s = np.zeros((C, H, W))
    for i in range(sm):
        for j in range(sm):
            s += base[:, i:i + H, j:j + W]
    s /= sm * sm
    f0 = np.round((s - s.min()) / (s.max() - s.min()) * 255)
    cx, cy = W / 2 + 17, H / 2 - 9
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sy, sx = cy + (yy - cy) / (1 + a), cx + (xx - cx) / (1 + a)
    y0, x0 = np.clip(np.floor(sy).astype(int), 0, H - 2), np.clip(np.floor(sx).astype(int), 0, W - 2)
    wy, wx = sy - y0, sx - x0
    f1 = (1 - wy) * ((1 - wx) * f0[:, y0, x0] + wx * f0[:, y0, x0 + 1]) + wy * ((1 - wx) * f0[:, y0 + 1, x0] + wx * f0[:, y0 + 1, x0 + 1])
    return (f0 / 255).astype(np.float32), (np.round(f1) / 255).astype(np.float32), (cx, cy)


def test_end_to_end_zoom_depth_is_closer_with_subpixel(dfe, cuda):
    """A zoom by 1 + a about the epipole is a polar shift of a * i rows at polar row i (alpha_polar = 1), i.e. one constant depth.  The
    features of matcher row y are centred on polar row y + (kH - 1) / 2, so the true polar flow there is a (y + 8); the true depth map
    is what the unchanged downstream stages (P2C sample, flow2depth) make of that flow.  Over the pixels with conf = 1 and a finite
    (not clamped to infty) depth in all three maps, the median relative depth error of the sub-pixel path is below the integer
    path's.  CPU prototype on the oracle composition (180 x 320 frames, polar 200 x 200, a = 12 / 177, seed 0): integer 0.0356,
    sub-pixel 0.0194; on the MI355X: see DESIGN.md section 4.21."""
    hImg, wImg, hIn, wIn = 180, 320, 200, 200
    layers = [[3, 1, 17, 5], [5, 17, 1, 10]]
    networkp = dict(hImg=hImg, wImg=wImg, hInput=hIn, wInput=wIn, hWin=15, layers=layers)
    net = dfe.getTesterNetwork(networkp, device=cuda, generator=torch.Generator().manual_seed(0))
    hm, hOut, wOut = dfe.radial_out_shape(networkp)
    a = 12.0 / (hm - 1 + 8)
    f0, f1, e2 = _zoom_pair(hImg, wImg, a, seed=0)
    res = {sp: dfe.radialFlowDepth(networkp, net, T(f0, cuda), T(f1, cuda), e2, alpha_polar=1.0, subpixel=sp) for sp in (False, True)}
    true_pf = (np.float32(a) * (np.arange(hm, dtype=np.float32) + 8))[:, None].repeat(wIn, 1)
    np2 = dict(networkp, hKernel=17, wKernel=17)
    cart = dfe.cartesian2polar(T(true_pf, cuda), dfe.getP2CMaskOF(np2, e2, 1.0, device=cuda))
    kout = dfe.getKOutput(np2)
    dt, ct = (t.cpu().numpy() for t in dfe.flow2depth(np2, cart, (e2[0] * kout, e2[1] * kout), 0.65))
    di, ci = res[False]["depth"].cpu().numpy(), res[False]["confs"].cpu().numpy()
    ds, cs = res[True]["depth"].cpu().numpy(), res[True]["confs"].cpu().numpy()
    m = (ct == 1) & (ci == 1) & (cs == 1) & (dt > 0) & (dt < 1) & (di < 1) & (ds < 1)
    assert m.mean() > 0.5
    e_int, e_sub = float(np.median(np.abs(di - dt)[m] / dt[m])), float(np.median(np.abs(ds - dt)[m] / dt[m]))
    pfi, pfs = res[False]["polar_flow"].cpu().numpy(), res[True]["polar_flow"].cpu().numpy()
    print("zoom a=%.5f: %d pixels; median relative depth error integer %.4f sub-pixel %.4f; median polar |flow - true| integer %.3f sub-pixel %.3f" % (
        a, int(m.sum()), e_int, e_sub, float(np.median(np.abs(pfi - true_pf))), float(np.median(np.abs(pfs - true_pf)))))
    assert e_sub < e_int
