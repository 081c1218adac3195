"""Sub-pixel flow of the single-scale step (dfe_flow_depth_pair_subpixel_f32 / _u8, dfe_flow_refine_subpixel_f32; include/dfe.h) against a
vectorised numpy reference of the definition: the five costs per pixel recomputed exactly (int64 on byte-valued frames, float64 otherwise)
at the arg-min cell dfe_ssd_flow_f32 picks, then the parabola rule in fp32, in the stated order.  Plus the accuracy the refinement is for:
end-point error on sub-pixel translations and depth error under a zoom, against the integer step."""

import numpy as np
import pytest
import torch

DFE_E_ARG, DFE_E_SHAPE = -1, -2


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def _texture(C_, H, W, rng, pad):
    """5x5 box-smoothed uniform byte noise on a canvas `pad` pixels larger on every side (float64, not rounded)."""
    base = rng.integers(0, 256, size=(C_, H + 2 * pad + 4, W + 2 * pad + 4)).astype(np.float64)
    sm = np.zeros((C_, H + 2 * pad, W + 2 * pad))
    for i in range(5):
        for j in range(5):
            sm += base[:, i : i + H + 2 * pad, j : j + W + 2 * pad]
    return sm / 25.0


def _bilinear(tex, py, px):
    """tex [C][h][w] sampled at (py, px) (arrays of one shape, inside the canvas)."""
    y0, x0 = np.floor(py).astype(np.int64), np.floor(px).astype(np.int64)
    wy, wx = py - y0, px - x0
    t = tex
    return (t[:, y0, x0] * (1 - wy) * (1 - wx) + t[:, y0, x0 + 1] * (1 - wy) * wx + t[:, y0 + 1, x0] * wy * (1 - wx)
            + t[:, y0 + 1, x0 + 1] * wy * wx)


def warped_pair(H, W, flow_fn, C_=3, seed=0, sigma=2.0):
    """Byte-valued float32 frames with frame1(p + flow(p)) = frame0(p): frame0 = texture, frame1(q) = texture(q - flow) with the flow given
    as an inverse map q -> q - flow, both with N(0, sigma) noise, rounded and clipped to bytes."""
    rng = np.random.default_rng(seed)
    pad = 24
    tex = _texture(C_, H, W, rng, pad)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f0 = tex[:, pad : pad + H, pad : pad + W]
    sy, sx = flow_fn(yy, xx)   # the frame-0 position that lands on q
    f1 = _bilinear(tex, sy + pad, sx + pad)
    out = []
    for f in (f0, f1):
        out.append(np.ascontiguousarray(np.clip(np.round(f + rng.standard_normal(f.shape) * sigma), 0, 255), np.float32))
    return out[0], out[1]


def translation(dy, dx):
    return lambda yy, xx: (yy - dy, xx - dx)


def zoom(a, cx, cy):
    """flow(p) = a (p - c): frame1(c + (1 + a)(p - c)) = frame0(p)."""
    return lambda yy, xx: (cy + (yy - cy) / (1 + a), cx + (xx - cx) / (1 + a))


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def ref_costs(f0, f1, idx, kh, kw, hWin, wWin, exact):
    """The five costs per output pixel at the arg-min cell of idx [Ho][Wo] (1-based): c0, (x-1, x+1), (y-1, y+1); int64 on byte-valued
    frames (exact), float64 otherwise.  Neighbours outside the window are evaluated at the centre cell (the rule ignores them)."""
    C_, H, W = f0.shape
    Ho, Wo = H - kh + 1 - hWin + 1, W - kw + 1 - wWin + 1
    dt = np.int64 if exact else np.float64
    a, b = f0.astype(dt), f1.astype(dt).reshape(C_, -1)
    id0 = idx.astype(np.int64) - 1
    r, s = id0 // wWin, id0 % wWin
    inx, iny = (s >= 1) & (s + 1 < wWin), (r >= 1) & (r + 1 < hWin)
    oy, ox = (hWin - 1) // 2, (wWin - 1) // 2
    yy, xx = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    cells = [(r, s), (r, np.where(inx, s - 1, s)), (r, np.where(inx, s + 1, s)), (np.where(iny, r - 1, r), s), (np.where(iny, r + 1, r), s)]
    out = []
    for rr, ss in cells:
        base = (yy + rr) * W + xx + ss
        acc = np.zeros((Ho, Wo), dt)
        for c in range(C_):
            for u in range(kh):
                for v in range(kw):
                    d = a[c, oy + u : oy + u + Ho, ox + v : ox + v + Wo] - b[c][base + u * W + v]
                    acc += d * d
        out.append(acc)
    return out, (r - oy, s - ox), (iny, inx)


def rule(cm, c0, cp, inside, ftype=np.float32):
    cm, c0, cp = (np.asarray(x).astype(ftype) for x in (cm, c0, cp))
    den = (cm - c0) + (cp - c0)
    with np.errstate(divide="ignore", invalid="ignore"):
        off = (cm - cp) / (ftype(2) * den)
    off = np.clip(off, ftype(-0.5), ftype(0.5)).astype(ftype)
    return np.where(inside & (den > 0), off, ftype(0)).astype(ftype), den


def ref_refine(f0, f1, idx, kh, kw, hWin, wWin, exact=True, ftype=np.float32):
    (c0, xm, xp, ym, yp), (dy, dx), (iny, inx) = ref_costs(f0, f1, idx, kh, kw, hWin, wWin, exact)
    oy, deny = rule(ym, c0, yp, iny, ftype)
    ox, denx = rule(xm, c0, xp, inx, ftype)
    fy, fx = (dy.astype(ftype) + oy).astype(ftype), (dx.astype(ftype) + ox).astype(ftype)
    return fy, fx, dict(deny=deny, denx=denx, ym=ym, yp=yp, xm=xm, xp=xp, iny=iny, inx=inx)


# ---- device calls ------------------------------------------------------------------------------------------------------------------
def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def pair(dfe, cuda, f0, f1, k, hWin, wWin, foe, subpixel, thr=0.21, novol=None, u8_scale=None, depth=True):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = f0.shape
    flow = torch.full((2, H, W), -7.0, device=cuda)
    sc, dd, cc = (torch.full((H, W), -7.0, device=cuda) for _ in range(3))
    dp, cp = (dd.data_ptr(), cc.data_ptr()) if depth else (None, None)
    if novol is not None:
        ctx.set_option("cv_novol", novol)
    try:
        if u8_scale is None:
            t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
            fn = lib.dfe_flow_depth_pair_subpixel_f32 if subpixel else lib.dfe_flow_depth_pair_f32
            ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, k, hWin, wWin, foe[0], foe[1], thr, flow.data_ptr(), sc.data_ptr(), dp, cp))
        else:
            # byte frames at an odd address (the conversion's unaligned path)
            n = f0.size
            buf = torch.zeros(2 * n + 2, dtype=torch.uint8, device=cuda)
            buf[1 : n + 1] = _dev(cuda, f0.astype(np.uint8).ravel())
            buf[n + 2 :] = _dev(cuda, f1.astype(np.uint8).ravel())
            fn = lib.dfe_flow_depth_pair_subpixel_u8 if subpixel else lib.dfe_flow_depth_pair_u8
            ctx.check(fn(ctx.handle, buf.data_ptr() + 1, buf.data_ptr() + n + 2, C_, H, W, k, hWin, wWin, foe[0], foe[1], thr, u8_scale, flow.data_ptr(),
                         sc.data_ptr(), dp, cp))
        torch.cuda.synchronize()
    finally:
        if novol is not None:
            ctx.set_option("cv_novol", None)
    return flow.cpu().numpy(), sc.cpu().numpy(), dd.cpu().numpy(), cc.cpu().numpy()


def ssd_idx(dfe, cuda, f0, f1, kh, kw, hWin, wWin):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = f0.shape
    Ho, Wo = H - kh + 1 - hWin + 1, W - kw + 1 - wWin + 1
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    idx = torch.full((Ho, Wo), -7, dtype=torch.int64, device=cuda)
    ctx.check(lib.dfe_ssd_flow_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, kh, kw, hWin, wWin, 0.21, idx.data_ptr(), None, None, None, None,
                                   None))
    torch.cuda.synchronize()
    return idx


def refine(dfe, cuda, f0, f1, idx, kh, kw, hWin, wWin, fill=-7.0):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = f0.shape
    Ho, Wo = idx.shape
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    fy, fx = (torch.full((Ho, Wo), fill, device=cuda) for _ in range(2))
    ctx.check(lib.dfe_flow_refine_subpixel_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, kh, kw, hWin, wWin, idx.data_ptr(), fy.data_ptr(),
                                               fx.data_ptr(), Wo, 0, 0))
    torch.cuda.synchronize()
    return fy.cpu().numpy(), fx.cpu().numpy()


def to_depth(dfe, cuda, flow, foe):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    _, H, W = flow.shape
    t = _dev(cuda, flow)
    d, c = (torch.empty((H, W), device=cuda) for _ in range(2))
    ctx.check(lib.dfe_flow_to_depth_cartesian(ctx.handle, t.data_ptr(), H, W, foe[0], foe[1], 0, d.data_ptr(), c.data_ptr()))
    torch.cuda.synchronize()
    return d.cpu().numpy(), c.cpu().numpy()


def _geom(H, W, k, hWin, wWin):
    Ho, Wo = H - k + 1 - hWin + 1, W - k + 1 - wWin + 1
    return Ho, Wo, (H - Ho) // 2, (W - Wo) // 2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1. bit-exact on byte-valued frames --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W,k,hWin,wWin", [(480, 640, 7, 33, 33), (101, 157, 5, 10, 13), (96, 130, 3, 9, 12)])
def test_bit_exact_on_byte_frames(dfe, cuda, H, W, k, hWin, wWin):
    f0, f1 = warped_pair(H, W, zoom(0.02, W / 2 + 23, H / 2 - 11), seed=1)
    foe = (W / 2 + 23.0, H / 2 - 11.0)
    Ho, Wo, pt, pl = _geom(H, W, k, hWin, wWin)
    idx = ssd_idx(dfe, cuda, f0, f1, k, k, hWin, wWin).cpu().numpy()
    efy, efx, _ = ref_refine(f0, f1, idx, k, k, hWin, wWin, exact=True)
    plain = pair(dfe, cuda, f0, f1, k, hWin, wWin, foe, subpixel=False)
    runs = [pair(dfe, cuda, f0, f1, k, hWin, wWin, foe, subpixel=True, novol=nv) for nv in (1, 0)]
    for flow, sc, dd, cc in runs:
        gy, gx = flow[0, pt : pt + Ho, pl : pl + Wo], flow[1, pt : pt + Ho, pl : pl + Wo]
        assert np.array_equal(_bits(gy), _bits(efy)), "fy: %d pixels differ" % np.count_nonzero(gy != efy)
        assert np.array_equal(_bits(gx), _bits(efx)), "fx: %d pixels differ" % np.count_nonzero(gx != efx)
        assert np.array_equal(_bits(sc), _bits(plain[1])), "scores moved"
        assert np.abs(flow - plain[0]).max() <= 0.5
        inner = np.zeros((H, W), bool)
        inner[pt : pt + Ho, pl : pl + Wo] = True
        assert not flow[:, ~inner].any() and not sc[~inner].any(), "border not zero"
        ed, ec = to_depth(dfe, cuda, flow, foe)
        assert np.array_equal(_bits(dd), _bits(ed)) and np.array_equal(_bits(cc), _bits(ec)), "depth / confidence differ from the formula"
        assert np.count_nonzero(flow != plain[0]) > 0.5 * Ho * Wo, "hardly any pixel refined"
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(_bits(a), _bits(b)), "cv_novol changed the sub-pixel outputs"


# ---- 2. non-integer frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_non_integer_frames_match_float64(dfe, cuda):
    H, W, k, win = 240, 320, 7, 33
    f0, f1 = warped_pair(H, W, translation(2.3, -4.7), seed=2)
    f0, f1 = f0 / np.float32(255), f1 / np.float32(255)
    Ho, Wo, pt, pl = _geom(H, W, k, win, win)
    idx = ssd_idx(dfe, cuda, f0, f1, k, k, win, win).cpu().numpy()
    efy, efx, aux = ref_refine(f0, f1, idx, k, k, win, win, exact=False, ftype=np.float64)
    flow = pair(dfe, cuda, f0, f1, k, win, win, (W / 2, H / 2), subpixel=True)[0]
    gy, gx = flow[0, pt : pt + Ho, pl : pl + Wo], flow[1, pt : pt + Ho, pl : pl + Wo]
    for g, e, den, cm, cp in ((gy, efy, aux["deny"], aux["ym"], aux["yp"]), (gx, efx, aux["denx"], aux["xm"], aux["xp"])):
        ok = den >= 1e-2 * np.maximum(cm, cp)
        assert np.count_nonzero(~ok) < 0.01 * ok.size, "%d of %d pixels excluded" % (np.count_nonzero(~ok), ok.size)
        err = np.abs(g.astype(np.float64) - e)[ok]
        assert err.max() <= 2e-3, "max error %.3g px" % err.max()
    stand = refine(dfe, cuda, f0, f1, torch.from_numpy(idx).to(cuda), k, k, win, win)
    assert np.array_equal(_bits(stand[0]), _bits(gy)) and np.array_equal(_bits(stand[1]), _bits(gx))


# ---- 3. uint8 entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1.0 / 255])
def test_u8_entry_equals_f32_on_converted_frames(dfe, cuda, scale):
    H, W, k, win = 200, 260, 7, 33
    f0, f1 = warped_pair(H, W, translation(-1.4, 3.6), seed=3)
    foe = (100.0, 90.0)
    got = pair(dfe, cuda, f0, f1, k, win, win, foe, subpixel=True, u8_scale=scale)
    s = np.float32(scale)
    want = pair(dfe, cuda, f0.astype(np.uint8).astype(np.float32) * s, f1.astype(np.uint8).astype(np.float32) * s, k, win, win, foe, subpixel=True)
    for a, b in zip(got, want):
        assert np.array_equal(_bits(a), _bits(b))


# ---- 4. stand-alone op -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_standalone_refine_equals_one_call(dfe, cuda):
    H, W, k, hWin, wWin = 150, 210, 7, 17, 21
    f0, f1 = warped_pair(H, W, translation(1.7, -2.2), seed=4)
    Ho, Wo, pt, pl = _geom(H, W, k, hWin, wWin)
    idx = ssd_idx(dfe, cuda, f0, f1, k, k, hWin, wWin)
    fy, fx = refine(dfe, cuda, f0, f1, idx, k, k, hWin, wWin)
    flow = pair(dfe, cuda, f0, f1, k, hWin, wWin, (W / 2, H / 2), subpixel=True)[0]
    assert np.array_equal(_bits(fy), _bits(flow[0, pt : pt + Ho, pl : pl + Wo]))
    assert np.array_equal(_bits(fx), _bits(flow[1, pt : pt + Ho, pl : pl + Wo]))
    # indices outside 1..hWin*wWin leave the pixel alone
    bad = idx.clone()
    bad[0, :5] = 0
    bad[1, :5] = -3
    bad[2, :5] = hWin * wWin + 1
    gy, gx = refine(dfe, cuda, f0, f1, bad, k, k, hWin, wWin)
    assert (gy[:3, :5] == -7).all() and (gx[:3, :5] == -7).all()
    assert np.array_equal(gy[3:], fy[3:]) and np.array_equal(gx[:, 5:], fx[:, 5:])
    # pitch / pad addressing as dfe_flow_tail's
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    py, px = (torch.full((H, W), -7.0, device=cuda) for _ in range(2))
    ctx.check(lib.dfe_flow_refine_subpixel_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, k, k, hWin, wWin, idx.data_ptr(), py.data_ptr(),
                                               px.data_ptr(), W, pt, pl))
    py, px = py.cpu().numpy(), px.cpu().numpy()
    assert np.array_equal(py[pt : pt + Ho, pl : pl + Wo], fy) and np.array_equal(px[pt : pt + Ho, pl : pl + Wo], fx)
    py[pt : pt + Ho, pl : pl + Wo] = -7
    assert (py == -7).all()


@pytest.mark.gpu
def test_standalone_refine_rectangular_patch(dfe, cuda):
    # a 5 x 7 patch: the kernel's any-patch form
    H, W, kh, kw, hWin, wWin = 90, 140, 5, 7, 11, 15
    f0, f1 = warped_pair(H, W, translation(-2.6, 3.3), seed=10)
    idx = ssd_idx(dfe, cuda, f0, f1, kh, kw, hWin, wWin)
    fy, fx = refine(dfe, cuda, f0, f1, idx, kh, kw, hWin, wWin)
    efy, efx, _ = ref_refine(f0, f1, idx.cpu().numpy(), kh, kw, hWin, wWin)
    assert np.array_equal(_bits(fy), _bits(efy)) and np.array_equal(_bits(fx), _bits(efx))
    assert np.abs(fy - efy.round()).max() <= 0.5


# ---- 5. edge rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_window_edge_and_flat_block_give_zero_offset(dfe, cuda):
    H, W, k, win = 160, 220, 7, 17
    half = (win - 1) // 2
    # left half moves by exactly (+3, +half): its arg-min lies on the window's right edge; the right half moves by (-half, -1.5)
    f0, f1a = warped_pair(H, W, translation(3, half), seed=6, sigma=0.0)
    _, f1b = warped_pair(H, W, translation(-half, -1.5), seed=6, sigma=0.0)
    f1 = f1a.copy()
    f1[:, :, W // 2 :] = f1b[:, :, W // 2 :]
    # a flat block in both frames, larger than any patch plus window around its centre pixels
    f0[:, 40:120, 60:100] = 77.0
    f1[:, 40:120, 60:100] = 77.0
    Ho, Wo, pt, pl = _geom(H, W, k, win, win)
    idx = ssd_idx(dfe, cuda, f0, f1, k, k, win, win).cpu().numpy()
    flow, sc, dd, cc = pair(dfe, cuda, f0, f1, k, win, win, (W / 2, H / 2), subpixel=True)
    plain = pair(dfe, cuda, f0, f1, k, win, win, (W / 2, H / 2), subpixel=False)[0]
    for a in (flow, sc, dd, cc):
        assert np.isfinite(a).all()
    gy, gx = flow[0, pt : pt + Ho, pl : pl + Wo], flow[1, pt : pt + Ho, pl : pl + Wo]
    iy, ix = plain[0, pt : pt + Ho, pl : pl + Wo], plain[1, pt : pt + Ho, pl : pl + Wo]
    id0 = idx - 1
    r, s = id0 // win, id0 % win
    xedge, yedge = (s == 0) | (s == win - 1), (r == 0) | (r == win - 1)
    assert np.count_nonzero(xedge) > 1000 and np.count_nonzero(yedge) > 1000
    assert np.array_equal(gx[xedge], ix[xedge]) and np.array_equal(gy[yedge], iy[yedge])
    # output pixels whose patch and whole window lie inside the flat block: every cost 0, no curvature
    flat = np.zeros((Ho, Wo), bool)
    flat[40 : 120 - (k - 1) - (win - 1), 60 : 100 - (k - 1) - (win - 1)] = True
    assert flat.any()
    assert (gx[flat] == 0).all() and (gy[flat] == 0).all()
    efy, efx, _ = ref_refine(f0, f1, idx, k, k, win, win)
    assert np.array_equal(_bits(gy), _bits(efy)) and np.array_equal(_bits(gx), _bits(efx))


# ---- 6. accuracy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dy,dx", [(2.3, -4.7), (0.5, 1.25)])
def test_translation_end_point_error(dfe, cuda, dy, dx):
    H, W, k, win = 160, 200, 7, 17
    f0, f1 = warped_pair(H, W, translation(dy, dx), seed=7)
    Ho, Wo, pt, pl = _geom(H, W, k, win, win)
    epe = []
    for sub in (False, True):
        flow = pair(dfe, cuda, f0, f1, k, win, win, (W / 2, H / 2), subpixel=sub)[0][:, pt : pt + Ho, pl : pl + Wo]
        epe.append(float(np.median(np.hypot(flow[0] - dy, flow[1] - dx))))
    print("translation (%g, %g): median end-point error integer %.3f px, sub-pixel %.3f px" % (dy, dx, epe[0], epe[1]))
    assert epe[1] <= 0.2 and epe[1] <= 0.5 * epe[0], epe


@pytest.mark.gpu
def test_zoom_depth_error(dfe, cuda):
    H, W, k, win, a = 240, 320, 7, 17, 0.03
    cx, cy = 140.0, 110.0
    f0, f1 = warped_pair(H, W, zoom(a, cx, cy), seed=8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Ho, Wo, pt, pl = _geom(H, W, k, win, win)
    sel = np.zeros((H, W), bool)
    sel[pt : pt + Ho, pl : pl + Wo] = True
    sel &= np.hypot(yy - cy, xx - cx) > 60
    err = []
    for sub in (False, True):
        depth = pair(dfe, cuda, f0, f1, k, win, win, (cx, cy), subpixel=sub)[2]
        err.append(float(np.median(np.abs(depth[sel] * a - 1.0))))
    print("zoom %.2f: median relative depth error integer %.4f, sub-pixel %.4f" % (a, err[0], err[1]))
    assert err[1] <= 0.5 * err[0], err


# ---- 7. Python -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_wrappers_match_the_entries(dfe, cuda):
    H, W, k, win = 120, 170, 7, 17
    f0, f1 = warped_pair(H, W, translation(1.3, 2.6), seed=9)
    foe = (80.0, 50.0)
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    for sub in (False, True):
        got = dfe.flowDepthPair(t0, t1, k, win, win, foe, subpixel=sub)
        want = pair(dfe, cuda, f0, f1, k, win, win, foe, subpixel=sub)
        for key, b in zip(("flow", "scores", "depth", "depth_conf"), want):
            assert np.array_equal(_bits(got[key].cpu().numpy()), _bits(b)), (sub, key)
    got = dfe.flowDepthPair(_dev(cuda, f0.astype(np.uint8)), _dev(cuda, f1.astype(np.uint8)), k, win, win, foe, subpixel=True, scale=1.0 / 255)
    want = pair(dfe, cuda, f0, f1, k, win, win, foe, subpixel=True, u8_scale=1.0 / 255)
    for key, b in zip(("flow", "scores", "depth", "depth_conf"), want):
        assert np.array_equal(_bits(got[key].cpu().numpy()), _bits(b)), ("u8", key)
    idx = ssd_idx(dfe, cuda, f0, f1, k, k, win, win)
    fy, fx = dfe.refineFlowSubpixel(t0, t1, idx, k, k, win, win)
    ey, ex = refine(dfe, cuda, f0, f1, idx, k, k, win, win)
    assert np.array_equal(_bits(fy.cpu().numpy()), _bits(ey)) and np.array_equal(_bits(fx.cpu().numpy()), _bits(ex))


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_codes(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, k, win = 60, 70, 7, 17
    t = torch.zeros((3, H, W), device=cuda)
    fl = torch.zeros((2, H, W), device=cuda)
    o = torch.zeros((H, W), device=cuda)
    p, f, op = t.data_ptr(), fl.data_ptr(), o.data_ptr()
    for fn in (lib.dfe_flow_depth_pair_subpixel_f32,):
        assert fn(ctx.handle, None, p, 3, H, W, k, win, win, 1.0, 1.0, 0.21, f, op, op, op) == DFE_E_ARG
        assert fn(ctx.handle, p, p, 3, H, W, k, win, win, 1.0, 1.0, 0.21, None, op, op, op) == DFE_E_ARG
        assert fn(ctx.handle, p, p, 3, H, W, k, win, win, 1.0, 1.0, 0.21, f, op, op, None) == DFE_E_ARG
        assert fn(ctx.handle, p, p, 3, 20, W, k, win, win, 1.0, 1.0, 0.21, f, op, op, op) == DFE_E_SHAPE
        assert fn(None, p, p, 3, H, W, k, win, win, 1.0, 1.0, 0.21, f, op, op, op) == DFE_E_ARG
    b = torch.zeros(3 * H * W, dtype=torch.uint8, device=cuda).data_ptr()
    fn = lib.dfe_flow_depth_pair_subpixel_u8
    assert fn(ctx.handle, None, b, 3, H, W, k, win, win, 1.0, 1.0, 0.21, 1.0, f, op, op, op) == DFE_E_ARG
    assert fn(ctx.handle, b, b, 3, H, W, k, win, win, 1.0, 1.0, 0.21, 1.0, f, op, None, op) == DFE_E_ARG
    assert fn(ctx.handle, b, b, 3, 20, W, k, win, win, 1.0, 1.0, 0.21, 1.0, f, op, op, op) == DFE_E_SHAPE
    Ho, Wo = H - k - win + 2, W - k - win + 2
    idx = torch.ones((Ho, Wo), dtype=torch.int64, device=cuda).data_ptr()
    fn = lib.dfe_flow_refine_subpixel_f32
    assert fn(ctx.handle, p, p, 3, H, W, k, k, win, win, None, op, op, Wo, 0, 0) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, H, W, k, k, win, win, idx, None, op, Wo, 0, 0) == DFE_E_ARG
    assert fn(ctx.handle, p, None, 3, H, W, k, k, win, win, idx, op, op, Wo, 0, 0) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, H, W, k, 0, win, win, idx, op, op, Wo, 0, 0) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, 22, W, k, k, win, win, idx, op, op, Wo, 0, 0) == DFE_E_SHAPE
    assert fn(ctx.handle, p, p, 3, H, W, k, k, win, win, idx, op, op, Wo - 1, 0, 0) == DFE_E_SHAPE
    assert dfe.lib().dfe_last_error(ctx.handle)
    torch.cuda.synchronize()
    with pytest.raises(dfe.DfeError):
        dfe.flowDepthPair(t[:, :20], t[:, :20], k, win, win, (1.0, 1.0))
