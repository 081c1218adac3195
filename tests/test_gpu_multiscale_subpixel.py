"""Sub-pixel flow of the raw-patch pyramid matcher (dfe_multiscale_flow_pair_subpixel_f32 / _u8, dfe_multiscale_refine_subpixel_f32;
include/dfe.h) against a numpy reference of the definition: the class id decoded to (scale, cell), the five costs
taken from the ORACLE's per-scale volumes at the scale's pixel, the parabola rule of tests/test_gpu_subpixel.py in fp32 in the stated
order.  "Bitwise" tests run on frames whose every cost at every scale is exactly representable (the test asserts that of its own
input), so that any summation order gives the oracle's bits.  Plus float frames against float64 costs, and the accuracy the refinement
is for."""

import functools

import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import refpath as rp
from tests.test_gpu_subpixel import _bits, rule, translation, warped_pair, zoom

pytestmark = pytest.mark.gpu
DFE_E_ARG, DFE_E_SHAPE = -1, -2


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def ring_widths(maxw, ratios):
    return [0] + [int(np.floor(maxw * (ratios[i] - ratios[i - 1]) / (2.0 * ratios[i]) + 0.5)) for i in range(1, len(ratios))]


def nclasses(maxh, maxw, ratios):
    return maxh * maxw + sum(2 * d * maxw + 2 * (maxh - 2 * d) * d for d in ring_widths(maxw, ratios)[1:])


def decode(idx, maxh, maxw, ratios):
    """1-based class ids -> (scale, cell row a, cell column b, valid): scale 1 the whole window row-major, a coarser scale its ring of
    width d in the blocks top, left, right, bottom (x2yxMultiNumber, opticalflow_model_multiscale.lua:83-132)."""
    idx = np.asarray(idx, np.int64)
    s_, a_, b_ = (np.zeros(idx.shape, np.int64) for _ in range(3))
    valid = np.zeros(idx.shape, bool)
    base = 0
    for s, d in enumerate(ring_widths(maxw, ratios)):
        if s == 0:
            cells = [(a, b) for a in range(maxh) for b in range(maxw)]
        else:
            cells = ([(a, b) for a in range(d) for b in range(maxw)] + [(a, b) for a in range(d, maxh - d) for b in range(d)]
                     + [(a, b) for a in range(d, maxh - d) for b in range(maxw - d, maxw)] + [(a, b) for a in range(maxh - d, maxh) for b in range(maxw)])
        tab = np.array(cells, np.int64)
        m = (idx - 1 >= base) & (idx - 1 < base + len(cells))
        n = (idx - 1 - base)[m]
        s_[m], a_[m], b_[m], valid[m] = s, tab[n, 0], tab[n, 1], True
        base += len(cells)
    return s_, a_, b_, valid


def ref_refine(vols, idx, maxh, maxw, ratios, ftype=np.float32):
    """The definition on per-scale volumes vols[s] [Hs][Ws][maxh][maxw]: -> flow [2][H][W] (ftype; NaN where idx is no class), the integer
    flow, the offsets in cells, and per axis (inside, den, cm, c0, cp)."""
    H, W = idx.shape
    s_, a_, b_, valid = decode(idx, maxh, maxw, ratios)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r_ = np.array(ratios, np.int64)[s_]
    cost = {k: np.zeros((H, W), vols[0].dtype) for k in ("c0", "ym", "yp", "xm", "xp")}
    iny, inx = (a_ >= 1) & (a_ + 1 < maxh), (b_ >= 1) & (b_ + 1 < maxw)
    for s, r in enumerate(ratios):
        m = valid & (s_ == s)
        ys, xs, a, b = yy[m] // r, xx[m] // r, a_[m], b_[m]
        v = vols[s]
        cost["c0"][m] = v[ys, xs, a, b]
        cost["ym"][m] = v[ys, xs, np.where(iny[m], a - 1, a), b]
        cost["yp"][m] = v[ys, xs, np.where(iny[m], a + 1, a), b]
        cost["xm"][m] = v[ys, xs, a, np.where(inx[m], b - 1, b)]
        cost["xp"][m] = v[ys, xs, a, np.where(inx[m], b + 1, b)]
    offy, deny = rule(cost["ym"], cost["c0"], cost["yp"], iny, ftype)
    offx, denx = rule(cost["xm"], cost["c0"], cost["xp"], inx, ftype)
    chh, chw = (maxh + 1) // 2, (maxw + 1) // 2
    iy, ix = (a_ + 1 - chh) * r_, (b_ + 1 - chw) * r_
    rf = r_.astype(ftype)
    fy = (iy.astype(ftype) + (rf * offy).astype(ftype)).astype(ftype)
    fx = (ix.astype(ftype) + (rf * offx).astype(ftype)).astype(ftype)
    flow = np.stack([np.where(valid, fy, np.nan), np.where(valid, fx, np.nan)]).astype(ftype)
    aux = dict(valid=valid, scale=s_, r=r_, iy=iy, ix=ix, offy=offy, offx=offx,
               y=(iny, deny, cost["ym"], cost["c0"], cost["yp"]), x=(inx, denx, cost["xm"], cost["c0"], cost["xp"]))
    return flow, aux


# ---- frames and their oracle chain, computed once per shape ---------------------------------------------------------------------------
def exact_pair(H, W, C_=3, seed=1):
    f0, f1 = warped_pair(H, W, zoom(0.1, 70, 40), C_=C_, seed=seed)
    return tuple(np.ascontiguousarray(np.floor(f / 16) / 16, np.float32) for f in (f0, f1))


@functools.lru_cache(maxsize=None)
def exact_case(H, W, C_, k, mh, mw, ratios):
    """Frames floor(byte / 16) / 16 and their oracle chain; asserts the property the bitwise tests rest on: every cost at every scale times
    256 r^4 is an integer below 2^24, so that every partial sum in any order is exact in fp32."""
    f0, f1 = exact_pair(H, W, C_)
    o = rp.multiscale_flow_oracle(f0, f1, k, mh, mw, list(ratios))
    for r, v in zip(ratios, o["vols"]):
        m = v.astype(np.float64) * 256 * r ** 4
        assert np.array_equal(m, np.round(m)) and m.max() < 2 ** 24, "costs of ratio %d are not exactly representable" % r
        v.setflags(write=False)
    return f0, f1, o


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _rr(ratios):
    from depth_estimation_amd._lib import ratios_array

    return ratios_array(list(ratios))


def standalone(dfe, cuda, f0, f1, k, mh, mw, ratios, idx, fill=-7.0):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = f0.shape
    rr, n = _rr(ratios)
    t0, t1, ti = _dev(cuda, f0), _dev(cuda, f1), _dev(cuda, np.asarray(idx, np.int64))
    flow = torch.full((2, H, W), fill, device=cuda)
    ctx.check(lib.dfe_multiscale_refine_subpixel_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, k, mh, mw, rr, n, ti.data_ptr(), flow.data_ptr()))
    torch.cuda.synchronize()
    return flow.cpu().numpy()


def one_call(dfe, cuda, f0, f1, k, mh, mw, ratios, subpixel, u8_scale=None, want_idx=True, f16_scale=0.0):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = f0.shape
    rr, n = _rr(ratios)
    flow = torch.full((2, H, W), -7.0, device=cuda)
    idx = torch.full((H, W), -7, dtype=torch.int64, device=cuda)
    ip = idx.data_ptr() if want_idx else None
    if u8_scale is None:
        t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
        fn = lib.dfe_multiscale_flow_pair_subpixel_f32 if subpixel else lib.dfe_multiscale_flow_pair_f32
        ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, k, mh, mw, rr, n, flow.data_ptr(), ip))
    else:   # byte frames at an odd address
        m = f0.size
        buf = torch.zeros(2 * m + 2, dtype=torch.uint8, device=cuda)
        buf[1 : m + 1] = _dev(cuda, f0.astype(np.uint8).ravel())
        buf[m + 2 :] = _dev(cuda, f1.astype(np.uint8).ravel())
        fn = lib.dfe_multiscale_flow_pair_subpixel_u8 if subpixel else lib.dfe_multiscale_flow_pair_u8
        ctx.check(fn(ctx.handle, buf.data_ptr() + 1, buf.data_ptr() + m + 2, C_, H, W, k, mh, mw, rr, n, u8_scale, f16_scale, flow.data_ptr(), ip))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), flow.cpu().numpy()


# ---- 1. every class of every scale, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C_,k,win,ratios", [
    (96, 128, 3, 7, 8, (1, 2, 4)),
    (100, 136, 3, 7, 8, (1, 2, 4)),      # ragged tiles
    (40, 56, 3, 7, 8, (1, 2)),
    (36, 52, 1, 5, 4, (1, 2)),           # the any-window path of the matcher, the 5 x 5 form of the kernel
    (40, 56, 3, 3, 8, (1, 2)),           # a 3 x 3 patch: the any-patch form of the kernel
])
def test_every_class_of_every_scale_bitwise(dfe, cuda, H, W, C_, k, win, ratios):
    f0, f1, o = exact_case(H, W, C_, k, win, win, ratios)
    ncls = nclasses(win, win, ratios)
    assert ncls == dfe.lib().dfe_multi_nclasses(win, win, *_rr(ratios))
    if win == 8 and ratios == (1, 2, 4):
        assert ncls == 160
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    # the planted map ((y W + x) 7 mod ncls) + 1; with the ratios {1, 2} ncls is 112 or 28, multiples of 7, and that map would reach
    # one class in seven: 11 there, so that the map still runs through every class
    mult = 7 if ncls % 7 else 11
    idx = ((yy * W + xx) * mult) % ncls + 1
    want, aux = ref_refine(o["vols"], idx, win, win, ratios)
    # the decode itself: the oracle's x2yx_multi
    rc, ey, ex = orc.x2yx_multi(win, win, list(ratios), idx)
    assert rc == 0 and np.array_equal(ey, aux["iy"]) and np.array_equal(ex, aux["ix"])
    # what the planted map covers: every class, 1000 pixels per scale and 100 edge-rule pixels per axis at the frames of 96 x 128 and
    # more; the two small frames have 2240 and 1872 pixels in all, of which the map gives the coarse scale 960 and 802
    floor_scale, floor_edge = (1000, 100) if H * W >= 96 * 128 else (800, 100)
    assert np.unique(idx).size == ncls
    counts = [int(np.count_nonzero(aux["scale"] == s)) for s in range(len(ratios))]
    assert min(counts) >= floor_scale, counts
    if (H, W) == (96, 128):
        assert counts == [4919, 3686, 3683]
    assert np.count_nonzero(~aux["y"][0]) >= floor_edge and np.count_nonzero(~aux["x"][0]) >= floor_edge
    assert np.array_equal(aux["offy"][~aux["y"][0]], np.zeros(np.count_nonzero(~aux["y"][0]), np.float32))
    got = standalone(dfe, cuda, f0, f1, k, win, win, ratios, idx)
    for ax, name in ((0, "fy"), (1, "fx")):
        bad = _bits(got[ax]) != _bits(want[ax])
        assert not bad.any(), "%s: %d pixels differ, first at %s (scales %s)" % (name, np.count_nonzero(bad), np.argwhere(bad)[0], np.unique(aux["scale"][bad]))
    assert np.abs(got[0] - aux["iy"]).max() <= ratios[-1] / 2 and (np.abs(got[0] - aux["iy"]) <= aux["r"] / 2).all()
    assert (np.abs(got[1] - aux["ix"]) <= aux["r"] / 2).all()
    # ids that are no class leave the fill
    bad_idx = idx.copy()
    bad_idx[0, :5], bad_idx[1, :5], bad_idx[2, :5] = 0, -3, ncls + 1
    g2 = standalone(dfe, cuda, f0, f1, k, win, win, ratios, bad_idx)
    assert (g2[:, :3, :5] == -7).all()
    keep = np.ones((H, W), bool)
    keep[:3, :5] = False
    assert np.array_equal(_bits(g2[:, keep]), _bits(got[:, keep]))


# ---- 2. the one-call entry on every path of the matcher ------------------------------------------------------------------------------
def test_one_call_equals_matcher_plus_standalone_bitwise(dfe, cuda):
    H, W, k, win, ratios = 136, 200, 7, 8, (1, 2, 4)
    f0, f1, o = exact_case(H, W, 3, k, win, win, ratios)
    ctx = dfe.get_ctx(0)
    pidx, pflow = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=False)
    assert np.array_equal(pidx, o["idx"])
    want = standalone(dfe, cuda, f0, f1, k, win, win, ratios, pidx)
    ref, aux = ref_refine(o["vols"], pidx, win, win, ratios)
    assert np.array_equal(_bits(want), _bits(ref)), "stand-alone refinement differs from the definition"
    runs = {}
    try:
        for name, opts in (("default", {}), ("volume path", dict(fine_fuse=0)), ("fused finest", dict(fine_fuse=1, mid_fuse=0)),
                           ("fused finest + second", dict(fine_fuse=1, mid_fuse=1)), ("lane <-> cell cascade", dict(cascade_px=0))):
            for key in ("fine_fuse", "mid_fuse", "cascade_px"):
                ctx.set_option(key, opts.get(key))
            runs[name] = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=True)
            assert ctx.last_kernel().startswith("ssd_cv_tiled_fine_kernel") == name.startswith("fused"), (name, ctx.last_kernel())
        ctx.set_option("fine_fuse", 1)
        runs["no idx asked"] = (pidx, one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=True, want_idx=False)[1])
    finally:
        for key in ("fine_fuse", "mid_fuse", "cascade_px"):
            ctx.set_option(key, None)
    for name, (gi, gf) in runs.items():
        assert np.array_equal(gi, pidx), name
        assert np.array_equal(_bits(gf), _bits(want)), "%s: %d values differ" % (name, np.count_nonzero(_bits(gf) != _bits(want)))
    gf = runs["default"][1]
    assert (np.abs(gf - pflow) <= aux["r"][None] / 2).all()
    moved = (gf != pflow).any(axis=0)
    assert np.count_nonzero(moved) > 0.5 * H * W, "hardly any pixel refined"
    # the plain entry after the sub-pixel one, same buffers' shapes: still the integer flow
    assert np.array_equal(one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=False)[1], pflow)


def test_graph_replay_keeps_the_entries_apart(dfe, cuda):
    """With graphs on, a ctx on a real stream replays the one-call as a captured graph keyed by buffers and shape from the third call
    with the same arguments on (the second captures).  The refinement launch is inside the captured region, and the key holds the
    sub-pixel switch: each entry's third call is a replay with its own result, and the other entry called on the SAME buffers right
    after it must not replay that graph.  Both with the caller's idx and without one (the class map in the arena)."""
    H, W, k, win, ratios = 96, 128, 7, 8, (1, 2, 4)
    f0, f1, o = exact_case(H, W, 3, k, win, win, ratios)
    lib = dfe.lib()
    rr, n = _rr(ratios)
    want_idx, want_plain = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=False)     # (default stream: direct launches)
    want_sub = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=True)[1]
    assert not np.array_equal(want_sub, want_plain)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        ctx = dfe.get_ctx(0)                                        # (a new ctx on the side stream: its launches can be captured)
        ctx.set_option("graphs", 1)
        try:
            t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
            flow = torch.empty((2, H, W), device=cuda)
            idx = torch.empty((H, W), dtype=torch.int64, device=cuda)
            entries = {"plain": (lib.dfe_multiscale_flow_pair_f32, want_plain), "subpixel": (lib.dfe_multiscale_flow_pair_subpixel_f32, want_sub)}

            def call(name, ip):
                fn, want = entries[name]
                flow.fill_(-7.0)
                idx.fill_(-7)
                ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, k, win, win, rr, n, flow.data_ptr(), ip))
                ctx.synchronize()
                assert np.array_equal(_bits(flow.cpu().numpy()), _bits(want)), name
                if ip is not None:
                    assert np.array_equal(idx.cpu().numpy(), want_idx), name
                return ctx.last_kernel()

            for ip in (idx.data_ptr(), None):
                for name in ("plain", "subpixel", "plain", "subpixel"):
                    kernels = [call(name, ip) for _ in range(3)]        # direct, capture + launch, replay
                    assert kernels[0] != "multiscale graph" and kernels[2] == "multiscale graph", (name, ip is None, kernels)
                for name in ("plain", "subpixel", "plain", "subpixel"):     # in turn: the key differs every time, no replay
                    assert call(name, ip) != "multiscale graph", (name, ip is None)
        finally:
            ctx.set_option("graphs", None)


# ---- 3. uint8 entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1.0 / 255])
def test_u8_entry_equals_f32_on_converted_frames(dfe, cuda, scale):
    H, W, k, win, ratios = 96, 128, 7, 8, (1, 2, 4)
    f0, f1 = warped_pair(H, W, zoom(0.1, 70, 40), seed=3)
    gi, gf = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=True, u8_scale=scale)
    s = np.float32(scale)
    wi, wf = one_call(dfe, cuda, f0.astype(np.uint8).astype(np.float32) * s, f1.astype(np.uint8).astype(np.float32) * s, k, win, win, ratios, subpixel=True)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gf), _bits(wf))
    assert np.count_nonzero(gf != np.round(gf)) > 0.5 * H * W


def test_u8_entry_with_f16_volumes_refines_its_own_classes(dfe, cuda):
    """f16_scale > 0 under the sub-pixel u8 entry: the matcher stores half volumes, the refinement's costs stay fp32 sums over the
    frames -- the class map of dfe_multiscale_flow_pair_u8 with that f16_scale, refined as the stand-alone entry refines it."""
    H, W, k, win, ratios = 96, 128, 7, 8, (1, 2, 4)
    f0, f1 = warped_pair(H, W, zoom(0.1, 70, 40), seed=3)
    fs = 2.0 ** -8
    pi, pf = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=False, u8_scale=1.0, f16_scale=fs)
    gi, gf = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=True, u8_scale=1.0, f16_scale=fs)
    assert np.array_equal(gi, pi)
    want = standalone(dfe, cuda, f0.astype(np.uint8).astype(np.float32), f1.astype(np.uint8).astype(np.float32), k, win, win, ratios, pi)
    assert np.array_equal(_bits(gf), _bits(want))
    assert np.count_nonzero((gf != pf).any(axis=0)) > 0.5 * H * W


# ---- 4. float frames against float64 costs ------------------------------------------------------------------------------------------
def volumes_f64(f0, f1, k, mh, mw, ratios):
    """Per-scale volumes in float64: box mean, zero pad (hp // 2 top / left, the rest bottom / right), k x k SSD of frame 0's patch at
    (ys + (mh-1)//2, xs + (mw-1)//2) against frame 1's at (ys + a, xs + b) (opticalflow_model_multiscale.lua:136-229)."""
    C_, H, W = f0.shape
    hp, wp = mh - 1 + k - 1, mw - 1 + k - 1
    oy, ox = (mh - 1) // 2, (mw - 1) // 2
    vols = []
    for r in ratios:
        Hs, Ws = H // r, W // r
        pads = []
        for f in (f0, f1):
            d = f.astype(np.float64).reshape(C_, Hs, r, Ws, r).mean(axis=(2, 4))
            p = np.zeros((C_, Hs + hp, Ws + wp))
            p[:, hp // 2 : hp // 2 + Hs, wp // 2 : wp // 2 + Ws] = d
            pads.append(p)
        v = np.zeros((Hs, Ws, mh, mw))
        a0 = pads[0][:, oy : oy + Hs + k - 1, ox : ox + Ws + k - 1]
        for a in range(mh):
            for b in range(mw):
                e = ((a0 - pads[1][:, a : a + Hs + k - 1, b : b + Ws + k - 1]) ** 2).sum(axis=0)
                acc = np.zeros((Hs, Ws))
                for i in range(k):
                    for j in range(k):
                        acc += e[i : i + Hs, j : j + Ws]
                v[:, :, a, b] = acc
        vols.append(v)
    return vols


def test_float_frames_match_float64(dfe, cuda):
    H, W, k, win, ratios = 96, 128, 7, 8, (1, 2, 4)
    f0, f1 = warped_pair(H, W, zoom(0.1, 70, 40), seed=8)
    f0, f1 = f0 / np.float32(255), f1 / np.float32(255)
    gi, gf = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=True)
    vols = volumes_f64(f0, f1, k, win, win, ratios)
    fp32 = [orc.pyramid_scale_volume(f0, f1, r, k, k, win, win) for r in ratios]
    print("fp32 oracle volumes against float64: max difference %.3g" % max(np.abs(a - b).max() for a, b in zip(fp32, vols)))
    _, aux = ref_refine(vols, gi, win, win, ratios, ftype=np.float64)
    assert aux["valid"].all()
    excluded = total = 0
    worst = 0.0
    for g, i_, off, (inside, den, cm, c0, cp) in ((gf[0], aux["iy"], aux["offy"], aux["y"]), (gf[1], aux["ix"], aux["offx"], aux["x"])):
        ok = np.abs(den) >= 1e-3 * np.maximum(np.maximum(cm, c0), cp)
        ok |= ~inside                                 # (the edge rule: off = 0 whatever the costs)
        excluded += np.count_nonzero(~ok)
        total += ok.size
        err = np.abs((g.astype(np.float64) - i_) / aux["r"] - off)[ok]
        worst = max(worst, float(err.max()))
    print("float frames: %d of %d axis samples excluded (%.2f %%), max error %.3g cells" % (excluded, total, 100.0 * excluded / total, worst))
    assert excluded <= 0.01 * total
    assert worst <= 2e-3
    stand = standalone(dfe, cuda, f0, f1, k, win, win, ratios, gi)
    assert np.array_equal(_bits(stand), _bits(gf))


# ---- 5. accuracy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", ["translation (1.3, -1.6)", "translation (2.4, 0.5)", "zoom 0.05"])
def test_end_point_error(dfe, cuda, motion):
    H, W, k, win, ratios = 96, 128, 7, 8, (1, 2, 4)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    if motion.startswith("translation"):
        dy, dx = (1.3, -1.6) if "1.3" in motion else (2.4, 0.5)
        fn, ty, tx = translation(dy, dx), np.full((H, W), dy), np.full((H, W), dx)
    else:
        a, cx, cy = 0.05, 70.0, 40.0
        fn, ty, tx = zoom(a, cx, cy), a * (yy - cy), a * (xx - cx)
    f0, f1 = warped_pair(H, W, fn, seed=7)
    f0, f1 = f0 / np.float32(255), f1 / np.float32(255)
    sel = (slice(20, -20), slice(20, -20))
    epe = []
    for sub in (False, True):
        flow = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=sub)[1]
        epe.append(float(np.median(np.hypot(flow[0][sel] - ty[sel], flow[1][sel] - tx[sel]))))
    print("%s: median end-point error integer %.3f px, sub-pixel %.3f px" % (motion, epe[0], epe[1]))
    assert epe[1] <= 0.2 and epe[1] <= 0.5 * epe[0], epe


# ---- 6. Python ----------------------------------------------------------------------------------------------------------------------
def test_python_forward_flow(dfe, cuda):
    H, W, k, win, ratios = 96, 128, 7, 8, (1, 2, 4)
    f0, f1, o = exact_case(H, W, 3, k, win, win, ratios)
    geo = dict(maxh=win, maxw=win, ratios=list(ratios), multiscale=True, hKernel=k, wKernel=k, hImg=H, wImg=W, output_extraction_method="max")
    model = dfe.getModelMultiscale(geo)
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    wi, wf = one_call(dfe, cuda, f0, f1, k, win, win, ratios, subpixel=True)
    plain = model.forwardFlow([t0, t1], True, one_call=True)
    assert "y_sub" not in plain
    for oc in (True, False):
        got = model.forwardFlow([t0, t1], True, one_call=oc, subpixel=True)
        assert np.array_equal(got["index"].cpu().numpy(), wi)
        assert np.array_equal(_bits(got["y_sub"].cpu().numpy()), _bits(wf[0])) and np.array_equal(_bits(got["x_sub"].cpu().numpy()), _bits(wf[1])), oc
        assert np.array_equal(_bits(got["full"].cpu().numpy()), _bits(wf)), oc
        for key in ("index", "y", "x", "confidences", "full_confidences"):
            assert torch.equal(got[key], plain[key]), (key, oc)
        assert got["y_sub"].dtype == torch.float32 and tuple(got["y_sub"].shape) == (H, W)
    with pytest.raises(ValueError, match="subpixel"):
        model.forwardFlow([t0, t1], True, f16_scale=1.0, subpixel=True)
    with pytest.raises(ValueError, match="subpixel"):
        dfe.getModelMultiscale(geo, True, True).forwardFlow([(t0, t1)] * 3, True, subpixel=True)
    geo_l = dict(geo, layers=[[3, 7, 7, 4]])
    with pytest.raises(ValueError, match="subpixel"):
        dfe.getModelMultiscale(geo_l, device=cuda).forwardFlow([t0, t1], True, subpixel=True)


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def test_error_codes(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, k, win = 48, 64, 7, 8
    rr, n = _rr((1, 2, 4))
    t = torch.zeros((3, H, W), device=cuda)
    fl = torch.zeros((2, H, W), device=cuda)
    ix = torch.ones((H, W), dtype=torch.int64, device=cuda)
    p, f, i = t.data_ptr(), fl.data_ptr(), ix.data_ptr()
    fn = lib.dfe_multiscale_flow_pair_subpixel_f32
    assert fn(ctx.handle, None, p, 3, H, W, k, win, win, rr, n, f, i) == DFE_E_ARG
    assert fn(ctx.handle, p, None, 3, H, W, k, win, win, rr, n, f, i) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, H, W, k, win, win, rr, n, None, i) == DFE_E_ARG      # flow is required
    assert fn(ctx.handle, p, p, 3, H, W, k, win, win, rr, n, f, None) == 0              # idx is not
    assert fn(ctx.handle, p, p, 3, 46, W, k, win, win, rr, n, f, i) == DFE_E_SHAPE
    assert fn(ctx.handle, p, p, 3, H, 62, k, win, win, rr, n, f, i) == DFE_E_SHAPE
    assert fn(None, p, p, 3, H, W, k, win, win, rr, n, f, i) == DFE_E_ARG
    b = torch.zeros(3 * H * W, dtype=torch.uint8, device=cuda).data_ptr()
    fn = lib.dfe_multiscale_flow_pair_subpixel_u8
    assert fn(ctx.handle, None, b, 3, H, W, k, win, win, rr, n, 1.0, 0.0, f, i) == DFE_E_ARG
    assert fn(ctx.handle, b, b, 3, H, W, k, win, win, rr, n, 1.0, 0.0, None, i) == DFE_E_ARG
    assert fn(ctx.handle, b, b, 3, H, W, k, win, win, rr, n, 0.0, 0.0, f, i) == DFE_E_ARG
    assert fn(ctx.handle, b, b, 3, 46, W, k, win, win, rr, n, 1.0, 0.0, f, i) == DFE_E_SHAPE
    assert fn(ctx.handle, b, b, 3, H, W, k, win, win, rr, n, 1.0, 0.0, f, None) == 0
    fn = lib.dfe_multiscale_refine_subpixel_f32
    assert fn(ctx.handle, None, p, 3, H, W, k, win, win, rr, n, i, f) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, H, W, k, win, win, rr, n, None, f) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, H, W, k, win, win, rr, n, i, None) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, H, W, 0, win, win, rr, n, i, f) == DFE_E_ARG
    assert fn(ctx.handle, p, p, 3, 46, W, k, win, win, rr, n, i, f) == DFE_E_SHAPE
    assert fn(ctx.handle, p, p, 3, H, W, k, win, win, rr, n, i, f) == 0
    assert lib.dfe_last_error(ctx.handle)
    torch.cuda.synchronize()
