"""The guided weighted median on the device (include/dfe.h): dfe_weighted_median_f32 against the numpy restatement
of its definition (tests/wmedian_ref.py) BIT FOR BIT -- the sample weight is an integer, so there is no tolerance -- on sparse fields that
hold every edge case, its argument errors, and flowDepthPair(..., median=...) against the composition of the public calls it stands for.
Every output is pre-filled with a sentinel.

Each case is one (shape, k, C) and runs Cg = 0, 1, 3; the other inputs rotate with the case so that every level meets every shape and k:
    density   1.0 / 0.3 / 0.02 of valid pixels (empty windows occur at the last), weights from {1, 0.5, 1e-3, 1e-6} plus the planted
              specials of test_gpu_fill.sparse_field; at density 1.0 every second form passes w = NULL
    values    random floats in +-16, or integers in -4 .. 4 (many ties)
    guide     random floats (a contracted multiply-add would change d2, and with it a weight), byte-valued, or floats with a planted NaN
    sigma     small enough that many r are 0, or large enough that none is
    filtered  given, and (Cg = 0) NULL in a second call."""
import re

import numpy as np
import pytest
import torch

from tests import refpath as rp
from tests.test_gpu_fill import SHAPES, sparse_field
from tests.wmedian_ref import sample_weight, weighted_median_ref

DFE_E_ARG, DFE_E_SHAPE = -1, -2
FILL = -7.0
KS = (1, 3, 7, 15)
CGS = (0, 1, 3)
DENSITIES = (1.0, 0.3, 0.02)


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _tbits(t):
    return _bits(t.cpu().numpy())


def wmedian(dfe, cuda, v, w, guide, sigma, k, region, want_filtered=True):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = v.shape
    tv, tw, tg = _dev(cuda, v), _dev(cuda, w), _dev(cuda, guide)
    out = torch.full((C_, H, W), FILL, device=cuda)
    filtered = torch.full((H, W), FILL, device=cuda)
    ctx.check(lib.dfe_weighted_median_f32(ctx.handle, tv.data_ptr(), C_, H, W, None if tw is None else tw.data_ptr(), None if tg is None else tg.data_ptr(),
                                          0 if guide is None else guide.shape[0], sigma, k, *region, out.data_ptr(), filtered.data_ptr() if want_filtered else None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), filtered.cpu().numpy()


def make_guide(kind, Cg, shape, region, seed):
    """(guide [Cg][H][W], small sigma, large sigma): at the small one many r are 0, at the large one none is"""
    rng = np.random.default_rng(seed)
    if kind == 1:
        g = rng.integers(0, 256, size=(Cg,) + shape).astype(np.float32)
        return g, 150.0, 1000.0                    # d2 <= 3 * 255^2 = 195075 < 1000^2
    g = rng.uniform(0, 4, size=(Cg,) + shape).astype(np.float32)
    if kind == 2:                                  # a NaN inside R: T = 0 there, a lost sample for its neighbours
        g[rng.integers(0, Cg), region[0] + region[2] // 2, region[1] + region[3] // 2] = np.nan
    return g, 2.0, 100.0                           # d2 <= 3 * 16 = 48 < 100^2


# ---- 1. the operator against the definition, bit for bit -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_bit_for_bit(dfe, cuda, name, k, C_):
    shape, region = SHAPES[name]
    ki, si = KS.index(k), list(SHAPES).index(name)
    for gi, Cg in enumerate(CGS):
        n = si + ki + C_ + gi
        density = DENSITIES[n % 3]
        v, w = sparse_field(C_, shape, region, density, seed=1000 * si + 100 * ki + 10 * C_ + gi)
        if (si + C_ + gi) % 2:                     # integers: many ties (the planted NaN / Inf stay)
            with np.errstate(invalid="ignore"):
                v = np.where(np.isfinite(v), np.round(v / 4), v).astype(np.float32)
        if density == 1.0 and (ki + gi) % 2:
            w = None
        guide, sigma = None, 0.0
        if Cg:
            guide, small, large = make_guide((ki + C_ + si) % 3, Cg, shape, region, seed=n)
            sigma = small if (si + ki + gi) % 2 else large
        want, wfilt = weighted_median_ref(v, w, guide, sigma, k, region)
        out, filtered = wmedian(dfe, cuda, v, w, guide, sigma, k, region)
        tag = "%s k=%d C=%d Cg=%d density=%g w=%s sigma=%g" % (name, k, C_, Cg, density, "NULL" if w is None else "given", sigma)
        assert not (out == FILL).any() and not (filtered == FILL).any(), tag + ": an element was not written"
        assert np.array_equal(_bits(filtered), _bits(wfilt)), tag + ": filtered: %d pixels differ" % np.count_nonzero(filtered != wfilt)
        assert np.array_equal(_bits(out), _bits(want)), tag + ": out: %d elements differ" % np.count_nonzero(_bits(out) != _bits(want))
        if Cg == 0:                                # filtered == NULL
            out2, filtered2 = wmedian(dfe, cuda, v, w, guide, sigma, k, region, want_filtered=False)
            assert np.array_equal(_bits(out2), _bits(want)) and (filtered2 == FILL).all(), tag + ": filtered NULL"


def test_the_rotation_reaches_every_level():
    """what test_bit_for_bit's docstring promises of its schedule, and that the small sigma does zero many weights and the large one none"""
    seen = set()
    for si in range(len(SHAPES)):
        for ki in range(len(KS)):
            for C_ in range(1, 5):
                for gi in range(3):
                    d = (si + ki + C_ + gi) % 3
                    seen.add(("density", si, ki, d))
                    seen.add(("ties", si, (si + C_ + gi) % 2))
                    seen.add(("null", (ki + gi) % 2 if d == 0 else 0))
                    if gi:
                        seen.add(("guide", si, ki, (ki + C_ + si) % 3))
                        seen.add(("sigma", si, gi, (si + ki + gi) % 2))
    assert len([s for s in seen if s[0] == "density"]) == 5 * 4 * 3 and len([s for s in seen if s[0] == "ties"]) == 5 * 2
    assert len([s for s in seen if s[0] == "guide"]) == 5 * 4 * 3 and len([s for s in seen if s[0] == "sigma"]) == 5 * 2 * 2
    assert ("null", 1) in seen and ("null", 0) in seen
    for kind in (0, 1):
        g, small, large = make_guide(kind, 3, (24, 40), (0, 0, 24, 40), seed=1)
        one = np.ones((24, 39), np.float32)
        for sigma, check in ((small, lambda z: 0.1 < z < 0.9), (large, lambda z: z == 0.0)):
            inv = np.float32(1) / (np.float32(sigma) * np.float32(sigma))
            wt = sample_weight(one, g[:, :, 1:], g[:, :, :-1], inv)       # horizontal neighbours
            assert check(float((wt == 0).mean())), (kind, sigma, float((wt == 0).mean()))


# ---- 2. the stated consequences on the device ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_consequences(dfe, cuda):
    rng = np.random.default_rng(2)
    v = rng.uniform(-9, 9, size=(2, 33, 70)).astype(np.float32)
    out, filtered = wmedian(dfe, cuda, v, None, None, 0.0, 1, (0, 0, 33, 70))
    assert np.array_equal(_bits(out), _bits(v)) and (filtered == 1).all(), "k = 1 copies v"
    for k in (5, 9):
        out, _ = wmedian(dfe, cuda, v, None, None, 0.0, k, (0, 0, 33, 70))
        h = k // 2
        win = np.lib.stride_tricks.sliding_window_view(v, (k, k), axis=(1, 2)).reshape(2, 33 - k + 1, 70 - k + 1, k * k)
        assert np.array_equal(out[:, h : 33 - h, h : 70 - h], np.median(win, axis=-1).astype(np.float32)), "unit weights, full window: the plain median"
    v2, w = v.copy(), np.ones((33, 70), np.float32)
    bad = rng.random((33, 70)) < 0.2
    v2[0, bad] = np.nan
    w[bad] = 0
    out, filtered = wmedian(dfe, cuda, v2, w, None, 0.0, 7, (0, 0, 33, 70))
    assert np.isfinite(out).all() and (filtered == 1).all(), "a NaN under a = 0 leaked"
    z = np.array([[[0.0, -0.0, 0.0, -0.0]]], np.float32)
    out, _ = wmedian(dfe, cuda, z, None, None, 0.0, 3, (0, 0, 1, 4))
    assert np.array_equal(_bits(out), _bits(weighted_median_ref(z, k=3)[0])) and np.signbit(out[0, 0, 0]) and not np.signbit(out[0, 0, 1])   # {+0, -0} -> -0; {+0, -0, +0} -> +0


# ---- 3. argument errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_launch_nothing(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W = 24, 40
    HW = H * W
    buf = torch.full((12, H, W), FILL, device=cuda)          # v: planes 0, 1 (C = 2), w: 4, guide: 5 .. 7 (Cg = 3), free: 8 .. 11
    buf[:9] = 1
    out2 = torch.full((4, H, W), FILL, device=cuda)
    filt = torch.full((H, W), FILL, device=cuda)
    plane = lambda i: buf.data_ptr() + 4 * HW * i
    vp, wp, gp, op, fp = plane(0), plane(4), plane(5), out2.data_ptr(), filt.data_ptr()
    fn = lib.dfe_weighted_median_f32
    call = lambda **kw: fn(*[{**dict(ctx=ctx.handle, v=vp, C=2, H=H, W=W, w=wp, guide=gp, Cg=3, sigma=1.0, k=5, y0=0, x0=0, Ho=H, Wo=W, out=op, filtered=fp), **kw}[key]
                             for key in ("ctx", "v", "C", "H", "W", "w", "guide", "Cg", "sigma", "k", "y0", "x0", "Ho", "Wo", "out", "filtered")])
    for kw in [dict(C=0), dict(C=5), dict(C=-1), dict(Cg=-1), dict(Cg=5), dict(k=0), dict(k=2), dict(k=17), dict(k=-1), dict(k=16), dict(v=None), dict(out=None),
               dict(ctx=None)]:
        assert call(**kw) == DFE_E_ARG, kw
    for reg in ((0, 0, H + 1, W), (0, 0, H, W + 1), (-1, 0, H, W), (0, -1, H, W), (1, 0, H, W), (0, 1, H, W), (0, 0, 0, W), (0, 0, H, 0), (0, 0, H, -3),
                (2**31 - 1, 0, 1, 1), (0, 0, 1, 2**31 - 1)):
        assert call(y0=reg[0], x0=reg[1], Ho=reg[2], Wo=reg[3]) == DFE_E_SHAPE, reg
        assert lib.dfe_last_error(ctx.handle).startswith(b"dfe_weighted_median_f32: region")
    assert call(H=0, Ho=1) == DFE_E_SHAPE
    # aliasing: out over v (wholly, and by its last plane only), over w, over the guide; filtered over an input; out over filtered
    for kw in [dict(out=vp), dict(out=plane(1)), dict(out=plane(3)), dict(out=plane(4)), dict(out=plane(7)), dict(out=plane(7), C=1), dict(filtered=plane(1)),
               dict(filtered=wp), dict(filtered=plane(6)), dict(filtered=op), dict(filtered=out2.data_ptr() + 4 * HW), dict(out=plane(9), v=plane(8), C=2)]:
        assert call(**kw) == DFE_E_ARG and re.match(rb"dfe_weighted_median_f32: \w+ overlaps", lib.dfe_last_error(ctx.handle)), kw
    torch.cuda.synchronize()
    assert (buf[9:] == FILL).all() and (buf[:9] == 1).all() and (out2 == FILL).all() and (filt == FILL).all(), "a refused call wrote"
    # neighbours in one buffer are fine: out right behind the guide
    assert call(out=plane(9)) == 0 and call(out=plane(9), w=None, guide=None, Cg=0, filtered=None) == 0
    torch.cuda.synchronize()
    assert (buf[9:11] == 1).all() and (buf[11] == FILL).all() and (filt == 1).all()
    # the Python call: its own checks, the library's errors, and the C call's bits
    v, w, g = buf[:2], buf[4], buf[5:8]
    with pytest.raises(dfe.DfeError):
        dfe.weightedMedian(v, w, region=(0, 0, H, W + 1))
    with pytest.raises(ValueError):
        dfe.weightedMedian(v, w, k=4)
    with pytest.raises(ValueError):
        dfe.weightedMedian(v, w[:, :5])
    with pytest.raises(ValueError):
        dfe.weightedMedian(buf[:5], w)
    with pytest.raises(TypeError):
        dfe.weightedMedian(v.double(), w)
    with pytest.raises(TypeError):
        dfe.weightedMedian(v, w, g.cpu())
    shape, region = SHAPES["inner"]
    vv, ww = sparse_field(2, shape, region, 0.3, seed=3)
    gg, small, _ = make_guide(0, 3, shape, region, seed=4)
    o, f = dfe.weightedMedian(_dev(cuda, vv), _dev(cuda, ww), _dev(cuda, gg), k=7, sigma=small, region=region)
    eo, ef = wmedian(dfe, cuda, vv, ww, gg, small, 7, region)
    assert np.array_equal(_tbits(o), _bits(eo)) and np.array_equal(_tbits(f), _bits(ef))
    o, f = dfe.weightedMedian(_dev(cuda, vv))                # the defaults: k = 7, no weight, no guide, the whole frame
    eo, ef = weighted_median_ref(vv, k=7)
    assert np.array_equal(_tbits(o), _bits(eo)) and np.array_equal(_tbits(f), _bits(ef))


# ---- 4. flowDepthPair(..., median=...) -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fill", [None, True])
@pytest.mark.parametrize("tol", [None, 1.0])
@pytest.mark.parametrize("u8", [False, True])
def test_flow_depth_pair_median(dfe, cuda, u8, tol, fill):
    """A 40 x 56 byte-valued pair, k = 5, a 9 x 9 window: the three new keys are the composition of the public calls (the source and
    weight planes as the docstring of flowDepthPair states them), bit for bit, and every other key is what a call without median gives."""
    H, W, k, win = 40, 56, 5, 9
    f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=5, max_flow=3)
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    if u8:
        t0, t1 = t0.to(torch.uint8), t1.to(torch.uint8)
    Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
    R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    old = dfe.flowDepthPair(t0, t1, k, win, win, foe, consistency=tol, fill=fill)
    for median, (mk, sigma) in ((5, (5, 0.0)), ((7, 30.0), (7, 30.0))):
        new = dfe.flowDepthPair(t0, t1, k, win, win, foe, consistency=tol, fill=fill, median=median)
        assert sorted(new) == sorted(list(old) + ["flow_median", "median_valid", "depth_median"])
        for key in old:
            assert np.array_equal(_tbits(new[key]), _tbits(old[key])), key
        wgt = (old["scores"] > 0).float()
        if tol is not None:
            wgt = wgt * old["consistent"]
        src = old["flow"]
        if fill:
            src, wgt = old["flow_dense"], torch.where(wgt > 0, old["filled"], 0.25 * old["filled"])
        med, valid = dfe.weightedMedian(src, wgt, t0.float(), mk, sigma, R)
        depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(2))
        ctx.check(lib.dfe_flow_to_depth_cartesian(ctx.handle, med.data_ptr(), H, W, foe[0], foe[1], 0, depth.data_ptr(), conf.data_ptr()))
        torch.cuda.synchronize()
        for key, want in (("flow_median", med), ("median_valid", valid), ("depth_median", depth)):
            assert np.array_equal(_tbits(new[key]), _tbits(want)), key
        # and the operator under it is the definition
        ref, rvalid = weighted_median_ref(src.cpu().numpy(), wgt.cpu().numpy(), f0 if sigma else None, sigma, mk, R)
        assert np.array_equal(_tbits(med), _bits(ref)) and np.array_equal(_tbits(valid), _bits(rvalid))
        wn = wgt.cpu().numpy()[R[0] : R[0] + Ho, R[1] : R[1] + Wo]
        print("u8=%s consistency=%s fill=%s median=%s: weight 1 on %.3f of R, 0.25 on %.3f, 0 on %.3f" % (u8, tol, fill, median, (wn == 1).mean(), (wn == 0.25).mean(), (wn == 0).mean()))
        assert (wn == 1).any(), "the scene has kept pixels"
        if tol is not None:
            assert (wn == (0.25 if fill else 0)).any(), "with the mask the scene has rejected pixels"
        if fill:
            assert not (wn == 0).any() and valid.cpu().numpy()[R[0] : R[0] + Ho, R[1] : R[1] + Wo].all(), "a filled field leaves no window empty"
