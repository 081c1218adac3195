"""Guided upsampling on the device (include/dfe.h): dfe_guided_upsample_f32 against the numpy restatement of its
definition (tests/upsample_ref.py) BIT FOR BIT -- the definition fixes every grouping and every order, so there is no tolerance -- on
sparse fields that hold every edge case, its argument errors, and guidedUpsample against the raw call.  Every output is pre-filled with a
sentinel.

Each case is one (shapes, r, C) and runs Cg = 0, 1, 3; the other inputs rotate with the case so that every level meets every shape and r:
    density   1.0 / 0.3 / 0.02 of valid samples (pixels without a sample occur at the last), weights from {1, 0.5, 1e-3, 1e-6} plus the
              planted specials of test_gpu_fill.sparse_field; at density 1.0 every second form passes w = NULL
    values    random floats in +-16 with |v| >= 2^-10 or 0 (no product is subnormal)
    guide     random floats (a contracted multiply-add would change d2, and with it a weight), byte-valued, or floats with a planted NaN
              in the full-resolution guide
    sigma     small enough that many rr are 0, or large enough that none is
    gain      NULL, or (2.5, -3, 0.5, 7)
    valid     given, and (Cg = 0) NULL in a second call."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_fill import sparse_field
from tests.upsample_ref import guided_upsample_ref, image_scale_ref

DFE_E_ARG, DFE_E_SHAPE = -1, -2
FILL = -7.0
SHAPES = {
    "same": ((7, 9), (7, 9)),
    "odd": ((7, 9), (20, 31)),               # ratios that are not integers
    "one": ((1, 1), (5, 6)),
    "row": ((1, 37), (1, 37)),
    "double": ((24, 40), (48, 80)),
    "x-only": ((24, 40), (24, 140)),         # one axis at ratio 1
    "tiles": ((24, 40), (70, 140)),          # several tiles, a ragged last one
    "tiny": ((3, 5), (70, 140)),             # a footprint far smaller than the tile
}
RS = (1, 2, 4)
CGS = (0, 1, 3)
DENSITIES = (1.0, 0.3, 0.02)
GAIN = (2.5, -3.0, 0.5, 7.0)


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _tbits(t):
    return _bits(t.cpu().numpy())


def upsample(dfe, cuda, v, size, w, gh, gl, sigma, r, gain, want_valid=True):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, Hl, Wl = v.shape
    tv, tw, th, tl = _dev(cuda, v), _dev(cuda, w), _dev(cuda, gh), _dev(cuda, gl)
    out = torch.full((C_,) + tuple(size), FILL, device=cuda)
    valid = torch.full(tuple(size), FILL, device=cuda)
    ctx.check(lib.dfe_guided_upsample_f32(ctx.handle, tv.data_ptr(), C_, Hl, Wl, None if tw is None else tw.data_ptr(), None if th is None else th.data_ptr(),
                                          None if tl is None else tl.data_ptr(), 0 if gh is None else gh.shape[0], sigma, r,
                                          None if gain is None else (ctypes.c_float * C_)(*gain), size[0], size[1], out.data_ptr(), valid.data_ptr() if want_valid else None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), valid.cpu().numpy()


def field(C_, shape, density, seed):
    """test_gpu_fill.sparse_field over the whole frame, |v| >= 2^-10 or 0 (its planted NaN and Inf stay)"""
    v, w = sparse_field(C_, shape, (0, 0) + shape, density, seed)
    with np.errstate(invalid="ignore"):
        v = np.where(np.abs(v) < 2.0**-10, np.float32(0), v).astype(np.float32)
    return v, w


def make_guides(kind, Cg, shape, size, seed):
    """(guide_hi [Cg][Hh][Wh], guide_lo [Cg][Hl][Wl], small sigma, large sigma): at the small one many rr are 0, at the large one none is"""
    rng = np.random.default_rng(seed)
    if kind == 1:
        gh = rng.integers(0, 256, size=(Cg,) + size).astype(np.float32)
        gl = rng.integers(0, 256, size=(Cg,) + shape).astype(np.float32)
        return gh, gl, 150.0, 1000.0               # d2 <= 3 * 255^2 = 195075 < 1000^2
    gh = rng.uniform(0, 4, size=(Cg,) + size).astype(np.float32)
    gl = rng.uniform(0, 4, size=(Cg,) + shape).astype(np.float32)
    if kind == 2:                                  # a NaN at a full-resolution pixel: valid = 0 there; one in the low-resolution guide: a lost sample
        gh[rng.integers(0, Cg), size[0] // 2, size[1] // 2] = np.nan
        gl[rng.integers(0, Cg), shape[0] // 2, shape[1] // 2] = np.nan
    return gh, gl, 2.0, 100.0                      # d2 <= 3 * 16 = 48 < 100^2


def _rotation(si, ri, C_, gi):
    n = si + ri + C_ + gi
    density = DENSITIES[n % 3]
    return dict(density=density, w_null=density == 1.0 and (ri + gi) % 2 == 1, kind=(ri + C_ + si) % 3, small=(si + ri + gi) % 2 == 1, gain=(si + C_ + gi) % 2 == 1)


# ---- 1. the operator against the definition, bit for bit -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_bit_for_bit(dfe, cuda, name, r, C_):
    shape, size = SHAPES[name]
    ri, si = RS.index(r), list(SHAPES).index(name)
    for gi, Cg in enumerate(CGS):
        rot = _rotation(si, ri, C_, gi)
        v, w = field(C_, shape, rot["density"], seed=1000 * si + 100 * ri + 10 * C_ + gi)
        if rot["w_null"]:
            w = None
        gh, gl, sigma = None, None, 0.0
        if Cg:
            gh, gl, small, large = make_guides(rot["kind"], Cg, shape, size, seed=si + ri + C_ + gi)
            sigma = small if rot["small"] else large
        gain = GAIN[:C_] if rot["gain"] else None
        want, wvalid = guided_upsample_ref(v, size, w, gh, gl, sigma, r, gain)
        out, valid = upsample(dfe, cuda, v, size, w, gh, gl, sigma, r, gain)
        tag = "%s r=%d C=%d Cg=%d density=%g w=%s sigma=%g gain=%s" % (name, r, C_, Cg, rot["density"], "NULL" if w is None else "given", sigma, gain)
        assert not (out == FILL).any() and not (valid == FILL).any(), tag + ": an element was not written"
        assert np.array_equal(_bits(valid), _bits(wvalid)), tag + ": valid: %d pixels differ" % np.count_nonzero(valid != wvalid)
        assert np.array_equal(_bits(out), _bits(want)), tag + ": out: %d elements differ" % np.count_nonzero(_bits(out) != _bits(want))
        if Cg == 0:                                # valid == NULL
            out2, valid2 = upsample(dfe, cuda, v, size, w, gh, gl, sigma, r, gain, want_valid=False)
            assert np.array_equal(_bits(out2), _bits(want)) and (valid2 == FILL).all(), tag + ": valid NULL"


def test_the_rotation_reaches_every_level():
    """what test_bit_for_bit's docstring promises of its schedule, that pixels without a sample occur at the lowest density, and that the
    small sigma does zero many rr and the large one none"""
    seen = set()
    for si in range(len(SHAPES)):
        for ri in range(len(RS)):
            for C_ in range(1, 5):
                for gi in range(3):
                    rot = _rotation(si, ri, C_, gi)
                    seen.add(("density", si, ri, rot["density"]))
                    seen.add(("null", rot["w_null"]))
                    seen.add(("gain", si, rot["gain"]))
                    if gi:
                        seen.add(("guide", si, ri, rot["kind"]))
                        seen.add(("sigma", si, gi, rot["small"]))
    assert len([s for s in seen if s[0] == "density"]) == 8 * 3 * 3 and len([s for s in seen if s[0] == "gain"]) == 8 * 2
    assert len([s for s in seen if s[0] == "guide"]) == 8 * 3 * 3 and len([s for s in seen if s[0] == "sigma"]) == 8 * 2 * 2
    assert ("null", True) in seen and ("null", False) in seen
    v, w = field(2, (24, 40), 0.02, seed=5)
    _, valid = guided_upsample_ref(v, (70, 140), w, r=1)
    assert 0 < valid.mean() < 1
    one = np.ones((1, 24, 40), np.float32)
    for kind in (0, 1):
        gh, gl, small, large = make_guides(kind, 3, (24, 40), (48, 80), seed=1)
        for sigma, check in ((small, lambda z: 0.1 < z < 0.99), (large, lambda z: z == 0.0)):
            # with unit values and weights valid = 0 exactly where every rr of the pixel's taps is 0
            _, val = guided_upsample_ref(one, (48, 80), None, gh, gl, sigma, 1)
            assert check(float((val == 0).mean())), (kind, sigma, float((val == 0).mean()))


# ---- 2. the stated consequences on the device ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_consequences(dfe, cuda):
    rng = np.random.default_rng(2)
    v = rng.uniform(-9, 9, size=(2, 33, 70)).astype(np.float32)
    v[0, 0, 0], v[1, 32, 69], v[0, 5, 5] = -0.0, -0.0, 0.0
    out, valid = upsample(dfe, cuda, v, (33, 70), None, None, None, 0.0, 1, None)
    assert np.array_equal(_bits(out), _bits(v)) and (valid == 1).all(), "equal sizes, r = 1: a bit copy, -0 included"
    out, _ = upsample(dfe, cuda, v, (33, 70), None, None, None, 0.0, 1, (2.5, -3.0))
    assert np.array_equal(_bits(out), _bits(np.array([2.5, -3.0], np.float32)[:, None, None] * v)), "... times gain"
    # r = 1 without guide or holes: dfe_image_scale_f32's bilinear interpolation up to rounding, the device's own
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    for size in ((80, 150), (33, 211), (97, 70)):
        out, valid = upsample(dfe, cuda, v, size, None, None, None, 0.0, 1, None)
        scaled = torch.full((2,) + size, FILL, device=cuda)
        ctx.check(lib.dfe_image_scale_f32(ctx.handle, _dev(cuda, v).data_ptr(), 2, 33, 70, size[0], size[1], scaled.data_ptr()))
        torch.cuda.synchronize()
        err = np.abs(out.astype(np.float64) - scaled.cpu().numpy()).max()
        print("33x70 -> %dx%d: |guided r=1 - imageScale| = %.3g (bound %.3g)" % (size + (err, 8 * 2.0**-24 * np.abs(v).max())))
        assert (valid == 1).all() and err <= 8 * 2.0**-24 * np.abs(v).max()
    # a NaN under a = 0 never leaks; a NaN in guide_hi at p gives valid = 0 there
    v2, w = v.copy(), np.ones((33, 70), np.float32)
    bad = rng.random((33, 70)) < 0.2
    v2[0, bad] = np.nan
    v2[1, bad] = np.inf
    w[bad] = 0
    gh = rng.uniform(0, 4, size=(3, 80, 150)).astype(np.float32)
    gl = image_scale_ref(gh, 33, 70)
    out, valid = upsample(dfe, cuda, v2, (80, 150), w, gh, gl, 100.0, 2, None)
    assert np.isfinite(out).all() and (valid == 1).all(), "a NaN under a = 0 leaked"
    gh[1, 40, 77] = np.nan
    out, valid = upsample(dfe, cuda, v2, (80, 150), w, gh, gl, 100.0, 2, None)
    assert valid[40, 77] == 0 and not out[:, 40, 77].any() and valid.sum() == 80 * 150 - 1 and np.isfinite(out).all()


# ---- 3. argument errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_launch_nothing(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    Hl, Wl, Hh, Wh = 12, 20, 24, 40
    lo, hi = Hl * Wl, Hh * Wh
    low = torch.full((7, Hl, Wl), 1.0, device=cuda)          # v: planes 0, 1 (C = 2), w: 2, guide_lo: 3 .. 5 (Cg = 3), free: 6
    high = torch.full((7, Hh, Wh), FILL, device=cuda)        # guide_hi: planes 0 .. 2, out: 3, 4, valid: 5, free: 6
    high[:3] = 1
    lp = lambda i: low.data_ptr() + 4 * lo * i
    hp = lambda i: high.data_ptr() + 4 * hi * i
    gain = (ctypes.c_float * 4)(2.0, 2.0, 2.0, 2.0)
    fn = lib.dfe_guided_upsample_f32
    keys = ("ctx", "v", "C", "Hl", "Wl", "w", "guide_hi", "guide_lo", "Cg", "sigma", "r", "gain", "Hh", "Wh", "out", "valid")
    base = dict(ctx=ctx.handle, v=lp(0), C=2, Hl=Hl, Wl=Wl, w=lp(2), guide_hi=hp(0), guide_lo=lp(3), Cg=3, sigma=1.0, r=2, gain=gain, Hh=Hh, Wh=Wh, out=hp(3), valid=hp(5))
    call = lambda **kw: fn(*[{**base, **kw}[key] for key in keys])
    nan_gain, inf_gain = (ctypes.c_float * 2)(1.0, float("nan")), (ctypes.c_float * 2)(float("inf"), 1.0)
    for kw in [dict(C=0), dict(C=5), dict(C=-1), dict(Cg=-1), dict(Cg=5), dict(r=0), dict(r=5), dict(r=-1), dict(v=None), dict(out=None), dict(ctx=None),
               dict(guide_hi=None), dict(guide_lo=None), dict(guide_hi=None, guide_lo=None), dict(Cg=0), dict(Cg=0, guide_hi=None), dict(Cg=0, guide_lo=None),
               dict(gain=nan_gain), dict(gain=inf_gain)]:
        assert call(**kw) == DFE_E_ARG, kw
    for kw in [dict(Hl=0), dict(Wl=0), dict(Hl=-1), dict(Hh=0), dict(Wh=-4), dict(Hl=Hh + 1), dict(Wl=Wh + 1), dict(Hh=Hl - 1), dict(Wh=Wl - 1), dict(Hh=32769), dict(Wh=32769),
               dict(Hl=32769, Hh=32769), dict(Wh=2**31 - 1), dict(Hl=2**31 - 1, Hh=2**31 - 1)]:
        assert call(**kw) == DFE_E_SHAPE, kw
    # aliasing: out or valid over v, w, either guide; out over valid
    for kw in [dict(out=lp(0)), dict(out=lp(1)), dict(out=lp(2)), dict(out=lp(5)), dict(out=hp(0)), dict(out=hp(2)), dict(out=hp(1), C=1), dict(valid=lp(1)),
               dict(valid=lp(2)), dict(valid=lp(4)), dict(valid=hp(2)), dict(valid=hp(3)), dict(valid=hp(4)), dict(out=hp(4))]:
        assert call(**kw) == DFE_E_ARG and re.match(rb"dfe_guided_upsample_f32: \w+ overlaps", lib.dfe_last_error(ctx.handle)), kw
    torch.cuda.synchronize()
    assert (low == 1).all() and (high[:3] == 1).all() and (high[3:] == FILL).all(), "a refused call wrote"
    # neighbours in one buffer are fine: out right behind the guide, valid right behind out
    assert call() == 0
    torch.cuda.synchronize()
    assert (high[3:5] == 2).all() and (high[5] == 1).all() and (high[6] == FILL).all() and (high[:3] == 1).all()
    assert call(w=None, guide_hi=None, guide_lo=None, Cg=0, gain=None, valid=None, out=hp(5)) == 0
    torch.cuda.synchronize()
    assert (high[5:7] == 1).all() and (high[3:5] == 2).all()


# ---- 4. guidedUpsample ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_call_is_the_raw_call(dfe, cuda):
    shape, size = (24, 40), (70, 140)
    v, w = field(2, shape, 0.3, seed=3)
    gh, gl, small, _ = make_guides(0, 3, shape, size, seed=4)
    tv, tw, th, tl = _dev(cuda, v), _dev(cuda, w), _dev(cuda, gh), _dev(cuda, gl)
    o, f = dfe.guidedUpsample(tv, size, tw, th, tl, r=4, sigma=small, gain=(2.5, -3))
    eo, ef = upsample(dfe, cuda, v, size, w, gh, gl, small, 4, (2.5, -3.0))
    assert np.array_equal(_tbits(o), _bits(eo)) and np.array_equal(_tbits(f), _bits(ef))
    # the defaults: r = 2, no weight, no guide, no gain
    o, f = dfe.guidedUpsample(tv, size)
    eo, ef = guided_upsample_ref(v, size, r=2)
    assert np.array_equal(_tbits(o), _bits(eo)) and np.array_equal(_tbits(f), _bits(ef))
    # gain = "flow": (Hh / Hl, Wh / Wl); the size from the guide; guide_lo = imageScale(guide, Wl, Hl); a 2-D guide is one channel
    o, f = dfe.guidedUpsample(tv, None, tw, th, sigma=small, gain="flow")
    lo_ = dfe.imageScale(th, shape[1], shape[0])
    eo, ef = upsample(dfe, cuda, v, size, w, gh, lo_.cpu().numpy(), small, 2, (70 / 24, 140 / 40))
    assert tuple(o.shape) == (2,) + size and np.array_equal(_tbits(o), _bits(eo)) and np.array_equal(_tbits(f), _bits(ef))
    o, f = dfe.guidedUpsample(tv[:1], None, tw, th[0], tl[0], r=1, sigma=small)
    eo, ef = upsample(dfe, cuda, v[:1], size, w, gh[:1], gl[:1], small, 1, None)
    assert np.array_equal(_tbits(o), _bits(eo)) and np.array_equal(_tbits(f), _bits(ef))
    # its own checks and the library's errors
    with pytest.raises(ValueError):
        dfe.guidedUpsample(tv)
    with pytest.raises(ValueError):
        dfe.guidedUpsample(tv, (23, 140))
    with pytest.raises(ValueError):
        dfe.guidedUpsample(tv, size, tw[:, :5])
    with pytest.raises(ValueError):
        dfe.guidedUpsample(tv, size, r=5)
    with pytest.raises(ValueError):
        dfe.guidedUpsample(tv[:1], size, gain="flow")
    with pytest.raises(TypeError):
        dfe.guidedUpsample(tv.double(), size)
    with pytest.raises(TypeError):
        dfe.guidedUpsample(tv, size, tw, th.cpu())
    with pytest.raises(dfe.DfeError):
        dfe.guidedUpsample(tv, size, gain=(1e39, 1.0))       # finite as a Python float, not as the float the library takes
