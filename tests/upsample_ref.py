"""Guided upsampling (dfe_guided_upsample_f32; include/dfe.h) restated in numpy, a numpy image.scale
(dfe_image_scale_f32's definition) and the two-surface scene that shows what the guide is for.  A helper, no tests.

The definition fixes the grouping of every product and the order of every sum; numpy float32 arrays round every operation separately,
as the kernel does without fused multiply-adds, so the device is compared bit for bit.  The code is vectorised over the output pixels
and loops over the (2r)^2 taps in the stated order.  dtype=np.float64 runs the same code in double (the tents are then the unrounded
quotients): what the float32 result is held against."""
import numpy as np

from tests.field_rule import validity

F = np.float32


def axis_taps(nl, nh, r, dtype=F):
    """per output coordinate x of an axis nl -> nh: (j [2r][nh] int64 tap indices, clipped into [0, nl) where the tap does not exist,
    t [2r][nh] the tents, 0 where the tap does not exist)"""
    x = np.arange(nh, dtype=np.int64)
    num, den = (2 * x + 1) * nl - nh, 2 * nh
    j0 = num // den                                                         # floor division: -1 for a negative num
    j = j0[None] + np.arange(-r + 1, r + 1, dtype=np.int64)[:, None]
    n = r * den - np.abs(num[None] - j * den)
    exists = (j >= 0) & (j < nl) & (n > 0)
    t = (n.astype(np.float64) / np.float64(r * den)).astype(dtype)
    return np.clip(j, 0, nl - 1), np.where(exists, t, dtype(0)).astype(dtype)


def inv_sigma2(guide_hi, sigma):
    """None without a range term, else the host's float32 1 / (sigma sigma)"""
    if guide_hi is None or len(guide_hi) == 0 or not F(sigma) > 0:
        return None
    with np.errstate(all="ignore"):
        return F(1.0) / (F(sigma) * F(sigma))


def guided_upsample_ref(v, size, w=None, guide_hi=None, guide_lo=None, sigma=0.0, r=2, gain=None, dtype=F):
    """(out [C][Hh][Wh], valid [Hh][Wh]) in dtype"""
    v = np.ascontiguousarray(v, F)
    C, Hl, Wl = v.shape
    Hh, Wh = size
    assert 1 <= C <= 4 and 1 <= r <= 4 and 1 <= Hl <= Hh <= 32768 and 1 <= Wl <= Wh <= 32768
    a = validity(v, w).astype(dtype)
    with np.errstate(invalid="ignore"):
        vz = np.where(a[None] > 0, v, F(0)).astype(dtype)                   # what is under a = 0 is never read into arithmetic
    inv_s2 = inv_sigma2(guide_hi, sigma)
    if inv_s2 is not None:
        gh, gl = np.asarray(guide_hi, F).astype(dtype), np.asarray(guide_lo, F).astype(dtype)
        assert gh.shape[1:] == (Hh, Wh) and gl.shape == (gh.shape[0], Hl, Wl)
        inv_s2 = dtype(inv_s2)
    jy, ty = axis_taps(Hl, Hh, r, dtype)
    jx, tx = axis_taps(Wl, Wh, r, dtype)
    S = np.zeros((Hh, Wh), dtype)
    N = np.zeros((C, Hh, Wh), dtype)
    have = np.zeros((Hh, Wh), bool)
    with np.errstate(all="ignore"):
        for i in range(2 * r):
            for j in range(2 * r):
                qy, qx = jy[i][:, None], jx[j][None, :]
                ar = a[qy, qx]
                if inv_s2 is not None:
                    d2 = None
                    for c in range(len(gh)):
                        d = gh[c] - gl[c][qy, qx]
                        s = d * d
                        d2 = s if d2 is None else d2 + s
                    rr = dtype(1) - d2 * inv_s2
                    rr = np.where(np.isfinite(rr) & (rr > 0), rr, dtype(0)).astype(dtype)   # max(0, .), not finite -> 0
                    ar = ar * rr
                wt = ar * (ty[i][:, None] * tx[j][None, :])
                assert wt.dtype == dtype
                ex = wt > 0                                                 # a > 0, rr > 0, both tents exist, no underflow to 0
                S = np.where(ex, np.where(have, S + wt, wt), S)
                for c in range(C):
                    term = wt * vz[c][qy, qx]
                    N[c] = np.where(ex, np.where(have, N[c] + term, term), N[c])
                have |= ex
        g = np.ones(C, dtype) if gain is None else np.asarray(gain, F).astype(dtype)
        out = np.where(have[None], g[:, None, None] * (N / np.where(have, S, dtype(1))[None]), dtype(0)).astype(dtype)
    return out, have.astype(dtype)


def image_scale_ref(src, Hd, Wd):
    """dfe_image_scale_f32 in numpy float32: src [C][Hs][Ws] -> [C][Hd][Wd]"""
    src = np.asarray(src, F)
    _, Hs, Ws = src.shape

    def taps(ns, nd):
        x = np.arange(nd, dtype=np.int64)
        num, den = (2 * x + 1) * ns - nd, 2 * nd
        neg = num < 0
        i0 = np.where(neg, 0, num // den)
        wgt = np.where(neg, 0.0, (num % den).astype(np.float64) / np.float64(den)).astype(F)
        i1 = np.minimum(i0 + 1, ns - 1)
        last = i0 >= ns - 1
        return np.where(last, ns - 1, i0), i1, np.where(last, F(0), wgt).astype(F)

    def lerp(p, q, wgt):
        with np.errstate(all="ignore"):
            return np.where(wgt == 0, p, p + wgt * (q - p)).astype(F)

    y0, y1, wy = taps(Hs, Hd)
    x0, x1, wx = taps(Ws, Wd)
    top = lerp(src[:, y0][:, :, x0], src[:, y0][:, :, x1], wx[None, None, :])
    bot = lerp(src[:, y1][:, :, x0], src[:, y1][:, :, x1], wx[None, None, :])
    return lerp(top, bot, wy[None, :, None])


# ---- the two-surface scene -----------------------------------------------------------------------------------------------------------
SCENE = dict(Hh=96, Wh=128, rect=(21, 33, 45, 61), inside=3.0, outside=-2.0, holes=0.30, band=2, r=2, sigma=40.0)


def two_surface_scene(seed, s=SCENE):
    """A bright rectangle (180 +- 5 on 60 +- 5, byte-valued) at odd offsets of a 96 x 128 frame, so that its edge cuts low-resolution
    pixels, and a 48 x 64 field that is `inside` on the low-resolution pixels wholly inside the rectangle and `outside` elsewhere (a mixed
    pixel carries the background's value); a share `holes` of the samples has weight 0 and a NaN value.
    Returns dict(v [1][Hl][Wl], w [Hl][Wl], guide_hi [1][Hh][Wh], guide_lo [1][Hl][Wl] (the 2 x 2 mean), truth [Hh][Wh], band: the
    pixels within `band` pixels of the rectangle's edge, on either side)."""
    Hh, Wh = s["Hh"], s["Wh"]
    Hl, Wl = Hh // 2, Wh // 2
    ry, rx, rh, rw = s["rect"]
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(Hh), np.arange(Wh), indexing="ij")
    inside = (yy >= ry) & (yy < ry + rh) & (xx >= rx) & (xx < rx + rw)
    b = s["band"]
    grown = (yy >= ry - b) & (yy < ry + rh + b) & (xx >= rx - b) & (xx < rx + rw + b)
    core = (yy >= ry + b) & (yy < ry + rh - b) & (xx >= rx + b) & (xx < rx + rw - b)
    guide_hi = (np.where(inside, 180, 60) + rng.integers(-5, 6, size=(Hh, Wh))).astype(F)[None]
    guide_lo = image_scale_ref(guide_hi, Hl, Wl)
    whole = inside.reshape(Hl, 2, Wl, 2).all(axis=(1, 3))
    v = np.where(whole, F(s["inside"]), F(s["outside"])).astype(F)[None]
    hole = rng.random((Hl, Wl)) < s["holes"]
    w = np.where(hole, 0, 1).astype(F)
    v[0, hole] = np.nan
    truth = np.where(inside, F(s["inside"]), F(s["outside"])).astype(F)
    return dict(v=v, w=w, guide_hi=guide_hi, guide_lo=guide_lo, truth=truth, band=grown & ~core)


def band_error(out, scene):
    """share of the band pixels off the true surface by more than 0.5 (a pixel without a value counts as off)"""
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(out, np.float64) - scene["truth"])
    return float((~(err <= 0.5))[scene["band"]].mean())
