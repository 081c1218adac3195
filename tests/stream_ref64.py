"""float64 references for the stream layer (csrc/image_scale.hip, csrc/stream.hip), written from the definitions in include/dfe.h and
DESIGN 4.24 -- not from the kernels."""
import numpy as np


def scale_taps(ns, nd, weights="float32"):
    """Per axis, in exact integer arithmetic: num = (2 x + 1) ns - nd, den = 2 nd.  num < 0: i0 = 0, w = 0.  Otherwise i0 = num // den,
    w = float32(double(num % den) / double(den)).  i1 = min(i0 + 1, ns - 1); if i0 >= ns - 1 then i0 = ns - 1 and w = 0.
    -> (i0 [nd] int64, i1 [nd] int64, w [nd] float64 holding the float32 weight).  weights="exact" leaves the weight unrounded,
    double(num % den) / double(den): the mapping itself, what a float64 interpolation computes."""
    i0, i1, w = np.zeros(nd, np.int64), np.zeros(nd, np.int64), np.zeros(nd, np.float64)
    for x in range(nd):
        num, den = (2 * x + 1) * ns - nd, 2 * nd          # Python integers: exact
        if num < 0:
            a, f = 0, 0.0
        else:
            a, f = num // den, float(num % den) / float(den)
        b = min(a + 1, ns - 1)
        if a >= ns - 1:
            a, f = ns - 1, 0.0
        if weights == "float32":
            f = float(np.float32(f))
        i0[x], i1[x], w[x] = a, b, f
    return i0, i1, w


def scale64(src, Hd, Wd, weights="float32"):
    """src [C][Hs][Ws] (any real dtype) -> float64 [C][Hd][Wd]: top = a + wx (b - a), bot alike, out = top + wy (bot - top), with the
    float32 weights of the definition (weights="exact": unrounded) and everything else in float64"""
    src = np.asarray(src, np.float64)
    if src.ndim == 2:
        return scale64(src[None], Hd, Wd, weights)[0]
    _, Hs, Ws = src.shape
    y0, y1, wy = scale_taps(Hs, Hd, weights)
    x0, x1, wx = scale_taps(Ws, Wd, weights)
    r0, r1 = src[:, y0, :], src[:, y1, :]
    top = r0[:, :, x0] + wx * (r0[:, :, x1] - r0[:, :, x0])
    bot = r1[:, :, x0] + wx * (r1[:, :, x1] - r1[:, :, x0])
    return top + wy[None, :, None] * (bot - top)


def paste_mul(mask, conf, oy, ox):
    """out = 0; out(y + oy, x + ox) = mask(y, x) conf(y + oy, x + ox) -- one float32 product per pixel, so exact in numpy float32"""
    mask, conf = np.asarray(mask, np.float32), np.asarray(conf, np.float32)
    out = np.zeros_like(conf)
    Hm, Wm = mask.shape
    out[oy:oy + Hm, ox:ox + Wm] = mask * conf[oy:oy + Hm, ox:ox + Wm]
    return out
