"""Hole filling by a confidence-weighted push-pull (dfe_fill_holes_f32; include/dfe.h) restated in numpy: the same
cells, orders and skips as the definition, evaluated in float64 on the fp32 inputs (or in any dtype: fp32 gives the rounding the device
does, up to its division).  Plus the scene the feature is for: a zoom field with random holes and a removed band.  Test infrastructure
(no test in this file)."""
import numpy as np

from tests.field_rule import validity


def fill_level_sizes(Ho, Wo, levels=0):
    """[(h, w)] of levels 0 .. L"""
    sizes = [(Ho, Wo)]
    while sizes[-1] != (1, 1):
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    lfull = len(sizes) - 1
    L = lfull if levels == 0 else min(levels, lfull)
    return sizes[: L + 1]


def _push(v, a):
    """level (v [C][h][w], a [h][w]) -> the next coarser one"""
    C, h, w = v.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    vp = np.zeros((C, 2 * hc, 2 * wc), v.dtype)
    ap = np.zeros((2 * hc, 2 * wc), a.dtype)      # children outside the grid: a = 0, skipped like any other
    vp[:, :h, :w], ap[:h, :w] = v, a
    s = np.zeros((hc, wc), a.dtype)
    n = np.zeros((C, hc, wc), v.dtype)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        ak, vk = ap[dy::2, dx::2], vp[:, dy::2, dx::2]
        m = ak != 0
        s = np.where(m, s + ak, s)
        n = np.where(m, n + ak * vk, n)
    pos = s > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        vc = np.where(pos, n / np.where(pos, s, 1), 0).astype(v.dtype)
    ac = np.where(pos, np.minimum(s, 1), 0).astype(a.dtype)
    return vc, ac


def _pull(v, a, f, g):
    """level l (v, a) and the pulled level l + 1 (f, g) -> (f_l, g_l)"""
    C, h, w = v.shape
    hp, wp = g.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    i, j = y >> 1, x >> 1
    i2, j2 = i + np.where(y & 1, 1, -1), j + np.where(x & 1, 1, -1)
    one = v.dtype.type
    S = np.zeros((h, w), v.dtype)
    U = np.zeros((C, h, w), v.dtype)
    for ii, jj, t in ((i, j, 9 / 16), (i, j2, 3 / 16), (i2, j, 3 / 16), (i2, j2, 1 / 16)):
        inside = (ii >= 0) & (ii < hp) & (jj >= 0) & (jj < wp)
        ic, jc = np.clip(ii, 0, hp - 1), np.clip(jj, 0, wp - 1)
        m = inside & (g[ic, jc] != 0)
        S = np.where(m, S + one(t), S)
        U = np.where(m, U + one(t) * f[:, ic, jc], U)
    pos = S > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        u = U / np.where(pos, S, 1)
    mix = a * v + (one(1) - a) * u
    fl = np.where(a == 1, v, np.where(a == 0, u, mix))
    fl = np.where(pos, fl, 0).astype(v.dtype)
    return fl, pos.astype(v.dtype)


def fill_holes_ref(v, w, region=None, levels=0, dtype=np.float64):
    """v [C][H][W], w [H][W] (read as fp32); region = (y0, x0, Ho, Wo), the whole frame by default.  Returns (out [C][H][W] in `dtype`,
    filled float32 [H][W], L)."""
    v = np.ascontiguousarray(v, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    C, H, W = v.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else region
    assert Ho > 0 and Wo > 0 and y0 >= 0 and x0 >= 0 and y0 + Ho <= H and x0 + Wo <= W and levels >= 0
    vr, wr = v[:, y0 : y0 + Ho, x0 : x0 + Wo], w[y0 : y0 + Ho, x0 : x0 + Wo]
    a32 = validity(vr, wr)
    a0 = a32.astype(dtype)
    v0 = np.where(a32 > 0, vr, 0).astype(dtype)   # what lies under a zero weight is never read
    sizes = fill_level_sizes(Ho, Wo, levels)
    L = len(sizes) - 1
    lev = [(v0, a0)]
    for l in range(L):
        lev.append(_push(*lev[-1]))
        assert lev[-1][1].shape == sizes[l + 1]
    f, g = lev[L][0], (lev[L][1] > 0).astype(dtype)
    for l in range(L - 1, -1, -1):
        f, g = _pull(lev[l][0], lev[l][1], f, g)
    out = np.zeros((C, H, W), dtype)
    filled = np.zeros((H, W), np.float32)
    out[:, y0 : y0 + Ho, x0 : x0 + Wo] = f
    filled[y0 : y0 + Ho, x0 : x0 + Wo] = g
    return out, filled, L


def fill_bound(L, vmax):
    """first-order rounding bound of an fp32 evaluation: at most 24 roundings per level on convex combinations of values within vmax"""
    return 24 * max(L, 1) * 2.0**-24 * vmax


def zoom_band_scene(H=64, W=96, region=(4, 6, 55, 83), zoom=0.05, holes=0.3, band=(40, 8), seed=0):
    """The flow of a `zoom` about the frame centre, [2][H][W] (y, x), with a share `holes` of random pixels and the columns band[0] ..
    band[0] + band[1] - 1 removed: returns (flow with NaN in the holes, w with 0 there and 1 elsewhere, the true flow, the hole map
    inside the region)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    true = np.stack([zoom * (yy - (H - 1) / 2), zoom * (xx - (W - 1) / 2)]).astype(np.float32)
    hole = rng.random((H, W)) < holes
    hole[:, band[0] : band[0] + band[1]] = True
    v = true.copy()
    v[:, hole] = np.nan
    w = np.where(hole, 0, 1).astype(np.float32)
    y0, x0, Ho, Wo = region
    inR = np.zeros((H, W), bool)
    inR[y0 : y0 + Ho, x0 : x0 + Wo] = True
    return v, w, true, hole & inR
