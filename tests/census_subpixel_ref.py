"""Sub-pixel flow on the raw census cost in numpy, written from the rule in include/dfe.h, not from the device's
walk: the equiangular ("vee") fit per axis through the integer census costs of the chosen cell and its two neighbours, on
census_ref.cost_volume for the single-scale matcher and on the integer per-scale volumes of the pyramid (census_pyramid_ref.scale_volume
with beta = 1 gives them as exact floats), with the class decode restated from its definition.  Every operation is float32 in the
rule's order.  Also the parabola of the SSD paths on the same costs, for comparison, and the sub-pixel scene of the quality table (no
tests here)."""
import numpy as np

F = np.float32


def vee(cm, c0, cp, inside):
    """the rule on one axis: integer arrays cm, c0, cp and a boolean array `inside` -> float32 offsets.
    m = max(cm - c0, cp - c0); off = clamp((cm - cp) / (2 m), -0.5, 0.5) where inside and m > 0, else 0"""
    cm, c0, cp = (np.asarray(v, np.int64) for v in (cm, c0, cp))
    m = np.maximum(cm - c0, cp - c0)
    ok = np.asarray(inside, bool) & (m > 0)
    num, den = (cm - cp).astype(F), (2 * m).astype(F)          # exact: below 2^24
    q = np.divide(num, den, out=np.zeros(num.shape, F), where=ok)   # one float32 division
    return np.where(ok, np.minimum(np.maximum(q, F(-0.5)), F(0.5)), F(0)).astype(F)


def parabola(cm, c0, cp, inside):
    """the SSD paths' rule (dfe_flow_refine_subpixel_f32) on the same costs: den = (cm - c0) + (cp - c0), off = (cm - cp) / (2 den)"""
    cm, c0, cp = (np.asarray(v, np.int64) for v in (cm, c0, cp))
    den = (cm - c0) + (cp - c0)
    ok = np.asarray(inside, bool) & (den > 0)
    q = np.divide((cm - cp).astype(F), (2 * den).astype(F), out=np.zeros(den.shape, F), where=ok)
    return np.where(ok, np.minimum(np.maximum(q, F(-0.5)), F(0.5)), F(0)).astype(F)


def _five(cost, yy, xx, r, s):
    """the costs of cell (r, s) and its four neighbours at the pixels (yy, xx) of a volume [..][..][h][w], and which axes have both
    neighbours inside the window; a neighbour outside it is replaced by the cell itself (its value is not used)"""
    h, w = cost.shape[2:]
    iny, inx = (r >= 1) & (r + 1 < h), (s >= 1) & (s + 1 < w)
    at = lambda a, b: np.asarray(cost[yy, xx, a, b]).astype(np.int64)
    return (at(r, s), at(r, np.where(inx, s - 1, s)), at(r, np.where(inx, s + 1, s)), at(np.where(iny, r - 1, r), s), at(np.where(iny, r + 1, r), s), inx, iny)


def refine(cost, idx, fy=None, fx=None, fit=vee):
    """what dfe_census_refine_subpixel_f32 leaves in fy / fx [Ha][Wa]: cost int [Ha][Wa][hWin][wWin] (census_ref.cost_volume), idx the
    1-based class map of any producer.  Pixels whose idx is no class keep what fy / fx held (zeros where none are given)."""
    Ha, Wa, hWin, wWin = cost.shape
    fy = np.zeros((Ha, Wa), F) if fy is None else np.array(fy, F)
    fx = np.zeros((Ha, Wa), F) if fx is None else np.array(fx, F)
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 1) & (idx <= hWin * wWin)
    yy, xx = np.nonzero(ok)
    n = idx[yy, xx] - 1
    r, s = n // wWin, n % wWin
    c0, cxm, cxp, cym, cyp, inx, iny = _five(cost, yy, xx, r, s)
    fy[yy, xx] = (r - (hWin - 1) // 2).astype(F) + fit(cym, c0, cyp, iny)
    fx[yy, xx] = (s - (wWin - 1) // 2).astype(F) + fit(cxm, c0, cxp, inx)
    return fy, fx


# ---- the pyramid: the class decode from its definition (x2yxMultiNumber) ----
def ring_widths(ratios, maxw):
    """d of every scale (0 for the first): round(maxw (r - r') / (2 r)) with r' the ratio before r, from maxw alone, on both axes"""
    return [0] + [int(np.floor(maxw * (ratios[i] - ratios[i - 1]) / (2.0 * ratios[i]) + 0.5)) for i in range(1, len(ratios))]


def class_table(maxh, maxw, ratios):
    """(scale, a, b) of every class id, 0-based, in the joined vector's order: the first scale's whole window row-major, then per coarser
    scale its ring of width d around the hole: the top d rows, the left and the right d columns of the rows between, the bottom d rows"""
    tab = [(0, a, b) for a in range(maxh) for b in range(maxw)]
    for s, d in enumerate(ring_widths(ratios, maxw)):
        if s == 0:
            continue
        tab += [(s, a, b) for a in range(d) for b in range(maxw)]
        tab += [(s, a, b) for a in range(d, maxh - d) for b in range(d)]
        tab += [(s, a, b) for a in range(d, maxh - d) for b in range(maxw - d, maxw)]
        tab += [(s, a, b) for a in range(maxh - d, maxh) for b in range(maxw)]
    return np.array(tab, np.int64)


def pyramid_refine(vols, idx, maxh, maxw, ratios, flow=None, fit=vee):
    """what dfe_multiscale_census_refine_subpixel_f32 leaves in flow [2][H][W]: vols[s] the integer census volume [H/r][W/r][maxh][maxw]
    of scale s (any dtype holding the integers), idx the 1-based class map [H][W].  Returns (flow, scale): scale [H][W] is the winning
    scale's number, -1 where idx is no class."""
    H, W = idx.shape
    flow = np.zeros((2, H, W), F) if flow is None else np.array(flow, F)
    tab = class_table(maxh, maxw, ratios)
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 1) & (idx <= len(tab))
    scale = np.full((H, W), -1, np.int64)
    oy, ox = (maxh - 1) // 2, (maxw - 1) // 2
    for s, rho in enumerate(ratios):
        cls = np.where(ok, idx - 1, 0)
        yy, xx = np.nonzero(ok & (tab[cls, 0] == s))
        if not len(yy):
            continue
        scale[yy, xx] = s
        a, b = tab[idx[yy, xx] - 1, 1], tab[idx[yy, xx] - 1, 2]
        c0, cxm, cxp, cym, cyp, inx, iny = _five(vols[s], yy // rho, xx // rho, a, b)
        rf = F(rho)
        flow[0, yy, xx] = ((a - oy) * rho).astype(F) + rf * fit(cym, c0, cyp, iny)      # product and sum rounded separately
        flow[1, yy, xx] = ((b - ox) * rho).astype(F) + rf * fit(cxm, c0, cxp, inx)
    return flow, scale


# ---- the sub-pixel scene: census_ref.scene's periodic texture moved by a fraction of a pixel with a Fourier shift ----
SCENE = dict(H=56, W=72, k=7, win=9, gain=0.5, offset=40.0, sigma=1.0, margin=8)
MOVES = ((2.3, -2.6), (1.5, -0.5), (-1.25, 2.75))
SEEDS = (0, 1, 2)


def scene(seed, move, C=1, H=SCENE["H"], W=SCENE["W"], margin=SCENE["margin"]):
    """two byte-valued uint8 frames [C][H][W]: frame 1 is frame 0's texture moved by `move` (y, x) -- f1(p + move) = f0(p), exact for the
    periodic texture -- times gain, plus offset, plus N(0, 1), floored and clipped to 0 .. 255"""
    rng = np.random.RandomState(seed)
    m = margin
    f0s, f1s = [], []
    for _ in range(C):
        t = rng.uniform(size=(H + 2 * m, W + 2 * m))
        for _ in range(4):                     # the 5-point mean, with wrap-around
            t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
        t = (t - t.min()) / (t.max() - t.min()) * 255.0
        ky, kx = np.fft.fftfreq(t.shape[0])[:, None], np.fft.fftfreq(t.shape[1])[None, :]
        moved = np.real(np.fft.ifft2(np.fft.fft2(t) * np.exp(-2j * np.pi * (ky * move[0] + kx * move[1]))))
        f0s.append(t[m:m + H, m:m + W])
        f1s.append(moved[m:m + H, m:m + W] * SCENE["gain"] + SCENE["offset"] + rng.normal(0.0, SCENE["sigma"], size=(H, W)))
    to_u8 = lambda f: np.clip(np.floor(np.stack(f)), 0, 255).astype(np.uint8)
    return to_u8(f0s), to_u8(f1s)


def median_epe(fy, fx, move, border=0):
    """the median end-point error of a flow field against the move, over the field less a border"""
    b = border
    fy, fx = np.asarray(fy, np.float64), np.asarray(fx, np.float64)
    if b:
        fy, fx = fy[b:-b, b:-b], fx[b:-b, b:-b]
    return float(np.median(np.hypot(fy - move[0], fx - move[1])))
