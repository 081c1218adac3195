"""What dfe_sgm_plane_pick_f32 reads off an aggregate, as include/dfe.h defines it, restated in numpy on top of
tests/sgm_plane_ref.py (plane_sum, arg_best, raw_at): float32 throughout, every operation rounded on its own, in the header's order.
Written from the definition -- the chosen cell, the cells at Chebyshev distance 2 or more from it, the three costs of an axis -- and not
from the device's waves, lanes or LDS rows.  Also a numpy SSD volume for byte frames and the wide band scene of the quality table."""
import functools

import numpy as np

from tests import census_ref as cr
from tests import sgm_plane_ref as pr

F = np.float32


def _offset(inside, cm, c0, cp):
    """the parabola's vertex on one axis: 0 where a neighbour lies outside the window or the curvature is not positive"""
    with np.errstate(all="ignore"):
        den = ((cm - c0).astype(F) + (cp - c0).astype(F)).astype(F)
        off = ((cm - cp).astype(F) / (F(2) * den).astype(F)).astype(F)
    off = np.minimum(np.maximum(off, F(-0.5)), F(0.5))
    return np.where(inside & (den > 0), off, F(0)).astype(F)


def pick(agg, subpixel=False, min_unique=0.0):
    """dict(idx, flow_y, flow_x, best, second, unique) of an aggregate [H][W][hWin][wWin] (float32)"""
    agg = np.ascontiguousarray(agg, F)
    H, W, hWin, wWin = agg.shape
    idx, fy, fx = pr.arg_best(agg)
    r, s = (idx - 1) // wWin, (idx - 1) % wWin
    best = pr.raw_at(agg, idx)
    dr = np.abs(np.arange(hWin)[None, None, :, None] - r[:, :, None, None])
    ds = np.abs(np.arange(wWin)[None, None, None, :] - s[:, :, None, None])
    second = np.where(np.maximum(dr, ds) >= 2, agg, F(np.inf)).min(axis=(-2, -1)).astype(F)
    with np.errstate(all="ignore"):
        u = ((second - best).astype(F) / second).astype(F)
    u = np.where(np.isinf(second) | ~(second > 0), F(0), u).astype(F)
    unique = np.where(u >= F(min_unique), u, F(0)).astype(F)
    if subpixel:
        flat = agg.reshape(H, W, -1)
        at = lambda rr, ss: np.take_along_axis(flat, (rr * wWin + ss)[..., None], -1)[..., 0]
        iny, inx = (r >= 1) & (r + 1 < hWin), (s >= 1) & (s + 1 < wWin)
        rm, rp, sm, sp = np.where(iny, r - 1, r), np.where(iny, r + 1, r), np.where(inx, s - 1, s), np.where(inx, s + 1, s)
        fy = (fy + _offset(iny, at(rm, s), best, at(rp, s))).astype(F)
        fx = (fx + _offset(inx, at(r, sm), best, at(r, sp))).astype(F)
    return dict(idx=idx, flow_y=fy, flow_x=fx, best=best.astype(F), second=second, unique=unique)


def plane_pick(C, P1, P2, paths, subpixel=False, min_unique=0.0):
    """what dfe_sgm_plane_pick_f32 returns, with agg: paths = 0 is the volume as it is"""
    agg = np.ascontiguousarray(C, F) if paths == 0 else pr.plane_sum(C, P1, P2, paths)
    return dict(pick(agg, subpixel, min_unique), agg=agg)


def ssd_volume(f0, f1, k, hWin, wWin, scale=1.0):
    """dfe_ssd_cost_volume_f32 of two uint8 frames [C][H][W] read as float(byte) * scale, scale a power of two: every term is a multiple
    of scale^2 and every sum stays below 2^24 of them, so the float32 result does not depend on the order of the sum.  [Ho][Wo][hWin][wWin]"""
    a, b = f0.astype(np.float64) * scale, f1.astype(np.float64) * scale
    C, H, W = a.shape
    Hp, Wp = H - k + 1, W - k + 1
    Ho, Wo = Hp - hWin + 1, Wp - wWin + 1
    oy, ox = (hWin - 1) // 2, (wWin - 1) // 2
    out = np.empty((Ho, Wo, hWin, wWin), F)
    for dy in range(hWin):
        for dx in range(wWin):
            # frame 0's pixel (y + oy + i, x + ox + j) against frame 1's (y + dy + i, x + dx + j), y + i = 0 .. Ho + k - 2
            d = a[:, oy:oy + Ho + k - 1, ox:ox + Wo + k - 1] - b[:, dy:dy + Ho + k - 1, dx:dx + Wo + k - 1]
            q = np.pad((d * d).sum(0).cumsum(0).cumsum(1), ((1, 0), (1, 0)))
            out[:, :, dy, dx] = q[k:, k:] - q[:-k, k:] - q[k:, :-k] + q[:-k, :-k]
    return out


# ---- the wide band scene: sgm_plane_ref.band_scene without the exposure change, a flat band of sixteen rows, more noise ----
WIDE = dict(rows=(28, 44), value=128.0, sigma=2.0, P1=400.0, P2=3200.0, min_unique=0.2)


def wide_band_scene(seed):
    """two uint8 frames [1][72][104]: band_scene's construction with gain 1 and offset 0, rows 28 .. 43 of the frame set to 128 and
    N(0, 2) added to both frames.  One RandomState(seed), drawn in the order texture, frame-0 noise, frame-1 noise."""
    s = cr.SCENE
    rng = np.random.RandomState(seed)
    H, W, m = s["H"], s["W"], s["margin"]
    t = rng.uniform(size=(H + 2 * m, W + 2 * m))
    for _ in range(4):                     # the 5-point mean, with wrap-around
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    t[m + WIDE["rows"][0]:m + WIDE["rows"][1]] = WIDE["value"]
    my, mx = s["move"]
    f0 = t[m:m + H, m:m + W] + rng.normal(0.0, WIDE["sigma"], size=(H, W))
    f1 = t[m - my:m - my + H, m - mx:m - mx + W] + rng.normal(0.0, WIDE["sigma"], size=(H, W))
    to_u8 = lambda f: np.clip(np.floor(f), 0, 255).astype(np.uint8)[None]
    return to_u8(f0), to_u8(f1)


@functools.lru_cache(maxsize=None)
def wide_volume(seed):
    """the SSD volume of the wide band scene at k = 7, 9 x 9"""
    f0, f1 = wide_band_scene(seed)
    return ssd_volume(f0, f1, cr.SCENE["k"], cr.SCENE["win"], cr.SCENE["win"])


@functools.lru_cache(maxsize=None)
def wide_pick(seed, paths):
    """pick() of the wide band scene: paths = 0 on the raw volume, else on the aggregate at WIDE's penalties, gated at WIDE's min_unique.
    Computed once per process and shared by the tests that read it (read only)"""
    return plane_pick(wide_volume(seed), WIDE["P1"], WIDE["P2"], paths, False, WIDE["min_unique"])


def wrong(p):
    """the mask of wrong vectors of a pick"""
    my, mx = cr.SCENE["move"]
    return (p["flow_y"] != my) | (p["flow_x"] != mx)
