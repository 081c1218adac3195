"""Edge-aware semi-global aggregation as include/dfe.h defines it (dfe_sgm_aggregate_guided_f32, dfe_sgm_plane_pick_guided_f32, DESIGN
section 4.38), restated in numpy: float32 throughout, every operation rounded on its own, in the header's order.  Written from the
definition -- a pixel p, its predecessor q = p - r, the penalty P2(p, r) of that pair -- and not from the device's penalty planes or its
walk along lines.  The step, the sum, the arg-min and the pick are the unchanged parts and come from tests/sgm_ref.py,
tests/sgm_plane_ref.py and tests/sgm_pick_ref.py.  Also the bar scene of the quality table."""
import functools

import numpy as np

from tests import sgm_pick_ref as kr
from tests import sgm_plane_ref as pr
from tests import sgm_ref as sr

F = np.float32
DIRS = sr.DIRS


def guided(guide, sigma):
    """whether a call is guided at all: a guide and sigma > 0 (NaN is not)"""
    return guide is not None and bool(np.float32(sigma) > 0)


def penalty(guide, py, px, qy, qx, sigma, P2, P2_edge):
    """P2(p, r) for the pixels p = (py, px) with predecessors q = (qy, qx) (index arrays of one shape, q inside the plane): float32"""
    shape = np.broadcast(py, px).shape
    if not guided(guide, sigma):
        return np.full(shape, P2, F)
    g = np.asarray(guide, F)
    s = F(sigma)
    with np.errstate(all="ignore"):
        inv_s2 = F(1) / (s * s)
        span = F(P2) - F(P2_edge)
        d2 = None
        for c in range(g.shape[0]):
            d = (g[c][py, px] - g[c][qy, qx]).astype(F)
            sq = (d * d).astype(F)
            d2 = sq if d2 is None else (d2 + sq).astype(F)
        w = (F(1) - (d2 * inv_s2).astype(F)).astype(F)
        w = np.where(np.isfinite(w), np.maximum(w, F(0)), F(0)).astype(F)
        pen = (F(P2_edge) + (span * w).astype(F)).astype(F)
    return np.where(w == F(1), F(P2), pen).astype(F)


def sgm_path(C, r, P1, P2, ring=0, guide=None, sigma=0.0, P2_edge=None):
    """L_r [H][W][D] of the radial family's volume C [H][W][D] for direction r (sgm_ref.sgm_path with the penalty of each step)"""
    C = np.ascontiguousarray(C, F)
    H, W, D = C.shape
    P2_edge = P1 if P2_edge is None else P2_edge
    dy, dx = DIRS[r]
    L = np.empty_like(C)
    rows = np.arange(H)
    if dy == 0:
        cols = (list(range(W - ring, W)) + list(range(W))) if dx > 0 else (list(range(ring - 1, -1, -1)) + list(range(W - 1, -1, -1)))
        cur = None
        for i, x in enumerate(cols):
            if i == 0:
                cur = C[:, x].copy()
            else:
                q = cols[i - 1]                                # p - r, the column taken modulo W on a ring
                assert q == (x - dx) % W
                pen = penalty(guide, rows, np.full(H, x), rows, np.full(H, q), sigma, P2, P2_edge)
                cur = sr._step(cur, C[:, x], P1, pen[:, None])
            if i >= ring:
                L[:, x] = cur
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    xs = np.arange(W)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]
            continue
        qx = xs - dx
        pen = penalty(guide, np.full(W, y), xs, np.full(W, y - dy), qx % W, sigma, P2, P2_edge)
        got = sr._step(L[y - dy][qx % W], C[y], P1, pen[:, None])
        if ring > 0:
            L[y] = got
        else:
            outside = (qx < 0) | (qx >= W)
            L[y] = np.where(outside[:, None], C[y], got)
    return L


def sgm_aggregate(C, P1, P2, paths=0x0f, ring=0, guide=None, sigma=0.0, P2_edge=None):
    """(agg [H][W][D], flow [H][W]) of dfe_sgm_aggregate_guided_f32"""
    assert 1 <= paths <= 255
    agg = None
    for r in range(8):
        if paths >> r & 1:
            L = sgm_path(C, r, P1, P2, ring, guide, sigma, P2_edge)
            agg = L if agg is None else (agg + L).astype(F)
    return agg, np.argmin(agg, axis=-1).astype(F)


def plane_path(C, r, P1, P2, guide=None, sigma=0.0, P2_edge=None):
    """L_r [H][W][hWin][wWin] of the plane family's volume C for direction r (sgm_plane_ref.plane_path with the penalty of each step)"""
    C = np.ascontiguousarray(C, F)
    H, W = C.shape[:2]
    P2_edge = P1 if P2_edge is None else P2_edge
    dy, dx = DIRS[r]
    L = np.empty_like(C)
    rows = np.arange(H)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            if i == 0:
                L[:, x] = C[:, x]
            else:
                pen = penalty(guide, rows, np.full(H, x), rows, np.full(H, x - dx), sigma, P2, P2_edge)
                L[:, x] = pr._step(L[:, x - dx], C[:, x], P1, pen[:, None, None])
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    xs = np.arange(W)
    for i, y in enumerate(ys):
        L[y] = C[y]
        if i == 0:
            continue
        qx = xs - dx
        inside = (qx >= 0) & (qx < W)
        if inside.any():
            px, qq = xs[inside], qx[inside]
            pen = penalty(guide, np.full(px.size, y), px, np.full(px.size, y - dy), qq, sigma, P2, P2_edge)
            L[y][inside] = pr._step(L[y - dy][qq], C[y][inside], P1, pen[:, None, None])
    return L


def plane_sum(C, P1, P2, paths=0x0f, guide=None, sigma=0.0, P2_edge=None):
    assert 1 <= paths <= 255
    agg = None
    for r in range(8):
        if paths >> r & 1:
            L = plane_path(C, r, P1, P2, guide, sigma, P2_edge)
            agg = L if agg is None else (agg + L).astype(F)
    return agg


def plane_pick(C, P1, P2, paths, subpixel=False, min_unique=0.0, guide=None, sigma=0.0, P2_edge=None):
    """what dfe_sgm_plane_pick_guided_f32 returns, with agg: paths = 0 is the volume as it is, and the guide is ignored"""
    agg = np.ascontiguousarray(C, F) if paths == 0 else plane_sum(C, P1, P2, paths, guide, sigma, P2_edge)
    return dict(kr.pick(agg, subpixel, min_unique), agg=agg)


# ---- the bar scene: a thin near object in front of a moving background ----
# 64 x 96 frames of one channel.  Two textures (uniform noise, the five-point mean with wrap-around four times, stretched to 0 .. 1):
# the background 40 + 50 t moving by (1, -2), and a bar of 5 x 48 pixels of the second texture, 150 + 50 t, moving by (-2, 3); N(0, 3) on
# both frames, floored to bytes.  One RandomState(seed), drawn in the order background texture, bar texture, frame-0 noise, frame-1
# noise.  The SSD volume at a k x k patch and a 9 x 9 window; the guide is frame 0 on the volume's region.  The constants are the
# issue's pilot's; they were not changed to make the figures below come out.
BAR = dict(H=64, W=96, margin=8, bg=(40.0, 50.0), bar=(150.0, 50.0), bg_move=(1, -2), bar_move=(-2, 3), bar_rows=(8, 56), bar_cols=(46, 51),
           noise=3.0, win=9, far=6, k=7, P1=8000.0, P2=200000.0, sigma=40.0, seeds=(0, 1, 2, 3))
BAR_K5 = dict(k=5, P1=4000.0, P2=100000.0, seeds=(0, 1, 2, 3, 4))


def _texture(rng, shape):
    t = rng.uniform(size=shape)
    for _ in range(4):
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
    return (t - t.min()) / (t.max() - t.min())


def bar_scene(seed):
    """(f0, f1 uint8 [1][H][W], bar [H][W] bool: the bar's pixels in frame 0)"""
    s = BAR
    H, W, m = s["H"], s["W"], s["margin"]
    rng = np.random.RandomState(seed)
    tb = s["bg"][0] + s["bg"][1] * _texture(rng, (H + 2 * m, W + 2 * m))
    to = s["bar"][0] + s["bar"][1] * _texture(rng, (H + 2 * m, W + 2 * m))
    mask = np.zeros((H + 2 * m, W + 2 * m), bool)
    mask[m + s["bar_rows"][0]:m + s["bar_rows"][1], m + s["bar_cols"][0]:m + s["bar_cols"][1]] = True

    def cut(a, move):                      # the canvas moved by `move`: out(p + move) = a(p)
        return a[m - move[0]:m - move[0] + H, m - move[1]:m - move[1] + W]

    f0 = np.where(cut(mask, (0, 0)), cut(to, (0, 0)), cut(tb, (0, 0)))
    f1 = np.where(cut(mask, s["bar_move"]), cut(to, s["bar_move"]), cut(tb, s["bg_move"]))
    f0 = f0 + rng.normal(0.0, s["noise"], size=(H, W))
    f1 = f1 + rng.normal(0.0, s["noise"], size=(H, W))
    to_u8 = lambda f: np.clip(np.floor(f), 0, 255).astype(np.uint8)[None]
    return to_u8(f0), to_u8(f1), cut(mask, (0, 0)).copy()


def bar_region(k):
    """(pad_t, pad_l, Ho, Wo): where the volume's plane is pasted in the frame (the single-scale step's rule)"""
    Ho, Wo = BAR["H"] - k + 1 - BAR["win"] + 1, BAR["W"] - k + 1 - BAR["win"] + 1
    return (BAR["H"] - Ho) // 2, (BAR["W"] - Wo) // 2, Ho, Wo


@functools.lru_cache(maxsize=None)
def bar_case(seed, k):
    """(volume [Ho][Wo][9][9], guide [1][Ho][Wo] float32, on_bar, far [Ho][Wo] bool) of the bar scene at a k x k patch; read only"""
    f0, f1, bar = bar_scene(seed)
    t, l, Ho, Wo = bar_region(k)
    vol = kr.ssd_volume(f0, f1, k, BAR["win"], BAR["win"])
    guide = np.ascontiguousarray(f0[:, t:t + Ho, l:l + Wo].astype(F))
    d = BAR["far"]
    near = np.zeros_like(bar)
    ys, xs = np.nonzero(bar)
    near[max(ys.min() - d, 0):ys.max() + d + 1, max(xs.min() - d, 0):xs.max() + d + 1] = True   # within `far` pixels of the bar
    crop = lambda a: a[t:t + Ho, l:l + Wo]
    return vol, guide, crop(bar), crop(~near)


def bar_shares(seed, paths, mode, k=BAR["k"]):
    """(share of wrong vectors on the bar, share on the pixels more than BAR['far'] px from it); mode: 'wta', 'fixed' or 'adaptive'"""
    vol, guide, on_bar, far = bar_case(seed, k)
    c = BAR if k == BAR["k"] else BAR_K5
    if mode == "wta":
        agg = vol
    elif mode == "fixed":
        agg = pr.plane_sum(vol, c["P1"], c["P2"], paths)
    else:
        agg = plane_sum(vol, c["P1"], c["P2"], paths, guide, BAR["sigma"], c["P1"])
    _, fy, fx = pr.arg_best(agg)
    wrong_bar = (fy != BAR["bar_move"][0]) | (fx != BAR["bar_move"][1])
    wrong_bg = (fy != BAR["bg_move"][0]) | (fx != BAR["bg_move"][1])
    return float(wrong_bar[on_bar].mean()), float(wrong_bg[far].mean())
