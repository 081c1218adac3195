"""Semi-global aggregation as include/dfe.h defines it (dfe_sgm_aggregate_f32), restated in numpy: float32 throughout,
every operation rounded on its own, in the header's order.  Written from the definition -- a pixel, its predecessor p - r, the start where
that predecessor lies outside the plane -- and not from the device's walk along lines.  Every path is available on its own (sgm_path)."""
import numpy as np

F = np.float32
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))   # (dy, dx) of bit r


def _step(prev, c, P1, P2):
    """L_r(p, .) from L_r(q, .) (prev [..., D]) and C(p, .) (c [..., D])"""
    inf = np.full(prev.shape[:-1] + (1,), np.inf, F)
    m = prev.min(axis=-1, keepdims=True)
    dn = np.concatenate([inf, prev[..., :-1]], axis=-1)      # L(q, d - 1)
    up = np.concatenate([prev[..., 1:], inf], axis=-1)       # L(q, d + 1)
    t = np.minimum(np.minimum(np.minimum(prev, (dn + F(P1)).astype(F)), (up + F(P1)).astype(F)), (m + F(P2)).astype(F))
    return (c + (t - m).astype(F)).astype(F)


def sgm_path(C, r, P1, P2, ring=0):
    """L_r [H][W][D] of the volume C [H][W][D] for direction r (0 .. 7)"""
    C = np.ascontiguousarray(C, F)
    H, W, D = C.shape
    dy, dx = DIRS[r]
    assert 0 <= ring <= W
    L = np.empty_like(C)
    if dy == 0:
        # a row's chain: on the plane from the border; on a ring from column W - G (direction 0) or G - 1 (direction 1) with L = C, through
        # the G warm-up columns, then once round -- only the second stretch is kept
        if dx > 0:
            cols = list(range(W - ring, W)) + list(range(W))
        else:
            cols = list(range(ring - 1, -1, -1)) + list(range(W - 1, -1, -1))
        cur = None
        for i, x in enumerate(cols):
            cur = C[:, x].copy() if i == 0 else _step(cur, C[:, x], P1, P2)
            if i >= ring:
                L[:, x] = cur
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    xs = np.arange(W)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]                                       # the predecessor's row lies outside
            continue
        qx = xs - dx                                          # the predecessor's column
        got = _step(L[y - dy][qx % W], C[y], P1, P2)
        if ring > 0:
            L[y] = got
        else:
            outside = (qx < 0) | (qx >= W)
            L[y] = np.where(outside[:, None], C[y], got)
    return L


def sgm_aggregate(C, P1, P2, paths=0x0f, ring=0):
    """(agg [H][W][D], flow [H][W]): the paths summed in ascending bit order, and the first minimum over d as float32"""
    assert 1 <= paths <= 255
    agg = None
    for r in range(8):
        if paths >> r & 1:
            L = sgm_path(C, r, P1, P2, ring)
            agg = L if agg is None else (agg + L).astype(F)
    return agg, np.argmin(agg, axis=-1).astype(F)              # (numpy's argmin: the first of equal minima)


# ---- the quality scene of DESIGN section 4.29 ----
SCENE = dict(H=48, W=96, D=16, P1=2.0, P2=16.0, ring=16, noise=0.5, cap=9.0, outliers=0.15, flat_rows=(10, 25, 40), seeds=(0, 1, 2))


def quality_scene(seed):
    """(volume [H][W][D], truth [H][W]): a ramp in y modulated by cos(2 pi x / W) (periodic in the angle) plus a raised block that
    straddles the seam at x = 0; costs min((d - truth)^2, cap) + N(0, noise); a share of the pixels replaced by U(0, cap) costs; three
    rows of flat costs."""
    s = SCENE
    H, W, D = s["H"], s["W"], s["D"]
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    truth = 2.0 + 8.0 * y / (H - 1) + 1.5 * np.cos(2 * np.pi * x / W)
    block = (y >= 14) & (y < 30) & ((x < 10) | (x >= W - 8))
    truth = np.where(block, truth + 3.0, truth)
    truth = np.clip(np.rint(truth), 0, D - 1)
    d = np.arange(D)[None, None, :]
    vol = np.minimum((d - truth[..., None]) ** 2, s["cap"]) + rng.normal(0.0, s["noise"], (H, W, D))
    out = rng.random((H, W)) < s["outliers"]
    vol[out] = rng.uniform(0.0, s["cap"], (int(out.sum()), D))
    for r in s["flat_rows"]:
        vol[r] = 4.0
    return vol.astype(F), truth.astype(F)


def off_by_more_than_one(flow, truth):
    return float((np.abs(flow - truth) > 1).mean())
