"""The census cost of the radial (polar) matcher in numpy, written from the definition in include/dfe.h, not from
the device's walk: signatures of a polar frame with wrap columns, the Hamming distance down the polar rows, the box whose columns are a
ring, the first minimum, the match score, the sub-pixel rule.  Whole arrays at a time; nothing here knows about tiles, lanes or labels
dealt to waves.  Also the polar exposure scene of the quality table."""
import numpy as np

from tests.census_ref import popcount, signature


def wrap(I, kw):
    """a polar frame [C][H][W] with its kw - 1 wrap columns, (kw - 1) // 2 on the left: padded column jp shows column (jp - lpad) mod W"""
    W = I.shape[2]
    lpad = (kw - 1) // 2
    return I[:, :, (np.arange(W + kw - 1) - lpad) % W]


def signatures(I, kh, kw):
    """[C][H][W] polar frame -> uint64 [C][H - kh + 1][W]: column x's patch is centred on polar column x"""
    return signature(wrap(I, kw), kh, kw)


def hamming(S0, S1, hWin):
    """h[y][x][d] = sum_c popcount(S0[c][y][x] ^ S1[c][y + d][x]): int64 [H1][W][hWin], H1 = Hp - hWin + 1"""
    C, Hp, W = S0.shape
    H1 = Hp - hWin + 1
    h = np.empty((H1, W, hWin), dtype=np.int64)
    for d in range(hWin):
        h[:, :, d] = popcount(S0[:, :H1] ^ S1[:, d:d + H1]).sum(0)
    return h


def aggregate(h, a):
    """cost[y][x][d] = sum_{u < a, v < a} h[y + u][(x + v - a // 2) mod W][d]: the rows shrink, the columns are a ring"""
    H1, W = h.shape[:2]
    assert a <= W
    Ha = H1 - a + 1
    cost = np.zeros((Ha,) + h.shape[1:], dtype=np.int64)
    for u in range(a):
        for v in range(a):
            cost += np.roll(h[u:u + Ha], -(v - a // 2), axis=1)      # rolled[x] = h[(x + v - a // 2) mod W]
    return cost


def cost_volume(S0, S1, hWin, a):
    return aggregate(hamming(S0, S1, hWin), a)


def match_score(best, nbits, C, a):
    """1.0f - (float)best / (float)(nbits C a^2): one rounded fp32 division, one rounded subtraction"""
    return (np.float32(1.0) - best.astype(np.float32) / np.float32(nbits * C * a * a)).astype(np.float32)


def subpixel(cost, bi):
    """dfe_radial_refine_subpixel_f32's rule on float32 costs [..][hWin] and their integer first minimum: every operation fp32"""
    c = cost.astype(np.float32)
    hWin = c.shape[-1]
    inside = (bi >= 1) & (bi + 1 < hWin)
    j = np.clip(bi, 1, max(hWin - 2, 1))[..., None]
    cm = np.take_along_axis(c, np.maximum(j - 1, 0), -1)[..., 0]
    c0 = np.take_along_axis(c, np.minimum(j, hWin - 1), -1)[..., 0]
    cp = np.take_along_axis(c, np.minimum(j + 1, hWin - 1), -1)[..., 0]
    den = ((cm - c0) + (cp - c0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        off = ((cm - cp) / (np.float32(2.0) * den)).astype(np.float32)
    off = np.minimum(np.maximum(off, np.float32(-0.5)), np.float32(0.5))
    off = np.where(inside & (den > 0), off, np.float32(0.0)).astype(np.float32)
    return (bi.astype(np.float32) + off).astype(np.float32)


def flow(S0, S1, nbits, hWin, a, sub=False, zero_last_row=False):
    """what dfe_census_radial_flow_f32 returns: dict(output float32 [Ha][W][hWin], flow, best, match float32 [Ha][W])"""
    cost = cost_volume(S0, S1, hWin, a)
    bi = cost.argmin(-1)                     # numpy's argmin is the first one: the strict scan from 0
    best = cost.min(-1)
    f = subpixel(cost, bi) if sub else bi.astype(np.float32)
    if zero_last_row:
        f = f.copy()
        f[-1] = 0
    return dict(output=cost.astype(np.float32), flow=f, best=best.astype(np.float32), match=match_score(best, nbits, S0.shape[0], a))


# ---- the polar exposure scene: a smooth random texture moved outward by a whole number of rows, the second frame darker, offset, noisy ----
SCENE = dict(H=64, W=96, k=7, hWin=8, move=3, gain=0.5, offset=40.0, sigma=1.0, margin=8)


def scene(seed):
    """two uint8 polar frames [1][64][96]: frame 1 is frame 0 moved 3 rows outward, times 0.5, plus 40, plus N(0, 1); both floored and
    clipped to 0 .. 255.  The truth is label 3."""
    rng = np.random.RandomState(seed)
    H, W, m, mv = SCENE["H"], SCENE["W"], SCENE["margin"], SCENE["move"]
    t = rng.uniform(size=(H + 2 * m, W))
    for _ in range(4):                     # the 5-point mean, with wrap-around
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    f0 = t[m:m + H]
    f1 = t[m - mv:m - mv + H] * SCENE["gain"] + SCENE["offset"] + rng.normal(0.0, SCENE["sigma"], size=(H, W))   # f1[y + 3] = f0[y]
    to_u8 = lambda f: np.clip(np.floor(f), 0, 255).astype(np.uint8)[None]
    return to_u8(f0), to_u8(f1)


def share_wrong(f):
    return float(np.mean(f != SCENE["move"]))


def ssd_flow(I0, I1, kh, kw, hWin, a):
    """float64 sum of squared differences over the same (k + a - 1)^2 ring support: the first minimum over d, [Ha][W]"""
    s = (kh + a - 1, kw + a - 1)
    P0, P1 = wrap(I0.astype(np.float64), s[1]), wrap(I1.astype(np.float64), s[1])
    C, H, W = I0.shape
    Hq = H - s[0] + 1
    Ha = Hq - hWin + 1
    cost = np.zeros((Ha, W, hWin))
    for d in range(hWin):
        for i in range(s[0]):
            for j in range(s[1]):
                df = P0[:, i:i + Ha, j:j + W] - P1[:, d + i:d + i + Ha, j:j + W]
                cost[:, :, d] += (df * df).sum(0)
    return cost.argmin(-1)
