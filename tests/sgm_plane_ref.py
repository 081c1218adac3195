"""Semi-global aggregation on a two-dimensional label plane as include/dfe.h defines it (dfe_sgm_plane_aggregate_f32),
restated in numpy: float32 throughout, every operation rounded on its own, in the header's order.  Written from the definition -- a pixel,
its predecessor p - r, the start where that predecessor lies outside the plane -- and not from the device's walk along lines; nothing here
knows about waves, lanes or padding cells.  Every path is available on its own (plane_path).  Also the band scene of the quality table."""
import functools

import numpy as np

from tests import census_ref as cr

F = np.float32
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))   # (dy, dx) of bit r


def _shift(prev, axis, by):
    """prev's label one cell away along `axis` (by = +1: the cell before, -1: the cell after), +Inf beyond the window"""
    out = np.full_like(prev, np.inf)
    src = [slice(None)] * prev.ndim
    dst = [slice(None)] * prev.ndim
    if by > 0:
        src[axis], dst[axis] = slice(None, -1), slice(1, None)
    else:
        src[axis], dst[axis] = slice(1, None), slice(None, -1)
    out[tuple(dst)] = prev[tuple(src)]
    return out


def _step(prev, c, P1, P2):
    """L_r(p, .) from L_r(q, .) (prev [..., hWin, wWin]) and C(p, .) (c, the same shape)"""
    P1, P2 = F(P1), F(P2)
    m = prev.min(axis=(-2, -1), keepdims=True)
    t = prev
    t = np.minimum(t, (_shift(prev, -1, +1) + P1).astype(F))      # (dy, dx - 1)
    t = np.minimum(t, (_shift(prev, -1, -1) + P1).astype(F))      # (dy, dx + 1)
    t = np.minimum(t, (_shift(prev, -2, +1) + P1).astype(F))      # (dy - 1, dx)
    t = np.minimum(t, (_shift(prev, -2, -1) + P1).astype(F))      # (dy + 1, dx)
    t = np.minimum(t, (m + P2).astype(F))
    return (c + (t - m).astype(F)).astype(F)


def plane_path(C, r, P1, P2):
    """L_r [H][W][hWin][wWin] of the volume C for direction r (0 .. 7)"""
    C = np.ascontiguousarray(C, F)
    H, W = C.shape[:2]
    dy, dx = DIRS[r]
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(L[:, x - dx], C[:, x], P1, P2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    xs = np.arange(W)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]                                            # the predecessor's row lies outside
            continue
        qx = xs - dx                                               # the predecessor's column
        inside = (qx >= 0) & (qx < W)
        L[y] = C[y]
        if inside.any():
            L[y][inside] = _step(L[y - dy][qx[inside]], C[y][inside], P1, P2)
    return L


def plane_sum(C, P1, P2, paths=0x0f):
    """the paths summed in ascending bit order"""
    assert 1 <= paths <= 255
    agg = None
    for r in range(8):
        if paths >> r & 1:
            L = plane_path(C, r, P1, P2)
            agg = L if agg is None else (agg + L).astype(F)
    return agg


def arg_best(agg):
    """(idx 1-based int64, flow_y, flow_x float32): the first minimum in class order, the centre class winning an exact tie"""
    H, W, hWin, wWin = agg.shape
    flat = agg.reshape(H, W, hWin * wWin)
    idx = flat.argmin(-1) + 1                                      # (numpy's argmin: the first of equal minima)
    mid = cr.middle_index(hWin, wWin)
    idx[flat[:, :, mid - 1] == flat.min(-1)] = mid
    idx = idx.astype(np.int64)
    fy, fx = cr.decode(idx, hWin, wWin)
    return idx, fy, fx


def plane_aggregate(C, P1, P2, paths=0x0f):
    """what dfe_sgm_plane_aggregate_f32 returns: dict(agg, idx, flow_y, flow_x)"""
    agg = plane_sum(C, P1, P2, paths)
    idx, fy, fx = arg_best(agg)
    return dict(agg=agg, idx=idx, flow_y=fy, flow_x=fx)


def raw_at(C, idx):
    """C(p, idx(p)) of a volume [H][W][hWin][wWin] and 1-based classes [H][W]"""
    H, W = idx.shape
    return np.take_along_axis(C.reshape(H, W, -1), (idx - 1)[..., None], -1)[..., 0]


# ---- the band scene: census_ref.scene with a flat band of six rows and noise in both frames ----
BAND = dict(rows=(33, 39), value=128.0, agg=3, P1=144.0, P2=864.0)


def band_scene(seed, gain=cr.SCENE["gain"], offset=cr.SCENE["offset"]):
    """two uint8 frames [1][72][104]: census_ref.scene's texture with rows 33 .. 38 of the frame set to 128 before the two frames are cut,
    N(0, 1) added to frame 0 as well as to frame 1; the same gain, offset, move, floor and clip.  One RandomState(seed), drawn in the order
    texture, frame-0 noise, frame-1 noise."""
    s = cr.SCENE
    rng = np.random.RandomState(seed)
    H, W, m = s["H"], s["W"], s["margin"]
    t = rng.uniform(size=(H + 2 * m, W + 2 * m))
    for _ in range(4):                     # the 5-point mean, with wrap-around
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    t[m + BAND["rows"][0]:m + BAND["rows"][1]] = BAND["value"]
    my, mx = s["move"]
    f0 = t[m:m + H, m:m + W] + rng.normal(0.0, s["sigma"], size=(H, W))
    f1 = t[m - my:m - my + H, m - mx:m - mx + W] * gain + offset + rng.normal(0.0, s["sigma"], size=(H, W))
    to_u8 = lambda f: np.clip(np.floor(f), 0, 255).astype(np.uint8)[None]
    return to_u8(f0), to_u8(f1)


@functools.lru_cache(maxsize=None)
def band_volume(seed):
    """the census cost volume of the band scene at k = 7, 9 x 9, agg = 3, as the float32 the device stores"""
    f0, f1 = band_scene(seed)
    k, win = cr.SCENE["k"], cr.SCENE["win"]
    return cr.cost_volume(cr.signature(f0, k, k), cr.signature(f1, k, k), win, win, BAND["agg"]).astype(F)


@functools.lru_cache(maxsize=None)
def band_flow(seed, paths):
    """(idx, flow_y, flow_x) of the band scene: paths = 0 is winner-takes-all on the raw volume, else the aggregate at BAND's penalties.
    Computed once per process and shared by the tests that read it (read only)"""
    vol = band_volume(seed)
    return arg_best(vol if paths == 0 else plane_sum(vol, BAND["P1"], BAND["P2"], paths))


def band_share_wrong(seed, paths):
    _, fy, fx = band_flow(seed, paths)
    return cr.share_wrong(fy, fx)
