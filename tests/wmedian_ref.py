"""The guided weighted median (dfe_weighted_median_f32; include/dfe.h) restated in numpy, and the two-motion scene
that shows what the guide is for.  A helper, no tests.

The definition is exact: the sample weight is made in float32 by a fixed sequence of operations (numpy float32 arrays round every
operation separately, as the kernel does without fused multiply-adds) and is an integer from there on, so the device is compared bit
for bit.  Two forms: wmedian_pixel is the definition read literally for one pixel (a stable sort by key, searchsorted on 2 cumsum);
weighted_median_ref does all pixels of R at once on [k * k][Ho][Wo] stacks, and the CPU tests hold the two against each other."""
import numpy as np

from tests.field_rule import validity

F = np.float32


def keys_of(v):
    """order-preserving integer image of the float32 bits (-0 below +0), as int64"""
    u = np.ascontiguousarray(v, F).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.int64)


def sample_weight(a_q, g_p, g_q, inv_s2):
    """wt(p, q) as int64 from a(q) and the guide values [Cg][...] at p and q (g_p None: no range term); float32 throughout"""
    a_q = np.asarray(a_q, F)
    with np.errstate(all="ignore"):
        if g_p is None:
            t = a_q
        else:
            d2 = None
            for c in range(len(g_p)):
                d = np.asarray(g_p[c], F) - np.asarray(g_q[c], F)
                s = d * d
                d2 = s if d2 is None else d2 + s
            r = F(1) - d2 * F(inv_s2)
            r = np.where(np.isfinite(r) & (r > 0), r, F(0)).astype(F)      # max(0, .), not finite -> 0
            t = a_q * r
        t = t * F(4096.0) + F(0.5)
        assert np.asarray(t).dtype == F
        return np.where(a_q > 0, t, F(0)).astype(np.uint32).astype(np.int64)


def inv_sigma2(guide, sigma):
    """None without a range term, else the host's float32 1 / (sigma sigma)"""
    if guide is None or len(guide) == 0 or not F(sigma) > 0:
        return None
    with np.errstate(all="ignore"):
        return F(1.0) / (F(sigma) * F(sigma))


def wmedian_pixel(v, w, guide, sigma, k, region, y, x):
    """the definition for the pixel (y, x) of the frame, inside R: (out [C] float32, filtered)"""
    v = np.asarray(v, F)
    y0, x0, Ho, Wo = region
    h = k // 2
    a = validity(v, w)
    inv_s2 = inv_sigma2(guide, sigma)
    ys = [yy for yy in range(y - h, y + h + 1) if y0 <= yy < y0 + Ho]
    xs = [xx for xx in range(x - h, x + h + 1) if x0 <= xx < x0 + Wo]
    qy, qx = (g.ravel() for g in np.meshgrid(ys, xs, indexing="ij"))
    if inv_s2 is None:
        wt = sample_weight(a[qy, qx], None, None, None)
    else:
        g = np.asarray(guide, F)
        wt = sample_weight(a[qy, qx], g[:, y, x][:, None], g[:, qy, qx], inv_s2)
    T = int(wt.sum())
    out = np.zeros(v.shape[0], F)
    if T == 0:
        return out, F(0)
    for c in range(v.shape[0]):
        vals = v[c, qy, qx][wt > 0]
        order = np.argsort(keys_of(vals), kind="stable")
        i = int(np.searchsorted(2 * np.cumsum(wt[wt > 0][order]), T, side="left"))
        out[c] = vals[order[i]]
    return out, F(1)


def weighted_median_ref(v, w=None, guide=None, sigma=0.0, k=7, region=None):
    """(out [C][H][W], filtered [H][W]) float32, zero outside R"""
    v = np.ascontiguousarray(v, F)
    C, H, W = v.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else region
    assert k % 2 == 1 and 1 <= k <= 15 and Ho > 0 and Wo > 0 and y0 >= 0 and x0 >= 0 and y0 + Ho <= H and x0 + Wo <= W
    h = k // 2
    R = (slice(y0, y0 + Ho), slice(x0, x0 + Wo))
    a = np.pad(validity(v, w)[R], h)                                        # samples outside R do not exist: a = 0
    keys = np.pad(keys_of(v)[(slice(None),) + R], ((0, 0), (h, h), (h, h)))
    bits = np.pad(v.view(np.uint32)[(slice(None),) + R], ((0, 0), (h, h), (h, h)))
    inv_s2 = inv_sigma2(guide, sigma)
    g = None if inv_s2 is None else np.pad(np.ascontiguousarray(guide, F)[(slice(None),) + R], ((0, 0), (h, h), (h, h)))
    shifts = [(dy, dx) for dy in range(k) for dx in range(k)]
    win = lambda plane, dy, dx: plane[..., dy : dy + Ho, dx : dx + Wo]
    g_p = None if g is None else win(g, h, h)
    wt = np.stack([sample_weight(win(a, dy, dx), g_p, None if g is None else win(g, dy, dx), inv_s2) for dy, dx in shifts])   # [k k][Ho][Wo]
    T = wt.sum(axis=0)
    out = np.zeros((C, H, W), F)
    filtered = np.zeros((H, W), F)
    filtered[R] = (T > 0).astype(F)
    for c in range(C):
        kc = np.stack([win(keys[c], dy, dx) for dy, dx in shifts])
        bc = np.stack([win(bits[c], dy, dx) for dy, dx in shifts])
        kc = np.where(wt > 0, kc, np.int64(1) << 40)                        # samples of weight 0 behind every key
        order = np.argsort(kc, axis=0, kind="stable")
        cum2 = 2 * np.cumsum(np.take_along_axis(wt, order, axis=0), axis=0)
        i = (cum2 >= T[None]).argmax(axis=0)                                # the first sorted sample with 2 S >= T
        sel = np.take_along_axis(bc, np.take_along_axis(order, i[None], axis=0), axis=0)[0]
        out[c][R] = np.where(T > 0, sel, np.uint32(0)).astype(np.uint32).view(F)
    return out, filtered


# ---- the two-motion scene ----------------------------------------------------------------------------------------------------------
SCENE = dict(H=64, W=96, rect=(20, 28, 24, 40), fg=(-2.0, 3.0), bg=(1.0, -2.0), band=2, corner=7, outliers=0.10, k=11, sigma=40.0)


def two_motion_scene(seed, s=SCENE):
    """A rectangle moving by fg over a background moving by bg; the `band` pixels inside the rectangle's edge carry the background's
    motion (what a fill, or a matcher's patch, leaves there) and a share `outliers` of all pixels a uniform random flow in +-8.
    Returns dict(flow [2][H][W] the damaged field, truth [2][H][W], guide [1][H][W] a byte-valued image (background 60 +- 5, rectangle
    180 +- 5), band: the band pixels at least `corner` pixels along the side from a corner, nonband: every pixel outside the band)."""
    H, W = s["H"], s["W"]
    ry, rx, rh, rw = s["rect"]
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inside = (yy >= ry) & (yy < ry + rh) & (xx >= rx) & (xx < rx + rw)
    b = s["band"]
    core = (yy >= ry + b) & (yy < ry + rh - b) & (xx >= rx + b) & (xx < rx + rw - b)
    band_all = inside & ~core
    m = s["corner"]
    along = ((yy >= ry + m) & (yy < ry + rh - m)) | ((xx >= rx + m) & (xx < rx + rw - m))
    fg, bg = np.array(s["fg"], F).reshape(2, 1, 1), np.array(s["bg"], F).reshape(2, 1, 1)
    truth = np.where(inside[None], fg, bg).astype(F)
    flow = np.where(core[None], fg, bg).astype(F)
    out = rng.random((H, W)) < s["outliers"]
    flow[:, out] = rng.uniform(-8, 8, size=(2, int(out.sum()))).astype(F)
    guide = (np.where(inside, 180, 60) + rng.integers(-5, 6, size=(H, W))).astype(F)[None]
    return dict(flow=flow, truth=truth, guide=guide, band=band_all & along, nonband=~band_all)


def scene_scores(out, scene):
    """(share of the band pixels within 0.5 px of the rectangle's motion, share of the non-band pixels off their true motion by >= 0.5 px)"""
    err = np.hypot(*(out.astype(np.float64) - scene["truth"]))
    return float((err[scene["band"]] < 0.5).mean()), float((err[scene["nonband"]] >= 0.5).mean())
