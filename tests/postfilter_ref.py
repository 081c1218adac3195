"""Plain numpy definitions of the kernels that turn a flow field into depth, confidence and mask (polar.hip, postfilters.hip, the
cartesian depth of postops.hip / cv_records.h), written from the reference's Lua and inline C -- not from oracle/dfe_oracle.c, which
tests/test_postfilter_ref_cpu.py holds against them.

Precision.  Where the reference's arithmetic is fp32 with every operation rounded by itself (a C `float` expression compiled without
fused multiply-adds), the definition does the same steps on np.float32 arrays, whose operations round one by one: it is comparable
bit for bit.  Where the summation order is free (OutputExtractor) or libm decides the last bit (the polar grids) the definition is
float64 and the tests state a bound."""
import numpy as np

F = np.float32
U = 2.0 ** -24   # unit roundoff of float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def one_ulp(ref):
    """|g - ref| <= 2^-23 |ref| + 2^-149: one float ulp -- half of it the final rounding, half for a double libm result that lies on
    the other side of a rounding boundary."""
    return 2.0 ** -23 * np.abs(np.asarray(ref, np.float64)) + 2.0 ** -149


# ---- image.warp(img, mask, 'bilinear', false)  radial/cartesian2polar.lua:91-93 ----------------------------------------------------
def warp_bilinear(img, mask, dtype=np.float64):
    """img [C][H][W], mask [2][Hd][Wd] (plane 0 = y, plane 1 = x, absolute 0-based coordinates) -> [C][Hd][Wd] in `dtype`.
    Coordinates are clamped to the image, NaN to 0.  The coordinates and weights are float32 whatever `dtype` is (wy = fy - y0 is
    exact); dtype=np.float32 rounds every product and sum of the two lerps by itself."""
    img, mask = np.asarray(img, F), np.asarray(mask, F)
    _, H, W = img.shape
    with np.errstate(invalid="ignore"):
        fy = np.where(mask[0] >= 0, np.minimum(mask[0], F(H - 1)), F(0)).astype(F)
        fx = np.where(mask[1] >= 0, np.minimum(mask[1], F(W - 1)), F(0)).astype(F)
    y0, x0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    wy, wx = (fy - y0.astype(F)).astype(dtype), (fx - x0.astype(F)).astype(dtype)
    p = img.astype(dtype)
    one = dtype(1)
    top = (one - wx) * p[:, y0, x0] + wx * p[:, y0, x1]
    bot = (one - wx) * p[:, y1, x0] + wx * p[:, y1, x1]
    return (one - wy) * top + wy * bot


def warp_bound(img):
    """Each lerp fl(fl(fl(1-w) a) + fl(w b)) errs by at most 3u M (M = max|img|); the outer lerp adds its own 3u M to the inner one's;
    one u for the second-order terms."""
    return 7 * U * float(np.abs(np.asarray(img, np.float64)).max())


# ---- flow -> depth -----------------------------------------------------------------------------------------------------------------
def _sq_sum(a, b):
    """fl(fl(a a) + fl(b b)) on float32 arrays"""
    return (a * a + b * b).astype(F)


def fused_sq_sums(a, b):
    """The two ways a compiler fuses a*a + b*b into a multiply and an fma: fl(a a + fl(b b)) and fl(fl(a a) + b b).  A float32 square
    is exact in float64; the sum is rounded to double before it is rounded to float, which moves a result only where the exact sum
    lies within 2^-29 ulp of a float tie."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return (a64 * a64 + (b * b).astype(F).astype(np.float64)).astype(F), ((a * a).astype(F).astype(np.float64) + b64 * b64).astype(F)


def radial_offsets(H, W, xc, yc):
    a = (np.arange(W, dtype=F) - F(xc))[None, :] + np.zeros((H, 1), F)
    b = (np.arange(H, dtype=F) - F(yc))[:, None] + np.zeros((1, W), F)
    return a.astype(F), b.astype(F)


def radial_distance(H, W, xc, yc):
    """d = sqrt(square((float)j - xcenter) + square((float)i - ycenter)): float squares and sum, the double sqrt of C, a float d"""
    a, b = radial_offsets(H, W, xc, yc)
    return np.sqrt(_sq_sum(a, b).astype(np.float64)).astype(F)


def flow_to_depth_radial(rflow, xc, yc, infty):
    """flow2depth, radial/radial_opticalflow_display.lua:6-58 -> (ret / infty, confs), float32"""
    f = np.asarray(rflow, F)
    H, W = f.shape
    infty = F(infty)
    d = radial_distance(H, W, xc, yc)
    far = d > F(10.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(far, np.where(f < F(0.1), infty, (d / f).astype(F)), F(0)).astype(F)   # ret zero-filled (:13)
        return (o / infty).astype(F), far.astype(F)                                        # confs filled with 1, 0 inside d <= 10


def flow_norm(flow):
    f = np.asarray(flow, F)
    return np.sqrt(_sq_sum(f[1], f[0]).astype(np.float64)).astype(F)


def flow_to_depth_cartesian(flow, mw, mh, fix_dot=False):
    """`radial` of test_opticalflow.lua:143-189 (flow plane 0 = dy, 1 = dx; (mw, mh) the focus of expansion; infty = W / 2) ->
    (depth, conf).  The confidence's dot product is px dx + dy dy as shipped (:181); fix_dot: px dx + py dy (this project's option)."""
    f = np.asarray(flow, F)
    _, H, W = f.shape
    infty = F(W / 2)
    px, py = radial_offsets(H, W, mw, mh)
    pn = np.sqrt(_sq_sum(px, py).astype(np.float64)).astype(F)
    dy, dx = f[0], f[1]
    dn = flow_norm(f)
    moving = dn >= F(0.2)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (pn / dn).astype(F)
        dot = (px * dx + (py * dy if fix_dot else dy * dy)).astype(F)
    r = np.where(moving, np.where(q < infty, q, infty), infty).astype(F)
    c = np.where(moving, dot > F(0.125), True).astype(F)
    return r, c


def c_round(x):
    """C's roundf: halves away from zero (in float64, where x + 0.5 is exact)"""
    x = np.asarray(x, np.float64)
    return np.trunc(x + np.copysign(0.5, x)).astype(np.int64)


def ardrone_histograms(xflow, mask):
    """[20][H][W]: per pixel the counts of round(xflow) = -8 .. 11 among the pixels with a non-zero mask in the half-open window
    [y-3, y+3) x [x-3, x+3), ardrone/ardrone_api.cpp:104-117 (values outside -8 .. 11 index past the reference's 20 bins: dropped)"""
    xflow, mask = np.asarray(xflow, F), np.asarray(mask, F)
    H, W = xflow.shape
    r = c_round(xflow)
    ya, yb = np.maximum(np.arange(H) - 3, 0), np.minimum(np.arange(H) + 3, H)
    xa, xb = np.maximum(np.arange(W) - 3, 0), np.minimum(np.arange(W) + 3, W)
    hist = np.zeros((20, H, W), np.int64)
    for v in range(20):
        hit = np.zeros((H + 1, W + 1), np.int64)
        hit[1:, 1:] = np.cumsum(np.cumsum((mask != 0) & (r == v - 8), 0), 1)
        hist[v] = hit[yb][:, xb] - hit[ya][:, xb] - hit[yb][:, xa] + hit[ya][:, xa]
    return hist


def flow_to_depth_ardrone(xflow, mask, m):
    """ARdroneAPI::computeDepthMapFromFlow, ardrone/ardrone_api.cpp:99-140 -> (depthMap, confidenceMap): the window's most frequent
    rounded flow (the first of equally full bins), depth m |x - W/2| / |mode|, 100 where |mode| < 1.1; confidence 1 where mask > 0.5
    off the middle column, else confidence 0 and depth 0 (uninitialised there)."""
    xflow, mask = np.asarray(xflow, F), np.asarray(mask, F)
    H, W = xflow.shape
    hist = ardrone_histograms(xflow, mask)
    mode = np.where(hist.max(0) > 0, hist.argmax(0) - 8, 0)   # argmax: the first maximum; no sample: im stays 0
    amode = np.abs(mode).astype(F)
    off = np.abs(np.arange(W) - W // 2).astype(F)[None, :]
    conf = (mask > F(0.5)) & (off != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(amode < F(1.1), F(100.0), ((F(m) * off).astype(F) / amode).astype(F))
    return np.where(conf, d, F(0)).astype(F), conf.astype(F)


# ---- postProcessImage, opticalflow_model.lua:323-472 -------------------------------------------------------------------------------
def rounded_span(flow):
    """(minimum, maximum) of floor(input + 0.5): the 'max' filter's 16 x 16 histogram holds a span of 15"""
    R = np.floor(np.asarray(flow, F) + F(0.5))
    return float(R.min()), float(R.max())


def window_codes(flow, mask, k, i, j):
    """the histogram codes vx + 16 vy of the masked pixels of the k x k window at (i, j)"""
    flow = np.asarray(flow, F)
    R = np.floor(flow + F(0.5)).astype(F)
    Rm = (R - R.min()).astype(np.int64)
    sel = np.asarray(mask)[i : i + k, j : j + k] != 0
    return (Rm[1] + 16 * Rm[0])[i : i + k, j : j + k][sel]


def postprocess_mode(flow, mask, k):
    """method 'max': the most frequent (vx, vy) of the rounded flow among the masked pixels of each window [i, i+k) x [j, j+k),
    i < h - k, j < w - k, written at (i + k/2, j + k/2); the lowest code vx + 16 vy of equally frequent ones, code 0 for an empty
    window; everything -- the untouched border too -- lifted by the minimum m.  None where the rounded flow spans more than 15."""
    flow, mask = np.asarray(flow, F), np.asarray(mask, F)
    _, H, W = flow.shape
    lo, hi = rounded_span(flow)
    if hi - lo > 15:
        return None
    out = np.zeros((2, H, W), F)
    for i in range(H - k):
        for j in range(W - k):
            im = int(np.bincount(window_codes(flow, mask, k, i, j), minlength=256).argmax())
            out[1, i + k // 2, j + k // 2] = im % 16
            out[0, i + k // 2, j + k // 2] = im // 16
    return (out + F(lo)).astype(F)


def window_values(flow, mask, k, i, j):
    sel = np.asarray(mask)[i : i + k, j : j + k] != 0
    return [np.sort(np.asarray(flow, F)[pl, i : i + k, j : j + k][sel]) for pl in range(2)]


def postprocess_median(flow, mask, k):
    """method 'med': per component t[n/2] of the n sorted masked window values -- the upper middle one where n is even -- 0 for an
    empty window and on the border"""
    flow = np.asarray(flow, F)
    _, H, W = flow.shape
    out = np.zeros((2, H, W), F)
    for i in range(H - k):
        for j in range(W - k):
            for pl, t in enumerate(window_values(flow, mask, k, i, j)):
                out[pl, i + k // 2, j + k // 2] = t[len(t) // 2] if len(t) else 0
    return out


# ---- enlargeMask, depth_estimation_api.lua:76-132 ----------------------------------------------------------------------------------
def _erode_line(v, n):
    """v: a writable 1-D view.  n pixels from the first set one (> 0.5) on are cleared, then n pixels back from the last one still set"""
    s = np.flatnonzero(v > 0.5)
    if s.size:
        v[s[0] : s[0] + n] = 0
    s = np.flatnonzero(v > 0.5)
    if s.size and n > 0:
        v[max(s[-1] - n + 1, 0) : s[-1] + 1] = 0


def enlarge_mask(mask, ix, iy):
    """rows first, then the columns of the row-eroded mask; returns a new array"""
    m = np.array(mask, F)
    for i in range(m.shape[0]):
        _erode_line(m[i], ix)
    for j in range(m.shape[1]):
        _erode_line(m[:, j], iy)
    return m


# ---- nn.OutputExtractor (OutputExtractor.lua:7-35) and the 'mean' marginal (opticalflow_model.lua:192) -----------------------------
def output_extractor(prob, maxh, maxw):
    """prob [...][maxh * maxw] -> (x, y, sx, sy) in float64: x = sum_k p_k j(k), y = sum_k p_k i(k) with 1-based cell coordinates
    k = (i - 1) maxw + j; sx, sy = sum_k |p_k| coord_k, what the bound scales with"""
    p = np.asarray(prob, F).astype(np.float64)
    k = np.arange(maxh * maxw)
    cx, cy = (k % maxw + 1).astype(np.float64), (k // maxw + 1).astype(np.float64)
    return p @ cx, p @ cy, np.abs(p) @ cx, np.abs(p) @ cy


def extractor_bound(N, s):
    """one rounding of each product, the ceil(N / 64) - 1 additions of a lane's partial sum and six butterfly additions, each at most
    u times the sum of the magnitudes (fused products only lower it); one u for the second-order terms"""
    return (-(-N // 64) + 7) * U * s


def marginal_sum(inp, A, B):
    """input:reshape(.., A, B):sum(last): TH adds floats into a double accumulator in index order, the result narrowed to float"""
    x = np.asarray(inp, F).reshape(-1, A, B)
    acc = np.zeros(x.shape[:2], np.float64)
    for b in range(B):
        acc += x[:, :, b]
    return acc.astype(F)


# ---- polar grids, radial/cartesian2polar.lua:4-89 ----------------------------------------------------------------------------------
def polar_grid_c2p(wdst, hdst, xc, yc, lpad, rpad, rmax, alpha=1.0):
    """getC2PMask -> float64 [2][hdst][lpad + wdst + rpad].  kr, ktheta, alpha, r and theta = ktheta * j are the inline C's float
    variables; pow, sin and cos are double; the padded columns repeat the last lpad and the first rpad core columns."""
    alpha, xc, yc = F(alpha), F(xc), F(yc)
    kr = F(float(F(rmax)) / float(hdst) ** float(alpha))
    ktheta = F(2 * np.pi / wdst)
    r = (float(kr) * np.arange(hdst, dtype=np.float64) ** float(alpha)).astype(F).astype(np.float64)[:, None]
    th = (ktheta * np.arange(wdst, dtype=F)).astype(F).astype(np.float64)[None, :]
    core = np.stack([r * np.sin(th) + float(yc), r * np.cos(th) + float(xc)])
    return np.concatenate([core[:, :, wdst - lpad :], core, core[:, :, :rpad]], 2)


def polar_grid_p2c(wsrc, hsrc, wdst, hdst, xc, yc, rmax, alpha=1.0):
    """getP2CMask -> float64 [2][hdst][wdst].  kx, ky (from the Lua numbers wsrc / 2 pi and hsrc / rmax^(1/alpha)), pi2 and
    invalpha = (1 / alpha) * 0.5f are float variables, x x + y y a float expression; pow, atan2 and fmod are double."""
    alpha = F(alpha)
    pi2 = float(F(2 * np.pi))
    kx = float(F(wsrc / (2 * np.pi)))
    ky = float(F(hsrc / float(rmax) ** (1.0 / float(alpha))))
    invalpha = float(F(1.0 / float(alpha)) * F(0.5))
    x, y = radial_offsets(hdst, wdst, xc, yc)
    s = _sq_sum(x, y).astype(np.float64)
    return np.stack([s ** invalpha * ky, np.fmod(np.arctan2(y.astype(np.float64), x.astype(np.float64)) + pi2, pi2) * kx])
