"""float64 numpy reference of the sparse corner tracker (csrc/tracker.hip), written from the definitions of DESIGN section 4 and
independent of the kernels: corner_response64, select64, pyr_down64, lk64 -- and the synthetic inputs the tracker tests share: a smooth
texture (a sum of random sinusoids, so that a frame moved by any sub-pixel amount is the same function evaluated elsewhere and the
planted truth is exact) and a two-view pair rendered from it by inverse warping through a smooth non-planar depth."""
import numpy as np

_cache = {}


# ------------------------------------------------------------------------------------------------------------------- inputs
def texture(n=24, lo=8.0, hi=40.0, seed=0):
    """tex(x, y) -> values in 0 .. 255: n sinusoids, wavelengths lo .. hi px, random orientation and phase.  The scaling is taken over a
    1024 x 1024 grid once, so it does not depend on the frame the caller evaluates."""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(lo, hi, n)
    th = rng.uniform(0, 2 * np.pi, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    kx, ky = 2 * np.pi / lam * np.cos(th), 2 * np.pi / lam * np.sin(th)

    def raw(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return np.sin(x[..., None] * kx + y[..., None] * ky + ph).sum(-1)

    g = np.arange(0, 1024, 4.0)
    v = raw(g[None, :], g[:, None])
    a, b = v.min(), v.max()
    return lambda x, y: (raw(x, y) - a) * (255.0 / (b - a))


def shifted_pair(H, W, dx, dy, seed=0):
    """(frame 0, frame 1) float32 [H][W] with frame1(p + d) = frame0(p): every point of frame 0 moves by d = (dx, dy)"""
    key = ("pair", H, W, dx, dy, seed)
    if key not in _cache:
        tex = texture(seed=seed)
        x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
        a, b = tex(x + 0 * y, y + 0 * x).astype(np.float32), tex(x - dx + 0 * y, y - dy + 0 * x).astype(np.float32)
        a.setflags(write=False); b.setflags(write=False)
        _cache[key] = (a, b)
    return _cache[key]


def rotation(a, b, c):
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def two_view_pair(H=240, W=320):
    """Frames of one textured surface seen from two poses, x2 = R x1 + t: frame 0 is tex(p), frame 1 at p2 is
    tex(pi(R^T (Z(p2) K^-1 p2 - t))) with the depth Z given in frame 2.  The default 240 x 320 pair is the one the tests use; other sizes
    (the timing tool) scale the camera and the depth pattern with the width.  -> dict(im0, im1 float32, K, R, T (unit), flow_max)"""
    key = ("two", H, W)
    if key not in _cache:
        s = W / 320.0
        K = np.array([[260.0 * s, 0, 160.0 * s], [0, 257.5 * s, 119.0 * s], [0, 0, 1]])
        R = rotation(0.015, -0.01, 0.0075)
        t = np.array([0.08, -0.03, -0.35])
        tex = texture(n=40, lo=6.0, hi=30.0, seed=3)
        x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        Z = 6 + 2.5 * np.sin(x / (37 * s)) * np.cos(y / (29 * s)) + 0.01 * (x / s - 160)
        p2 = np.stack([x, y, np.ones_like(x)], -1)
        X2 = (p2 @ np.linalg.inv(K).T) * Z[..., None]
        X1 = (X2 - t) @ R                                      # R^T (X2 - t), row vectors
        q = X1 @ K.T
        sx, sy = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
        im0, im1 = tex(x, y).astype(np.float32), tex(sx, sy).astype(np.float32)
        im0.setflags(write=False); im1.setflags(write=False)
        _cache[key] = dict(im0=im0, im1=im1, K=K, R=R, T=t / np.linalg.norm(t), flow_max=float(np.hypot(x - sx, y - sy).max()))
    return _cache[key]


# the end-to-end route on the two-view pair.  RANSAC distance: the tracker's median Sampson distance to the planted F is 0.06 px and its
# 75 % quantile 0.12 px, so 0.3 px keeps the good tracks and drops the biased ones (windows half outside the frame, the depth relief) that
# 1 px lets into the refit
ROUTE = dict(quality=0.01, min_dist=10, max_points=300, win=21, levels=3, max_iters=30, eps=0.01, min_eig=1e-4, ransac=0.3, iterations=512, seed=0)


# --------------------------------------------------------------------------------------------------------------- definitions
def corner_response64(Y):
    """-> (resp, a, c): gx = (Y(y, x+1) - Y(y, x-1)) / 2 with clamped indices, gy likewise; a, b, c = sums of gx^2, gx gy, gy^2 over the
    3 x 3 block (clamped indices); resp = ((a + c) - sqrt((a - c)^2 + 4 b^2)) / 2"""
    Y = np.asarray(Y, np.float64)
    H, W = Y.shape
    xi, yi = np.arange(W), np.arange(H)
    gx = (Y[:, np.minimum(xi + 1, W - 1)] - Y[:, np.maximum(xi - 1, 0)]) / 2
    gy = (Y[np.minimum(yi + 1, H - 1), :] - Y[np.maximum(yi - 1, 0), :]) / 2

    def box(p):
        q = np.pad(p, 1, mode="edge")                           # the product AT the clamped position
        return sum(q[i:i + H, j:j + W] for i in range(3) for j in range(3))

    a, b, c = box(gx * gx), box(gx * gy), box(gy * gy)
    return 0.5 * ((a + c) - np.sqrt((a - c) ** 2 + 4 * b * b)), a, c


def select64(resp, quality, min_dist, max_points):
    """The corners of a float32 response map by the definition -> (pts [n][2] = (x, y) float32, responses [n] float32, n_kept before the
    cut to max_points).  Exact: only comparisons of float32 values and one float32 product."""
    resp = np.asarray(resp, np.float32)
    H, W = resp.shape
    empty = (np.zeros((0, 2), np.float32), np.zeros(0, np.float32), 0)
    if np.isnan(resp).all():
        return empty
    M = np.nanmax(resp)
    if not M > 0:
        return empty
    with np.errstate(invalid="ignore"):
        thr = np.float32(quality) * np.float32(M)
        cand = (resp > 0) & (resp >= thr)
        R2 = int(np.floor(float(min_dist) ** 2))
        r = int(np.floor(np.sqrt(R2)))
        idx = np.arange(H * W).reshape(H, W)
        dominated = np.zeros((H, W), bool)
        for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
            for dx in range(-min(r, W - 1), min(r, W - 1) + 1):
                if (dy == 0 and dx == 0) or dy * dy + dx * dx > R2:
                    continue
                # p = (y, x) against q = (y + dy, x + dx), where both are inside the frame
                ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
                yq, xq = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
                vp, vq = resp[ys, xs], resp[yq, xq]
                dominated[ys, xs] |= (vq > vp) | ((vq == vp) & (idx[yq, xq] < idx[ys, xs]))
    kept = np.flatnonzero((cand & ~dominated).reshape(-1))
    v = resp.reshape(-1)[kept]
    order = np.lexsort((kept, -v.astype(np.float64)))
    kept, v = kept[order][:max_points], v[order][:max_points]
    return np.stack([kept % W, kept // W], 1).astype(np.float32), v, int(order.size)


def corners64(Y, quality, min_dist, max_points):
    """response in float64, rounded to float32 as the device's map is, then the selection"""
    return select64(corner_response64(Y)[0].astype(np.float32), quality, min_dist, max_points)[0]


def _reflect(i, n):
    if n == 1:
        return np.zeros_like(i)
    per = 2 * (n - 1)
    m = np.mod(i, per)
    return np.where(m < n, m, per - m)


def pyr_down64(I):
    I = np.asarray(I, np.float64)
    H, W = I.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    w = np.array([1, 4, 6, 4, 1]) / 16.0
    out = np.zeros((Ho, Wo))
    for i in range(5):
        ry = _reflect(2 * np.arange(Ho) + i - 2, H)
        for j in range(5):
            rx = _reflect(2 * np.arange(Wo) + j - 2, W)
            out += w[i] * w[j] * I[np.ix_(ry, rx)]
    return out


def sample64(I, x, y):
    """bilinear sample, the coordinates clamped to the frame first (a NaN coordinate reads position 0: such a point is lost anyway)"""
    H, W = I.shape
    x = np.clip(np.where(np.isnan(x), 0.0, x), 0, W - 1)
    y = np.clip(np.where(np.isnan(y), 0.0, y), 0, H - 1)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - x0, y - y0
    top = I[y0, x0] + fx * (I[y0, x1] - I[y0, x0])
    bot = I[y1, x0] + fx * (I[y1, x1] - I[y1, x0])
    return top + fy * (bot - top)


def lk64(Y0, Y1, pts, win=21, levels=3, max_iters=30, eps=0.01, min_eig=1e-4, max_err=0.0):
    """Pyramidal Lucas-Kanade by the definition, all points at once.  -> dict(pts1 [N][2], status [N] (0 / 1), err [N], lam [N] (level-0
    eigenvalue / win^2), grad [N] (largest |grad T| of the level-0 window), edge [N] (distance of the unclamped result to the frame edge,
    negative outside; -inf for a point or a result that is not finite))"""
    P0, P1 = [np.asarray(Y0, np.float64)], [np.asarray(Y1, np.float64)]
    for _ in range(levels - 1):
        P0.append(pyr_down64(P0[-1])); P1.append(pyr_down64(P1[-1]))
    H, W = P0[0].shape
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    N = pts.shape[0]
    finite = np.isfinite(pts).all(1)
    p = np.where(finite[:, None], pts, 0.0)
    h = (win - 1) // 2
    o = np.arange(-h, h + 1, dtype=np.float64)
    ox, oy = o[None, None, :], o[None, :, None]                    # [N][row = y offset][column = x offset]
    g, v = np.zeros((N, 2)), np.zeros((N, 2))
    lost = ~finite
    err, lam0, grad0 = np.zeros(N), np.zeros(N), np.zeros(N)
    with np.errstate(all="ignore"):
        for L in range(levels - 1, -1, -1):
            I0, I1 = P0[L], P1[L]
            c = p / 2.0 ** L
            cx, cy = c[:, 0, None, None], c[:, 1, None, None]
            T = sample64(I0, cx + ox, cy + oy)
            Tx = (sample64(I0, cx + ox + 1, cy + oy) - sample64(I0, cx + ox - 1, cy + oy)) / 2
            Ty = (sample64(I0, cx + ox, cy + oy + 1) - sample64(I0, cx + ox, cy + oy - 1)) / 2
            a, b, cc = (Tx * Tx).sum((1, 2)), (Tx * Ty).sum((1, 2)), (Ty * Ty).sum((1, 2))
            lam = 0.5 * ((a + cc) - np.sqrt((a - cc) ** 2 + 4 * b * b)) / win ** 2
            weak = lam < min_eig
            if L == 0:
                lost |= weak
                lam0, grad0 = lam, np.hypot(Tx, Ty).max((1, 2))
            v = np.zeros((N, 2))
            act = ~weak
            for _ in range(max_iters):
                k = np.flatnonzero(act)
                if k.size == 0:
                    break
                bxp, byp = (c[k, 0] + g[k, 0] + v[k, 0])[:, None, None], (c[k, 1] + g[k, 1] + v[k, 1])[:, None, None]
                r = T[k] - sample64(I1, bxp + ox, byp + oy)
                bx, by = (r * Tx[k]).sum((1, 2)), (r * Ty[k]).sum((1, 2))
                det = a[k] * cc[k] - b[k] ** 2
                d = np.stack([(cc[k] * bx - b[k] * by) / det, (a[k] * by - b[k] * bx) / det], 1)
                v[k] += d
                if L == 0:
                    err[k] = np.abs(r).mean((1, 2))
                act[k] = ~((d ** 2).sum(1) < eps * eps)
            if L > 0:
                g = 2 * (g + v)
        d = g + v
        q = p + d
        edge = np.minimum(np.minimum(q[:, 0], W - 1 - q[:, 0]), np.minimum(q[:, 1], H - 1 - q[:, 1]))
        inside = (q[:, 0] >= 0) & (q[:, 0] <= W - 1) & (q[:, 1] >= 0) & (q[:, 1] <= H - 1)
        lost |= ~np.isfinite(d).all(1) | ~inside
        if max_err > 0:
            lost |= err > max_err
    return dict(pts1=np.where(lost[:, None], pts, q), status=(~lost).astype(np.int32), err=np.where(lost, 0.0, err), lam=lam0, grad=grad0,
                edge=np.where(np.isfinite(edge) & finite, edge, -np.inf))
