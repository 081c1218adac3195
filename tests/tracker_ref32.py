"""lk32: the tracker's definition restated in float32 numpy, next to lk64 of tests/tracker_ref64.py and written
from the same text, not from the kernel: the pyramid, the bilinear samples, T / Tx / Ty, the products, the sums and v += delta are float32;
the eigenvalue and the 2 x 2 solve are taken in double from the float32 sums, as the text says.  What is left open by the text -- the
order of the sums (numpy's pairwise sum here, per-lane partial sums and a wave tree on the device) -- is all it differs from the device in.
Its distance to lk64 says how much float32 rounding the definition itself carries on a given input, so that the bound the device is held to
does not depend on what the kernel happens to return."""
import numpy as np

from tests.tracker_ref64 import _reflect

F = np.float32


def pyr_down32(I):
    """out(y, x) = sum_i w_i (sum_j w_j in(rho(2y + i), rho(2x + j))), float32 products and sums"""
    I = np.asarray(I, F)
    H, W = I.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    w = (np.array([1, 4, 6, 4, 1], F) / F(16)).astype(F)
    out = np.zeros((Ho, Wo), F)
    for i in range(5):
        ry = _reflect(2 * np.arange(Ho) + i - 2, H)
        h = np.zeros((Ho, Wo), F)
        for j in range(5):
            h += w[j] * I[np.ix_(ry, _reflect(2 * np.arange(Wo) + j - 2, W))]
        out += w[i] * h
    return out


def sample32(I, x, y):
    """bilinear sample in float32, the coordinates clamped to the frame first (a NaN coordinate reads position 0)"""
    H, W = I.shape
    x = np.clip(np.where(np.isnan(x), F(0), x), F(0), F(W - 1)).astype(F)
    y = np.clip(np.where(np.isnan(y), F(0), y), F(0), F(H - 1)).astype(F)
    xf, yf = np.floor(x), np.floor(y)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - xf, y - yf
    top = I[y0, x0] + fx * (I[y0, x1] - I[y0, x0])
    bot = I[y1, x0] + fx * (I[y1, x1] - I[y1, x0])
    return top + fy * (bot - top)


def lk32(Y0, Y1, pts, win=21, levels=3, max_iters=30, eps=0.01, min_eig=1e-4, max_err=0.0):
    """-> dict(pts1 [N][2] float32, status [N], err [N] float32), the fields of lk64 that the device returns"""
    P0, P1 = [np.asarray(Y0, F)], [np.asarray(Y1, F)]
    for _ in range(levels - 1):
        P0.append(pyr_down32(P0[-1])); P1.append(pyr_down32(P1[-1]))
    H, W = P0[0].shape
    pts = np.asarray(pts, F).reshape(-1, 2)
    N = pts.shape[0]
    finite = np.isfinite(pts).all(1)
    p = np.where(finite[:, None], pts, F(0)).astype(F)
    h = (win - 1) // 2
    o = np.arange(-h, h + 1).astype(F)
    ox, oy = o[None, None, :], o[None, :, None]
    one, half = F(1), F(0.5)
    g, v = np.zeros((N, 2), F), np.zeros((N, 2), F)
    lost = ~finite
    errsum = np.zeros(N, F)
    eps2 = F(eps) * F(eps)
    with np.errstate(all="ignore"):
        for L in range(levels - 1, -1, -1):
            I0, I1 = P0[L], P1[L]
            c = p * F(1.0 / 2 ** L)
            cx, cy = c[:, 0, None, None], c[:, 1, None, None]
            T = sample32(I0, cx + ox, cy + oy)
            Tx = (sample32(I0, cx + (ox + one), cy + oy) - sample32(I0, cx + (ox - one), cy + oy)) * half
            Ty = (sample32(I0, cx + ox, cy + (oy + one)) - sample32(I0, cx + ox, cy + (oy - one))) * half
            assert T.dtype == Tx.dtype == Ty.dtype == F
            a, b, cc = ((Tx * Tx).sum((1, 2), dtype=F).astype(np.float64), (Tx * Ty).sum((1, 2), dtype=F).astype(np.float64),
                        (Ty * Ty).sum((1, 2), dtype=F).astype(np.float64))
            lam = 0.5 * ((a + cc) - np.sqrt((a - cc) ** 2 + 4 * b * b)) / win ** 2
            weak = lam < np.float64(F(min_eig))
            if L == 0:
                lost |= weak
            v = np.zeros((N, 2), F)
            act = ~weak
            det = a * cc - b * b
            for _ in range(max_iters):
                k = np.flatnonzero(act)
                if k.size == 0:
                    break
                bxp, byp = (c[k, 0] + g[k, 0] + v[k, 0])[:, None, None], (c[k, 1] + g[k, 1] + v[k, 1])[:, None, None]
                r = T[k] - sample32(I1, bxp + ox, byp + oy)
                assert r.dtype == F
                bx, by = (r * Tx[k]).sum((1, 2), dtype=F).astype(np.float64), (r * Ty[k]).sum((1, 2), dtype=F).astype(np.float64)
                d = np.stack([(cc[k] * bx - b[k] * by) / det[k], (a[k] * by - b[k] * bx) / det[k]], 1).astype(F)
                v[k] += d
                if L == 0:
                    errsum[k] = np.abs(r).sum((1, 2), dtype=F)
                act[k] = ~(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < eps2)
            if L > 0:
                g = F(2) * (g + v)
        d = g + v
        q = p + d
        assert q.dtype == F
        inside = (q[:, 0] >= 0) & (q[:, 0] <= F(W - 1)) & (q[:, 1] >= 0) & (q[:, 1] <= F(H - 1))
        err = (errsum.astype(np.float64) / win ** 2).astype(F)
        lost |= ~np.isfinite(d).all(1) | ~inside
        if max_err > 0:
            lost |= err > F(max_err)
    return dict(pts1=np.where(lost[:, None], pts, q), status=(~lost).astype(np.int32), err=np.where(lost, F(0), err))
