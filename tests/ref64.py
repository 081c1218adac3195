"""Plain-torch references of the backward path, in any dtype (float64 for the reference, float32 on the CPU for the chain
bound's anchor).  Written from the operations' definitions, not from the kernels or the oracle:
  * nn.SpatialConvolution       valid cross-correlation (F.conv2d) + bias;
  * nn.SpatialConvolutionMap    a sum of per-connection conv2d's over a 1-based (from, to) table + bias;
  * nn.SpatialMatching          out[y][x][dy][dx] = sum_k (in1[k][y][x] - in2[k][y+dy][x+dx])^2 (radial: maxw = 1);
  * soft-max, log-soft-max, tanh, and Torch7's Log2 (clamps its input to >= eps IN PLACE, so the gradient is gradOut / max(x, eps)).
Gradients come from torch.autograd; the closed forms sit beside them for the kernels whose inputs are outputs
(soft-max / log-soft-max / tanh backward take the forward's float32 output, not the logits)."""
import numpy as np
import torch
import torch.nn.functional as F


def t64(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).detach().cpu().to(dtype)


def conv(x, w, b, conn=None, nOut=None):
    """x [nIn][H][W]; w [nOut][nIn][kH][kW] (dense) or [nConn][kH][kW] with conn [nConn][2] (from, to) 1-based; b [nOut]"""
    if conn is None:
        return F.conv2d(x[None], w, b)[0]
    conn = np.asarray(conn)
    kH, kW = w.shape[1], w.shape[2]
    Ho, Wo = x.shape[1] - kH + 1, x.shape[2] - kW + 1
    planes = [[] for _ in range(nOut)]
    for c, (i, o) in enumerate(conn.tolist()):
        planes[o - 1].append(F.conv2d(x[i - 1][None, None], w[c][None, None])[0, 0])
    zero = torch.zeros((Ho, Wo), dtype=x.dtype)
    return torch.stack([sum(p, zero) for p in planes]) + b[:, None, None]


def spatial_convolution64(x, w, b=None):
    """nn.SpatialConvolution's forward in float64 numpy, from its definition: out[o][y][x] = b[o] + sum_{i,u,v} w[o][i][u][v] in[i][y+u][x+v].
    Returns (value, sum|w . in| + |b|): the second bounds the rounding error of any float32 summation order -- T + 1 sequentially added,
    separately rounded terms are within (T + 1) 2^-24 of it, T = nIn kH kW."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    kH, kW = w.shape[2], w.shape[3]
    win = np.lib.stride_tricks.sliding_window_view(x, (kH, kW), axis=(1, 2))          # [nIn][Ho][Wo][kH][kW]
    val = np.einsum("oiuv,iyxuv->oyx", w, win, optimize=True)
    mag = np.einsum("oiuv,iyxuv->oyx", np.abs(w), np.abs(win), optimize=True)
    if b is not None:
        b = np.asarray(b, np.float64)
        val, mag = val + b[:, None, None], mag + np.abs(b)[:, None, None]
    return val, mag


def conv_backward(x, w, go, conn=None, nOut=None, dtype=torch.float64):
    """(gradInput, gradWeight, gradBias) by autograd, from zero"""
    x, w, go = t64(x, dtype).requires_grad_(), t64(w, dtype).requires_grad_(), t64(go, dtype)
    nOut = w.shape[0] if conn is None else nOut
    b = torch.zeros(nOut, dtype=dtype, requires_grad=True)
    conv(x, w, b, conn, nOut).backward(go)
    return x.grad, w.grad, b.grad


def conv_backward_closed(x, w, go, conn=None, nOut=None):
    """The same in closed form (dense: gradInput = full correlation with the flipped kernel, gradWeight = correlation of the input
    with gradOut), float64"""
    x, w, go = t64(x), t64(w), t64(go)
    if conn is None:
        gi = F.conv_transpose2d(go[None], w)[0]
        gw = F.conv2d(x[:, None], go[:, None]).transpose(0, 1)
    else:
        gi = torch.zeros_like(x)
        gw = torch.zeros_like(w)
        for c, (i, o) in enumerate(np.asarray(conn).tolist()):
            gi[i - 1] += F.conv_transpose2d(go[o - 1][None, None], w[c][None, None])[0, 0]
            gw[c] = F.conv2d(x[i - 1][None, None], go[o - 1][None, None])[0, 0]
    return gi, gw, go.sum((1, 2))


def matching(in1, in2, maxh, maxw):
    K, H1, W1 = in1.shape
    cols = [((in1 - in2[:, dy : dy + H1, dx : dx + W1]) ** 2).sum(0) for dy in range(maxh) for dx in range(maxw)]
    return torch.stack(cols, -1).reshape(H1, W1, maxh, maxw)


def matching_backward(in1, in2, go, maxh, maxw):
    """closed form, float64: (g1, g2, sum|terms| of g1, sum|terms| of g2); go [H1][W1][maxh][maxw] (or [H1][W1][maxh] radial)"""
    in1, in2 = t64(in1), t64(in2)
    K, H1, W1 = in1.shape
    go = t64(go).reshape(H1, W1, maxh, maxw)
    g1, g2, a1, a2 = torch.zeros_like(in1), torch.zeros_like(in2), torch.zeros_like(in1), torch.zeros_like(in2)
    for dy in range(maxh):
        for dx in range(maxw):
            t = 2 * (in1 - in2[:, dy : dy + H1, dx : dx + W1]) * go[:, :, dy, dx]
            g1 += t
            g2[:, dy : dy + H1, dx : dx + W1] -= t
            a1 += t.abs()
            a2[:, dy : dy + H1, dx : dx + W1] += t.abs()
    return g1, g2, a1, a2


def matching_backward_autograd(in1, in2, go, maxh, maxw):
    a, b = t64(in1).requires_grad_(), t64(in2).requires_grad_()
    matching(a, b, maxh, maxw).backward(t64(go).reshape(a.shape[1], a.shape[2], maxh, maxw))
    return a.grad, b.grad


def softmax_backward(out, go):
    """gradIn = out * (gradOut - sum(gradOut * out)) over the last dimension, float64, from the float32 output"""
    out, go = t64(out), t64(go)
    return out * (go - (go * out).sum(-1, keepdim=True))


def log_softmax_backward(out, go):
    """gradIn = gradOut - exp(out) * sum(gradOut), float64, from the float32 output"""
    out, go = t64(out), t64(go)
    return go - out.exp() * go.sum(-1, keepdim=True)


def log2(x, eps):
    """Torch7's Log2: forward log(max(x, eps)); backward gradOut / max(x, eps) for EVERY element (the input was clamped in place)"""
    xc = x + (x.clamp(min=eps) - x).detach()
    return xc.log()


def single_scale_chain(params, p1, p2, maxh, maxw, method="max", dtype=torch.float64):
    """getModel(geometry, training_mode) of the single-scale trainer in `dtype`: a filter stack with SHARED weights on both patches
    -> SpatialMatching -> Minus -> soft-max over the window -> Log2(1e-10) ('max') or OutputExtractor ('mean').
    params: list of (weight, bias, conn, nOut) per convolution, tanh between them.  Returns (output(s), leaf tensors)."""
    leaves = []
    ps = []
    for w, b, conn, nOut in params:
        w, b = t64(w, dtype).requires_grad_(), t64(b, dtype).requires_grad_()
        leaves += [w, b]
        ps.append((w, b, conn, nOut))
    x1, x2 = t64(p1, dtype).requires_grad_(), t64(p2, dtype).requires_grad_()

    def filt(x):
        for li, (w, b, conn, nOut) in enumerate(ps):
            x = conv(x, w, b, conn, nOut)
            if li != len(ps) - 1:
                x = torch.tanh(x)
        return x

    f1, f2 = filt(x1), filt(x2)
    H1, W1 = f1.shape[1], f1.shape[2]
    cost = matching(f1, f2, maxh, maxw).reshape(H1, W1, maxh * maxw)
    p = torch.softmax(-cost, -1)
    if method == "mean":
        k = torch.arange(maxh * maxw)
        xs, ys = (k % maxw + 1).to(dtype), (k // maxw + 1).to(dtype)
        return [(p * xs).sum(-1), (p * ys).sum(-1)], leaves + [x1, x2]
    return log2(p, float(np.float32(1e-10))), leaves + [x1, x2]


def radial_chain(params, prev, cur, hWin, dtype=torch.float64):
    """getTrainerNetwork (radial): prev cropped by SpatialPadding(0, 0, 0, -hWin + 1), the shared filter stack (convolutions only,
    tanh where `params` says so) on both, SpatialRadialMatching(hWin) -> Minus -> LogSoftMax over the hWin displacements.
    params: list of ("conv", w, b) / ("tanh",)"""
    leaves, ps = [], []
    for p in params:
        if p[0] == "conv":
            w, b = t64(p[1], dtype).requires_grad_(), t64(p[2], dtype).requires_grad_()
            leaves += [w, b]
            ps.append(("conv", w, b))
        else:
            ps.append(p)
    xp, xc = t64(prev, dtype).requires_grad_(), t64(cur, dtype).requires_grad_()

    def filt(x):
        for p in ps:
            x = conv(x, p[1], p[2]) if p[0] == "conv" else torch.tanh(x)
        return x

    f1, f2 = filt(xp[:, : xp.shape[1] - hWin + 1]), filt(xc)
    cost = matching(f1, f2, hWin, 1).reshape(f1.shape[1], f1.shape[2], hWin)
    return torch.log_softmax(-cost, -1), leaves + [xp, xc]


def grads(out, leaves, gradOut):
    """d out / d leaves contracted with gradOut (a tensor, or a list of tensors for a list of outputs)"""
    if isinstance(out, (list, tuple)):
        torch.autograd.backward(list(out), [t64(g, out[0].dtype).reshape(o.shape) for o, g in zip(out, gradOut)])
    else:
        out.backward(t64(gradOut, out.dtype).reshape(out.shape))
    return [l.grad for l in leaves]


# ---------------------------------------------------------------------------------------------------------------------------------
# Ego-motion, rectification and focus of expansion (csrc/egopose.hip, csrc/egomotion.hip), float64 numpy from the definitions
def sampson64(F, p1, p2):
    """Sampson distance in pixels of the correspondences p1 -> p2 ([N][2], (x, y)) to the fundamental matrix F (p2^T F p1 = 0):
    |p2^T F p1| / sqrt((F p1)_1^2 + (F p1)_2^2 + (F^T p2)_1^2 + (F^T p2)_2^2)."""
    F = np.asarray(F, np.float64)
    h1 = np.concatenate([np.asarray(p1, np.float64), np.ones((len(p1), 1))], 1)
    h2 = np.concatenate([np.asarray(p2, np.float64), np.ones((len(p2), 1))], 1)
    a, b = h1 @ F.T, h2 @ F
    return np.abs((h2 * a).sum(1)) / np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


def fund_from_pose64(K, R, T):
    """F = K^-T [T]x R K^-1 with unit Frobenius norm (x2 ~ R x1 + T)"""
    K, R, T = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(T, np.float64)
    Tx = np.array([[0, -T[2], T[1]], [T[2], 0, -T[0]], [-T[1], T[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ Tx @ R @ Ki
    return F / np.linalg.norm(F)


def pose_fit64(K, p1, p2):
    """(R, T) with x2 ~ R x1 + T, |T| = 1, by the linear eight-point method over ALL the given correspondences ([N][2] pixels), written
    with numpy's SVD: rows kron(x2, x1) of the epipolar constraint in camera coordinates, the right singular vector of the smallest
    singular value, projection onto the essential manifold (singular values 1, 1, 0), the four decompositions, and the one that puts
    most points in front of both cameras (depths from the least-squares solution of z2 x2 = z1 R x1 + T).  No RANSAC: give it inliers."""
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    a = np.concatenate([np.asarray(p1, np.float64), np.ones((len(p1), 1))], 1) @ Ki.T
    b = np.concatenate([np.asarray(p2, np.float64), np.ones((len(p2), 1))], 1) @ Ki.T
    A = (b[:, :, None] * a[:, None, :]).reshape(-1, 9)
    E = np.linalg.svd(A, full_matrices=False)[2][-1].reshape(3, 3)
    U, _, Vt = np.linalg.svd(E)
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    Wm = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    best = None
    for R in (U @ Wm @ Vt, U @ Wm.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            ra = a @ R.T
            # [ra  -b] (z1, z2)^T = -t per point, normal equations
            m00, m01, m11 = (ra * ra).sum(1), -(ra * b).sum(1), (b * b).sum(1)
            r0, r1 = -(ra @ t), b @ t
            det = m00 * m11 - m01 * m01
            z1, z2 = (r0 * m11 - m01 * r1) / det, (m00 * r1 - m01 * r0) / det
            good = int(((z1 > 0) & (z2 > 0)).sum())
            if best is None or good > best[0]:
                best = (good, R, t)
    return best[1], best[2]


def bilinear64(img, sy, sx):
    """bilinear sample of img [C][H][W] at float64 (sy, sx), coordinates clamped to the frame, the far neighbour clamped to the last
    row / column (its weight is 0 there)"""
    img = np.asarray(img, np.float64)
    H, W = img.shape[1:]
    sy, sx = np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    wy, wx = sy - y0, sx - x0
    top = (1 - wx) * img[:, y0, x0] + wx * img[:, y0, x1]
    bot = (1 - wx) * img[:, y1, x0] + wx * img[:, y1, x1]
    return (1 - wy) * top + wy * bot


def lipschitz64(img):
    """(gy, gx): the largest |difference| of vertically / horizontally adjacent pixels of img [C][H][W] -- the Lipschitz constants of its
    bilinear interpolant along y and x (0 for a single row / column)"""
    img = np.asarray(img, np.float64)
    gy = np.abs(np.diff(img, axis=1)).max() if img.shape[1] > 1 else 0.0
    gx = np.abs(np.diff(img, axis=2)).max() if img.shape[2] > 1 else 0.0
    return float(gy), float(gx)


def local_lipschitz64(img, sy, sx):
    """per-pixel (gy, gx) [H'][W'] for sources (sy, sx): the largest |difference| of vertically / horizontally adjacent pixels of img
    [C][H][W] (over the channels) in the source's bilinear cell and the eight cells around it -- a coordinate error far below one pixel
    cannot leave them, so this is the Lipschitz constant of the interpolant along the way from the exact to the perturbed source.
    Sources outside the frame (or non-finite) are clamped; their value is not used."""
    img = np.asarray(img, np.float64)
    _, H, W = img.shape
    dy = np.zeros((H + 3, W + 2))                          # dy[1 + y][1 + x] = max_c |img[y+1][x] - img[y][x]|, 0 outside
    dx = np.zeros((H + 2, W + 3))
    if H > 1:
        dy[1:H, 1 : W + 1] = np.abs(np.diff(img, axis=1)).max(0)
    if W > 1:
        dx[1 : H + 1, 1:W] = np.abs(np.diff(img, axis=2)).max(0)
    # vertical differences a 3 x 3 block of cells around (y0, x0) can see: rows y0-1 .. y0+1 (pairs), columns x0-1 .. x0+2; likewise dx
    my = np.zeros((H, W))
    mx = np.zeros((H, W))
    for a in range(3):
        for b in range(4):
            my = np.maximum(my, np.pad(dy, ((0, 0), (1, 1)))[a : a + H, b : b + W])
            mx = np.maximum(mx, np.pad(dx, ((1, 1), (0, 0)))[b : b + H, a : a + W])
    y0 = np.clip(np.floor(np.nan_to_num(sy, nan=0.0, posinf=0.0, neginf=0.0)), 0, H - 1).astype(np.int64)
    x0 = np.clip(np.floor(np.nan_to_num(sx, nan=0.0, posinf=0.0, neginf=0.0)), 0, W - 1).astype(np.int64)
    return my[y0, x0], mx[y0, x0]


def homography_warp64(img, K, R, inverse=False):
    """removeEgoMotion from its definition: out(p) = bilinear(img, Hm p), Hm = K R K^-1 (inverse: R^T), for pixels whose source lies in
    front of the camera (Z > 0) and inside [0, W-1] x [0, H-1]; 0 elsewhere.  Returns dict(out [C][H][W], val (the sample at the clamped
    source whatever the mask says: what a pixel on the frame edge carries if it is taken as inside), mask [H][W] bool, sy, sx (the
    float64 source; NaN / inf where Z = 0), Z, edge = distance of the source to the nearest frame edge in pixels (inf where Z <= 0),
    cerr_y, cerr_x = a bound on the error of a float32 evaluation of the source coordinates, roundings counted (u = 2^-24, first order,
    times 1.001 for the rest): X = h0 x + h1 y + h2 with the coefficients rounded to float32 (u per term), two products (u each), the
    first sum (u on the two products), the second (u on all three): |dX| <= 4 u (|h0 x| + |h1 y|) + 2 u |h2|; a fused multiply-add
    only removes roundings.  Then sx = X / Z: |dsx| <= (dX + |sx| dZ) / |Z| + u |sx|)."""
    img = np.asarray(img, np.float64)
    _, H, W = img.shape
    K, R = np.asarray(K, np.float64), np.asarray(R, np.float64)
    Hm = K @ (R.T if inverse else R) @ np.linalg.inv(K)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    X = Hm[0, 0] * xs + Hm[0, 1] * ys + Hm[0, 2]
    Y = Hm[1, 0] * xs + Hm[1, 1] * ys + Hm[1, 2]
    Z = Hm[2, 0] * xs + Hm[2, 1] * ys + Hm[2, 2]
    aH = np.abs(Hm)
    u = 1.001 * 2.0 ** -24
    dX, dY, dZ = (4 * u * (aH[r, 0] * xs + aH[r, 1] * ys) + 2 * u * aH[r, 2] for r in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        sx, sy = X / Z, Y / Z
        mask = (Z > 0) & (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        edge = np.where(Z > 0, np.minimum(np.minimum(np.abs(sx), np.abs(sx - (W - 1))), np.minimum(np.abs(sy), np.abs(sy - (H - 1)))), np.inf)
        cerr_x = (dX + np.abs(sx) * dZ) / np.abs(Z) + u * np.abs(sx)
        cerr_y = (dY + np.abs(sy) * dZ) / np.abs(Z) + u * np.abs(sy)
    val = bilinear64(img, np.nan_to_num(np.where(Z > 0, sy, 0), posinf=0.0), np.nan_to_num(np.where(Z > 0, sx, 0), posinf=0.0))
    return dict(out=np.where(mask, val, 0.0), val=val, mask=mask, sy=sy, sx=sx, Z=Z, edge=edge, cerr_y=cerr_y, cerr_x=cerr_x)


def undistort64(img, K, dist5):
    """undistortImage from its definition, the inverse map of the radial-tangential model (k1, k2, p1, p2, k3) of the .cal files:
    (xn, yn) = ((x - cx) / fx, (y - cy) / fy), r2 = xn^2 + yn^2, xd = xn (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 xn yn + p2 (r2 + 2 xn^2),
    yd likewise, source = (fx xd + cx, fy yd + cy); out = bilinear(img, source) inside [0, W-1] x [0, H-1], else 0.  (The model has no
    skew: only fx, fy, cx, cy of K are used, as the library documents.)  Returns dict(out, val (the sample at the clamped source whatever the mask says), mask, sy, sx, edge, cerr_y, cerr_x); the
    coordinate error bound of a float32 evaluation counts its roundings and carries them through (_undistort_budget)."""
    img = np.asarray(img, np.float64)
    _, H, W = img.shape
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3 = [float(v) for v in np.asarray(dist5, np.float64).reshape(-1)]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    xn, yn = (xs - cx) / fx, (ys - cy) / fy
    r2 = xn * xn + yn * yn
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    sx, sy = xd * fx + cx, yd * fy + cy
    cerr_x = _undistort_budget(xs, xn, yn, fx, cx, fy, cy, ys, (k1, k2, k3), p1, p2, rad, xd)
    cerr_y = _undistort_budget(ys, yn, xn, fy, cy, fx, cx, xs, (k1, k2, k3), p2, p1, rad, yd)
    mask = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
    edge = np.minimum(np.minimum(np.abs(sx), np.abs(sx - (W - 1))), np.minimum(np.abs(sy), np.abs(sy - (H - 1))))
    val = bilinear64(img, sy, sx)
    return dict(out=np.where(mask, val, 0.0), val=val, mask=mask, sy=sy, sx=sx, edge=edge, cerr_x=cerr_x, cerr_y=cerr_y)


def _undistort_budget(xs, xn, yn, fx, cx, fy, cy, ys, k, p1, p2, rad, xd):
    """Bound on the error of sx = fx xd + cx evaluated in float32 as the library does, every rounding counted once (u = 2^-24, first
    order, times 1.001 for the rest; a fused multiply-add only removes roundings).  Written for the x coordinate; the y coordinate is the
    same expression with the roles of x and y, and of p1 and p2, exchanged.
      xn = (x - cx) / fx        cx, fx rounded to float32, one subtraction, one division:  e_xn = u (|cx| / |fx| + 3 |xn|)
      r2 = xn xn + yn yn        two products, one sum:                                     e_r2 = 2 |xn| e_xn + 2 |yn| e_yn + 2 u r2
      rad = 1 + r2 (k1 + r2 (k2 + r2 k3))   Horner, 6 operations on partial results <= 1 + P, coefficients rounded (u P), P = sum |k_i| r2^i:
                                                                                           e_rad = P' e_r2 + u P + 6 u (1 + P)
      xd = xn rad + 2 p1 xn yn + p2 (r2 + 2 xn xn)
           t1 = xn rad:               |rad| e_xn + |xn| e_rad + u |t1|
           t2 = 2 p1 xn yn:           |2 p1| (|yn| e_xn + |xn| e_yn) + 3 u |t2|      (p1 rounded, two products)
           t3 = p2 (r2 + 2 xn xn):    |p2| (e_r2 + 4 |xn| e_xn + 3 u s) + 2 u |t3|   (s = r2 + 2 xn^2: one product, one sum; p2 rounded, one product)
           two sums:                  2 u (|t1| + |t2| + |t3|)
      sx = xd fx + cx           fx rounded, one product, cx rounded, one sum:              |fx| e_xd + 3 u |fx xd| + 2 u |cx|"""
    u = 1.001 * 2.0 ** -24
    k1, k2, k3 = (abs(v) for v in k)
    axn, ayn = np.abs(xn), np.abs(yn)
    e_xn = u * (abs(cx) / abs(fx) + 3 * axn)
    e_yn = u * (abs(cy) / abs(fy) + 3 * ayn)
    r2 = xn * xn + yn * yn
    e_r2 = 2 * axn * e_xn + 2 * ayn * e_yn + 2 * u * r2
    P = r2 * (k1 + r2 * (k2 + r2 * k3))
    dP = k1 + r2 * (2 * k2 + r2 * 3 * k3)
    e_rad = dP * e_r2 + u * P + 6 * u * (1 + P)
    t1, t2, s = axn * np.abs(rad), 2 * abs(p1) * axn * ayn, r2 + 2 * xn * xn
    t3 = abs(p2) * s
    e_xd = (np.abs(rad) * e_xn + axn * e_rad + u * t1) + (2 * abs(p1) * (ayn * e_xn + axn * e_yn) + 3 * u * t2) \
        + (abs(p2) * (e_r2 + 4 * axn * e_xn + 3 * u * s) + 2 * u * t3) + 2 * u * (t1 + t2 + t3)
    return abs(fx) * e_xd + 3 * u * np.abs(fx * xd) + 2 * u * abs(cx)


def foe64(flow, conf=None, min_flow=0.5, iterations=2, huber=2.0):
    """Focus of expansion of a dense flow field [2][H][W] (plane 0 = y, 1 = x): the point c minimising sum w (n . (c - p))^2 over the
    pixels p with a usable vector, n = (-v, u) / |flow| the unit normal of the flow line through p.  Usable: finite flow of non-zero
    length >= min_flow, and conf > 0 where conf is given (a NaN confidence is not usable).  The 2 x 2 normal equations are solved with
    np.linalg.solve; `iterations` Huber re-weightings w = min(1, huber / |n . (c - p)|), seeded at (W / 2, H / 2).  Returns ((x, y), sum
    of the weights); raises np.linalg.LinAlgError when the normal matrix is singular."""
    v, u = np.asarray(flow[0], np.float64), np.asarray(flow[1], np.float64)
    H, W = u.shape
    with np.errstate(invalid="ignore", over="ignore"):
        mag = np.sqrt(u * u + v * v)
        ok = np.isfinite(mag) & (mag > 0) & (mag >= min_flow)
        if conf is not None:
            ok &= np.asarray(conf, np.float64) > 0
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    y, x, nx, ny = ys[ok], xs[ok], -v[ok] / mag[ok], u[ok] / mag[ok]
    npd = nx * x + ny * y
    c = np.array([W / 2.0, H / 2.0])
    wsum = 0.0
    for it in range(iterations + 1):
        w = np.ones_like(nx)
        if it > 0:
            r = np.abs(nx * (c[0] - x) + ny * (c[1] - y))
            w = np.where(r <= huber, 1.0, huber / np.maximum(r, 1e-300))
        A = np.array([[np.sum(w * nx * nx), np.sum(w * nx * ny)], [np.sum(w * nx * ny), np.sum(w * ny * ny)]])
        b = np.array([np.sum(w * nx * npd), np.sum(w * ny * npd)])
        wsum = float(np.sum(w))
        if not abs(np.linalg.det(A)) > 1e-9 * (A[0, 0] + A[1, 1]) ** 2 + 1e-300:
            raise np.linalg.LinAlgError("foe64: the flow lines do not intersect in a point")
        c = np.linalg.solve(A, b)
    return (float(c[0]), float(c[1])), wsum
