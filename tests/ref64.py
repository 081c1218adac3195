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
