"""GPU suite (-m gpu): the backward kernels (csrc/backward.hip, csrc/matching_backward.hip) and the two trainers' whole-network
gradients against FLOAT64 torch on the CPU (tests/ref64.py, itself pinned against the oracle by test_backward_ref64_cpu.py), at the
trainers' shapes, the grid-stride limits (8192 blocks of 256 threads; 32768 rows per pass for the row kernels) and the edges.

Every kernel is checked twice:
  EXACT: small integer inputs, weights and gradOutputs, sizes such that every partial sum stays below 2^24 -- every sum is then exact
    in any order and the GPU result must EQUAL the float64 one.  A wrong index, plane, border, connection or reduction lane is caught
    with zero tolerance.  (The exp / log kernels use rows of -inf with one finite entry, whose results are 0 / -inf exactly: this
    assumes exp(0) = 1, exp(-inf) = 0 and log(1) = 0 are returned exactly, as IEEE 754 recommends.)
  FLOAT: randn data, |g - g64| <= bound, every element.

THE BOUNDS.  u = 2^-24.  A sum of terms each carrying at most n roundings along its path (its product, the additions after it, the
reduction levels it passes) is within gamma_n sum|terms|, gamma_n = n u / (1 - n u), in any order (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., sections 3.1 and 4.2; a fused multiply-add only removes roundings).  sum|terms| is computed in float64
from |inputs|.  alpha = 1.01 covers 1 / (1 - n u) <= 1.0006 (n <= 9248 here), the float64 reference's own error (< n 2^-53 sum|terms|)
and second-order terms; it is not fitted to what passes.  n per kernel, along the kernel's actual accumulation path:
  conv_grad_input / conv_map_grad_input   n = nOut kH kW (the gather's sequential chain, separately rounded products)
  conv_acc_grad_weight / _bias             n = ceil(P / 256) (each thread's strided chain) + 6 (shuffle levels) + 3 (the 4-way sum)
                                             + 1 (scale) + 1 (accumulate)
  matching_grad1 / grad2                   n = maxh maxw + 2 (the chain, plus the difference and the product of each term)
Elementwise and row kernels (first order in u; every float64 quantity below is computed from the float32 inputs the kernel reads):
  tanh_backward       gi = go (1 - o o): three roundings, |err| <= 3 u |go| (1 + o^2)
  Log2 backward       gi = go / x, correctly rounded (clang's HIP default, -fhip-fp32-correctly-rounded-divide-sqrt): u |gi|
  Log2 forward        logf: 2 ulp <= 4 u |log x|
  softmax_backward    s = sum go out (ceil(N / 64) + 6 = n_s roundings), gi = out (go - s): u |out| (2 |go - s| + n_s sum|go out|)
  log_softmax_bwd     s = sum go (n_s), gi = go - expf(out) s: u (|gi| + 5 e |s| + n_s e sum|go|), e = exp(out)
  log_softmax         d_j = fl(r_j - m) (u |d_j|), e_j = expf(d_j) (2 ulp), s = sum e_j (n_s), l = m + logf(s), out = r - l:
                      u (|out| + |l| + 4 |log s| + n_s + 4 + D), D = sum e_j |d_j| / s (the inputs' roundings seen through exp)
The ulp errors of expf and logf are taken as 2 ulp each (assumed: the larger of the values the HIP and CUDA math-API tables list for
them); 1 ulp <= 2 u |result| for normal results.  Underflow: a rounding whose result is sub-normal errs by up to 2^-150 absolutely
(fl(a op b) = (a op b)(1 + d) + e, |e| <= 2^-150; Higham section 2.1).  A soft-max output of a row entry 100 below its maximum is
sub-normal, and so is soft-max backward's last product with it; that product and the sub-normal terms it came from give at most two
such roundings, so every float bound carries + BETA = 2^-149.  Sub-normal exp results add < N 2^-148 to s >= 1, far inside alpha.

WHOLE NETWORKS.  A float32 chain has no cheap first-order bound, so it is anchored on torch float32 on the CPU: the same network in
float32 gives e32 = max|g32 - g64| per tensor, and the GPU must give max|g - g64| <= 4 e32 + 8 u max|g64|.  The 4 is fixed in advance; a
wiring error (a branch not adding its share to the shared gradients, a scale applied twice) gives errors of the order of g itself.

The largest observed error-to-bound ratio per kernel is printed at the end of the module (pytest -s)."""
import math

import numpy as np
import pytest
import torch

from tests import ref64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ALPHA = 1.01
BETA = 2.0 ** -149
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print("max error / bound  %-28s %.3g" % (k, RATIOS[k]))


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def randn(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def exact(name, g, ref):
    g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    assert g.shape == ref.shape, (name, g.shape, ref.shape)
    bad = g.astype(np.float64) != ref
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        name, bad.sum(), bad.size, np.argwhere(bad)[0], g[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])
    RATIOS.setdefault(name, 0.0)


def bounded(name, g, ref, bound):
    g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    bound = (bound.numpy() if isinstance(bound, torch.Tensor) else np.asarray(bound)) + BETA
    assert g.shape == ref.shape, (name, g.shape, ref.shape)
    err = np.abs(g.astype(np.float64) - ref)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d of %d elements outside the bound, first at %s: %r vs %r (bound %r)" % (
        name, bad.sum(), bad.size, np.argwhere(bad)[0], g[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])],
        np.broadcast_to(bound, ref.shape)[tuple(np.argwhere(bad)[0])])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r.max()) if r.size else 0.0)


def _n_red(P):
    return math.ceil(P / 256) + 6 + 3 + 1 + 1


# ------------------------------------------------------------------ convolutions
def _conv_gpu(dfe, cuda, x, w, go, conn=None, nOut=None, scale=1.0, gw0=None, gb0=None, bias=True):
    """one updateGradInput + accGradParameters through the C ABI; returns (gi, gw, gb) as numpy"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    nIn, H, W = x.shape
    kH, kW = w.shape[-2], w.shape[-1]
    tx, tw, tgo = T(x, cuda), T(w, cuda), T(go, cuda)
    gi = torch.full_like(tx, float("nan"))
    gw = T(gw0, cuda) if gw0 is not None else torch.zeros_like(tw)
    gb = (T(gb0, cuda) if gb0 is not None else torch.zeros(go.shape[0], device=cuda)) if bias else None
    gbp = gb.data_ptr() if bias else None
    if conn is None:
        nOut = w.shape[0]
        ctx.check(lib.dfe_spatial_convolution_grad_input_f32(ctx.handle, tgo.data_ptr(), tw.data_ptr(), nIn, nOut, H, W, kH, kW, gi.data_ptr()))
        ctx.check(lib.dfe_spatial_convolution_acc_grad_f32(ctx.handle, tx.data_ptr(), tgo.data_ptr(), nIn, nOut, H, W, kH, kW, float(scale),
                                                           gw.data_ptr(), gbp))
    else:
        tc = torch.from_numpy(np.ascontiguousarray(conn, np.int32)).to(cuda)
        nc = tc.shape[0]
        ctx.check(lib.dfe_spatial_convolution_map_grad_input_f32(ctx.handle, tgo.data_ptr(), tw.data_ptr(), tc.data_ptr(), nc, nIn, nOut, H, W,
                                                                 kH, kW, gi.data_ptr()))
        ctx.check(lib.dfe_spatial_convolution_map_acc_grad_f32(ctx.handle, tx.data_ptr(), tgo.data_ptr(), tc.data_ptr(), nc, nIn, nOut, H, W,
                                                               kH, kW, float(scale), gw.data_ptr(), gbp))
    return gi.cpu().numpy(), gw.cpu().numpy(), (gb.cpu().numpy() if bias else None)


def _conv_case(dfe, cuda, rng, tag, nIn, nOut, kH, kW, H, W, conn=None):
    wshape = (nOut, nIn, kH, kW) if conn is None else (len(conn), kH, kW)
    nOutP = nOut
    Ho, Wo = H - kH + 1, W - kW + 1
    P = Ho * Wo
    # EXACT: accumulating 0.5 * grad on top of integer gradients, then the same without a gradBias
    x, w, go = ints(rng, (nIn, H, W)), ints(rng, wshape), ints(rng, (nOutP, Ho, Wo))
    gw0, gb0 = ints(rng, wshape), ints(rng, (nOutP,))
    gi, gw, gb = _conv_gpu(dfe, cuda, x, w, go, conn, nOutP, 0.5, gw0, gb0)
    rgi, rgw, rgb = ref64.conv_backward(x, w, go, conn, nOutP)
    exact(tag + " grad_input", gi, rgi)
    exact(tag + " acc_grad_weight", gw, ref64.t64(gw0) + 0.5 * rgw)
    exact(tag + " acc_grad_bias", gb, ref64.t64(gb0) + 0.5 * rgb)
    _, gw_nb, _ = _conv_gpu(dfe, cuda, x, w, go, conn, nOutP, 0.5, gw0, None, bias=False)
    assert np.array_equal(gw_nb, gw)
    # FLOAT
    x, w, go = randn(rng, (nIn, H, W)), randn(rng, wshape), randn(rng, (nOutP, Ho, Wo))
    gi, gw, gb = _conv_gpu(dfe, cuda, x, w, go, conn, nOutP)
    rgi, rgw, rgb = ref64.conv_backward(x, w, go, conn, nOutP)
    agi, agw, agb = ref64.conv_backward(np.abs(x), np.abs(w), np.abs(go), conn, nOutP)
    n_gi = (nOutP if conn is None else np.bincount(np.asarray(conn)[:, 0], minlength=nIn + 1).max()) * kH * kW
    bounded(tag + " grad_input", gi, rgi, ALPHA * n_gi * U * agi)
    bounded(tag + " acc_grad_weight", gw, rgw, ALPHA * _n_red(P) * U * agw)
    bounded(tag + " acc_grad_bias", gb, rgb, ALPHA * _n_red(P) * U * agb)
    return gi


@pytest.mark.parametrize("nIn,nOut,kH,kW,H,W", [
    (3, 8, 5, 5, 20, 20),        # single-scale trainer, layer 1 on patch 1 (P = 256)
    (3, 8, 5, 5, 35, 35),        # ... on patch 2
    (3, 5, 1, 17, 17, 17),       # radial trainer, layer 1 on the cropped previous patch
    (3, 5, 1, 17, 31, 17),       # ... on the current patch
    (5, 10, 17, 1, 17, 1),       # radial layer 2: Ho = Wo = 1, P = 1 (the 1 x 1 feature map)
    (5, 10, 17, 1, 31, 1),
    (3, 32, 17, 17, 40, 40),     # version2's 3 -> 32 17 x 17: 27 744 weight blocks
    (3, 4, 5, 5, 5, 5),          # H = kH, W = kW: P = 1, 255 idle threads
    (2, 3, 3, 3, 17, 19),        # P = 255
    (2, 3, 3, 3, 18, 18),        # P = 256
    (2, 3, 3, 3, 3, 259),        # P = 257, Ho = 1
    (2, 3, 3, 3, 260, 3),        # P = 258, Wo = 1
    (3, 2, 3, 3, 720, 1280),     # nIn H W = 2 764 800 > 8192 x 256: the gather's second grid-stride pass
])
def test_convolution_backward_dense(dfe, cuda, nIn, nOut, kH, kW, H, W):
    rng = np.random.default_rng(nIn * 1000 + nOut * 100 + kH * 10 + kW + H)
    _conv_case(dfe, cuda, rng, "conv", nIn, nOut, kH, kW, H, W)


def _table(kind, dfe):
    if kind == "trainer":            # opticalflow.lua defaults: tables.random(8, 10, 4), 16 x 16 kernels
        return dfe.tables_random(8, 10, 4, generator=torch.Generator().manual_seed(5)).numpy(), 8, 10
    if kind == "unread":             # planes 3 and 6 feed no connection: their gradInput is exactly 0
        return np.array([(1, 1), (2, 1), (4, 2), (1, 2), (5, 3)], np.int32), 6, 3
    if kind == "shuffled":           # rows not grouped by output plane
        t = dfe.tables_random(5, 6, 2, generator=torch.Generator().manual_seed(6)).numpy()
        return t[np.random.default_rng(7).permutation(len(t))], 5, 6
    if kind == "full":
        return np.array([(i, o) for o in range(1, 4) for i in range(1, 5)], np.int32), 4, 3
    if kind == "fanin1":             # one connection per output plane, in reverse order
        return np.array([(6 - o, o) for o in range(1, 6)], np.int32), 5, 5
    raise ValueError(kind)


@pytest.mark.parametrize("kind,kH,kW,H,W", [
    ("trainer", 16, 16, 16, 16),     # patch 1's features: P = 1
    ("trainer", 16, 16, 31, 31),     # patch 2's: 16 x 16
    ("unread", 3, 3, 9, 9),
    ("shuffled", 4, 3, 11, 13),
    ("full", 3, 5, 12, 20),
    ("fanin1", 5, 5, 21, 21),
])
def test_convolution_map_backward(dfe, cuda, kind, kH, kW, H, W):
    conn, nIn, nOut = _table(kind, dfe)
    rng = np.random.default_rng(H * W + kH)
    gi = _conv_case(dfe, cuda, rng, "conv_map", nIn, nOut, kH, kW, H, W, conn=conn)
    unread = sorted(set(range(1, nIn + 1)) - set(conn[:, 0].tolist()))
    assert (kind == "unread") == bool(unread)
    for i in unread:
        assert (gi[i - 1] == 0).all()


def test_accumulate_semantics(dfe, cuda):
    """backward(x, go, scale) adds scale * grad to what is there (0.5, then 1 -> 1.5 grad, exactly on integers); gradInput is the same
    every time; zeroGradParameters clears both buffers."""
    rng = np.random.default_rng(9)
    conn = np.array([(1, 1), (3, 1), (2, 2), (1, 3), (3, 3)], np.int32)
    for m in (dfe.network.SpatialConvolution(3, 4, 3, 2, device=cuda), dfe.network.SpatialConvolutionMap(torch.from_numpy(conn), 3, 2, device=cuda)):
        x = ints(rng, (3, 9, 11))
        m.weight.copy_(T(ints(rng, tuple(m.weight.shape)), cuda))
        go = ints(rng, (m.nOutputPlane, 8, 9))
        isMap = isinstance(m, dfe.network.SpatialConvolutionMap)
        rgi, rgw, rgb = ref64.conv_backward(x, m.weight.cpu().numpy(), go, conn if isMap else None, m.nOutputPlane)
        m.gradWeight.fill_(7.0)
        m.gradBias.fill_(-3.0)
        m.zeroGradParameters()
        assert int(m.gradWeight.count_nonzero()) == 0 and int(m.gradBias.count_nonzero()) == 0
        exact("accumulate grad_input", m.backward(T(x, cuda), T(go, cuda), 0.5), rgi)
        exact("accumulate acc_grad_weight", m.gradWeight, 0.5 * rgw)
        exact("accumulate grad_input", m.backward(T(x, cuda), T(go, cuda), 1.0), rgi)
        exact("accumulate acc_grad_weight", m.gradWeight, 1.5 * rgw)
        exact("accumulate acc_grad_bias", m.gradBias, 1.5 * rgb)
        m.zeroGradParameters()
        assert int(m.gradWeight.count_nonzero()) == 0 and int(m.gradBias.count_nonzero()) == 0


# ------------------------------------------------------------------ row kernels: soft-max backward, log-soft-max forward / backward
def _row_kernels(dfe, cuda, x, out_sm, go, tag):
    """the three row kernels on P x N float32 rows; float bounds.  x: log-soft-max input; out_sm: soft-max output (soft-max backward's
    input); go: gradOutput"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    P, N = x.shape
    n_s = math.ceil(N / 64) + 6
    tx, tgo, tsm = T(x, cuda), T(go, cuda), T(out_sm, cuda)
    # log-soft-max forward
    out = torch.full_like(tx, float("nan"))
    ctx.check(lib.dfe_log_softmax_f32(ctx.handle, tx.data_ptr(), P, N, out.data_ptr()))
    r = ref64.t64(x)
    m = r.max(-1, keepdim=True).values
    d = r - m
    e = d.exp()
    s = e.sum(-1, keepdim=True)
    l = m + s.log()
    o64 = r - l
    D = (e * d.abs()).sum(-1, keepdim=True) / s
    bounded("log_softmax" + tag, out, o64, ALPHA * U * (o64.abs() + l.abs() + 4 * s.log().abs() + n_s + 4 + D))
    # log-soft-max backward, from the kernel's own float32 output
    out32 = out.cpu().numpy()
    gi = torch.full_like(tx, float("nan"))
    ctx.check(lib.dfe_log_softmax_backward_f32(ctx.handle, out.data_ptr(), tgo.data_ptr(), P, N, gi.data_ptr()))
    g64 = ref64.log_softmax_backward(out32, go)
    e = ref64.t64(out32).exp()
    sg = ref64.t64(go).sum(-1, keepdim=True)
    ag = ref64.t64(go).abs().sum(-1, keepdim=True)
    bounded("log_softmax_backward" + tag, gi, g64, ALPHA * U * (g64.abs() + 5 * e * sg.abs() + n_s * e * ag))
    # soft-max backward
    gi = torch.full_like(tx, float("nan"))
    ctx.check(lib.dfe_softmax_backward_f32(ctx.handle, tsm.data_ptr(), tgo.data_ptr(), P, N, gi.data_ptr()))
    o, g = ref64.t64(out_sm), ref64.t64(go)
    s = (g * o).sum(-1, keepdim=True)
    bounded("softmax_backward" + tag, gi, ref64.softmax_backward(out_sm, go),
            ALPHA * U * o.abs() * (2 * (g - s).abs() + n_s * (g * o).abs().sum(-1, keepdim=True)))


def _rows(rng, P, N):
    x = (rng.standard_normal((P, N)) * 3).astype(np.float32)
    specials = [lambda v: v + np.float32(1e4), lambda v: v - np.float32(1e4), None, lambda v: np.full_like(v, 2.5)]
    for p in range(min(P, 4)):
        if p == 2:
            x[p, rng.integers(N)] = x[p].max() + 100        # one entry 100 above the rest
        else:
            x[p] = specials[p](x[p])
    sm = torch.softmax(torch.from_numpy(x).double(), -1).float().numpy()
    return x, sm, randn(rng, (P, N))


@pytest.mark.parametrize("N", [1, 15, 16, 63, 64, 65, 81, 256, 289, 1089])
def test_row_kernels(dfe, cuda, N):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    rng = np.random.default_rng(N)
    for P in (1, 3, 5, 4099):
        # EXACT.  log-soft-max of a row of -inf with one integer entry k at column p % N: 0 there, -inf elsewhere (every row and lane
        # lands in its own place); its backward from that output: go - [j == k] sum(go); soft-max backward on integers
        kcol = np.arange(P) % N
        x = np.full((P, N), -np.inf, np.float32)
        x[np.arange(P), kcol] = ints(rng, P)
        want = np.full((P, N), -np.inf)
        want[np.arange(P), kcol] = 0.0
        tx, out = T(x, cuda), torch.empty((P, N), device=cuda)
        ctx.check(lib.dfe_log_softmax_f32(ctx.handle, tx.data_ptr(), P, N, out.data_ptr()))
        exact("log_softmax", out, want)
        go = ints(rng, (P, N))
        gi = torch.empty_like(out)
        tgo = T(go, cuda)                                        # (kept alive: a freed temporary's block is handed out again)
        ctx.check(lib.dfe_log_softmax_backward_f32(ctx.handle, out.data_ptr(), tgo.data_ptr(), P, N, gi.data_ptr()))
        exact("log_softmax_backward", gi, ref64.t64(go) - (ref64.t64(want) == 0).double() * ref64.t64(go).sum(-1, keepdim=True))
        o = ints(rng, (P, N))
        to = T(o, cuda)
        ctx.check(lib.dfe_softmax_backward_f32(ctx.handle, to.data_ptr(), tgo.data_ptr(), P, N, gi.data_ptr()))
        exact("softmax_backward", gi, ref64.softmax_backward(o, go))
        # FLOAT: offsets of +-1e4, a row with one entry 100 above the rest, a constant row (-log N)
        x, sm, go = _rows(rng, P, N)
        _row_kernels(dfe, cuda, x, sm, go, "")


def test_row_kernels_beyond_one_grid_pass(dfe, cuda):
    """P = 40 000 rows > 8192 blocks x 4 rows: the row loop's second pass"""
    rng = np.random.default_rng(40000)
    x, sm, go = _rows(rng, 40000, 81)
    _row_kernels(dfe, cuda, x, sm, go, "")


def test_row_modules(dfe, cuda):
    """LogSoftMaxRows (Minus -> LogSoftMax of the radial trainer: the kernel runs on -x, the gradient is negated back) and SoftMaxWindow
    (after getModel's Minus: soft-max of its input x; gradInput of x's shape) against float64 autograd."""
    rng = np.random.default_rng(3)
    H1, W, N = 7, 5, 15
    x = (rng.standard_normal((H1, W, N)) * 4).astype(np.float32)
    go = randn(rng, (H1, W, N))
    n_s = math.ceil(N / 64) + 6
    ls = dfe.radial.LogSoftMaxRows()
    out = ls.forward(T(x, cuda))
    r = -ref64.t64(x)
    m = r.max(-1, keepdim=True).values
    d = r - m
    e = d.exp()
    s = e.sum(-1, keepdim=True)
    o64 = torch.log_softmax(r, -1)
    D = (e * d.abs()).sum(-1, keepdim=True) / s
    bounded("log_softmax", out, o64, ALPHA * U * (o64.abs() + (m + s.log()).abs() + 4 * s.log().abs() + n_s + 4 + D))
    gi = ls.backward(T(x, cuda), T(go, cuda))
    out32 = out.cpu().numpy()
    g64 = -ref64.log_softmax_backward(out32, go)                 # d/dx of log_softmax(-x)
    e = ref64.t64(out32).exp()
    bounded("log_softmax_backward", gi, g64,
            ALPHA * U * (g64.abs() + 5 * e * ref64.t64(go).sum(-1, keepdim=True).abs() + n_s * e * ref64.t64(go).abs().sum(-1, keepdim=True)))
    # SoftMaxWindow on a matcher-shaped input (H x W x maxh x maxw after the Minus)
    mh, mw = 4, 5
    x = (rng.standard_normal((3, 6, mh, mw)) * 3).astype(np.float32)
    go = randn(rng, (3, 6, mh * mw))
    sw = dfe.network.SoftMaxWindow()
    out = sw.forward(T(x, cuda))
    assert tuple(out.shape) == (3, 6, mh * mw)
    gi = sw.backward(T(x, cuda), T(go, cuda))
    assert tuple(gi.shape) == x.shape
    o, g = ref64.t64(out.cpu().numpy()), ref64.t64(go)
    s = (g * o).sum(-1, keepdim=True)
    n_s = math.ceil(mh * mw / 64) + 6
    bounded("softmax_backward", gi.reshape(3, 6, mh * mw), ref64.softmax_backward(o, g),
            ALPHA * U * o.abs() * (2 * (g - s).abs() + n_s * (g * o).abs().sum(-1, keepdim=True)))


# ------------------------------------------------------------------ elementwise: tanh backward, Log2
@pytest.mark.parametrize("n", [1000, 2_500_001])
def test_tanh_and_log2_backward(dfe, cuda, n):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    rng = np.random.default_rng(n)
    # tanh backward: exact on integers, then float outputs of tanh
    o, go = ints(rng, n, -2, 2), ints(rng, n)
    gi = torch.full((n,), float("nan"), device=cuda)
    to, tgo = T(o, cuda), T(go, cuda)
    ctx.check(lib.dfe_tanh_backward_f32(ctx.handle, to.data_ptr(), tgo.data_ptr(), n, gi.data_ptr()))
    exact("tanh_backward", gi, ref64.t64(go) * (1 - ref64.t64(o) ** 2))
    o, go = np.tanh(randn(rng, n) * 2).astype(np.float32), randn(rng, n)
    to, tgo = T(o, cuda), T(go, cuda)
    ctx.check(lib.dfe_tanh_backward_f32(ctx.handle, to.data_ptr(), tgo.data_ptr(), n, gi.data_ptr()))
    o64, g64 = ref64.t64(o), ref64.t64(go)
    bounded("tanh_backward", gi, g64 * (1 - o64 ** 2), ALPHA * 3 * U * g64.abs() * (1 + o64 ** 2))
    # Log2(1e-10): the input is clamped IN PLACE to >= eps; forward log, backward gradOut / (clamped) input
    eps = np.float32(1e-10)
    x = np.abs(randn(rng, n)) * 4
    x[rng.random(n) < 0.1] = 0.0
    x[rng.random(n) < 0.05] = -1.0
    x[rng.random(n) < 0.05] = 1e-12
    x[rng.random(n) < 0.05] = 1.0
    lg = dfe.Log2(1e-10)
    tx = T(x, cuda)
    out = lg.forward(tx)
    xc = np.maximum(x, eps)
    assert np.array_equal(tx.cpu().numpy(), xc)
    l64 = ref64.t64(xc).log()
    bounded("log_clamp (Log2 forward)", out, l64, ALPHA * 4 * U * l64.abs())
    assert (out.cpu().numpy()[x == 1.0] == 0).all()
    go = randn(rng, n)
    gi = lg.backward(tx, T(go, cuda))
    q = ref64.t64(go) / ref64.t64(xc)
    bounded("div (Log2 backward)", gi, q, ALPHA * U * q.abs())
    p2 = np.exp2(rng.integers(-3, 4, n)).astype(np.float32)          # powers of two: exact
    go = ints(rng, n)
    gi = lg.backward(T(p2, cuda), T(go, cuda))
    exact("div (Log2 backward)", gi, ref64.t64(go) / ref64.t64(p2))


# ------------------------------------------------------------------ spatial and radial matching backward
@pytest.mark.parametrize("K,H1,W1,mh,mw", [
    (1, 1, 1, 16, 16),           # patch mode (frame 0's features are 1 x 1), single-scale window
    (10, 1, 1, 16, 16),
    (32, 1, 1, 17, 17),
    (10, 7, 9, 17, 17),
    (32, 5, 6, 10, 16),
    (10, 1, 1, 15, 1),           # the radial trainer: hWin = 15, 10 features of 1 x 1
    (1, 12, 20, 15, 1),
    (32, 260, 260, 2, 2),        # K H1 W1 = 2 163 200 > 8192 x 256: both kernels take a second grid-stride pass
])
def test_matching_backward(dfe, cuda, K, H1, W1, mh, mw):
    rng = np.random.default_rng(K * 100 + H1 + mh)
    radial = mw == 1
    gshape = (H1, W1, mh) if radial else (H1, W1, mh, mw)
    mod = dfe.nn.SpatialRadialMatching(mh) if radial else dfe.nn.SpatialMatching(mh, mw, False)
    n = mh * mw + 2
    tag = "matching_grad%d" + (" (radial)" if radial else "")
    for integer in (True, False):
        gen = (lambda s: ints(rng, s, -4, 4)) if integer else (lambda s: randn(rng, s))
        in1, in2, go = gen((K, H1, W1)), gen((K, H1 + mh - 1, W1 + mw - 1)), gen(gshape)
        g1, g2 = mod.backward([T(in1, cuda), T(in2, cuda)], T(go, cuda))
        r1, r2, a1, a2 = ref64.matching_backward(in1, in2, go, mh, mw)
        if integer:
            exact(tag % 1, g1, r1)
            exact(tag % 2, g2, r2)
        else:
            bounded(tag % 1, g1, r1, ALPHA * n * U * a1)
            bounded(tag % 2, g2, r2, ALPHA * n * U * a2)


# ------------------------------------------------------------------ whole networks against float64
SINGLE = dict(maxh=16, maxw=16, hImg=180, wImg=320, layers=[[3, 5, 5, 8], [4, 16, 16, 10]], training_mode=True)   # opticalflow.lua defaults


def _chain_check(tag, gpu, ref_fn, gradOut):
    """every element of every gradient: |g - g64| <= 4 e32 + 8 u |g64|_inf, e32 = the CPU float32 chain's error"""
    out64, leaves64 = ref_fn(torch.float64)
    g64 = ref64.grads(out64, leaves64, gradOut)
    out32, leaves32 = ref_fn(torch.float32)
    g32 = ref64.grads(out32, leaves32, gradOut)
    assert len(gpu) == len(g64)
    for i, (g, r, c) in enumerate(zip(gpu, g64, g32)):
        g = g.cpu().double()
        assert tuple(g.shape) == tuple(r.shape), (tag, i, tuple(g.shape), tuple(r.shape))
        e32 = float((c.double() - r).abs().max())
        bound = 4 * e32 + 8 * U * float(r.abs().max())
        err = float((g - r).abs().max())
        assert float(r.abs().max()) > 0, (tag, i)
        assert err <= bound, "%s tensor %d: max error %.3g > bound %.3g (e32 %.3g, |g64| %.3g)" % (tag, i, err, bound, e32, float(r.abs().max()))
        RATIOS[tag] = max(RATIOS.get(tag, 0.0), err / bound)


def _single_scale(dfe, cuda, method, seed=1):
    geo = dict(SINGLE, output_extraction_method=method)
    model = dfe.getModel(geo, device=cuda, generator=torch.Generator().manual_seed(seed))
    rng = np.random.default_rng(seed)
    p1 = rng.random((3, 20, 20)).astype(np.float32)               # patch 1 narrowed by prepareInput: 1 x 1 features
    p2 = rng.random((3, 35, 35)).astype(np.float32)               # its 16 x 16 search region
    filt = model.modules[0].modules[0]
    c1, cm = filt.modules[0], filt.modules[2]
    assert isinstance(cm, dfe.network.SpatialConvolutionMap) and tuple(cm.connTable.shape) == (40, 2)
    return model, p1, p2, c1, cm


def _single_scale_grads(model, p1, p2, c1, cm, df, cuda):
    model.zeroGradParameters()
    model.forward([T(p1, cuda), T(p2, cuda)])
    gi = model.backward([T(p1, cuda), T(p2, cuda)], df)
    return [c1.gradWeight.clone(), c1.gradBias.clone(), cm.gradWeight.clone(), cm.gradBias.clone(), gi[0].clone(), gi[1].clone()]


def _single_ref(c1, cm, p1, p2, method):
    params = [(c1.weight.cpu(), c1.bias.cpu(), None, 8), (cm.weight.cpu(), cm.bias.cpu(), cm.connTable.numpy(), 10)]
    return lambda dt: ref64.single_scale_chain(params, p1, p2, 16, 16, method, dt)


def test_single_scale_trainer_gradients(dfe, cuda):
    """getModel(geometry, training_mode) at opticalflow.lua's defaults, patch mode, ClassNLL's df_do; then the same with the module-by-
    module filter (Sequential.fuse = False: bitwise the same gradients) and with the first layer on the matrix cores (within the bound)."""
    model, p1, p2, c1, cm = _single_scale(dfe, cuda, "max")
    out = model.forward([T(p1, cuda), T(p2, cuda)])
    assert tuple(out.shape) == (1, 1, 256)
    df = torch.zeros_like(out)
    df.view(-1)[117] = -1.0
    g = _single_scale_grads(model, p1, p2, c1, cm, df, cuda)
    _chain_check("chain single-scale", g, _single_ref(c1, cm, p1, p2, "max"), df.cpu())
    for f in model.modules[0].modules:
        f.fuse = False
    g2 = _single_scale_grads(model, p1, p2, c1, cm, df, cuda)
    for a, b in zip(g, g2):
        assert torch.equal(a, b)
    for f in model.modules[0].modules:
        f.fuse = True
    c1.kernel = "mfma"
    g3 = _single_scale_grads(model, p1, p2, c1, cm, df, cuda)
    _chain_check("chain single-scale mfma", g3, _single_ref(c1, cm, p1, p2, "max"), df.cpu())


def test_single_scale_mean_trainer_gradients(dfe, cuda):
    """output_extraction_method = 'mean' (opticalflow.lua:296-312): OutputExtractor's soft arg-max, MSECriterion's df_do on {x, y}"""
    model, p1, p2, c1, cm = _single_scale(dfe, cuda, "mean", seed=4)
    x, y = model.forward([T(p1, cuda), T(p2, cuda)])
    assert tuple(x.shape) == (1, 1) and tuple(y.shape) == (1, 1)
    tx, ty = 5.0, 11.0                                             # target_crit = x2yx(target), 1-based
    df = [torch.full((1, 1), float(x) - tx, device=cuda), torch.full((1, 1), float(y) - ty, device=cuda)]   # MSE: 2 (o - t) / 2
    g = _single_scale_grads(model, p1, p2, c1, cm, df, cuda)
    _chain_check("chain single-scale mean", g, _single_ref(c1, cm, p1, p2, "mean"), [d.cpu() for d in df])


def test_output_extractor_backward(dfe, cuda):
    """OutputExtractor.lua:37-42 per pixel: gradInput[.., k] = gx * column(k) + gy * row(k), 1-based; exact on integers"""
    rng = np.random.default_rng(2)
    H, W, mh, mw = 3, 4, 5, 7
    oe = dfe.OutputExtractor(mh, mw)
    inp = T(rng.random((H, W, mh * mw)), cuda)
    oe.forward(inp)
    gx, gy = ints(rng, (H, W)), ints(rng, (H, W))
    gi = oe.backward(inp, [T(gx, cuda), T(gy, cuda)])
    k = np.arange(mh * mw)
    exact("output_extractor_backward", gi, gx[..., None].astype(np.float64) * (k % mw + 1) + gy[..., None] * (k // mw + 1))
    with pytest.raises(ValueError):
        oe.backward(inp, [T(gx[:1], cuda), T(gy, cuda)])


def test_radial_trainer_gradients(dfe, cuda):
    """getTrainerNetwork at train_radial_opticalflow.lua's defaults ({{3,1,17,5},{5,17,1,10}}, hWin = 15), ClassNLL's df_do"""
    networkp = dict(hImg=180, wImg=320, hInput=200, wInput=200, hWin=15, layers=[[3, 1, 17, 5], [5, 17, 1, 10]])
    net = dfe.getTrainerNetwork(networkp, device=cuda, generator=torch.Generator().manual_seed(8))
    rng = np.random.default_rng(8)
    prev, cur = rng.random((3, 31, 17)).astype(np.float32), rng.random((3, 31, 17)).astype(np.float32)
    out = net.forward([T(prev, cuda), T(cur, cuda)])
    assert tuple(out.shape) == (1, 1, 15)
    df = torch.zeros_like(out)
    df[0, 0, 6] = -1.0
    net.zeroGradParameters()
    gi = net.backward([T(prev, cuda), T(cur, cuda)], df)
    filt = net.modules[0].modules[0].modules[1]
    c1, c2 = filt.modules
    g = [c1.gradWeight, c1.gradBias, c2.gradWeight, c2.gradBias, gi[0], gi[1]]
    params = [("conv", c1.weight.cpu(), c1.bias.cpu()), ("conv", c2.weight.cpu(), c2.bias.cpu())]
    _chain_check("chain radial", g, lambda dt: ref64.radial_chain(params, prev, cur, 15, dt), df.cpu())
