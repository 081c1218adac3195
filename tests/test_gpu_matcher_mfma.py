"""GPU suite (-m gpu): the matrix-core feature matcher (dfe_set_option("fm_mfma", 1), csrc/feat_matching_mfma.hip) against a FLOAT64
statement of the operation, at the shapes, offsets and size limits test_gpu_matcher_full.py does not reach.

nn.SpatialMatching(mh, mw): cost[y][x][dy][dx] = sum_k (a_k - b_k)^2, a = in1[:, y, x], b = in2[:, y + dy, x + dx].  The reference
(_ssd64) sums that in float64 on the device from the same float32 features; with it come N = |a|^2 + |b|^2 per cell, which the
matrix-core bound is relative to.

THE BOUND.  u = 2^-24 (unit roundoff of fp32, round to nearest).  The banded GEMM computes ONE accumulation of n = K + 2 terms
t = |a|^2, |b|^2, (-2 a_k) b_k (the norms ride as an extra k-step; the MFMA may add the four products of a k-step in any order).  For any
order, a floating-point sum of n terms, each product rounded once and each addition once, is within (n - 1) u sum|t| + u sum|products|
of the exact sum (first order in u; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), and 2 |a_k b_k| <= a_k^2 + b_k^2
gives sum|t| <= 2 N.  The norms themselves are fp32 fmaf chains of K terms, each within K u |a|^2 (resp. |b|^2) of the exact one.
Together:  |c - c64| <= u (2 (K + 1) N + 2 N + K N) <= 4 u (K + 2) N  -- alpha = 4, no constant fitted to what passes.  The exact kernels
(the default) sum (a_k - b_k)^2 itself: each term within 3 u of its exact value (difference, square), K - 1 additions of non-negative
terms, so |c - c64| <= u (K + 2) c64 <= 4 u (K + 2) c64 -- relative to the COST, the stronger statement, checked on the same reference.
beta = 1e-30 only absorbs denormal flushing where N == 0.  Observed errors are about u sqrt(K) N, well inside; a wrong plane, row,
column or stage gives errors of the order of the cost itself.

Arg-min: the index equals the float64 FIRST minimum wherever the two best float64 costs are more than twice the pixel's widest band
apart; the count of pixels that differ at all is reported and bounded.  The arg-min form runs the same fmaf chain as the volume form (the
same k order, 8 or 16 planes per stage), so its index also equals the first minimum of the matrix-core volume, bit for bit."""
import numpy as np
import pytest
import torch

from depth_estimation_amd._lib import FilterLayer

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ALPHA = 4.0
BETA = 1e-30


def _ssd64(in1, in2, mh, mw, y0=0, y1=None):
    """float64 reference on output rows y0 .. y1 (default: all): in1 [K][H1][W1], in2 [K][H2][W2] float32 device tensors ->
    (cost, N) [rows][W1][mh][mw] float64, cost = sum_k (a_k - b_k)^2, N = |a|^2 + |b|^2"""
    y1 = in1.shape[1] if y1 is None else y1
    a = in1[:, y0:y1].double()
    b = in2[:, y0 : y1 + mh - 1].double()
    h, w = a.shape[1:]
    na, nb = (a * a).sum(0), (b * b).sum(0)
    cost = torch.empty((h, w, mh, mw), dtype=torch.float64, device=a.device)
    nrm = torch.empty_like(cost)
    for dy in range(mh):
        for dx in range(mw):
            bs = b[:, dy : dy + h, dx : dx + w]
            cost[:, :, dy, dx] = ((a - bs) ** 2).sum(0)
            nrm[:, :, dy, dx] = na + nb[dy : dy + h, dx : dx + w]
    return cost, nrm


def _first_min_index(vol):
    """[H][W][h][w] -> int64 0-based index of the FIRST minimum of every window (whatever torch.argmin does on ties)"""
    H1, W1 = vol.shape[:2]
    v = vol.reshape(H1, W1, -1)
    ar = torch.arange(v.shape[2], device=vol.device)
    out = torch.empty((H1, W1), dtype=torch.int64, device=vol.device)
    for y0 in range(0, H1, 64):
        blk = v[y0 : y0 + 64]
        out[y0 : y0 + 64] = torch.where(blk == blk.min(dim=2, keepdim=True).values, ar, v.shape[2]).min(dim=2).values
    return out


def _mfma_kernel(K, mh, volume):
    """the instantiation dfe_fm_launch_mfma launches (feat_matching_mfma.hip): the volume form stages 8 planes, the arg-min form 16 where K % 16 == 0"""
    if volume:
        return "fmm_kernel<%d,%d,false>" % (mh, mh)
    return "fmm_kernel<%d,%d,true,%d>" % (mh, mh, 16 if K % 16 == 0 else 8)


def _features(cuda, K, H1, W1, mh, seed, offset=0.0, bias=False):
    """randn maps + offset (+ a per-plane bias), with a shifted copy planted so that many windows hold a near-zero cost next to large ones"""
    g = torch.Generator(device=cuda).manual_seed(seed)
    in1 = torch.randn((K, H1, W1), generator=g, device=cuda)
    in2 = torch.randn((K, H1 + mh - 1, W1 + mh - 1), generator=g, device=cuda)
    if H1 > 20 and W1 > 20:
        in2[:, 3 : 3 + H1, 5 : 5 + W1] = in1 + 0.05 * torch.randn((K, H1, W1), generator=g, device=cuda)
    shift = torch.full((K, 1, 1), float(offset), device=cuda)
    if bias:
        shift += 10.0 * torch.randn((K, 1, 1), generator=g, device=cuda)
    return (in1 + shift).contiguous(), (in2 + shift).contiguous()


def _check_against_float64(dfe, cuda, in1, in2, mh):
    """exact volume, matrix-core volume and matrix-core arg-min form, each against _ssd64 of the whole map; returns (vol, c64, N)"""
    ctx = dfe.get_ctx(0)
    lib = dfe.lib()
    K, H1, W1 = in1.shape
    mw = mh
    c64, nrm = _ssd64(in1, in2, mh, mw)
    exact = torch.full((H1, W1, mh, mw), float("nan"), device=cuda)
    ctx.check(lib.dfe_spatial_matching_f32(ctx.handle, in1.data_ptr(), in2.data_ptr(), K, H1, W1, mh, mw, exact.data_ptr()))
    assert not ctx.last_kernel().startswith("fmm_kernel"), ctx.last_kernel()
    with ctx.options(fm_mfma=1):
        vol = torch.full((H1, W1, mh, mw), float("nan"), device=cuda)
        ctx.check(lib.dfe_spatial_matching_f32(ctx.handle, in1.data_ptr(), in2.data_ptr(), K, H1, W1, mh, mw, vol.data_ptr()))
        assert ctx.last_kernel() == "fmm_kernel", (ctx.last_kernel(), _mfma_kernel(K, mh, True))
        idx = torch.full((H1, W1), -7, dtype=torch.int64, device=cuda)
        xf, yf = torch.full((H1, W1), float("nan"), device=cuda), torch.full((H1, W1), float("nan"), device=cuda)
        ctx.check(lib.dfe_spatial_matching_argmin_f32(ctx.handle, in1.data_ptr(), in2.data_ptr(), K, H1, W1, mh, mw, idx.data_ptr(), xf.data_ptr(), yf.data_ptr()))
        assert ctx.last_kernel() == "fmm_kernel+argmin", (ctx.last_kernel(), _mfma_kernel(K, mh, False))
    torch.cuda.synchronize()
    assert int(torch.isnan(exact).sum()) == 0 and int(torch.isnan(vol).sum()) == 0, "cells left unwritten"
    # the exact kernel: relative to the cost
    eerr = (exact.double() - c64).abs()
    ebad = eerr > ALPHA * U * (K + 2) * c64 + BETA
    assert not bool(ebad.any()), "exact kernel: %d cells outside 4 u (K + 2) c, worst error %g" % (int(ebad.sum()), float(eerr.max()))
    # the matrix-core volume: relative to |a|^2 + |b|^2
    tol = ALPHA * U * (K + 2) * nrm + BETA
    err = (vol.double() - c64).abs()
    bad = err > tol
    assert not bool(bad.any()), "matrix-core volume: %d cells outside 4 u (K + 2) N, worst error / bound %g" % (int(bad.sum()), float((err / tol).max()))
    # the arg-min form: the first minimum of its own volume, bit for bit, and the float64 first minimum outside near-ties
    assert torch.equal(idx, _first_min_index(vol) + 1)
    want = _first_min_index(c64)
    srt = torch.sort(c64.reshape(H1, W1, -1), dim=2).values
    clear = (srt[..., 1] - srt[..., 0]) > 2 * tol.reshape(H1, W1, -1).amax(dim=2)
    differ = idx != want + 1
    assert not bool((differ & clear).any()), "%d pixels differ from the float64 first minimum outside near-ties" % int((differ & clear).sum())
    ndiff = int(differ.sum())
    assert ndiff <= 0.01 * idx.numel() + 2, "differing pixels: %d of %d" % (ndiff, idx.numel())
    i0 = idx - 1
    lWin, tWin = (mw + 1) // 2 - 1, (mh + 1) // 2 - 1
    assert torch.equal(yf, (i0 // mw - tWin).to(torch.float32)) and torch.equal(xf, (i0 % mw - lWin).to(torch.float32))
    if H1 > 20 and W1 > 20 and K >= 8:       # (one or two planes: some random cell of a window comes as close as the planted one)
        assert float((idx[4:-4, 8:-8] == 3 * mw + 5 + 1).float().mean()) > 0.95, "the planted shift is not what the interior finds"
    return vol, c64, nrm


SHAPES = [
    # 16 x 16 windows with K % 16 == 0: the arg-min form is fmm_kernel<16,16,true,16>; 2128 / 589 tiles (several per block: the cross-tile
    # prefetch, the norm buffers' tile parity and the XCD permutation for MH = 16)
    (16, 448, 608, 16),
    (32, 448, 608, 16),
    (16, 241, 301, 16),
    (32, 241, 301, 16),
    # 17 x 17: K = 16 (volume: 2 stages, arg-min: 1 of 16 planes) and K = 48 (6 and 3 stages); W1 = 1 (mod 16), H1 = 1 (mod 8)
    (16, 201, 257, 17),
    (48, 201, 257, 17),
    # the guard's K limits and a ragged last stage (zero-filled planes), at W1 = 1 (mod 16) and H1 = 1 (mod 8)
    (1, 97, 161, 17),
    (17, 65, 113, 17),
    (256, 57, 129, 16),
    (256, 41, 49, 17),
    # one-pixel rows / columns
    (3, 1, 17, 17),
    (8, 9, 1, 16),
]


@pytest.mark.parametrize("K,H1,W1,mh", SHAPES)
def test_matrix_core_matcher_against_float64(dfe, cuda, K, H1, W1, mh):
    in1, in2 = _features(cuda, K, H1, W1, mh, seed=K * 1000 + H1 + W1 + mh)
    _check_against_float64(dfe, cuda, in1, in2, mh)


@pytest.mark.parametrize("offset,bias", [(0.0, False), (4.0, False), (30.0, False), (0.0, True)])
@pytest.mark.parametrize("K,H1,W1,mh", [(32, 241, 301, 17), (16, 448, 608, 16)])
def test_matrix_core_matcher_offset_features_against_float64(dfe, cuda, K, H1, W1, mh, offset, bias):
    """a = randn + c, b = randn + c (c = 0, 4, 30), or + a per-plane bias of scale 10: the costs are the same as without the shift (SSD is
    shift-invariant) but N = |a|^2 + |b|^2 grows as 2 K c^2, and with it the matrix-core error.  Features like these come from a filter
    stack whose last layer has a bias and no tanh, or from raw intensities (prefilter).  The bound relative to N holds; the earlier
    statement (1e-5 |c| + 1e-6 max |c|, relative to the costs) does not at c = 30 -- the count of cells outside it is printed."""
    in1, in2 = _features(cuda, K, H1, W1, mh, seed=K + H1 + int(offset) + (7 if bias else 0), offset=offset, bias=bias)
    vol, c64, _ = _check_against_float64(dfe, cuda, in1, in2, mh)
    old_bad = (vol.double() - c64).abs() > 1e-5 * c64 + 1e-6 * float(c64.max())
    print("offset %g bias %s: %d of %d cells outside 1e-5 |c| + 1e-6 max|c|" % (offset, bias, int(old_bad.sum()), old_bad.numel()))


LIMIT = [
    # K (H1 + 16) (W1 + 16) = 63 x 3641 x 4681 = 2^30 - 1 floats: the matrix cores, the last planes' byte offsets just below 2^32
    (63, 3625, 4665, True),
    # 64 x 4096 x 4096 = 2^30: past what 32-bit byte offsets address -- the exact kernels
    (64, 4080, 4080, False),
]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("K,H1,W1,takes", LIMIT)
def test_matrix_core_matcher_size_limit(dfe, cuda, K, H1, W1, takes):
    """fm_try_mfma (csrc/fm_select.h) admits K H2 W2 < 2^30 floats of in2 (the LDS-DMA requests are 32-bit byte offsets from the map's base;
    the guard once admitted 2^31, where they wrap inside the buffer: wrong costs, no fault).  On both sides of the limit, one arg-min launch:
    the kernel named, and the index against the float64 first minimum on the first and the last output rows (whose planes lie furthest
    into in2).  About 4.3 GB per map; freed at the end."""
    ctx = dfe.get_ctx(0)
    lib = dfe.lib()
    mh = mw = 17
    assert (K * (H1 + mh - 1) * (W1 + mw - 1) < (1 << 30)) == takes
    g = torch.Generator(device=cuda).manual_seed(K)
    in1 = torch.randn((K, H1, W1), generator=g, device=cuda)
    in2 = torch.randn((K, H1 + mh - 1, W1 + mw - 1), generator=g, device=cuda)
    idx = torch.full((H1, W1), -7, dtype=torch.int64, device=cuda)
    try:
        with ctx.options(fm_mfma=1):
            ctx.check(lib.dfe_spatial_matching_argmin_f32(ctx.handle, in1.data_ptr(), in2.data_ptr(), K, H1, W1, mh, mw, idx.data_ptr(), None, None))
            kern = ctx.last_kernel()
        torch.cuda.synchronize()
        if takes:
            assert kern == "fmm_kernel+argmin", kern
        else:
            assert not kern.startswith("fmm_kernel"), kern
        assert int((idx < 1).sum()) == 0 and int((idx > mh * mw).sum()) == 0
        for y0, y1 in [(0, 2), (H1 - 2, H1)]:
            c64, nrm = _ssd64(in1, in2, mh, mw, y0, y1)
            tol = ALPHA * U * (K + 2) * nrm + BETA
            srt = torch.sort(c64.reshape(y1 - y0, W1, -1), dim=2).values
            clear = (srt[..., 1] - srt[..., 0]) > 2 * tol.reshape(y1 - y0, W1, -1).amax(dim=2)
            assert float(clear.float().mean()) > 0.5
            want = _first_min_index(c64) + 1
            got = idx[y0:y1]
            assert torch.equal(got[clear], want[clear]), "rows %d..%d: %d pixels differ from the float64 first minimum" % (
                y0, y1, int((got != want)[clear].sum()))
            del c64, nrm
    finally:
        del in1, in2, idx
        torch.cuda.empty_cache()


@pytest.mark.timeout(600)
def test_filtered_pair_prefilter_planes_past_the_lean_matchers_limit(dfe, cuda):
    """dfe_flow_pair_filtered_f32 with nlayers = 0 (prefilter) reads patch 1 as a view of the whole map: planes H W floats apart.  The
    one-kernel matcher (feat_matching_flat.hip) declines planes of 2^29 floats or more; its predicate used to look at H1 W1 only, so at
    H W >= 2^29 > H1 W1 the call planned no volume and then failed with "the matcher declined a shape its predicate took".  Now the
    predicate sees the view: the stand-alone ops are planned, whose volume (H1 W1 17 17 floats, twice: 1.2 TB) does not fit -- the
    documented DFE_E_ALLOC, no output written (include/dfe.h), never a silent result; and the failed allocation does not surface again
    as the error of the caller's next HIP call."""
    ctx = dfe.get_ctx(0)
    lib = dfe.lib()
    H = W = 23171
    maxh = maxw = 17
    H1, W1 = H - maxh + 1, W - maxw + 1
    assert H * W >= (1 << 29) and H1 * W1 < (1 << 29)
    I0 = torch.zeros((1, H, W), device=cuda)
    I1 = torch.zeros((1, H, W), device=cuda)
    scores = torch.full((H1, W1), 7.0, device=cuda)
    try:
        rc = lib.dfe_flow_pair_filtered_f32(ctx.handle, I0.data_ptr(), I1.data_ptr(), 1, H, W, (FilterLayer * 1)(), 0, maxh, maxw, 0, 0.0, H1, W1,
                                            None, None, None, scores.data_ptr())
        msg = lib.dfe_last_error(ctx.handle).decode()
        torch.cuda.synchronize()
        assert rc == -3, (rc, msg)                                    # DFE_E_ALLOC
        assert "declined" not in msg, msg
        # the failed allocation is not left behind as the thread's last HIP error: the next launch (here torch's) runs
        assert bool((scores == 7.0).all()), "an output was written by a call that failed"
    finally:
        del I0, I1, scores
        torch.cuda.empty_cache()
