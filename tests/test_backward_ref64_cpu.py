"""CPU suite: the float64 references of tests/ref64.py (what tests/test_gpu_backward.py measures the backward kernels against) pinned
against the oracle's gradients at tiny shapes -- bit for bit on small integers (every sum exact in any order), within a few fp32 ulps on
floats -- and autograd against the closed forms, so the reference itself is checked on every CPU run."""
import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import ref64


def _ints(rng, shape, lo=-4, hi=4):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


@pytest.mark.parametrize("kH,kW,use_map", [(3, 3, False), (1, 4, False), (3, 1, False), (2, 3, True)])
def test_conv_reference_equals_oracle(kH, kW, use_map):
    rng = np.random.default_rng(kH * 7 + kW)
    nIn, nOut, H, W = 3, 4, 6, 7
    conn = np.array([(1, 1), (3, 1), (2, 2), (1, 3), (2, 3), (3, 4), (1, 4)], np.int32) if use_map else None
    wshape = (len(conn), kH, kW) if use_map else (nOut, nIn, kH, kW)
    for integer in (True, False):
        gen = (lambda s: _ints(rng, s)) if integer else (lambda s: rng.standard_normal(s).astype(np.float32))
        x, w, go = gen((nIn, H, W)), gen(wshape), gen((nOut, H - kH + 1, W - kW + 1))
        egi, egw, egb = orc.spatial_convolution_backward(x, w, go, conn=conn, nOut=nOut)
        gi, gw, gb = ref64.conv_backward(x, w, go, conn, nOut)
        cgi, cgw, cgb = ref64.conv_backward_closed(x, w, go, conn, nOut)
        for r, c, e in ((gi, cgi, egi), (gw, cgw, egw), (gb, cgb, egb)):
            if integer:
                assert np.array_equal(r.numpy(), e) and np.array_equal(c.numpy(), e)
            else:
                assert np.allclose(r.numpy(), e, rtol=1e-5, atol=1e-5) and np.allclose(r.numpy(), c.numpy(), rtol=1e-12, atol=1e-12)
        # the forward too: the reference convolution is the oracle's
        b = gen((nOut,))
        ref = ref64.conv(ref64.t64(x), ref64.t64(w), ref64.t64(b), conn, nOut).numpy()
        eo = orc.spatial_convolution_map(x, w, b, conn, nOut) if use_map else orc.spatial_convolution(x, w, b)
        assert np.array_equal(ref, eo) if integer else np.allclose(ref, eo, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("K,H1,W1,mh,mw", [(2, 3, 4, 3, 2), (1, 1, 1, 4, 4), (3, 2, 5, 5, 1)])
def test_matching_reference_equals_oracle(K, H1, W1, mh, mw):
    rng = np.random.default_rng(K + mh)
    for integer in (True, False):
        gen = (lambda s: _ints(rng, s)) if integer else (lambda s: rng.standard_normal(s).astype(np.float32))
        in1, in2, go = gen((K, H1, W1)), gen((K, H1 + mh - 1, W1 + mw - 1)), gen((H1, W1, mh, mw))
        g1, g2, a1, a2 = ref64.matching_backward(in1, in2, go, mh, mw)
        ag1, ag2 = ref64.matching_backward_autograd(in1, in2, go, mh, mw)
        assert torch.allclose(g1, ag1, rtol=1e-12, atol=1e-12) and torch.allclose(g2, ag2, rtol=1e-12, atol=1e-12)
        assert (a1 >= g1.abs()).all() and (a2 >= g2.abs()).all()
        if mw == 1:
            e1, e2 = orc.radial_matching_backward(in1, in2, go.reshape(H1, W1, mh), mh)
        else:
            e1, e2 = orc.spatial_matching_backward(in1, in2, go, mh, mw)
        if integer:
            assert np.array_equal(g1.numpy(), e1) and np.array_equal(g2.numpy(), e2)
        else:
            assert np.allclose(g1.numpy(), e1, rtol=1e-5, atol=1e-5) and np.allclose(g2.numpy(), e2, rtol=1e-5, atol=1e-5)
        fwd = orc.radial_matching(in1, in2, mh) if mw == 1 else orc.spatial_matching(in1, in2, mh, mw)
        ref = ref64.matching(ref64.t64(in1), ref64.t64(in2), mh, mw).numpy().reshape(fwd.shape)
        assert np.array_equal(ref, fwd) if integer else np.allclose(ref, fwd, rtol=1e-5, atol=1e-5)


def test_rowwise_references_equal_oracle_and_autograd():
    rng = np.random.default_rng(11)
    for N in (1, 7, 70):
        x = (rng.standard_normal((5, N)) * 3).astype(np.float32)
        go = rng.standard_normal((5, N)).astype(np.float32)
        # log-soft-max: forward and backward
        out = orc.log_softmax(x)
        assert np.allclose(torch.log_softmax(ref64.t64(x), -1).numpy(), out, rtol=1e-5, atol=1e-5)
        assert np.allclose(ref64.log_softmax_backward(out, go).numpy(), orc.log_softmax_backward(out, go), rtol=1e-5, atol=1e-5)
        xv = ref64.t64(x).requires_grad_()
        torch.log_softmax(xv, -1).backward(ref64.t64(go))
        assert np.allclose(ref64.log_softmax_backward(torch.log_softmax(ref64.t64(x), -1), go).numpy(), xv.grad.numpy(), rtol=1e-12, atol=1e-12)
        # soft-max backward (softmin of the negated input is the soft-max of the input)
        sm = orc.softmin(-x)
        assert np.allclose(ref64.softmax_backward(sm, go).numpy(), orc.softmax_backward(sm, go), rtol=1e-5, atol=1e-6)
        xv = ref64.t64(x).requires_grad_()
        torch.softmax(xv, -1).backward(ref64.t64(go))
        assert np.allclose(ref64.softmax_backward(torch.softmax(ref64.t64(x), -1), go).numpy(), xv.grad.numpy(), rtol=1e-12, atol=1e-12)
        # tanh backward
        th = orc.tanh(x)
        xv = ref64.t64(x).requires_grad_()
        torch.tanh(xv).backward(ref64.t64(go))
        assert np.allclose(xv.grad.numpy(), orc.tanh_backward(th, go), rtol=1e-5, atol=1e-6)
    # integer data: soft-max backward is exact in any order
    out, go = _ints(rng, (4, 33)), _ints(rng, (4, 33))
    assert np.array_equal(ref64.softmax_backward(out, go).numpy(), orc.softmax_backward(out, go))
    # Log2: the clamp passes gradOut / eps through, as Log.lua's in-place clamp does
    x = torch.tensor([0.0, 1e-12, 0.5, 2.0], dtype=torch.float64, requires_grad=True)
    eps = float(np.float32(1e-10))
    y = ref64.log2(x, eps)
    y.backward(torch.ones(4, dtype=torch.float64))
    assert torch.equal(y.detach(), torch.tensor([eps, eps, 0.5, 2.0], dtype=torch.float64).log())
    assert torch.equal(x.grad, 1 / torch.tensor([eps, eps, 0.5, 2.0], dtype=torch.float64))
