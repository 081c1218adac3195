"""radialFlowDepth(sgm=...) on the device: the one call dfe_radial_flow_depth_pair_sgm_f32 against the same steps as
staged public calls, bit for bit, with the sub-pixel refinement and the zeroed last row on and off; the polar flow against the numpy
restatement of the aggregation on the matcher's volume; and sgm=None against the entries as they were.  Two of the small configurations of
tests/radial_cases.py: A (hWin 15, odd sizes) and D (hWin 8).  (device_case, KEYS and np_rule are taken from the test modules that define
them: existing test files stay as they are, so the helpers could not move to a shared module.)

OPEN, DESIGN section 4.29: run in one pytest process BEHIND tests/test_gpu_sgm.py, test_one_call_equals_staged_and_the_definition[A] fails
at its second combination (subpixel off, zero_last_row on) on `output`: the STAGED matcher volume differs from the one call's in 95 084 and
in 150 510 of 168 750 elements in two runs (first cell 0.1257 / 0.1590 against 0.000814).  The wrong values are neither the aggregate nor
a path plane of this case (those hold 0.000814 and 0.0065 there): they are a matcher volume of a wrong feature map.  In a third run
the staged route's second feature map (the convolution modules' output, a torch tensor at the start of a segment torch had just
taken from the driver) held 0.0 in 2 624 of its 147 500 cells; the staged route repeated at once wrote the right values there and
gave the one call's volume.  This file alone passes, as do the same calls in the same order from a plain script on one context."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import radial_cases as rc
from tests.sgm_ref import sgm_aggregate
from tests.test_gpu_radial_edges import KEYS, device_case
from tests.test_gpu_radial_subpixel import np_rule

pytestmark = pytest.mark.gpu
SGM = {"A": dict(P1=0.02, P2=0.2, paths=0xff), "D": (0.01, 0.05)}      # D: the defaults, 4 paths and ring = hWin


def _where(x, y):
    """where two tensors of one shape differ: how many elements, the first and last flat index, and the values at the first"""
    d = (x != y).flatten().nonzero().flatten()
    if d.numel() == 0:
        return " (NaN only)"
    i = int(d[0])
    return " (%d of %d elements, flat %d .. %d; at the first: %r against %r; data_ptr %x against %x)" % (
        d.numel(), x.numel(), i, int(d[-1]), float(x.flatten()[i]), float(y.flatten()[i]), x.data_ptr(), y.data_ptr())


@pytest.mark.parametrize("name", sorted(SGM))
def test_one_call_equals_staged_and_the_definition(dfe, cuda, name):
    Cc, hIn, wIn, hWin, layers, alpha, e2 = rc.CASES[name]
    networkp, net, a, b = device_case(dfe, cuda, name)
    sgm = SGM[name]
    sg = sgm if isinstance(sgm, dict) else dict(P1=sgm[0], P2=sgm[1])
    want_agg = None
    for sub in (False, True):
        for zl in (False, True):
            tag = "case %s subpixel %s zero_last_row %s" % (name, sub, zl)
            one, stg = (dfe.radialFlowDepth(networkp, net, a, b, e2, alpha_polar=alpha, one_call=oc, want_volume=True, zero_last_row=zl, subpixel=sub, sgm=sgm)
                        for oc in (True, False))
            for k in KEYS + ("aggregate",):
                assert torch.equal(one[k], stg[k]), tag + ": " + k + _where(one[k], stg[k])
            if want_agg is None:
                want_agg, want_flow = sgm_aggregate(one["output"].cpu().numpy(), sg["P1"], sg["P2"], sg.get("paths", 0x0f), sg.get("ring", hWin))
                _, want_sub = np_rule(want_agg)
            assert np.array_equal(one["aggregate"].cpu().numpy().view(np.int32), want_agg.view(np.int32)), tag
            ref = (want_sub if sub else want_flow).copy()
            if zl:
                ref[-1] = 0
            assert np.array_equal(one["polar_flow"].cpu().numpy(), ref), tag
            # without the volumes the aggregate stays in the library's scratch: same flow, same depth
            lean = dfe.radialFlowDepth(networkp, net, a, b, e2, alpha_polar=alpha, zero_last_row=zl, subpixel=sub, sgm=sgm)
            assert "aggregate" not in lean and "output" not in lean
            for k in KEYS[1:]:
                assert torch.equal(lean[k], one[k]), tag + ": lean " + k
    plain = dfe.radialFlowDepth(networkp, net, a, b, e2, alpha_polar=alpha, want_volume=True)
    assert torch.equal(plain["output"], one["output"]), "the matcher's volume is the plain call's"
    assert not torch.equal(plain["polar_flow"], one["polar_flow"]), "the aggregation changes the flow"


@pytest.mark.parametrize("name", sorted(SGM))
def test_sgm_none_is_the_call_as_it_was(dfe, cuda, name):
    Cc, hIn, wIn, hWin, layers, alpha, e2 = rc.CASES[name]
    networkp, net, a, b = device_case(dfe, cuda, name)
    from depth_estimation_amd._lib import RadialParams
    from depth_estimation_amd.radial import _separable_weights

    w1, b1, w2, b2, th = _separable_weights(net, networkp)
    for sub in (False, True):
        for oc in (True, False):
            dflt = dfe.radialFlowDepth(networkp, net, a, b, e2, alpha_polar=alpha, one_call=oc, want_volume=True, subpixel=sub)
            none = dfe.radialFlowDepth(networkp, net, a, b, e2, alpha_polar=alpha, one_call=oc, want_volume=True, subpixel=sub, sgm=None)
            assert sorted(dflt) == sorted(none) == sorted(KEYS)
            prm = RadialParams(Cc, rc.HIMG, rc.WIMG, hIn, wIn, hWin, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), float(alpha), 0.65, 0)
            outs = {k: torch.empty_like(dflt[k]) for k in KEYS}
            ctx = dfe.get_ctx(0)
            entry = dfe.lib().dfe_radial_flow_depth_pair_subpixel_f32 if sub else dfe.lib().dfe_radial_flow_depth_pair_f32
            ctx.check(entry(ctx.handle, C.byref(prm), a.data_ptr(), b.data_ptr(), float(e2[0]), float(e2[1]), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                            b2.data_ptr(), *(outs[k].data_ptr() for k in KEYS)))
            for k in KEYS:
                assert torch.equal(dflt[k], none[k]) and torch.equal(dflt[k], outs[k]), (sub, oc, k)


def test_sgm_argument_errors(dfe, cuda):
    Cc, hIn, wIn, hWin, layers, alpha, e2 = rc.CASES["D"]
    networkp, net, a, b = device_case(dfe, cuda, "D")
    for bad in ((1.0,), (1.0, 2.0, 3.0), "ab", 1.0, dict(P1=1.0), dict(P1=1.0, P2=2.0, rings=3), (2.0, 1.0), (-1.0, 1.0), dict(P1=1.0, P2=2.0, paths=0),
                dict(P1=1.0, P2=2.0, ring=wIn + 1), dict(P1=1.0, P2=float("nan"))):
        for oc in (True, False):
            with pytest.raises(ValueError):
                dfe.radialFlowDepth(networkp, net, a, b, e2, one_call=oc, sgm=bad)
    from depth_estimation_amd._lib import RadialParams
    from depth_estimation_amd.radial import _separable_weights

    w1, b1, w2, b2, th = _separable_weights(net, networkp)
    prm = RadialParams(Cc, rc.HIMG, rc.WIMG, hIn, wIn, hWin, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), 1.0, 0.65, 0)
    hm = dfe.radial_out_shape(networkp)[0]
    vol = torch.zeros((hm, wIn, hWin), device=cuda)
    ctx, fn = dfe.get_ctx(0), dfe.lib().dfe_radial_flow_depth_pair_sgm_f32
    call = lambda P1, P2, paths, ring, v, g: fn(ctx.handle, C.byref(prm), a.data_ptr(), b.data_ptr(), float(e2[0]), float(e2[1]), w1.data_ptr(), b1.data_ptr(),
                                                w2.data_ptr(), b2.data_ptr(), P1, P2, paths, ring, 0, v, g, None, None, None, None)
    assert call(1.0, 2.0, 0x0f, 8, None, None) == 0
    assert call(1.0, 2.0, 0, 8, None, None) == -1
    assert call(2.0, 1.0, 0x0f, 8, None, None) == -1
    assert call(1.0, 2.0, 0x0f, wIn + 1, None, None) == -1
    assert call(1.0, 2.0, 0x0f, 8, vol.data_ptr(), vol.data_ptr()) == -1
    torch.cuda.synchronize()
