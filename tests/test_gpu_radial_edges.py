"""The radial one-call path (dfe_radial_flow_depth_pair_f32 / _subpixel_f32, csrc/radial_pipeline.hip) at the cases of
tests/radial_cases.py: odd and ragged shapes of its row / column filters, every instantiation and the generic fall-backs, the planar and
the interleaved warp, hWin 8 / 12 / 16, one matcher row and whole matcher blocks, alpha_polar != 1, epipoles on the corner, on the edge,
outside the frame and at fractions of a pixel.

Each case is checked stage by stage, so that no tolerance compounds: one call == staged module path bit for bit; the volume against the
oracle; the polar flow against the device's OWN volume (first minimum, sub-pixel rule) and against the oracle's wherever the oracle's two
best costs are further apart than twice the volume's measured error; the cartesian flow against the oracle's P2C stage fed the device's
own polar flow; depth and confidences against the oracle's flow2depth fed the device's own cartesian flow.  tests/test_radial_cases_cpu.py
holds the cases to the conditions that keep these checks from being vacuous.

Open finding (MI355X, not yet explained): in the FIRST pass of a process over the cases, check 1 fails from run to run at some of B, C, D, E
on `output` (and what follows from it), and passes in a second pass of the same process.  Wherever it failed the one call's volume equalled
the oracle's (E below) and the STAGED features were off by up to 0.6 in strips of 2 to 64 columns of single rows; the first wrong tensor
is the staged row filter's output, i.e. conv_batch_kernel<17,2>, <17,2>+tanh, <17,4> or <5,1> with kH = 1 (csrc/filters.hip, reached
through dfe_spatial_convolution[_tanh]_f32).  A, F and H, whose row filter has 5 output planes at 17 taps and therefore runs conv_kernel,
never failed.  Once the one call of case E (its 6-plane row filter goes through the same kernel) was off at 40 pixels.  Measured where
check 1 passed: E = 0 (A, C, D, E, F), 4.1e-8 = 1.8e-6 max|oracle| (B), 1.5e-8 = 6.0e-7 (H), 4.7e-8 (G); pixels with 0 < gap <= 2E at
most 0.18 % (B); the cartesian flow at most 0.014 of its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import radial_cases as rc

pytestmark = pytest.mark.gpu
DFE_E_SHAPE = -2
KEYS = ("output", "polar_flow", "flow", "depth", "confs")


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def device_case(dfe, cuda, name):
    """(networkp, tester network holding the weights of rc.weights, previous frame, frame) on the device"""
    networkp = rc.networkp(name)
    net = dfe.getTesterNetwork(networkp, device=cuda, generator=torch.Generator().manual_seed(0))
    convs = [m for m in net.modules[0].modules[1].modules if hasattr(m, "weight")]
    w1, b1, w2, b2, _ = rc.weights(name)
    for t, a in zip((convs[0].weight, convs[0].bias, convs[1].weight, convs[1].bias), (w1, b1, w2, b2)):
        assert tuple(t.shape) == a.shape
        t.copy_(T(a, cuda))
    f0, f1 = rc.frames(rc.CASES[name][0])
    return networkp, net, T(f0, cuda), T(f1, cuda)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_one_call_equals_staged_and_each_stage_its_oracle(dfe, cuda, name):
    Cc, hIn, wIn, hWin, layers, alpha, e2 = rc.CASES[name]
    networkp, net, a, b = device_case(dfe, cuda, name)
    ref, g, grid = rc.reference(name), rc.geometry(name), rc.p2c_grid(name)
    assert dfe.radial_out_shape(networkp) == (g["hm"], g["hOut"], g["wOut"])
    seam = rc.seam_set(name)
    assert seam.mean() <= rc.SEAM_CAP
    dy, dx = rc.coord_tol(grid[0]), rc.coord_tol(grid[1])
    volume, worst = None, 0.0
    for sub in (False, True):
        for zl in (False, True):
            tag = "case %s subpixel %s zero_last_row %s" % (name, sub, zl)
            one, stg = (dfe.radialFlowDepth(networkp, net, a, b, e2, alpha_polar=alpha, one_call=oc, want_volume=True, zero_last_row=zl, subpixel=sub)
                        for oc in (True, False))
            # 1. one call == staged, every output
            assert tuple(one["output"].shape) == (g["hm"], wIn, hWin) and tuple(one["flow"].shape) == (g["hOut"], g["wOut"]), tag
            differ = [k for k in KEYS if not torch.equal(one[k], stg[k])]
            assert not differ, "%s: one call != staged at %s" % (tag, differ)
            out, pf, cart, depth, confs = (one[k].cpu().numpy() for k in KEYS)
            if volume is None:
                # 3. the volume against the oracle: the bound of test_radial_path_one_call_equals_staged_and_oracle (sampling-coordinate
                #    jitter through two convolutions)
                volume = out
                E = float(np.abs(out.astype(np.float64) - ref["output"]).max())
                vmax = float(np.abs(ref["output"]).max())
                assert E <= 2e-3 * vmax, "%s: max |volume - oracle| = %.3e = %.3e max|oracle|" % (tag, E, E / vmax)
                gap = rc.cost_gap(ref["output"]).astype(np.float64)
                near = float(((gap > 0) & (gap <= 2 * E)).mean())
                print("case %s: E = max |volume - oracle| = %.3e = %.3e of max|oracle|; oracle pixels with 0 < gap <= 2E: %.2f %%, gap == 0: %.2f %%" % (
                    name, E, E / vmax, 100 * near, 100 * float((gap == 0).mean())))
                assert near < rc.TIE_CAP, tag
            assert np.array_equal(out, volume), tag
            # 4. the arg-min: of the device's own volume exactly, of the oracle's wherever 2E cannot change the winner
            first, refined = rc.subpixel_rule(out)
            assert np.array_equal(first, (out == out.min(-1, keepdims=True)).argmax(-1)), tag     # the first cell equal to the row minimum
            mine = refined if sub else first.astype(np.float32)
            rf = ref["polar_flow"].copy()
            if zl:
                mine[-1], rf[-1] = 0, 0
            assert np.array_equal(pf, mine), tag
            if not sub:
                assert ((pf == rf) | (gap <= 2 * E)).all(), "%s: polar flow differs from the oracle's at %d pixels whose costs are apart" % (
                    tag, int(((pf != rf) & (gap > 2 * E)).sum()))
            # 5. the cartesian flow: the oracle's P2C stage on the device's own polar flow
            cref = orc.warp_bilinear(pf[None], grid)[0]
            bound = (dy + dx) * rc.tap_range(pf, grid) + 1e-6 * np.maximum(1, np.abs(cref))
            ratio = np.where(seam, 0, np.abs(cart.astype(np.float64) - cref) / bound)
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1).all(), "%s: cartesian flow off its bound at %d pixels, worst %.3g x the bound" % (tag, int((ratio > 1).sum()), ratio.max())
            # 6. depth and confidences: the oracle's flow2depth on the device's own cartesian flow
            dref, conf_ref = orc.flow_to_depth_radial(cart, g["cx"], g["cy"], g["infty"])
            assert np.array_equal(confs, conf_ref), tag
            assert np.allclose(depth, dref, rtol=1e-6, atol=0), tag
            assert np.isfinite(depth).all() and np.isfinite(cart).all(), tag
    print("case %s: largest cartesian-flow deviation %.3g of its bound" % (name, worst))


@pytest.mark.parametrize("sub", [False, True])
def test_direct_entry_equals_the_wrapper(dfe, cuda, sub):
    """dfe_radial_flow_depth_pair[_subpixel]_f32 through RadialParams for case C (5 planes: the planar warp; alpha_polar 0.8)"""
    from depth_estimation_amd._lib import RadialParams
    from depth_estimation_amd.radial import _separable_weights

    Cc, hIn, wIn, hWin, layers, alpha, e2 = rc.CASES["C"]
    networkp, net, a, b = device_case(dfe, cuda, "C")
    wrapped = dfe.radialFlowDepth(networkp, net, a, b, e2, alpha_polar=alpha, one_call=True, want_volume=True, subpixel=sub)
    w1, b1, w2, b2, th = _separable_weights(net, networkp)
    prm = RadialParams(Cc, rc.HIMG, rc.WIMG, hIn, wIn, hWin, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), alpha, 0.65, 0)
    outs = {k: torch.full_like(wrapped[k], float("nan")) for k in KEYS}
    ctx = dfe.get_ctx(0)
    entry = dfe.lib().dfe_radial_flow_depth_pair_subpixel_f32 if sub else dfe.lib().dfe_radial_flow_depth_pair_f32
    ctx.check(entry(ctx.handle, C.byref(prm), a.data_ptr(), b.data_ptr(), float(e2[0]), float(e2[1]), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                    b2.data_ptr(), *(outs[k].data_ptr() for k in KEYS)))
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(outs[k], wrapped[k]), k


@pytest.mark.parametrize("name", ["C", "E"])
def test_polar_grids_with_an_exponent(dfe, cuda, name):
    """getC2PMask / getP2CMask at alpha 0.8 and 1.25 (the pow tables' stand-alone twins) against the oracle: the 2e-5 of
    test_polar_grids_and_warp (one float ulp at |v| < 256), scaled with the float spacing beyond 256; wrap columns equal their sources."""
    Cc, hIn, wIn, hWin, layers, alpha, e2 = rc.CASES[name]
    g = rc.geometry(name)
    m = dfe.getC2PMask(rc.WIMG, rc.HIMG, wIn, hIn, e2[0], e2[1], 8, 8, g["rmax"], alpha, device=cuda).cpu().numpy()
    ref = orc.polar_grid_c2p(rc.WIMG, rc.HIMG, wIn, hIn, e2[0], e2[1], 8, 8, g["rmax"], alpha)
    assert m.shape == ref.shape == (2, hIn, wIn + 16)
    err = np.abs(m.astype(np.float64) - ref)
    assert (err <= 2e-5 * np.maximum(1, np.abs(ref) / 256)).all(), "C2P: worst %.3e" % err.max()
    assert np.array_equal(m[:, :, :8], m[:, :, wIn:wIn + 8]) and np.array_equal(m[:, :, wIn + 8:], m[:, :, 8:16])
    p = dfe.getP2CMask(wIn, g["hm"], g["wOut"], g["hOut"], g["xc"], g["yc"], g["nrmax"], alpha, device=cuda).cpu().numpy()
    pref = rc.p2c_grid(name)
    err = np.abs(p.astype(np.float64) - pref)
    err[1][rc.seam_set(name)] = 0
    assert (err <= 2e-5 * np.maximum(1, np.abs(pref) / 256)).all(), "P2C: worst %.3e" % err.max()
    of = dfe.getP2CMaskOF(dict(rc.networkp(name), hKernel=17, wKernel=layers[0][2]), e2, alpha, device=cuda).cpu().numpy()
    assert np.array_equal(of, p)


def test_argument_edges(dfe, cuda):
    """a polar width below the wrap columns and a polar height without a matcher row are refused before anything is launched; a window
    without an instantiation takes the staged path"""
    from depth_estimation_amd._lib import RadialParams

    ctx, lib = dfe.get_ctx(0), dfe.lib()
    fr = torch.zeros((3, rc.HIMG, rc.WIMG), device=cuda)
    w1, w2 = torch.zeros((5, 3, 1, 17), device=cuda), torch.zeros((10, 5, 17, 1), device=cuda)
    for entry in (lib.dfe_radial_flow_depth_pair_f32, lib.dfe_radial_flow_depth_pair_subpixel_f32):
        call = lambda prm: entry(ctx.handle, C.byref(prm), fr.data_ptr(), fr.data_ptr(), 80.0, 44.0, w1.data_ptr(), None, w2.data_ptr(), None, None, None,
                                 None, None, None)
        assert call(RadialParams(3, rc.HIMG, rc.WIMG, 64, 7, 15, 5, 17, 10, 17, 0, 1.0, 0.65, 0)) == DFE_E_SHAPE    # wInput 7 < lpad 8
        assert call(RadialParams(3, rc.HIMG, rc.WIMG, 30, 64, 15, 5, 17, 10, 17, 0, 1.0, 0.65, 0)) == DFE_E_SHAPE   # hm = 0
    torch.cuda.synchronize()
    networkp, net, a, b = device_case(dfe, cuda, "F")
    with pytest.raises(ValueError):
        dfe.radialFlowDepth(dict(networkp, hInput=30), net, a, b, (80.0, 44.0))
    with pytest.raises(dfe.DfeError):
        dfe.radialFlowDepth(dict(networkp, hInput=64, wInput=7), net, a, b, (80.0, 44.0))
    networkp = dict(networkp, hInput=70, wInput=100, hWin=10)
    net = dfe.getTesterNetwork(networkp, device=cuda, generator=torch.Generator().manual_seed(0))
    one, stg = (dfe.radialFlowDepth(networkp, net, a, b, (80.0, 44.0), one_call=oc, want_volume=True) for oc in (True, False))
    assert tuple(one["output"].shape) == (70 - 16 - 9, 100, 10)
    for k in KEYS:
        assert torch.equal(one[k], stg[k]), k
