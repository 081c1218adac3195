"""GPU suite: the single-scale trained model with output_extraction_method = 'mean' (the reference's deployed setting,
depth_estimation_api.lua:25-31) -- getModel's SpatialMatching -> Minus -> SoftMax over the window, then processOutput's 'mean' branch
(opticalflow_model.lua:171-199, 218-226): y, x = the soft arg-max of the window (1-based cells) minus centered2onebased(0, 0),
confidence = extractOutput(row marginals, 0.11) then scores > 0, index = yx2x(floor(y + 0.5), floor(x + 0.5)).

One call (dfe_flow_pair_filtered_mean_f32; 16- / 17-wide windows: the matcher's soft-arg-max epilogue, no volume) == the module path bit
for bit; both against an oracle composed here from tests/oracle (spatial_matching, softmin, output_extractor, marginal_sum,
extract_output).  Tolerance against the oracle: a probability of the device and of the oracle differ by a relative (N + 4) 2^-24 at most
(each side's window sum is exact to N / 2 roundings, plus the exponential's last place and the division); over the window that moves
sum_k p_k c_k (c_k <= m = max(maxh, maxw)) by (N + 4) 2^-24 m, and each side's fp32 weighted sum of N terms is exact to N 2^-24 m: y and x
agree within MEAN_TOL = (3 N + 4) 2^-24 m.  A row marginal (<= 1) agrees within (N + 6) 2^-24.  Indices and confidences must be equal
except where y or x lies within MEAN_TOL of a .5 rounding boundary, or a marginal within its bound of 0.11."""
import math

import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import refpath as rp

pytestmark = pytest.mark.gpu

TM_LAYERS = [(3, 5, 5, 4), (4, 5, 5, 4), (4, 5, 5, 10)]          # the vga-learned stack (tests/time_matching.lua:13)
MEAN_KERNEL = "feat_matching_flat_mean_kernel"


def mean_tol(mh, mw):
    N = mh * mw
    return (3 * N + 4) * 2.0 ** -24 * max(mh, mw)


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _geo(layers, mh, mw, hImg, wImg, **kw):
    return dict(layers=[list(l) for l in layers], maxh=mh, maxw=mw, multiscale=False, output_extraction_method="mean", hImg=hImg, wImg=wImg, **kw)


def _pair(H, W, seed, gain):
    f0, f1, _, _ = rp.synth_pair(H, W, C=3, seed=seed, max_flow=5, noise_sigma=1.0)
    return f0 / np.float32(255) * np.float32(gain), f1 / np.float32(255) * np.float32(gain)


def _same(one, stg):
    for k in ("index", "y", "x", "full", "full_confidences"):
        assert one[k].dtype == stg[k].dtype, k
        assert torch.equal(one[k], stg[k]), k
    assert torch.equal(one["confidences"].to(torch.float32), stg["confidences"].to(torch.float32))


def mean_oracle(feat0, feat1, mh, mw):
    """prepareInput's narrow of patch 1, SpatialMatching -> Minus -> SoftMax, then getOutputConfidences2 and the index of processOutput's
    'mean' branch, all on the oracle (feat0 / feat1: the two feature maps, the un-narrowed patch 1)."""
    y0, x0 = math.ceil(mh / 2) - 1, math.ceil(mw / 2) - 1
    a = np.ascontiguousarray(feat0[:, y0 : y0 + feat0.shape[1] - mh + 1, x0 : x0 + feat0.shape[2] - mw + 1], np.float32)
    vol = orc.spatial_matching(a, np.ascontiguousarray(feat1, np.float32), mh, mw)
    H1, W1 = vol.shape[:2]
    N = mh * mw
    prob = orc.softmin(vol.reshape(-1, N)).reshape(H1, W1, N)
    x, y = orc.output_extractor(prob, mh, mw)
    marg = orc.marginal_sum(prob, mh, mw).reshape(H1, W1, mh)
    scores = np.zeros((H1, W1), np.float32)
    imaxs = np.zeros((H1, W1), np.int64)
    orc.extract_output(marg, 0.11, imaxs, scores)
    index = ((np.floor(y + np.float32(0.5)) - np.float32(1)) * np.float32(mw) + np.floor(x + np.float32(0.5))).astype(np.int64)
    return dict(prob=prob, x=x, y=y, marg=marg, confidences=(scores > 0).astype(np.float32), index=index)


def _check_oracle(one, ref, mh, mw):
    tol = mean_tol(mh, mw)
    yo, xo = math.ceil(mh / 2), math.ceil(mw / 2)
    gy, gx = one["y"].cpu().numpy() + yo, one["x"].cpu().numpy() + xo         # back to 1-based cells (exact: small integers)
    assert np.abs(gy - ref["y"]).max() <= tol and np.abs(gx - ref["x"]).max() <= tol
    half = lambda v: np.abs(v - np.floor(v) - 0.5) <= tol
    near = half(ref["y"]) | half(ref["x"])
    gi = one["index"].cpu().numpy()
    assert ((gi == ref["index"]) | near).all(), "%d indices differ away from a rounding boundary" % int(((gi != ref["index"]) & ~near).sum())
    medge = (np.abs(ref["marg"].astype(np.float64) - 0.11) <= (mh * mw + 6) * 2.0 ** -24).any(axis=2)
    gc = one["confidences"].cpu().numpy()
    assert ((gc == ref["confidences"]) | medge).all()


@pytest.mark.parametrize("H,W,layers,mh,mw,gain,wgain", [
    (64, 300, TM_LAYERS, 16, 16, 1.0, 100.0),         # the vga-learned stack and window, high-contrast weights
    (64, 300, TM_LAYERS, 16, 16, 1.0, 1.0),           # ... freshly initialised: windows close to uniform
    (50, 330, [(3, 9, 9, 8)], 17, 17, 30.0, 1.0),     # 17 x 17: the extra-row task, one lane with two marginal rows
    (44, 301, [(3, 5, 5, 6)], 12, 17, 30.0, 1.0),     # 12 rows of a 17-wide window, W1 % 4 = 1
    (40, 290, [(3, 3, 3, 5)], 6, 16, 30.0, 1.0),      # fewer window rows than a DPP row has lanes
    (48, 64, [(3, 5, 5, 4), (4, 3, 3, 6)], 9, 9, 1.0, 30.0),   # a window the kernel does not take: the stand-alone ops
])
def test_mean_one_call_equals_modules_and_oracle(dfe, cuda, H, W, layers, mh, mw, gain, wgain):
    gen = torch.Generator().manual_seed(H + mh)
    geo = _geo(layers, mh, mw, H, W)
    model = dfe.getModel(geo, True, False, device=cuda, generator=gen)
    [m for m in model.modules[0].modules[0].modules if getattr(m, "weight", None) is not None][-1].weight.mul_(wgain)
    f0, f1 = _pair(H, W, H + W, gain)
    t0, t1 = T(f0, cuda), T(f1, cuda)
    ctx = dfe.get_ctx(0)
    one = model.forwardFlow([t0, t1], None, one_call=True)
    hk, wk = 1 + sum(l[2] - 1 for l in layers), 1 + sum(l[1] - 1 for l in layers)
    W1 = W - wk + 1 - mw + 1
    fused = mw in (16, 17) and W1 >= 253
    assert (ctx.last_kernel() == MEAN_KERNEL) == fused, ctx.last_kernel()
    stg = model.forwardFlow([t0, t1], None, one_call=False)
    _same(one, stg)
    assert one["y"].dtype == torch.float32 and (one["y"] != torch.round(one["y"])).any(), "sub-pixel flow is expected"
    feat0, feat1 = model.modules[0].modules[0].output.cpu().numpy(), model.modules[0].modules[1].output.cpu().numpy()
    ref = mean_oracle(feat0, feat1, mh, mw)
    assert np.abs(model.modules[3].output.cpu().numpy() - ref["prob"]).max() <= (mh * mw + 4) * 2.0 ** -24
    _check_oracle(one, ref, mh, mw)
    # the centre paste: zero outside the output region
    H1 = one["index"].shape[0]
    ho, wo = (H - H1) // 2, (W - W1) // 2
    full = one["full"].clone()
    full[:, ho : ho + H1, wo : wo + W1] = 0
    assert not full.any()


@pytest.mark.parametrize("mh,mw,layers", [(16, 16, TM_LAYERS), (17, 17, [(3, 7, 7, 8)])])
def test_mean_prefiltered_pair(dfe, cuda, mh, mw, layers):
    """geometry.prefilter: the caller's feature maps, patch 1's narrow read as a view -- one call == the module path, bit for bit."""
    gen = torch.Generator().manual_seed(mh)
    H, W = 70, 310
    geo = _geo(layers, mh, mw, H, W, prefilter=True)
    filt = dfe.getFilter(geo, device=cuda, generator=gen)
    [m for m in filt.modules if getattr(m, "weight", None) is not None][-1].weight.mul_(30.0)
    f0, f1 = _pair(H, W, 11, 1.0)
    a, b = filt.forward(T(f0, cuda)).clone(), filt.forward(T(f1, cuda)).clone()
    model = dfe.getModel(geo, True, True)
    ctx = dfe.get_ctx(0)
    one = model.forwardFlow([a, b], None, one_call=True)
    assert ctx.last_kernel() == MEAN_KERNEL
    stg = model.forwardFlow([a, b], None, one_call=False)
    _same(one, stg)
    _check_oracle(one, mean_oracle(a.cpu().numpy(), b.cpu().numpy(), mh, mw), mh, mw)


def test_mean_vga_learned_workload(dfe, cuda):
    """The bench's vga-learned shape (640 x 480 frames, the stack above, 16 x 16: 453 x 613 outputs) with 'mean': one call == modules."""
    H, W, mh, mw = 480, 640, 16, 16
    gen = torch.Generator().manual_seed(1)
    geo = _geo(TM_LAYERS, mh, mw, H, W)
    model = dfe.getModel(geo, True, False, device=cuda, generator=gen)
    [m for m in model.modules[0].modules[0].modules if getattr(m, "weight", None) is not None][-1].weight.mul_(30.0)
    f0, f1, _, _ = rp.synth_pair(H, W, C=3, seed=2, max_flow=6, noise_sigma=0)
    t0, t1 = T(f0 / np.float32(255), cuda), T(f1 / np.float32(255), cuda)
    ctx = dfe.get_ctx(0)
    one = model.forwardFlow([t0, t1], None, one_call=True)
    assert ctx.last_kernel() == MEAN_KERNEL
    assert tuple(one["index"].shape) == (453, 613)
    stg = model.forwardFlow([t0, t1], None, one_call=False)
    _same(one, stg)


def _planted(mh, mw):
    """Feature maps (prefilter) with two planted regions: rows 4..8 of patch 1 copy in2 at displacement (3, 4) over features of amplitude
    30 -- one cost 0, every other cost in the thousands: exp underflows to 0 and the window is one-hot; rows 14..18, columns 60..119 sit
    in a constant block of both maps -- every cost 0, every p = 1 / N."""
    rng = np.random.default_rng(23)
    K, H1, W1 = 6, 30, 300
    H2, W2 = H1 + mh - 1, W1 + mw - 1
    b = (rng.standard_normal((K, H2, W2)) * 30).astype(np.float32)
    a_full = (rng.standard_normal((K, H2, W2)) * 30).astype(np.float32)
    ny, nx = (mh + 1) // 2 - 1, (mw + 1) // 2 - 1
    a = a_full[:, ny : ny + H1, nx : nx + W1]
    a[:, 4:9] = b[:, 4 + 3 : 9 + 3, 4 : 4 + W1]
    b[:, 14 : 19 + mh, 60 : 120 + mw] = 0.5
    a[:, 14:19, 60:120] = 0.5
    return a_full, b, H1, W1


def test_mean_planted_windows_and_every_output_written(dfe, cuda):
    """A flat 16 x 16 window: every p = 2^-8, cell coordinates are integers, so both sums are exact -- y = x = 8.5 (0.5 after centring),
    index = 8 * 16 + 9, and no confidence (each row marginal is 1 / 16 < 0.11).  A one-hot window: the exact cell, confident.  Outputs
    pre-filled with NaN (index with -7) on a full frame larger than the output on every side: every element gets written, the border 0 --
    for the fused kernel and for the stand-alone ops (9 x 9)."""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    for mh, mw in ((16, 16), (9, 9)):
        a_full, b, H1, W1 = _planted(mh, mw)
        K, H2, W2 = b.shape
        hImg, wImg = H2 + 7, W2 + 4
        ta, tb = T(a_full, cuda), T(b, cuda)
        full = torch.full((2, hImg, wImg), float("nan"), device=cuda)
        fc = torch.full((hImg, wImg), float("nan"), device=cuda)
        idx = torch.full((H1, W1), -7, dtype=torch.int64, device=cuda)
        ctx.check(lib.dfe_flow_pair_filtered_mean_f32(ctx.handle, ta.data_ptr(), tb.data_ptr(), K, H2, W2, None, 0, mh, mw, hImg, wImg, full.data_ptr(),
                                                      fc.data_ptr(), idx.data_ptr()))
        torch.cuda.synchronize()
        assert (ctx.last_kernel() == MEAN_KERNEL) == (mw == 16)
        assert not torch.isnan(full).any() and not torch.isnan(fc).any() and (idx >= 1).all()
        ho, wo = (hImg - H1) // 2, (wImg - W1) // 2
        assert ho >= 1 and wo >= 1 and hImg - ho - H1 >= 1 and wImg - wo - W1 >= 1
        y, x, c = full[0, ho : ho + H1, wo : wo + W1], full[1, ho : ho + H1, wo : wo + W1], fc[ho : ho + H1, wo : wo + W1]
        border = full.clone()
        border[:, ho : ho + H1, wo : wo + W1] = 0
        assert not border.any() and fc.sum().item() == c.sum().item()
        yo, xo = (mh + 1) // 2, (mw + 1) // 2
        # one-hot: displacement (3, 4) -> cell (4, 5), 1-based
        assert (y[4:9] == 4 - yo).all() and (x[4:9] == 5 - xo).all() and (c[4:9] == 1).all() and (idx[4:9] == 3 * mw + 5).all()
        # flat
        if mh == 16:
            assert (y[14:19, 60:120] == 0.5).all() and (x[14:19, 60:120] == 0.5).all()
            assert (idx[14:19, 60:120] == 8 * 16 + 9).all() and (c[14:19, 60:120] == 0).all()
        else:
            # 81 cells of 1 / 81: not exact, but the mean cell is (5, 5) within the tolerance, and each row marginal 1 / 9 > 0.11
            assert (torch.abs(y[14:19, 60:120]) <= mean_tol(9, 9)).all() and (torch.abs(x[14:19, 60:120]) <= mean_tol(9, 9)).all()
            assert (idx[14:19, 60:120] == 4 * 9 + 5).all() and (c[14:19, 60:120] == 1).all()
        # the module path on the same maps
        geo = _geo([[K, 1, 1, K]], mh, mw, hImg, wImg, prefilter=True)
        stg = dfe.getModel(geo, True, True).forwardFlow([ta, tb], None, one_call=False)
        assert torch.equal(stg["full"], full) and torch.equal(stg["full_confidences"], fc) and torch.equal(stg["index"], idx)


def test_mean_model_forward_flow_no_longer_crashes(dfe, cuda):
    """getModel with 'mean' appends an OutputExtractor; forwardFlow used to hand its {x, y} list to processOutput.  Now both ways work
    and agree; a model whose last module was replaced (same count, other type) runs its modules, also with one_call=True."""
    gen = torch.Generator().manual_seed(9)
    H, W = 60, 290
    geo = _geo(TM_LAYERS, 16, 16, H, W)
    model = dfe.getModel(geo, True, False, device=cuda, generator=gen)
    assert isinstance(model.modules[-1], dfe.glue.OutputExtractor)
    f0, f1 = _pair(H, W, 4, 10.0)
    t0, t1 = T(f0, cuda), T(f1, cuda)
    one = model.forwardFlow([t0, t1], 0.5, one_call=True)             # (the threshold is not used by 'mean')
    stg = model.forwardFlow([t0, t1], None, one_call=False)
    _same(one, stg)
    model.modules[-1] = dfe.glue.Log2(1e-10)
    patched = model.forwardFlow([t0, t1], None, one_call=True)
    ref = model.forwardFlow([t0, t1], None, one_call=False)
    _same(patched, ref)
    assert not torch.equal(patched["full"], one["full"])
