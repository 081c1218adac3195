"""The dense-field operators: what a flow or depth field goes through behind the matcher (not in the reference: include/dfe.h, DESIGN
sections 4.25 - 4.28).  Each takes float32 CUDA planes, values [C][H][W] with a confidence plane [H][W] and, where it has one, a guide
image [Cg][H][W], over a region of the frame.

    flowConsistency(fw, bw, tol, region=None)
        dfe_flow_consistency_f32: the forward-backward mask and residual of any two flow fields
    fillHoles(values, weight, region=None, levels=0)
        dfe_fill_holes_f32: a dense field from the confident pixels of a sparse one (confidence-weighted push-pull)
    weightedMedian(values, weight=None, guide=None, k=7, sigma=0.0, region=None)
        dfe_weighted_median_f32: per channel the lower weighted median of the k x k window, weights from a confidence plane and a guide image
    guidedUpsample(values, size=None, weight=None, guide=None, guide_lo=None, r=2, sigma=0.0, gain=None)
        dfe_guided_upsample_f32: a field at a higher resolution, the mean of the low-resolution samples around each pixel weighted by a tent,
        a confidence plane and the agreement of the frame at both resolutions (joint bilateral upsampling)
    forwardWarp(values, weight, flow, key=None, region=None, gain=None, bias=None, decay=1.0)
        dfe_forward_warp_f32: a field scattered along its own flow to the next frame's grid, a z-buffer on `key` deciding collisions
    temporalFuse(prior, wprior, meas, wmeas, tol, wmax=8.0, region=None)
        dfe_temporal_fuse_f32: a propagated prior and a new measurement fused pointwise, weights counting observations
    temporalStep(state, wstate, flow, meas, wmeas, tol, wmax=8.0, key=None, region=None, gain=None, bias=None, decay=1.0, want_prior=False,
                 splat="nearest", ztol=0.0, quant=1024.0, min_cover=0.0)
        dfe_temporal_step_f32: the two in one call (the filter above them: temporal.py); splat="bilinear":
        dfe_temporal_step_splat_f32, forwardSplat in place of forwardWarp
    forwardSplat(values, weight, flow, key=None, region=None, gain=None, bias=None, decay=1.0, ztol=0.0, quant=1024.0, min_cover=0.0)
        dfe_forward_splat_f32: the sub-pixel forward warp, every source spread over the four pixels around where it lands, summed in
        integers
"""
import ctypes

import torch

from ._lib import lib
from .context import get_ctx, ptr


def _check_planes(name, values, weight=None, guide=None, dims="H x W", joint=False):
    """ValueError unless values is C x H x W with C = 1 .. 4, weight (if given) H x W and guide (if given) Cg x H x W with Cg = 1 .. 4.
    dims: how the message names the two sizes; joint: one message for values and weight (fillHoles, whose weight is not optional)"""
    hw = tuple(values.shape[1:])
    bad_values = values.dim() != 3 or not 1 <= values.shape[0] <= 4
    bad_weight = weight is not None and (weight.dim() != 2 or tuple(weight.shape) != hw)
    if joint and (bad_values or bad_weight):
        raise ValueError("%s: values C x %s (C = 1 .. 4) and weight %s expected, got %s and %s" % (name, dims, dims, tuple(values.shape), tuple(weight.shape)))
    if bad_values:
        raise ValueError("%s: values C x %s (C = 1 .. 4) expected, got %s" % (name, dims, tuple(values.shape)))
    if bad_weight:
        raise ValueError("%s: weight %s expected, got %s for values %s" % (name, dims, tuple(weight.shape), tuple(values.shape)))
    if guide is not None and (guide.dim() != 3 or not 1 <= guide.shape[0] <= 4 or tuple(guide.shape[1:]) != hw):
        raise ValueError("%s: guide Cg x %s (Cg = 1 .. 4) expected, got %s for values %s" % (name, dims, tuple(guide.shape), tuple(values.shape)))


def _on_device(name, tensors, dtype=torch.float32, expected="float32 CUDA tensors expected", apart="tensors on different devices"):
    """The tensors that are given (None stays None), contiguous: TypeError unless all are CUDA tensors of `dtype` (None: any), ValueError
    unless they lie on one device.  expected / apart: the two messages behind the caller's name"""
    given = [t for t in tensors if t is not None]
    if not all(t.is_cuda and (dtype is None or t.dtype == dtype) for t in given):
        raise TypeError("%s: %s" % (name, expected))
    if any(t.device != given[0].device for t in given):
        raise ValueError("%s: %s" % (name, apart))
    return [None if t is None else t.contiguous() for t in tensors]


def _region_or_frame(region, H, W):
    """(y0, x0, Ho, Wo): the whole frame by default"""
    return (0, 0, H, W) if region is None else tuple(int(v) for v in region)


def flowConsistency(fw, bw, tol, region=None):
    """Forward-backward check of two float32 flow fields [2][H][W] (plane 0 = y, plane 1 = x; fw from frame 0 to frame 1, bw back) over
    region = (y0, x0, Ho, Wo), the whole frame by default (include/dfe.h: dfe_flow_consistency_f32).  Returns (mask, err), float32 [H][W]:
    mask 1 where |fw(p) + bw(p + fw(p))| <= tol, err that residual (+Inf where p + fw(p) leaves the region or a flow is not finite); both 0
    outside the region."""
    shapes = "two 2 x H x W flows of one shape expected, got %s and %s" % (tuple(fw.shape), tuple(bw.shape))
    fw, bw = _on_device("flowConsistency", (fw, bw), expected="two float32 CUDA tensors expected", apart=shapes)
    if fw.dim() != 3 or fw.shape[0] != 2 or fw.shape != bw.shape:
        raise ValueError("flowConsistency: " + shapes)
    _, H, W = fw.shape
    y0, x0, Ho, Wo = _region_or_frame(region, H, W)
    mask = torch.empty((H, W), dtype=torch.float32, device=fw.device)
    err = torch.empty_like(mask)
    ctx = get_ctx(fw)
    ctx.check(lib().dfe_flow_consistency_f32(ctx.handle, ptr(fw), ptr(bw), H, W, y0, x0, Ho, Wo, float(tol), ptr(mask), ptr(err)))
    return mask, err


def fillHoles(values, weight, region=None, levels=0):
    """Dense field from the confident pixels of a sparse one (include/dfe.h: dfe_fill_holes_f32): values float32 [C][H][W], 1 <= C <= 4,
    weight float32 [H][W] (>= 1 fully trusted, below 1e-6 or not finite a hole), region = (y0, x0, Ho, Wo), the whole frame by default;
    levels = 0 fills from any distance, n > 0 from at most n pyramid levels (holes farther than about 2^n pixels from every valid pixel
    stay unfilled).  Returns (out [C][H][W], filled [H][W]): pixels of weight >= 1 keep their bits, the others are blended with / replaced
    by the confidence-weighted push-pull interpolation; filled is 1 where a value was found; both 0 outside the region."""
    _check_planes("fillHoles", values, weight, joint=True)
    values, weight = _on_device("fillHoles", (values, weight), expected="two float32 CUDA tensors expected",
                                apart="values on %s, weight on %s" % (values.device, weight.device))
    C, H, W = values.shape
    y0, x0, Ho, Wo = _region_or_frame(region, H, W)
    out = torch.empty_like(values)
    filled = torch.empty((H, W), dtype=torch.float32, device=values.device)
    ctx = get_ctx(values)
    ctx.check(lib().dfe_fill_holes_f32(ctx.handle, ptr(values), C, H, W, ptr(weight), y0, x0, Ho, Wo, int(levels), ptr(out), ptr(filled)))
    return out, filled


def weightedMedian(values, weight=None, guide=None, k=7, sigma=0.0, region=None):
    """Guided weighted median (include/dfe.h: dfe_weighted_median_f32): values float32 [C][H][W], 1 <= C <= 4; weight float32 [H][W] or None
    (all ones; below 1e-6 or not finite: the sample does not exist; above 1 counts as 1); guide float32 [Cg][H][W], Cg <= 4, or None;
    k odd in 1 .. 15; sigma > 0 with a guide: a sample weighs max(0, 1 - |guide(p) - guide(q)|^2 / sigma^2) times its weight, else the
    weight alone; region = (y0, x0, Ho, Wo), the whole frame by default.  Returns (out [C][H][W], filtered [H][W]): per channel the lower
    weighted median of the k x k window clipped to the region (the bits of an input sample), filtered 1 where the window held a sample
    of positive weight, else both 0; both 0 outside the region."""
    _check_planes("weightedMedian", values, weight, guide)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= 15 or k % 2 == 0:
        raise ValueError("weightedMedian: k=%r must be odd, 1 .. 15" % (k,))
    values, weight, guide = _on_device("weightedMedian", (values, weight, guide))
    C, H, W = values.shape
    y0, x0, Ho, Wo = _region_or_frame(region, H, W)
    out = torch.empty_like(values)
    filtered = torch.empty((H, W), dtype=torch.float32, device=values.device)
    ctx = get_ctx(values)
    ctx.check(lib().dfe_weighted_median_f32(ctx.handle, ptr(values), C, H, W, None if weight is None else ptr(weight), None if guide is None else ptr(guide),
                                            0 if guide is None else guide.shape[0], float(sigma), k, y0, x0, Ho, Wo, ptr(out), ptr(filtered)))
    return out, filtered


def guidedUpsample(values, size=None, weight=None, guide=None, guide_lo=None, r=2, sigma=0.0, gain=None):
    """Guided upsampling (include/dfe.h: dfe_guided_upsample_f32): values float32 [C][Hl][Wl], 1 <= C <= 4, to size = (Hh, Wh) >= (Hl, Wl),
    by default the guide's; weight float32 [Hl][Wl] or None (all ones; below 1e-6 or not finite: the sample does not exist; above 1 counts
    as 1); guide float32 [Cg][Hh][Wh] or [Hh][Wh] (one channel), Cg <= 4, or None; guide_lo the same frame at [Cg][Hl][Wl], by default
    imageScale(guide, Wl, Hl); r in 1 .. 4: 2r x 2r low-resolution samples around each pixel under a tent of radius r; sigma > 0 with a
    guide: a sample also weighs max(0, 1 - |guide(p) - guide_lo(q)|^2 / sigma^2); gain None, C numbers, or "flow" for C = 2 planes (y, x):
    (Hh / Hl, Wh / Wl), so that vectors stay in pixels of the grid they are on.  Returns (out [C][Hh][Wh], valid [Hh][Wh]): the weighted
    mean times gain and 1 where a sample was found, else both 0."""
    _check_planes("guidedUpsample", values, weight, dims="Hl x Wl")
    C, Hl, Wl = values.shape
    if guide is None and guide_lo is not None:
        raise ValueError("guidedUpsample: guide_lo without a guide")
    if guide is not None:
        if guide.dim() == 2:
            guide = guide.unsqueeze(0)
        if guide.dim() != 3 or not 1 <= guide.shape[0] <= 4:
            raise ValueError("guidedUpsample: guide Cg x Hh x Wh (Cg = 1 .. 4) or Hh x Wh expected, got %s" % (tuple(guide.shape),))
        if size is None:
            size = tuple(guide.shape[1:])
    if size is None:
        raise ValueError("guidedUpsample: without a guide the size = (Hh, Wh) must be given")
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(n, int) and not isinstance(n, bool) for n in size)):
        raise ValueError("guidedUpsample: size=%r: (Hh, Wh) expected" % (size,))
    Hh, Wh = size
    if not (Hl <= Hh <= 32768 and Wl <= Wh <= 32768 and Hl >= 1 and Wl >= 1):
        raise ValueError("guidedUpsample: size %d x %d for values %d x %d: every size 1 .. 32768, and none may shrink" % (Hh, Wh, Hl, Wl))
    if guide is not None and tuple(guide.shape[1:]) != (Hh, Wh):
        raise ValueError("guidedUpsample: guide %s for the size %d x %d" % (tuple(guide.shape), Hh, Wh))
    if guide_lo is not None:
        if guide_lo.dim() == 2:
            guide_lo = guide_lo.unsqueeze(0)
        if tuple(guide_lo.shape) != (guide.shape[0], Hl, Wl):
            raise ValueError("guidedUpsample: guide_lo %d x %d x %d expected, got %s" % (guide.shape[0], Hl, Wl, tuple(guide_lo.shape)))
    if not isinstance(r, int) or isinstance(r, bool) or not 1 <= r <= 4:
        raise ValueError("guidedUpsample: r=%r must be 1 .. 4" % (r,))
    if isinstance(gain, str):
        if gain != "flow" or C != 2:
            raise ValueError("guidedUpsample: gain=%r: \"flow\" is for C = 2 planes (y, x)" % (gain,))
        gain = (Hh / Hl, Wh / Wl)
    if gain is not None:
        try:
            gain = [float(g) for g in gain]
        except TypeError:
            raise ValueError("guidedUpsample: gain=%r: None, %d numbers or \"flow\" expected" % (gain, C)) from None
        if len(gain) != C or not all(g == g and abs(g) != float("inf") for g in gain):
            raise ValueError("guidedUpsample: gain=%r: %d finite numbers expected" % (gain, C))
    values, weight, guide, guide_lo = _on_device("guidedUpsample", (values, weight, guide, guide_lo))
    if guide is not None and guide_lo is None:
        from .stream import imageScale

        guide_lo = imageScale(guide, Wl, Hl).contiguous()
    out = torch.empty((C, Hh, Wh), dtype=torch.float32, device=values.device)
    valid = torch.empty((Hh, Wh), dtype=torch.float32, device=values.device)
    ctx = get_ctx(values)
    ctx.check(lib().dfe_guided_upsample_f32(ctx.handle, ptr(values), C, Hl, Wl, None if weight is None else ptr(weight), None if guide is None else ptr(guide),
                                            None if guide_lo is None else ptr(guide_lo), 0 if guide is None else guide.shape[0], float(sigma), r,
                                            None if gain is None else (ctypes.c_float * C)(*gain), Hh, Wh, ptr(out), ptr(valid)))
    return out, valid


def _check_flow_key(name, values, flow, key):
    """ValueError unless flow is 2 x H x W and key (if given) H x W for values C x H x W"""
    hw = tuple(values.shape[1:])
    if flow.dim() != 3 or flow.shape[0] != 2 or tuple(flow.shape[1:]) != hw:
        raise ValueError("%s: flow 2 x H x W expected, got %s for values %s" % (name, tuple(flow.shape), tuple(values.shape)))
    if key is not None and (key.dim() != 2 or tuple(key.shape) != hw):
        raise ValueError("%s: key H x W expected, got %s for values %s" % (name, tuple(key.shape), tuple(values.shape)))


def _host_floats(name, what, v, C):
    """None, or a ctypes array of the C finite numbers v (ValueError otherwise)"""
    if v is None:
        return None
    try:
        v = [float(g) for g in v]
    except TypeError:
        raise ValueError("%s: %s=%r: None or %d numbers expected" % (name, what, v, C)) from None
    if len(v) != C or not all(g == g and abs(g) != float("inf") for g in v):
        raise ValueError("%s: %s=%r: %d finite numbers expected" % (name, what, v, C))
    return (ctypes.c_float * C)(*v)


def _check_decay(name, decay):
    decay = float(decay)
    if not 0.0 < decay <= 1.0:
        raise ValueError("%s: decay=%r must lie in (0, 1]" % (name, decay))
    return decay


def _check_tol_wmax(name, tol, wmax):
    tol, wmax = float(tol), float(wmax)
    if not tol >= 0.0:
        raise ValueError("%s: tol=%r must be >= 0" % (name, tol))
    if not 1e-6 <= wmax < float("inf"):
        raise ValueError("%s: wmax=%r must be finite and >= 1e-6" % (name, wmax))
    return tol, wmax


def _optr(t):
    return None if t is None else ptr(t)


def forwardWarp(values, weight, flow, key=None, region=None, gain=None, bias=None, decay=1.0):
    """Forward warp with a z-buffer (include/dfe.h: dfe_forward_warp_f32): values float32 [C][H][W], 1 <= C <= 4, and weight float32 [H][W]
    (finite and >= 1e-6: the sample exists; NOT clipped at 1: it counts observations) scattered along flow float32 [2][H][W] (plane 0 = y,
    plane 1 = x, from this grid to the next frame's) over region = (y0, x0, Ho, Wo), the whole frame by default.  Each source lands on the
    nearest pixel (.5 rounds up); of the sources of one target the one with the smallest key [H][W] wins (pass depth: the nearer surface
    covers the farther), for equal keys or key None the smallest index y W + x.  gain, bias: None or C numbers (out = gain v + bias);
    decay in (0, 1] multiplies the weight.  Returns (out [C][H][W], wout [H][W], src int32 [H][W]): src the winner's index, -1 and zeros
    where nothing landed and outside the region."""
    _check_planes("forwardWarp", values, weight, joint=True)
    _check_flow_key("forwardWarp", values, flow, key)
    C, H, W = values.shape
    gain, bias, decay = _host_floats("forwardWarp", "gain", gain, C), _host_floats("forwardWarp", "bias", bias, C), _check_decay("forwardWarp", decay)
    values, weight, flow, key = _on_device("forwardWarp", (values, weight, flow, key))
    y0, x0, Ho, Wo = _region_or_frame(region, H, W)
    out = torch.empty_like(values)
    wout = torch.empty((H, W), dtype=torch.float32, device=values.device)
    src = torch.empty((H, W), dtype=torch.int32, device=values.device)
    ctx = get_ctx(values)
    ctx.check(lib().dfe_forward_warp_f32(ctx.handle, ptr(values), C, H, W, ptr(weight), ptr(flow), _optr(key), y0, x0, Ho, Wo, gain, bias, decay,
                                         ptr(out), ptr(wout), ptr(src)))
    return out, wout, src


def temporalFuse(prior, wprior, meas, wmeas, tol, wmax=8.0, region=None):
    """A propagated prior and a new measurement fused pointwise (include/dfe.h: dfe_temporal_fuse_f32): prior, meas float32 [C][H][W],
    1 <= C <= 4, wprior, wmeas float32 [H][W] counting observations (capped at wmax; below 1e-6, not finite or over a value that is not
    finite: a hole); region = (y0, x0, Ho, Wo), the whole frame by default.  Returns (out, wout, flag): where only one side exists its bits
    and weight (flag 1: prior, 2: measurement); where |prior - meas| <= tol the mean weighted by the two weights, the weights summed (3);
    else the heavier side's bits with the lighter side's weight taken off (4: the prior survives, 5: the measurement takes over; on a tie
    the measurement with its weight); flag 0 and zeros where neither exists and outside the region."""
    _check_planes("temporalFuse", prior, wprior, joint=True)
    if tuple(meas.shape) != tuple(prior.shape) or tuple(wmeas.shape) != tuple(wprior.shape):
        raise ValueError("temporalFuse: meas %s and wmeas %s expected, got %s and %s" % (tuple(prior.shape), tuple(wprior.shape), tuple(meas.shape), tuple(wmeas.shape)))
    tol, wmax = _check_tol_wmax("temporalFuse", tol, wmax)
    prior, wprior, meas, wmeas = _on_device("temporalFuse", (prior, wprior, meas, wmeas))
    C, H, W = prior.shape
    y0, x0, Ho, Wo = _region_or_frame(region, H, W)
    out = torch.empty_like(prior)
    wout = torch.empty((H, W), dtype=torch.float32, device=prior.device)
    flag = torch.empty_like(wout)
    ctx = get_ctx(prior)
    ctx.check(lib().dfe_temporal_fuse_f32(ctx.handle, ptr(prior), ptr(wprior), ptr(meas), ptr(wmeas), C, H, W, y0, x0, Ho, Wo, tol, wmax, ptr(out), ptr(wout),
                                          ptr(flag)))
    return out, wout, flag


def _check_splat(name, ztol, quant, min_cover):
    ztol, quant, min_cover = float(ztol), float(quant), float(min_cover)
    if not 0.0 <= ztol < float("inf"):
        raise ValueError("%s: ztol=%r must be finite and >= 0" % (name, ztol))
    if not 0.0 < quant < float("inf"):
        raise ValueError("%s: quant=%r must be finite and > 0" % (name, quant))
    if not 0.0 <= min_cover <= 1.0:
        raise ValueError("%s: min_cover=%r must lie in [0, 1]" % (name, min_cover))
    return ztol, quant, min_cover


def forwardSplat(values, weight, flow, key=None, region=None, gain=None, bias=None, decay=1.0, ztol=0.0, quant=1024.0, min_cover=0.0):
    """Sub-pixel forward warp (include/dfe.h: dfe_forward_splat_f32): forwardWarp's arguments, but every source is spread over the four
    pixels around where it lands with tent weights on a 1 / 128 grid, and a target is the mean of what reached it, weighted by tent weight
    times source weight.  The sums are 64-bit integers (values on the 1 / quant grid, weights on the 1 / 256 grid, capped at 256), so the
    result does not depend on the order of arrival: the same bits in every run.  Of the sources that reach a target only those whose key
    lies within ztol of the smallest one contribute (pass depth: what the nearer surface covers does not leak through); key None: all.  A
    target needs tent weights of at least min_cover in all (1 = one whole source).  Returns (out [C][H][W], wout [H][W], cover [H][W]):
    wout the mean observation count, scaled down where cover < 1; cover the tent weights that arrived; zeros where nothing did and
    outside the region.  Defined while at most 256 taps contribute to one target."""
    _check_planes("forwardSplat", values, weight, joint=True)
    _check_flow_key("forwardSplat", values, flow, key)
    C, H, W = values.shape
    gain, bias, decay = _host_floats("forwardSplat", "gain", gain, C), _host_floats("forwardSplat", "bias", bias, C), _check_decay("forwardSplat", decay)
    ztol, quant, min_cover = _check_splat("forwardSplat", ztol, quant, min_cover)
    values, weight, flow, key = _on_device("forwardSplat", (values, weight, flow, key))
    y0, x0, Ho, Wo = _region_or_frame(region, H, W)
    out = torch.empty_like(values)
    wout = torch.empty((H, W), dtype=torch.float32, device=values.device)
    cover = torch.empty_like(wout)
    ctx = get_ctx(values)
    ctx.check(lib().dfe_forward_splat_f32(ctx.handle, ptr(values), C, H, W, ptr(weight), ptr(flow), _optr(key), y0, x0, Ho, Wo, gain, bias, decay, ztol, quant,
                                          min_cover, ptr(out), ptr(wout), ptr(cover)))
    return out, wout, cover


def temporalStep(state, wstate, flow, meas, wmeas, tol, wmax=8.0, key=None, region=None, gain=None, bias=None, decay=1.0, want_prior=False, splat="nearest",
                 ztol=0.0, quant=1024.0, min_cover=0.0):
    """forwardWarp of (state, wstate) along flow, then temporalFuse of that prior with (meas, wmeas), in one call whose prior stays in
    registers (include/dfe.h: dfe_temporal_step_f32); the same bits as the two calls.  Returns a dict: out, wout, flag, and with want_prior
    also prior, wprior, src.  splat="bilinear": forwardSplat with ztol, quant and min_cover in place of forwardWarp
    (dfe_temporal_step_splat_f32); want_prior then adds prior, wprior, cover and no src."""
    _check_planes("temporalStep", state, wstate, joint=True)
    _check_flow_key("temporalStep", state, flow, key)
    if tuple(meas.shape) != tuple(state.shape) or tuple(wmeas.shape) != tuple(wstate.shape):
        raise ValueError("temporalStep: meas %s and wmeas %s expected, got %s and %s" % (tuple(state.shape), tuple(wstate.shape), tuple(meas.shape), tuple(wmeas.shape)))
    if splat not in ("nearest", "bilinear"):
        raise ValueError("temporalStep: splat=%r: \"nearest\" or \"bilinear\"" % (splat,))
    C, H, W = state.shape
    gain, bias, decay = _host_floats("temporalStep", "gain", gain, C), _host_floats("temporalStep", "bias", bias, C), _check_decay("temporalStep", decay)
    tol, wmax = _check_tol_wmax("temporalStep", tol, wmax)
    if splat == "bilinear":
        ztol, quant, min_cover = _check_splat("temporalStep", ztol, quant, min_cover)
    state, wstate, flow, key, meas, wmeas = _on_device("temporalStep", (state, wstate, flow, key, meas, wmeas))
    y0, x0, Ho, Wo = _region_or_frame(region, H, W)
    r = dict(out=torch.empty_like(state), wout=torch.empty((H, W), dtype=torch.float32, device=state.device))
    r["flag"] = torch.empty_like(r["wout"])
    if want_prior:
        r["prior"], r["wprior"] = torch.empty_like(state), torch.empty_like(r["wout"])
        if splat == "bilinear":
            r["cover"] = torch.empty_like(r["wout"])
        else:
            r["src"] = torch.empty((H, W), dtype=torch.int32, device=state.device)
    ctx = get_ctx(state)
    if splat == "bilinear":
        ctx.check(lib().dfe_temporal_step_splat_f32(ctx.handle, ptr(state), C, H, W, ptr(wstate), ptr(flow), _optr(key), y0, x0, Ho, Wo, gain, bias, decay, ztol,
                                                    quant, min_cover, ptr(meas), ptr(wmeas), tol, wmax, ptr(r["out"]), ptr(r["wout"]), ptr(r["flag"]),
                                                    _optr(r.get("prior")), _optr(r.get("wprior")), _optr(r.get("cover"))))
        return r
    ctx.check(lib().dfe_temporal_step_f32(ctx.handle, ptr(state), C, H, W, ptr(wstate), ptr(flow), _optr(key), y0, x0, Ho, Wo, gain, bias, decay, ptr(meas),
                                          ptr(wmeas), tol, wmax, ptr(r["out"]), ptr(r["wout"]), ptr(r["flag"]), _optr(r.get("prior")), _optr(r.get("wprior")),
                                          _optr(r.get("src"))))
    return r
