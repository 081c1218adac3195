"""The census matching cost: an exposure-robust single-scale matcher (not in the reference: include/dfe.h).

    censusTransform(img, k=7)
        dfe_census_transform_f32 / _u8: the signature of every k x k (or kh x kw) patch, its cells compared with its centre
    censusCostVolume(sig0, sig1, hWin, wWin, agg=3)
        dfe_census_cost_volume_f32: Hamming distances summed over the channels and an agg x agg box, as a float volume (the staged route)
    censusFlow(sig0, sig1, nbits, hWin, wWin, agg=3, refine=False)
        dfe_census_flow_f32: the first minimum of that cost with the centre rule, its match score and the decoded flow; no volume
    censusRefineSubpixel(sig0, sig1, hWin, wWin, idx, agg=3, flow_y=None, flow_x=None, pad_t=0, pad_l=0)
        dfe_census_refine_subpixel_f32: the vee fit through the chosen cell's raw census cost and its neighbours' 
    censusFlowDepthPair(img1, img2, k, hWin, wWin, foe, agg=3, scale=1.0, consistency=None, gate=False, fill=None, median=None, sgm=None,
                        subpixel=False, refine=False)
        dfe_census_flow_depth_pair_f32 / _u8: frames -> flow, match score, depth, depth confidence, with flowDepthPair's keys;
        sgm=(P1, P2): dfe_census_flow_depth_pair_sgm_f32 / _u8, the cost aggregated along image paths before the arg-min;
        with subpixel=True or min_unique in the dict: the _sgm2_ entries, which add the key unique;
        refine=True: dfe_census_flow_depth_pair_subpixel_f32 / _u8, the flow refined on the raw cost
    censusPyramidScaleVolume(i0, i1, r, k, maxh, maxw, agg=3, beta=None)
        dfe_census_pyramid_scale_volume_f32: one scale of the census pyramid's volumes, staged (the matcher itself is
        MultiscaleModel.forwardFlow(..., census=True), multiscale.py)
"""
import torch

from ._lib import lib
from .context import get_ctx, ptr
from .fields import _on_device, flowConsistency
from .sgm_plane import MAX_CELLS, _sgm_pick_arg
from .subpixel import _frames, _median_arg, _with_fill


def _patch(k, name):
    kh, kw = k if isinstance(k, (tuple, list)) and len(k) == 2 else (k, k)
    ok = all(isinstance(n, int) and not isinstance(n, bool) and n >= 3 and n % 2 == 1 for n in (kh, kw))
    if not ok or kh * kw > 64:
        raise ValueError("%s: k=%r: odd sides of at least 3 with at most 64 cells expected" % (name, k))
    return kh, kw


def _region(name, C, Hp, Wp, hWin, wWin, agg):
    """(Ha, Wa) of the aggregated cost, after the checks of the window, agg and the channel count"""
    if not all(isinstance(n, int) and not isinstance(n, bool) for n in (hWin, wWin)) or hWin < 1 or wWin < 1:
        raise ValueError("%s: window %r x %r" % (name, hWin, wWin))
    if hWin * wWin > MAX_CELLS:
        raise ValueError("%s: window %d x %d has more than %d cells" % (name, hWin, wWin, MAX_CELLS))
    if not isinstance(agg, int) or isinstance(agg, bool) or agg not in (1, 3, 5):
        raise ValueError("%s: agg=%r must be 1, 3 or 5" % (name, agg))
    if not 1 <= C <= 4:
        raise ValueError("%s: %d channels (1 .. 4)" % (name, C))
    Ha, Wa = Hp - hWin + 1 - agg + 1, Wp - wWin + 1 - agg + 1
    if Ha < 1 or Wa < 1:
        raise ValueError("%s: %d x %d patch positions leave no pixel for a %d x %d window summed over %d x %d" % (name, Hp, Wp, hWin, wWin, agg, agg))
    return Ha, Wa


def _sigs(sig0, sig1, name):
    if not (isinstance(sig0, torch.Tensor) and isinstance(sig1, torch.Tensor)) or sig0.dtype != torch.int64 or sig1.dtype != torch.int64:
        raise TypeError("%s: two int64 signature tensors expected" % name)
    if sig0.dim() != 3 or sig0.shape != sig1.shape:
        raise ValueError("%s: two C x Hp x Wp signature tensors of one shape expected, got %s and %s" % (name, tuple(sig0.shape), tuple(sig1.shape)))
    return sig0, sig1


def censusTransform(img, k=7):
    """Census signatures of a C x H x W frame (float32 or uint8, 1 <= C <= 4): int64 [C][Hp][Wp] holding the bits, Hp = H - kh + 1,
    Wp = W - kw + 1, a patch indexed by its top-left corner.  k is an int or (kh, kw), odd sides of at least 3, kh kw <= 64.  Bit b is set
    iff the b-th cell of the patch, row-major with the centre skipped, is strictly below the centre (include/dfe.h)."""
    kh, kw = _patch(k, "censusTransform")
    if not isinstance(img, torch.Tensor) or img.dtype not in (torch.float32, torch.uint8):
        raise TypeError("censusTransform: a float32 or uint8 frame expected")
    if img.dim() != 3 or not 1 <= img.shape[0] <= 4:
        raise ValueError("censusTransform: a C x H x W frame (C = 1 .. 4) expected, got %s" % (tuple(img.shape),))
    C, H, W = img.shape
    if H < kh or W < kw or H > 32768 or W > 32768:
        raise ValueError("censusTransform: frame %d x %d for a %d x %d patch (up to 32768 a side)" % (H, W, kh, kw))
    (img,) = _on_device("censusTransform", (img,), dtype=None, expected="CUDA tensors expected")
    sig = torch.empty((C, H - kh + 1, W - kw + 1), dtype=torch.int64, device=img.device)
    ctx = get_ctx(img)
    fn = lib().dfe_census_transform_u8 if img.dtype == torch.uint8 else lib().dfe_census_transform_f32
    ctx.check(fn(ctx.handle, ptr(img), C, H, W, kh, kw, ptr(sig)))
    return sig


def censusCostVolume(sig0, sig1, hWin, wWin, agg=3):
    """The aggregated census cost of two signature tensors [C][Hp][Wp]: float32 [Ha][Wa][hWin][wWin], the SSD volume's geometry and class
    order, Ha = Hp - hWin + 1 - agg + 1 (include/dfe.h).  The staged route: censusFlow gives the same flow without the volume."""
    sig0, sig1 = _sigs(sig0, sig1, "censusCostVolume")
    C, Hp, Wp = sig0.shape
    Ha, Wa = _region("censusCostVolume", C, Hp, Wp, hWin, wWin, agg)
    sig0, sig1 = _on_device("censusCostVolume", (sig0, sig1), dtype=None, expected="CUDA tensors expected")
    out = torch.empty((Ha, Wa, hWin, wWin), dtype=torch.float32, device=sig0.device)
    ctx = get_ctx(sig0)
    ctx.check(lib().dfe_census_cost_volume_f32(ctx.handle, ptr(sig0), ptr(sig1), C, Hp, Wp, hWin, wWin, agg, ptr(out)))
    return out


def censusRefineSubpixel(sig0, sig1, hWin, wWin, idx, agg=3, flow_y=None, flow_x=None, pad_t=0, pad_l=0):
    """The sub-pixel refinement on the raw census cost, alone (dfe_census_refine_subpixel_f32; include/dfe.h): for
    every pixel of idx [Ha][Wa] (int64, the 1-based class of censusFlow) the vee fit per axis through the aggregated cost of the class's
    cell and its two neighbours', re-formed from the signatures.  Returns (flow_y, flow_x): the given float32 planes (one shape
    [Hf][Wf], contiguous, Hf >= pad_t + Ha, Wf >= pad_l + Wa), written in place at [y + pad_t][x + pad_l], or new Ha x Wa planes of
    zeros.  Pixels whose idx is outside 1 .. hWin wWin keep what the planes held.  Meant for agg >= 3 or several channels: one channel
    without a box has too few bits to refine on."""
    name = "censusRefineSubpixel"
    sig0, sig1 = _sigs(sig0, sig1, name)
    C, Hp, Wp = sig0.shape
    Ha, Wa = _region(name, C, Hp, Wp, hWin, wWin, agg)
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64:
        raise TypeError("%s: an int64 class map expected" % name)
    if tuple(idx.shape) != (Ha, Wa):
        raise ValueError("%s: idx %s, the region is %d x %d" % (name, tuple(idx.shape), Ha, Wa))
    if not all(isinstance(n, int) and not isinstance(n, bool) and n >= 0 for n in (pad_t, pad_l)):
        raise ValueError("%s: pads %r, %r: ints of at least 0 expected" % (name, pad_t, pad_l))
    if (flow_y is None) != (flow_x is None):
        raise ValueError("%s: flow_y and flow_x go together" % name)
    if flow_y is not None:
        for t in (flow_y, flow_x):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError("%s: float32 flow planes expected" % name)
        if flow_y.dim() != 2 or flow_y.shape != flow_x.shape or not (flow_y.is_contiguous() and flow_x.is_contiguous()):
            raise ValueError("%s: two contiguous planes of one shape expected" % name)
        if flow_y.shape[0] < pad_t + Ha or flow_y.shape[1] < pad_l + Wa:
            raise ValueError("%s: planes %s hold no %d x %d region at (%d, %d)" % (name, tuple(flow_y.shape), Ha, Wa, pad_t, pad_l))
    sig0, sig1, idx = _on_device(name, (sig0, sig1, idx), dtype=None, expected="CUDA tensors expected")
    if flow_y is None:
        flow_y = torch.zeros((pad_t + Ha, pad_l + Wa), dtype=torch.float32, device=sig0.device)
        flow_x = torch.zeros_like(flow_y)
    elif flow_y.device != sig0.device or flow_x.device != sig0.device:
        raise TypeError("%s: the flow planes are on another device" % name)
    ctx = get_ctx(sig0)
    ctx.check(lib().dfe_census_refine_subpixel_f32(ctx.handle, ptr(sig0), ptr(sig1), C, Hp, Wp, hWin, wWin, agg, ptr(idx), ptr(flow_y), ptr(flow_x),
                                                   flow_y.shape[1], pad_t, pad_l))
    return flow_y, flow_x


def censusFlow(sig0, sig1, nbits, hWin, wWin, agg=3, refine=False):
    """The fused sweep: dict(idx int64 (1-based class, first minimum, the centre wins an exact tie), best (the cost), match
    (1 - best / (nbits C agg^2)), flow_y, flow_x), all [Ha][Wa].  nbits = kh kw - 1 of the transform that made the signatures.
    refine=True: flow_y / flow_x are refined by censusRefineSubpixel behind the sweep; idx, best and match are untouched.  Meant for
    agg >= 3 or several channels."""
    sig0, sig1 = _sigs(sig0, sig1, "censusFlow")
    C, Hp, Wp = sig0.shape
    if not isinstance(nbits, int) or isinstance(nbits, bool) or not 1 <= nbits <= 63:
        raise ValueError("censusFlow: nbits=%r (1 .. 63: the patch's cells less its centre)" % (nbits,))
    Ha, Wa = _region("censusFlow", C, Hp, Wp, hWin, wWin, agg)
    sig0, sig1 = _on_device("censusFlow", (sig0, sig1), dtype=None, expected="CUDA tensors expected")
    dev = sig0.device
    res = {"idx": torch.empty((Ha, Wa), dtype=torch.int64, device=dev)}
    for key in ("best", "match", "flow_y", "flow_x"):
        res[key] = torch.empty((Ha, Wa), dtype=torch.float32, device=dev)
    ctx = get_ctx(sig0)
    ctx.check(lib().dfe_census_flow_f32(ctx.handle, ptr(sig0), ptr(sig1), C, Hp, Wp, nbits, hWin, wWin, agg, ptr(res["idx"]), ptr(res["best"]),
                                        ptr(res["match"]), ptr(res["flow_y"]), ptr(res["flow_x"])))
    if refine:
        ctx.check(lib().dfe_census_refine_subpixel_f32(ctx.handle, ptr(sig0), ptr(sig1), C, Hp, Wp, hWin, wWin, agg, ptr(res["idx"]), ptr(res["flow_y"]),
                                                       ptr(res["flow_x"]), Wa, 0, 0))
    return res


def _pair(a, b, k, hWin, wWin, agg, fx, fy, scale, sgm=None, subpixel=False, refine=False):
    C, H, W = a.shape
    flow = torch.empty((2, H, W), dtype=torch.float32, device=a.device)
    match = torch.empty((H, W), dtype=torch.float32, device=a.device)
    depth = torch.empty_like(match)
    conf = torch.empty_like(match)
    ctx = get_ctx(a)
    res = {"flow": flow, "scores": match}
    # the entry: plain, _subpixel_ (refine: the plain arguments), _sgm_ (P1, P2, paths) or, with subpixel or a named min_unique, _sgm2_
    # (... subpixel, min_unique, and unique behind match)
    name, mid, outs = "dfe_census_flow_depth_pair_", (), (ptr(flow), ptr(match))
    if refine:
        name += "subpixel_"
    elif sgm is not None and sgm[5] is not None:   # the guided entry: _sgm2_'s arguments, then sigma and P2_edge; frame `a` guides
        res["unique"] = torch.empty_like(match)
        name, mid, outs = name + "sgm_guided_", sgm[:3] + (int(bool(subpixel)), sgm[3]) + sgm[5], outs + (ptr(res["unique"]),)
    elif sgm is not None and (subpixel or sgm[4]):
        res["unique"] = torch.empty_like(match)
        name, mid, outs = name + "sgm2_", sgm[:3] + (int(bool(subpixel)), sgm[3]), outs + (ptr(res["unique"]),)
    elif sgm is not None:
        name, mid = name + "sgm_", sgm[:3]
    head = (ctx.handle, ptr(a), ptr(b), C, H, W, k, hWin, wWin, agg, fx, fy)
    if a.dtype == torch.uint8:
        rc = getattr(lib(), name + "u8")(*head, scale, *mid, *outs, ptr(depth), ptr(conf))
    else:
        rc = getattr(lib(), name + "f32")(*head, *mid, *outs, ptr(depth), ptr(conf))
    ctx.check(rc)
    res.update(depth=depth, depth_conf=conf)
    return res


def censusFlowDepthPair(img1, img2, k, hWin, wWin, foe, agg=3, scale=1.0, consistency=None, gate=False, fill=None, median=None, sgm=None,
                        subpixel=False, refine=False):
    """One frame pair through the census matcher: C x H x W frames (float32 or uint8, 1 <= C <= 4), a k x k patch (k odd, 3 .. 7), an
    hWin x wWin search window, the Hamming cost summed over an agg x agg box (1, 3 or 5), foe = (x, y) focus of expansion.  Returns the keys
    of flowDepthPair: flow [2][H][W] (y, x), scores [H][W] = the match score 1 - best / ((k k - 1) C agg^2), depth, depth_conf, zero outside
    the centre-pasted Ha x Wa region at ((H - Ha) // 2, (W - Wa) // 2), Ha = H - k + 1 - hWin + 1 - agg + 1.  scale is accepted for uint8
    frames as flowDepthPair accepts it and changes no bit: the bytes are compared as they are.
    consistency=tol: the call also runs from img2 to img1 and the dict gains flow_bw, consistent and consistency_err =
    flowConsistency(flow, flow_bw, tol, region); gate=True multiplies scores and depth_conf by consistent.  fill and median: as in
    flowDepthPair, over the region above, with weight 1 where scores > 0 (and consistent).
    sgm: None, (P1, P2) or dict(P1=, P2=, paths=0x0f) -- the aggregated census cost goes through
    semiGlobalAggregatePlane before the arg-min, in both directions of consistency= (dfe_census_flow_depth_pair_sgm_f32 / _u8); scores is
    then the match score of the raw cost at the chosen class.  None leaves every bit and every launch as it is.
    subpixel=True (with sgm only, else ValueError) or min_unique in the sgm dict: the
    dfe_census_flow_depth_pair_sgm2_f32 / _u8 entries -- the flow moves by the per-axis parabola through the AGGREGATE, and the dict gains
    unique [H][W], the uniqueness (second - best) / second of the aggregate gated by min_unique, 0 outside the region; scores keeps its
    meaning, and fill and median still weigh by scores > 0.
    sigma= or P2_edge= (None: P1) in the sgm dict: dfe_census_flow_depth_pair_sgm_guided_f32 / _u8 -- the call's
    first frame on the region guides P2, which falls to P2_edge across its edges (sigma in the frame's units, bytes times scale for uint8
    frames: scale matters here only); the dict gains unique as above.  With consistency= the backward call is guided by ITS first frame, img2.
    refine=True (without sgm, else ValueError): dfe_census_flow_depth_pair_subpixel_f32 / _u8 -- the step runs
    unchanged, then its flow moves per axis by the vee fit through the RAW census cost of the chosen cell and its two neighbours'; depth and
    depth_conf are made from the refined flow, scores and the border are the step's.  With consistency= both directions are refined; gate,
    fill and median work as before on the refined flow.  Meant for agg >= 3 or several channels: one channel without a box has too few
    bits to refine on, and the refined flow is then no better than the integer one."""
    median = _median_arg(median)
    sgm = _sgm_pick_arg(sgm, "censusFlowDepthPair")
    if subpixel and sgm is None:
        raise ValueError("censusFlowDepthPair: subpixel=True refines on the aggregate: it needs sgm=")
    if refine and sgm is not None:
        raise ValueError("censusFlowDepthPair: refine=True refines on the raw cost: with sgm= use subpixel=True, which refines on the aggregate")
    for t in (img1, img2):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.uint8) or t.dtype != img1.dtype:
            raise TypeError("censusFlowDepthPair: two float32 or two uint8 frames expected")
    if img1.dim() != 3 or img1.shape != img2.shape:
        raise ValueError("censusFlowDepthPair: two C x H x W frames of one shape expected, got %s and %s" % (tuple(img1.shape), tuple(img2.shape)))
    a, b = img1, img2
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError("censusFlowDepthPair: k=%r: an odd int expected" % (k,))
    _patch(k, "censusFlowDepthPair")
    C, H, W = a.shape
    if H < k or W < k or H > 32768 or W > 32768:
        raise ValueError("censusFlowDepthPair: frame %d x %d for a %d x %d patch (up to 32768 a side)" % (H, W, k, k))
    Ha, Wa = _region("censusFlowDepthPair", C, H - k + 1, W - k + 1, hWin, wWin, agg)
    if not float(scale) > 0:
        raise ValueError("censusFlowDepthPair: scale=%r must be positive" % (scale,))
    a, b = _frames(a, b, "censusFlowDepthPair")   # (the device check comes last: every check above needs none)
    R = ((H - Ha) // 2, (W - Wa) // 2, Ha, Wa)
    fx, fy = float(foe[0]), float(foe[1])
    res = _pair(a, b, k, hWin, wWin, agg, fx, fy, float(scale), sgm, subpixel, bool(refine))
    if consistency is not None:
        bw = _pair(b, a, k, hWin, wWin, agg, fx, fy, float(scale), sgm, subpixel, bool(refine))["flow"]
        mask, err = flowConsistency(res["flow"], bw, float(consistency), R)
        res.update(flow_bw=bw, consistent=mask, consistency_err=err)
        if gate:
            res["scores"] = res["scores"] * mask
            res["depth_conf"] = res["depth_conf"] * mask
    return _with_fill(res, fill, median, a, k, hWin, wWin, fx, fy, region=R)


def _pyramid_args(name, C, k, agg, beta):
    """(k, agg, beta) of a census pyramid call after its checks; beta=None: 0.25 / (C agg^2)"""
    if isinstance(k, bool) or not isinstance(k, int) or k < 3 or k % 2 == 0 or k * k > 64:
        raise ValueError("%s: k=%r: an odd int of at least 3 with k k <= 64 expected" % (name, k))
    if not isinstance(agg, int) or isinstance(agg, bool) or agg not in (1, 3, 5):
        raise ValueError("%s: agg=%r must be 1, 3 or 5" % (name, agg))
    if not 1 <= C <= 4:
        raise ValueError("%s: %d channels (1 .. 4)" % (name, C))
    if beta is None:
        beta = 0.25 / (C * agg * agg)
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not (0.0 < float(beta) < float("inf")):
        raise ValueError("%s: beta=%r must be finite and positive" % (name, beta))
    return k, agg, float(beta)


def censusPyramidScaleVolume(i0, i1, r, k, maxh, maxw, agg=3, beta=None):
    """One scale of the census pyramid (include/dfe.h), staged: two float32 frames C x H x W (1 <= C <= 4), H and W
    multiples of r, box down-sampled by r, zero-padded for the receptive field k + agg - 1, their k x k census signatures, the Hamming cost
    summed over the channels and an agg x agg box for every cell of the maxh x maxw window, times beta (None: 0.25 / (C agg^2)).  float32
    [H/r][W/r][maxh][maxw], the geometry and class order of dfe_pyramid_scale_volume_f32 (dfe_census_pyramid_scale_volume_f32)."""
    name = "censusPyramidScaleVolume"
    for t in (i0, i1):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("%s: two float32 frames expected" % name)
    if i0.dim() != 3 or i0.shape != i1.shape:
        raise ValueError("%s: two C x H x W frames of one shape expected, got %s and %s" % (name, tuple(i0.shape), tuple(i1.shape)))
    C, H, W = i0.shape
    k, agg, beta = _pyramid_args(name, C, k, agg, beta)
    if not all(isinstance(n, int) and not isinstance(n, bool) and n >= 1 for n in (r, maxh, maxw)):
        raise ValueError("%s: r=%r, window %r x %r: positive ints expected" % (name, r, maxh, maxw))
    if maxh * maxw > MAX_CELLS:
        raise ValueError("%s: window %d x %d has more than %d cells" % (name, maxh, maxw, MAX_CELLS))
    if H % r or W % r or H < r or W < r:
        raise ValueError("%s: frame %d x %d is not a multiple of ratio %d" % (name, H, W, r))
    i0, i1 = _on_device(name, (i0, i1), dtype=None, expected="CUDA tensors expected")
    out = torch.empty((H // r, W // r, maxh, maxw), dtype=torch.float32, device=i0.device)
    ctx = get_ctx(i0)
    ctx.check(lib().dfe_census_pyramid_scale_volume_f32(ctx.handle, ptr(i0), ptr(i1), C, H, W, r, k, maxh, maxw, agg, beta, ptr(out)))
    return out
