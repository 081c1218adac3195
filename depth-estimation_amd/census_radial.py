"""The census cost for the radial (polar) matcher: an exposure-robust polar flow that needs no trained weights (not in the reference:
include/dfe.h).

    censusRadialCostVolume(sig0, sig1, hWin, agg=3)
        dfe_census_radial_cost_volume_f32: Hamming distances down the polar rows, summed over the channels and an agg x agg box whose
        columns are a ring, as a float volume [Ha][W][hWin] (the staged route, any hWin)
    censusRadialFlow(sig0, sig1, nbits, hWin, agg=3, subpixel=False, zero_last_row=False, want_volume=False)
        dfe_census_radial_flow_f32: the first minimum of that cost, its value and its match score in one launch; the volume on request only
    censusRadialFlowDepth(prev_img, img, e2, hInput, wInput, hWin, k=7, agg=3, ...)
        dfe_census_radial_flow_depth_pair_f32: frames -> polar flow, match score, cartesian flow, depth, confidence, with radialFlowDepth's keys
"""
import ctypes as C

import torch

from ._lib import lib, CensusRadialParams
from .census import _patch, _sigs, censusTransform
from .context import get_ctx, ptr
from .fields import _on_device
from .radial import (_sgm_params, cartesian2polar, flow2depth, getC2PMask, getKOutput, getP2CMaskOF, getRMax, refineRadialFlowSubpixel,
                     semiGlobalAggregate)

FUSED_WINDOWS = (8, 12, 15, 16)   # hWin of dfe_census_radial_flow_f32's instantiations


def _int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _region(name, C, Hp, W, hWin, agg):
    """Ha of the aggregated cost, after the checks of the window, agg and the channel count"""
    if not _int(hWin) or hWin < 1:
        raise ValueError("%s: hWin=%r" % (name, hWin))
    if not _int(agg) or agg not in (1, 3, 5):
        raise ValueError("%s: agg=%r must be 1, 3 or 5" % (name, agg))
    if not 1 <= C <= 4:
        raise ValueError("%s: %d channels (1 .. 4)" % (name, C))
    if Hp > 32768 or W > 32768:
        raise ValueError("%s: %d x %d patch positions (up to 32768 each)" % (name, Hp, W))
    if agg > W:
        raise ValueError("%s: agg=%d on a ring of %d columns" % (name, agg, W))
    Ha = Hp - hWin + 1 - agg + 1
    if Ha < 1:
        raise ValueError("%s: %d rows of patch positions leave no row for a window of %d summed over %d rows" % (name, Hp, hWin, agg))
    return Ha


def _nbits(name, nbits):
    if not _int(nbits) or not 1 <= nbits <= 63:
        raise ValueError("%s: nbits=%r (1 .. 63: the patch's cells less its centre)" % (name, nbits))


def _fused_window(name, hWin):
    if hWin not in FUSED_WINDOWS:
        raise ValueError("%s: hWin=%r has no fused instantiation %r: use censusRadialCostVolume" % (name, hWin, FUSED_WINDOWS))


def censusRadialCostVolume(sig0, sig1, hWin, agg=3):
    """The aggregated radial census cost of two signature tensors [C][Hp][W] of polar frames (censusTransform of a frame with kw - 1 wrap
    columns): float32 [Ha][W][hWin], Ha = Hp - hWin + 1 - agg + 1, label d = frame 1's row y + d, the box's columns taken modulo W
    (include/dfe.h).  Any hWin >= 1."""
    sig0, sig1 = _sigs(sig0, sig1, "censusRadialCostVolume")
    Cc, Hp, W = sig0.shape
    Ha = _region("censusRadialCostVolume", Cc, Hp, W, hWin, agg)
    sig0, sig1 = _on_device("censusRadialCostVolume", (sig0, sig1), dtype=None, expected="CUDA tensors expected")
    out = torch.empty((Ha, W, hWin), dtype=torch.float32, device=sig0.device)
    ctx = get_ctx(sig0)
    ctx.check(lib().dfe_census_radial_cost_volume_f32(ctx.handle, ptr(sig0), ptr(sig1), Cc, Hp, W, hWin, agg, ptr(out)))
    return out


def censusRadialFlow(sig0, sig1, nbits, hWin, agg=3, subpixel=False, zero_last_row=False, want_volume=False):
    """The fused matcher: dict(flow (the first minimum over d as float; with subpixel plus refineRadialFlowSubpixel's offset; its last row
    0 with zero_last_row), best (the cost at the first minimum), match (1 - best / (nbits C agg^2))), all [Ha][W], and with want_volume
    output [Ha][W][hWin].  nbits = kh kw - 1 of the transform that made the signatures; hWin in (8, 12, 15, 16)."""
    sig0, sig1 = _sigs(sig0, sig1, "censusRadialFlow")
    Cc, Hp, W = sig0.shape
    _nbits("censusRadialFlow", nbits)
    Ha = _region("censusRadialFlow", Cc, Hp, W, hWin, agg)
    _fused_window("censusRadialFlow", hWin)
    sig0, sig1 = _on_device("censusRadialFlow", (sig0, sig1), dtype=None, expected="CUDA tensors expected")
    dev = sig0.device
    res = {key: torch.empty((Ha, W), dtype=torch.float32, device=dev) for key in ("flow", "best", "match")}
    vol = torch.empty((Ha, W, hWin), dtype=torch.float32, device=dev) if want_volume else None
    ctx = get_ctx(sig0)
    ctx.check(lib().dfe_census_radial_flow_f32(ctx.handle, ptr(sig0), ptr(sig1), Cc, Hp, W, nbits, hWin, agg, 1 if subpixel else 0, 1 if zero_last_row else 0,
                                               ptr(vol) if want_volume else None, ptr(res["flow"]), ptr(res["best"]), ptr(res["match"])))
    if want_volume:
        res["output"] = vol
    return res


def censusRadialFlowDepth(prev_img, img, e2, hInput, wInput, hWin, k=7, agg=3, kinfty=0.65, alpha_polar=1.0, one_call=True, want_volume=False,
                          zero_last_row=False, subpixel=False, sgm=None):
    """radialFlowDepth with the census matcher in the network's place, so without a network: polar warps of both C x hImg x wImg float32
    frames around the epipole e2 (hInput x wInput, (kw - 1) // 2 wrap columns on the left), their census signatures (k an int or (kh, kw)),
    the radial census cost summed over an agg x agg ring box, its first minimum, back to cartesian through getP2CMaskOF with
    hKernel = kh + agg - 1, flow2depth.  prev_img is the previous frame after the caller's ego-motion correction.  Returns a dict
    polar_flow, match (the census match score [hMatch][wInput]), flow (cartesian), depth, confs [, output = the matcher volume
    [, aggregate]], hMatch = hInput - (kh - 1) - (hWin - 1) - (agg - 1).  hWin in (8, 12, 15, 16).
    one_call: everything inside dfe_census_radial_flow_depth_pair_f32; else the staged public calls -- same numbers bit for bit.
    zero_last_row, subpixel: as in radialFlowDepth.
    sgm: None, (P1, P2) or dict(P1=, P2=, paths=0x0f, ring=hWin) as in radialFlowDepth -- the volume goes through semiGlobalAggregate before
    the arg-min, subpixel then refines on the aggregate, want_volume also returns it as `aggregate`, and match is the score of the RAW cost
    at the chosen integer label."""
    name = "censusRadialFlowDepth"
    kh, kw = _patch(k, name)
    for t in (prev_img, img):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("%s: two float32 frames expected" % name)
    if img.dim() != 3 or tuple(prev_img.shape) != tuple(img.shape):
        raise ValueError("%s: two C x hImg x wImg frames of one shape expected, got %s and %s" % (name, tuple(prev_img.shape), tuple(img.shape)))
    Cc, hImg, wImg = img.shape
    if not all(_int(v) and v >= 1 for v in (hInput, wInput)) or hInput < kh or max(hImg, wImg, hInput, wInput + kw - 1) > 32768:
        raise ValueError("%s: polar size %r x %r for a %d x %d patch (up to 32768 a side)" % (name, hInput, wInput, kh, kw))
    if kw - 1 - (kw - 1) // 2 > wInput:
        raise ValueError("%s: wInput %d below the patch width" % (name, wInput))
    hm = _region(name, Cc, hInput - kh + 1, wInput, hWin, agg)
    _fused_window(name, hWin)
    if not (float(alpha_polar) > 0 and float(kinfty) > 0):
        raise ValueError("%s: alpha_polar=%r and kinfty=%r must be positive" % (name, alpha_polar, kinfty))
    networkp = dict(hImg=hImg, wImg=wImg, hInput=hInput, wInput=wInput, hWin=hWin, hKernel=kh + agg - 1, wKernel=kw)
    kOutput = hm / hInput
    hOut, wOut = int(hImg * kOutput), int(wImg * kOutput)
    if hOut < 1 or wOut < 1:
        raise ValueError("%s: %d matcher rows of %d leave no cartesian output" % (name, hm, hInput))
    sg_paths = 0
    sg_P1 = sg_P2 = 0.0
    sg_ring = 0
    if sgm is not None:
        sg = dict(sgm) if isinstance(sgm, dict) else dict(zip(("P1", "P2"), sgm)) if isinstance(sgm, (tuple, list)) and len(sgm) == 2 else None
        if sg is None or not {"P1", "P2"} <= set(sg) <= {"P1", "P2", "paths", "ring"}:
            raise ValueError("%s: sgm=%r: None, (P1, P2) or dict(P1=, P2=, paths=, ring=) expected" % (name, sgm))
        sg_paths, sg_ring = sg.get("paths", 0x0f), sg.get("ring", min(hWin, wInput))
        sg_P1, sg_P2 = _sgm_params(sg["P1"], sg["P2"], sg_paths, sg_ring, wInput, name + "(sgm=)")
    prev_img, img = _on_device(name, (prev_img, img), dtype=None, expected="CUDA tensors expected")
    prev_img, img = prev_img.contiguous(), img.contiguous()
    dev = img.device
    nbits = kh * kw - 1
    ret = {}
    if one_call:
        prm = CensusRadialParams(Cc, hImg, wImg, hInput, wInput, hWin, kh, kw, agg, float(alpha_polar), float(kinfty), 1 if zero_last_row else 0)
        vol = torch.empty((hm, wInput, hWin), dtype=torch.float32, device=dev) if want_volume else None
        aggv = torch.empty_like(vol) if want_volume and sgm is not None else None
        pf, match = (torch.empty((hm, wInput), dtype=torch.float32, device=dev) for _ in range(2))
        cart, depth, conf = (torch.empty((hOut, wOut), dtype=torch.float32, device=dev) for _ in range(3))
        ctx = get_ctx(img)
        ctx.check(lib().dfe_census_radial_flow_depth_pair_f32(ctx.handle, C.byref(prm), ptr(prev_img), ptr(img), float(e2[0]), float(e2[1]), sg_P1, sg_P2,
                                                              sg_paths, sg_ring, 1 if subpixel else 0, ptr(vol) if vol is not None else None,
                                                              ptr(aggv) if aggv is not None else None, ptr(pf), ptr(match), ptr(cart), ptr(depth), ptr(conf)))
        ret.update(polar_flow=pf, match=match, flow=cart, depth=depth, confs=conf)
        if want_volume:
            ret["output"] = vol
            if sgm is not None:
                ret["aggregate"] = aggv
        return ret
    rmax = getRMax(hImg, wImg, e2)
    mask = getC2PMask(wImg, hImg, wInput, hInput, e2[0], e2[1], (kw - 1) // 2, kw - 1 - (kw - 1) // 2, rmax, alpha_polar, device=dev)
    sig0, sig1 = censusTransform(cartesian2polar(prev_img, mask), (kh, kw)), censusTransform(cartesian2polar(img, mask), (kh, kw))
    if sgm is None:
        r = censusRadialFlow(sig0, sig1, nbits, hWin, agg, subpixel=subpixel, zero_last_row=zero_last_row, want_volume=want_volume)
        idx, match = r["flow"], r["match"]
        if want_volume:
            ret["output"] = r["output"]
    else:
        output = censusRadialCostVolume(sig0, sig1, hWin, agg)
        idx, costs = semiGlobalAggregate(output, sg_P1, sg_P2, sg_paths, sg_ring, want_volume=want_volume or subpixel)
        # the score of the raw cost at the chosen label: one rounded division by a device scalar, one rounded subtraction
        raw = output.gather(2, idx.to(torch.int64).unsqueeze(2)).squeeze(2)
        match = 1.0 - raw / torch.full((), float(nbits * Cc * agg * agg), dtype=torch.float32, device=dev)
        if subpixel:
            idx = refineRadialFlowSubpixel(costs, idx)
        if zero_last_row:
            idx[-1].zero_()
        if want_volume:
            ret.update(output=output, aggregate=costs)
    p2c = getP2CMaskOF(networkp, e2, alpha_polar, device=dev)
    cart = cartesian2polar(idx, p2c)
    kout = getKOutput(networkp)
    depth, conf = flow2depth(networkp, cart, (e2[0] * kout, e2[1] * kout), kinfty)
    ret.update(polar_flow=idx, match=match, flow=cart, depth=depth, confs=conf)
    return ret
