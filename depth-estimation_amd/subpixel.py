"""The single-scale raw-patch step as one call, with its opt-in sub-pixel flow (not in the reference: include/dfe.h).

    flowDepthPair(img1, img2, k, hWin, wWin, foe, threshold=0.21, subpixel=False, scale=1.0, consistency=None, gate=False, fill=None, median=None)
        dfe_flow_depth_pair_f32 / _u8, or their _subpixel_ forms: frames -> flow, extractOutput scores, depth, depth confidence;
        consistency=tol: dfe_flow_depth_pair_fb_f32 / _u8, both directions and the forward-backward mask
        fill=True: the rejected pixels filled from the kept ones, flow_dense / filled / depth_dense
        median=k or (k, sigma): flow (or flow_dense) through the guided weighted median, flow_median / median_valid / depth_median
    flowConsistency(fw, bw, tol, region=None)
        dfe_flow_consistency_f32: the forward-backward mask and residual of any two flow fields
    fillHoles(values, weight, region=None, levels=0)
        dfe_fill_holes_f32: a dense field from the confident pixels of a sparse one (confidence-weighted push-pull)
    weightedMedian(values, weight=None, guide=None, k=7, sigma=0.0, region=None)
        dfe_weighted_median_f32: per channel the lower weighted median of the k x k window, weights from a confidence plane and a guide image
    guidedUpsample(values, size=None, weight=None, guide=None, guide_lo=None, r=2, sigma=0.0, gain=None)
        dfe_guided_upsample_f32: a field at a higher resolution, the mean of the low-resolution samples around each pixel weighted by a tent,
        a confidence plane and the agreement of the frame at both resolutions (joint bilateral upsampling)
    refineFlowSubpixel(img1, img2, idx, hKer, wKer, hWin, wWin)
        dfe_flow_refine_subpixel_f32: the sub-pixel flow of an arg-min index map (dfe_ssd_flow_f32's 1-based idx)
"""
import ctypes

import torch

from ._lib import lib
from .context import get_ctx, ptr


def _frames(img1, img2, name):
    if not (img1.is_cuda and img2.is_cuda):
        raise TypeError("%s: CUDA tensors expected" % name)
    if img1.dtype != img2.dtype or img1.dtype not in (torch.float32, torch.uint8):
        raise TypeError("%s: two float32 or two uint8 frames expected, got %s and %s" % (name, img1.dtype, img2.dtype))
    if img1.dim() != 3 or img1.shape != img2.shape:
        raise ValueError("%s: two C x H x W frames of one shape expected, got %s and %s" % (name, tuple(img1.shape), tuple(img2.shape)))
    return img1.contiguous(), img2.contiguous()


def _kept_weight(res):
    """1 where the step kept the pixel: extractOutput's score above 0 (a rejected pixel carries score 0, and so does one the gate removed)
    and, with consistency, the forward-backward mask"""
    wgt = (res["scores"] > 0).to(torch.float32)
    if "consistent" in res:
        wgt = wgt * res["consistent"]
    return wgt


def _median_arg(median):
    """median=k or (k, sigma) of flowDepthPair -> (k, sigma), or None"""
    if median is None or median is False:
        return None
    k, sigma = median if isinstance(median, (tuple, list)) and len(median) == 2 else (median, 0.0)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= 15 or k % 2 == 0 or not isinstance(sigma, (int, float)):
        raise ValueError("flowDepthPair: median=%r: an odd window 1 .. 15, or (window, sigma), expected" % (median,))
    return k, float(sigma)


def _with_fill(res, fill, median, guide, k, hWin, wWin, fx, fy, region=None):
    """the keys of flowDepthPair(..., fill=..., median=...) from the step's own outputs, which stay as they are; region = (y0, x0, Ho, Wo)
    of the step's output, by default the single-scale SSD step's"""
    want_fill = not (fill is None or fill is False)
    if not want_fill and median is None:
        return res
    flow, scores = res["flow"], res["scores"]
    _, H, W = flow.shape
    Ho, Wo = H - k + 1 - hWin + 1, W - k + 1 - wWin + 1
    R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo) if region is None else tuple(int(v) for v in region)
    wgt = _kept_weight(res)
    ctx = get_ctx(flow)

    def depth_of(field):
        depth = torch.empty_like(scores)
        conf = torch.empty_like(scores)
        ctx.check(lib().dfe_flow_to_depth_cartesian(ctx.handle, ptr(field), H, W, fx, fy, 0, ptr(depth), ptr(conf)))
        return depth

    src = flow
    if want_fill:
        dense, filled = fillHoles(flow, wgt, R, 0 if fill is True else int(fill))
        res.update(flow_dense=dense, filled=filled, depth_dense=depth_of(dense))
        src, wgt = dense, torch.where(wgt > 0, filled, 0.25 * filled)   # a filled value votes, but weighs less than a measured one
    if median is not None:
        med, valid = weightedMedian(src, wgt, guide.to(torch.float32), median[0], median[1], R)
        res.update(flow_median=med, median_valid=valid, depth_median=depth_of(med))
    return res


def flowDepthPair(img1, img2, k, hWin, wWin, foe, threshold=0.21, subpixel=False, scale=1.0, consistency=None, gate=False, fill=None, median=None):
    """One frame pair through the single-scale step: C x H x W frames (float32, or uint8 read as float(byte) * scale), a k x k patch,
    an hWin x wWin search window, foe = (x, y) focus of expansion.  Returns dict(flow [2][H][W] (y, x), scores, depth, depth_conf [H][W]),
    zero outside the centre-pasted output region.  subpixel=True: the flow is refined to sub-pixel precision and depth follows it;
    scores are the same either way.
    consistency=tol (pixels): the step also runs from img2 to img1 and the dict gains flow_bw [2][H][W], consistent [H][W] (1 where following
    the forward flow and then the backward flow found there returns within tol, else 0) and consistency_err [H][W] (that residual; +Inf
    where the forward flow leaves the output region or a flow is not finite).  gate=True multiplies scores and depth_conf by consistent.
    fill=True (or an int: the `levels` of fillHoles): the dict gains flow_dense [2][H][W] = fillHoles(flow, wgt, R, levels) with R the
    output region and wgt 1 where scores > 0 (and, with consistency, where consistent is 1 as well), filled [H][W] (1 where a value was
    found), and depth_dense [H][W], the depth of flow_dense (dfe_flow_to_depth_cartesian, fix_dot = 0).  The other keys are unchanged.
    median=k or (k, sigma): the dict gains flow_median [2][H][W], median_valid [H][W] = weightedMedian(src, wgt, img1 as float32, k, sigma, R)
    and depth_median [H][W], the depth of flow_median made as depth_dense is.  Without fill, src = flow and wgt is the plane above; with
    fill, src = flow_dense and wgt = filled, 0.25 where the pixel was a hole.  sigma is in the frame's own units (bytes for uint8 frames);
    0, the default, is the unguided median.  Frames of more than 4 channels cannot guide (ValueError).  The other keys are unchanged."""
    median = _median_arg(median)
    a, b = _frames(img1, img2, "flowDepthPair")
    C, H, W = a.shape
    flow = torch.empty((2, H, W), dtype=torch.float32, device=a.device)
    scores = torch.empty((H, W), dtype=torch.float32, device=a.device)
    depth = torch.empty_like(scores)
    conf = torch.empty_like(scores)
    ctx = get_ctx(a)
    fx, fy = float(foe[0]), float(foe[1])
    l = lib()
    if consistency is not None:
        bw = torch.empty_like(flow)
        mask = torch.empty_like(scores)
        err = torch.empty_like(scores)
        tail = (int(bool(subpixel)), float(consistency), int(bool(gate)), ptr(flow), ptr(scores), ptr(depth), ptr(conf), ptr(bw), ptr(mask), ptr(err))
        if a.dtype == torch.uint8:
            rc = l.dfe_flow_depth_pair_fb_u8(ctx.handle, ptr(a), ptr(b), C, H, W, k, hWin, wWin, fx, fy, threshold, float(scale), *tail)
        else:
            rc = l.dfe_flow_depth_pair_fb_f32(ctx.handle, ptr(a), ptr(b), C, H, W, k, hWin, wWin, fx, fy, threshold, *tail)
        ctx.check(rc)
        return _with_fill({"flow": flow, "scores": scores, "depth": depth, "depth_conf": conf, "flow_bw": bw, "consistent": mask, "consistency_err": err},
                          fill, median, a, k, hWin, wWin, fx, fy)
    if a.dtype == torch.uint8:
        fn = l.dfe_flow_depth_pair_subpixel_u8 if subpixel else l.dfe_flow_depth_pair_u8
        rc = fn(ctx.handle, ptr(a), ptr(b), C, H, W, k, hWin, wWin, fx, fy, threshold, float(scale), ptr(flow), ptr(scores), ptr(depth), ptr(conf))
    else:
        fn = l.dfe_flow_depth_pair_subpixel_f32 if subpixel else l.dfe_flow_depth_pair_f32
        rc = fn(ctx.handle, ptr(a), ptr(b), C, H, W, k, hWin, wWin, fx, fy, threshold, ptr(flow), ptr(scores), ptr(depth), ptr(conf))
    ctx.check(rc)
    return _with_fill({"flow": flow, "scores": scores, "depth": depth, "depth_conf": conf}, fill, median, a, k, hWin, wWin, fx, fy)


def flowConsistency(fw, bw, tol, region=None):
    """Forward-backward check of two float32 flow fields [2][H][W] (plane 0 = y, plane 1 = x; fw from frame 0 to frame 1, bw back) over
    region = (y0, x0, Ho, Wo), the whole frame by default (include/dfe.h: dfe_flow_consistency_f32).  Returns (mask, err), float32 [H][W]:
    mask 1 where |fw(p) + bw(p + fw(p))| <= tol, err that residual (+Inf where p + fw(p) leaves the region or a flow is not finite); both 0
    outside the region."""
    if not (fw.is_cuda and bw.is_cuda) or fw.dtype != torch.float32 or bw.dtype != torch.float32:
        raise TypeError("flowConsistency: two float32 CUDA tensors expected")
    if fw.dim() != 3 or fw.shape[0] != 2 or fw.shape != bw.shape or fw.device != bw.device:
        raise ValueError("flowConsistency: two 2 x H x W flows of one shape expected, got %s and %s" % (tuple(fw.shape), tuple(bw.shape)))
    fw, bw = fw.contiguous(), bw.contiguous()
    _, H, W = fw.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else (int(v) for v in region)
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
    if values.dim() != 3 or not 1 <= values.shape[0] <= 4 or weight.dim() != 2 or tuple(weight.shape) != tuple(values.shape[1:]):
        raise ValueError("fillHoles: values C x H x W (C = 1 .. 4) and weight H x W expected, got %s and %s" % (tuple(values.shape), tuple(weight.shape)))
    if not (values.is_cuda and weight.is_cuda) or values.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("fillHoles: two float32 CUDA tensors expected")
    if values.device != weight.device:
        raise ValueError("fillHoles: values on %s, weight on %s" % (values.device, weight.device))
    values, weight = values.contiguous(), weight.contiguous()
    C, H, W = values.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else (int(v) for v in region)
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
    if values.dim() != 3 or not 1 <= values.shape[0] <= 4:
        raise ValueError("weightedMedian: values C x H x W (C = 1 .. 4) expected, got %s" % (tuple(values.shape),))
    if weight is not None and (weight.dim() != 2 or tuple(weight.shape) != tuple(values.shape[1:])):
        raise ValueError("weightedMedian: weight H x W expected, got %s for values %s" % (tuple(weight.shape), tuple(values.shape)))
    if guide is not None and (guide.dim() != 3 or not 1 <= guide.shape[0] <= 4 or tuple(guide.shape[1:]) != tuple(values.shape[1:])):
        raise ValueError("weightedMedian: guide Cg x H x W (Cg = 1 .. 4) expected, got %s for values %s" % (tuple(guide.shape), tuple(values.shape)))
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= 15 or k % 2 == 0:
        raise ValueError("weightedMedian: k=%r must be odd, 1 .. 15" % (k,))
    planes = [t for t in (values, weight, guide) if t is not None]
    if not all(t.is_cuda and t.dtype == torch.float32 for t in planes):
        raise TypeError("weightedMedian: float32 CUDA tensors expected")
    if any(t.device != values.device for t in planes):
        raise ValueError("weightedMedian: tensors on different devices")
    values, weight, guide = (None if t is None else t.contiguous() for t in (values, weight, guide))
    C, H, W = values.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else (int(v) for v in region)
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
    if values.dim() != 3 or not 1 <= values.shape[0] <= 4:
        raise ValueError("guidedUpsample: values C x Hl x Wl (C = 1 .. 4) expected, got %s" % (tuple(values.shape),))
    C, Hl, Wl = values.shape
    if weight is not None and (weight.dim() != 2 or tuple(weight.shape) != (Hl, Wl)):
        raise ValueError("guidedUpsample: weight Hl x Wl expected, got %s for values %s" % (tuple(weight.shape), tuple(values.shape)))
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
    planes = [t for t in (values, weight, guide, guide_lo) if t is not None]
    if not all(t.is_cuda and t.dtype == torch.float32 for t in planes):
        raise TypeError("guidedUpsample: float32 CUDA tensors expected")
    if any(t.device != values.device for t in planes):
        raise ValueError("guidedUpsample: tensors on different devices")
    if guide is not None and guide_lo is None:
        from .stream import imageScale

        guide_lo = imageScale(guide, Wl, Hl)
    values, weight, guide, guide_lo = (None if t is None else t.contiguous() for t in (values, weight, guide, guide_lo))
    out = torch.empty((C, Hh, Wh), dtype=torch.float32, device=values.device)
    valid = torch.empty((Hh, Wh), dtype=torch.float32, device=values.device)
    ctx = get_ctx(values)
    ctx.check(lib().dfe_guided_upsample_f32(ctx.handle, ptr(values), C, Hl, Wl, None if weight is None else ptr(weight), None if guide is None else ptr(guide),
                                            None if guide_lo is None else ptr(guide_lo), 0 if guide is None else guide.shape[0], float(sigma), r,
                                            None if gain is None else (ctypes.c_float * C)(*gain), Hh, Wh, ptr(out), ptr(valid)))
    return out, valid


def refineFlowSubpixel(img1, img2, idx, hKer, wKer, hWin, wWin):
    """Sub-pixel flow of float32 C x H x W frames from the arg-min index map idx [Ho][Wo] (int64, 1-based, as dfe_ssd_flow_f32 and
    compute_cartesian_groundtruth_cross_correlation give it).  Returns (fy, fx), float32 [Ho][Wo]; pixels whose idx is not a cell of the
    window are NaN."""
    a, b = _frames(img1, img2, "refineFlowSubpixel")
    if a.dtype != torch.float32:
        raise TypeError("refineFlowSubpixel: float32 frames expected")
    C, H, W = a.shape
    Ho, Wo = H - hKer + 1 - hWin + 1, W - wKer + 1 - wWin + 1
    if idx.dtype != torch.int64 or tuple(idx.shape) != (Ho, Wo) or idx.device != a.device:
        raise ValueError("refineFlowSubpixel: idx must be int64 [%d][%d] on %s, got %s %s" % (Ho, Wo, a.device, idx.dtype, tuple(idx.shape)))
    idx = idx.contiguous()
    fy = torch.full((Ho, Wo), float("nan"), dtype=torch.float32, device=a.device)
    fx = torch.full_like(fy, float("nan"))
    ctx = get_ctx(a)
    ctx.check(lib().dfe_flow_refine_subpixel_f32(ctx.handle, ptr(a), ptr(b), C, H, W, hKer, wKer, hWin, wWin, ptr(idx), ptr(fy), ptr(fx), Wo, 0, 0))
    return fy, fx
