"""The single-scale raw-patch step as one call, with its opt-in sub-pixel flow (not in the reference: include/dfe.h).

    flowDepthPair(img1, img2, k, hWin, wWin, foe, threshold=0.21, subpixel=False, scale=1.0, consistency=None, gate=False, fill=None, median=None,
                  sgm=None)
        dfe_flow_depth_pair_f32 / _u8, or their _subpixel_ forms: frames -> flow, extractOutput scores, depth, depth confidence;
        sgm=(P1, P2): dfe_flow_depth_pair_sgm_f32 / _u8, the SSD cost aggregated along image paths before the arg-min; scores are then the
        uniqueness of the aggregate and subpixel refines on it
        consistency=tol: dfe_flow_depth_pair_fb_f32 / _u8, both directions and the forward-backward mask
        fill=True: the rejected pixels filled from the kept ones, flow_dense / filled / depth_dense
        median=k or (k, sigma): flow (or flow_dense) through the guided weighted median, flow_median / median_valid / depth_median
    refineFlowSubpixel(img1, img2, idx, hKer, wKer, hWin, wWin)
        dfe_flow_refine_subpixel_f32: the sub-pixel flow of an arg-min index map (dfe_ssd_flow_f32's 1-based idx)
"""
import torch

from ._lib import lib
from .context import get_ctx, ptr
from .fields import fillHoles, weightedMedian
from .sgm_plane import _sgm_pick_arg


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


def flowDepthPair(img1, img2, k, hWin, wWin, foe, threshold=0.21, subpixel=False, scale=1.0, consistency=None, gate=False, fill=None, median=None,
                  sgm=None):
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
    0, the default, is the unguided median.  Frames of more than 4 channels cannot guide (ValueError).  The other keys are unchanged.
    sgm: None, (P1, P2) or dict(P1=, P2=, paths=0x0f, min_unique=0.0) -- the whole SSD volume goes through
    semiGlobalPick before the arg-min (dfe_flow_depth_pair_sgm_f32 / _u8).  scores is then the uniqueness of the aggregate, (second - best) /
    second gated by min_unique, and threshold is ignored; subpixel=True refines on the aggregate, not on the raw costs.  fill and median work
    unchanged, through scores > 0.  consistency= together with sgm= raises ValueError.  None leaves every bit and every launch as it is.
    sigma= or P2_edge= (None: P1) in the sgm dict: dfe_flow_depth_pair_sgm_guided_f32 / _u8 -- img1 on the output
    region guides P2, which falls to P2_edge across its edges; sigma is in the frame's own units (bytes times scale for uint8 frames)."""
    median = _median_arg(median)
    sgm = _sgm_pick_arg(sgm, "flowDepthPair")
    if sgm is not None and consistency is not None:
        raise ValueError("flowDepthPair: consistency= together with sgm= is not available")
    a, b = _frames(img1, img2, "flowDepthPair")
    C, H, W = a.shape
    flow = torch.empty((2, H, W), dtype=torch.float32, device=a.device)
    scores = torch.empty((H, W), dtype=torch.float32, device=a.device)
    depth = torch.empty_like(scores)
    conf = torch.empty_like(scores)
    ctx = get_ctx(a)
    fx, fy = float(foe[0]), float(foe[1])
    l = lib()
    if sgm is not None:
        P1, P2, paths, min_unique, _, edge = sgm
        name = "dfe_flow_depth_pair_sgm_" + ("" if edge is None else "guided_")     # (sigma, P2_edge behind min_unique: frame 0 guides)
        tail = (P1, P2, paths, int(bool(subpixel)), min_unique) + (edge or ()) + (ptr(flow), ptr(scores), ptr(depth), ptr(conf))
        if a.dtype == torch.uint8:
            rc = getattr(l, name + "u8")(ctx.handle, ptr(a), ptr(b), C, H, W, k, hWin, wWin, fx, fy, float(scale), *tail)
        else:
            rc = getattr(l, name + "f32")(ctx.handle, ptr(a), ptr(b), C, H, W, k, hWin, wWin, fx, fy, *tail)
        ctx.check(rc)
        return _with_fill({"flow": flow, "scores": scores, "depth": depth, "depth_conf": conf}, fill, median, a, k, hWin, wWin, fx, fy)
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
