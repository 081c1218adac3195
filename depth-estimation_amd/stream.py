"""Video to depth in one session: the reference's only public entry point, nextFrameDepth() of depth_estimation_api.lua:134-198 (the
drone's C++ calls it once per camera frame, ardrone/ardrone_api.cpp:77-84; test_opticalflow.lua:276-367 runs the same loop offline), over
the library's stream object (include/dfe.h: dfe_stream_*), and image.scale (imageScale), the one stage of that loop that had no kernel.

    api = DepthEstimationAPI(geometry, filter, K, distP)      # what the script's top level sets up (:25-72)
    for frame in camera:
        r = api.nextFrameDepth(frame)                          # None for the first frame, then (im_scaled, xflow, mask)  (:196)
"""
import ctypes as C

import torch

from ._lib import DfeError, FilterLayer, StreamParams, StreamPost, StreamPostOut, lib
from .context import get_ctx, ptr
from .opticalflow_model import _g
from .sfm2 import _d, _sfm, _tracker_params

RECTIFY = {"features": 0, "image": 1}


def imageScale(src, width, height):
    """image.scale(src, width, height), bilinear (depth_estimation_api.lua:71,144): src C x H x W or H x W, float32 or uint8 (uint8: the
    byte values as floats) -> float32 C x height x width.  The definition is the library's own (dfe_image_scale_f32 in include/dfe.h):
    pixel centres at half-integers, edge clamp, no anti-aliasing."""
    squeeze = src.dim() == 2
    if squeeze:
        src = src.unsqueeze(0)
    if src.dim() != 3 or src.dtype not in (torch.float32, torch.uint8):
        raise TypeError("imageScale: a float32 or uint8 C x H x W (or H x W) tensor expected")
    src = src.contiguous()
    Cc, H, W = src.shape
    out = torch.empty((Cc, int(height), int(width)), dtype=torch.float32, device=src.device)
    ctx = get_ctx(src)
    if src.dtype == torch.uint8:
        ctx.check(lib().dfe_image_scale_u8(ctx.handle, ptr(src), 1.0, Cc, H, W, int(height), int(width), ptr(out)))
    else:
        ctx.check(lib().dfe_image_scale_f32(ctx.handle, ptr(src), Cc, H, W, int(height), int(width), ptr(out)))
    return out[0] if squeeze else out


def stream_params(geometry, filter, K, distP, C_, Hsrc, Wsrc, rectify="features", threshold=None, fixMaskOffset=False, minInlierRatio=0.2, calibration=None,
                  maxPoints=None, pointsQuality=None, pointsMinDistance=None, trackerWinSize=None, trackerLevels=None, trackerMaxIters=None, trackerEps=None,
                  trackerMinEig=None, trackerMaxErr=None, ransacMaxDist=None, iterations=512, seed=0):
    """dfe_stream_params for a geometry, a getFilter module (or None: raw frames are the features) and a camera -> (struct, keepalive).
    The sfm keywords are getEgoMotion2's, with the same defaults (the `calibration` dict's sfm table, then sfm2.SFM_DEFAULTS)."""
    from .multiscale import filter_layers_array

    if rectify not in RECTIFY:
        raise ValueError("rectify = %r: 'features' or 'image'" % (rectify,))
    p = StreamParams()
    p.C, p.Hsrc, p.Wsrc, p.hImg, p.wImg = int(C_), int(Hsrc), int(Wsrc), int(_g(geometry, "hImg")), int(_g(geometry, "wImg"))
    p.K = _d(K, 9)
    p.has_dist = 0 if distP is None else 1
    if distP is not None:
        p.dist = _d(distP, 5)
    keep = None
    if filter is not None:
        arr, nl, keep = filter_layers_array([filter])
        p.layers, p.nlayers = C.cast(arr, C.POINTER(FilterLayer)), nl
        keep = (arr, keep)
    p.maxh, p.maxw = int(_g(geometry, "maxh")), int(_g(geometry, "maxw"))
    method = _g(geometry, "output_extraction_method", "max")
    if method not in ("max", "mean"):
        raise ValueError("output_extraction_method = %r: 'max' or 'mean'" % (method,))
    p.extraction = 2 if method == "mean" else (1 if threshold is not None else 0)
    p.threshold = float(threshold or 0.0)
    p.rectify, p.fix_mask_offset = RECTIFY[rectify], int(bool(fixMaskOffset))
    p.tracker = _tracker_params(_sfm(calibration, "max_points", maxPoints), _sfm(calibration, "points_quality", pointsQuality),
                                _sfm(calibration, "points_min_dist", pointsMinDistance), _sfm(calibration, "tracker_win_size", trackerWinSize),
                                _sfm(calibration, "tracker_levels", trackerLevels), _sfm(calibration, "tracker_max_iters", trackerMaxIters),
                                _sfm(calibration, "tracker_eps", trackerEps), _sfm(calibration, "tracker_min_eig", trackerMinEig),
                                _sfm(calibration, "tracker_max_err", trackerMaxErr))
    p.ransac_max_dist = float(_sfm(calibration, "ransac2_max_dist", ransacMaxDist))
    p.iterations, p.seed, p.min_inlier_ratio = int(iterations), int(seed), float(minInlierRatio)
    return p, keep


def stream_shapes(params):
    """dfe_stream_shapes (host only) -> dict(Hf, Wf, H1, W1, oy, ox, ix, iy)"""
    v = [C.c_int() for _ in range(8)]
    rc = lib().dfe_stream_shapes(C.byref(params), *[C.byref(x) for x in v])
    if rc != 0:
        raise DfeError(rc, lib().dfe_last_error(None).decode())
    return dict(zip(("Hf", "Wf", "H1", "W1", "oy", "ox", "ix", "iy"), (x.value for x in v)))


POST_KEYS = ("consistency", "fill", "median", "temporal")
POST_TEMPORAL_KEYS = ("tol", "wmax", "decay", "gain", "bias", "key_channel", "splat", "ztol", "quant", "min_cover")


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def stream_post(post):
    """dfe_stream_post (include/dfe.h) from DepthEstimationAPI's post= dict: consistency=tol (None / 0: off), fill=True | levels (False /
    None: off), median=k | (k, sigma) (None: off; sigma <= 0: unguided), temporal=dict(tol=, wmax=8.0, decay=1.0, gain=None, bias=None,
    splat="nearest", ztol=None, quant=1024.0, min_cover=0.25): TemporalFilter's keywords for the one depth channel (key_channel, if given,
    is 0).  ValueError for what the library would refuse."""
    from .fields import _check_decay, _check_splat, _check_tol_wmax, _host_floats

    if not isinstance(post, dict) or set(post) - set(POST_KEYS):
        raise ValueError("post=%r: a dict with keys of %s expected" % (post, POST_KEYS))
    o = StreamPost()
    tol = post.get("consistency")
    if tol is not None:
        tol = float(tol)
        if not tol >= 0.0:
            raise ValueError("post: consistency=%r must be >= 0" % (tol,))
        o.consistency_tol = tol
    fill = post.get("fill")
    if not (fill is None or isinstance(fill, bool) or (_is_int(fill) and fill >= 0)):
        raise ValueError("post: fill=%r: True, False or a number of levels >= 0" % (fill,))
    if fill is not None and fill is not False:
        o.fill, o.fill_levels = 1, 0 if fill is True else int(fill)
    median = post.get("median")
    if median is not None:
        k, sigma = median if isinstance(median, (tuple, list)) and len(median) == 2 else (median, 0.0)
        if not _is_int(k) or not 1 <= k <= 15 or k % 2 == 0:
            raise ValueError("post: median=%r: k or (k, sigma) with k odd, 1 .. 15" % (median,))
        o.median_k, o.median_sigma = k, float(sigma)
    t = post.get("temporal")
    if t is not None:
        if not isinstance(t, dict) or "tol" not in t or set(t) - set(POST_TEMPORAL_KEYS):
            raise ValueError("post: temporal=%r: a dict with tol and keys of %s expected" % (t, POST_TEMPORAL_KEYS))
        if t.get("key_channel", 0) != 0:
            raise ValueError("post: temporal key_channel=%r: the session's filter has one channel, depth (0)" % (t["key_channel"],))
        splat = t.get("splat", "nearest")
        if splat not in ("nearest", "bilinear"):
            raise ValueError("post: temporal splat=%r: \"nearest\" or \"bilinear\"" % (splat,))
        o.temporal = 1
        o.t_tol, o.t_wmax = _check_tol_wmax("post: temporal", t["tol"], t.get("wmax", 8.0))
        o.t_decay = _check_decay("post: temporal", t.get("decay", 1.0))
        for what, has, val in (("gain", "t_has_gain", "t_gain"), ("bias", "t_has_bias", "t_bias")):
            v = t.get(what)
            if v is not None:
                v = _host_floats("post: temporal", what, v if isinstance(v, (tuple, list)) else (v,), 1)
                setattr(o, has, 1)
                setattr(o, val, v[0])
        o.t_splat = 1 if splat == "bilinear" else 0
        ztol = t.get("ztol")
        o.t_ztol, o.t_quant, o.t_min_cover = (o.t_tol if ztol is None else float(ztol)), float(t.get("quant", 1024.0)), float(t.get("min_cover", 0.25))
        if o.t_splat:
            _check_splat("post: temporal", o.t_ztol, o.t_quant, o.t_min_cover)
    return o


class DepthEstimationAPI:
    """depth_estimation_api.lua as an object.  geometry: hImg, wImg, maxh, maxw, output_extraction_method ('max' / 'mean'; the script sets
    'mean', :31); filter: the getFilter module (loaded.filter, :28) or None for raw frames; K 3 x 3 and distP (k1, k2, p1, p2, k3) of the
    camera frame (:32-47; distP None: no undistortion, the gopro branch of test_opticalflow.lua:279); rectify 'features' (the script, :147)
    or 'image' (test_opticalflow.lua:284); threshold: processOutput's, for 'max' (the script passes nil, :168); fixMaskOffset: paste the
    mask at the features' centre, not one pixel up and left of it as the script does (:177-179); minInlierRatio: the bad-image gate
    (:159); u8Scale: what a uint8 frame is multiplied by (1 / 255: image.load's range); calibration=, and the remaining keywords: the
    tracker's and the RANSAC's, as sfm2.getEgoMotion2 takes them.  The stream is made when the first frame shows the camera's size.
    temporal: None, or dict(tol=, wmax=, decay=, gain=, bias=, key_channel=, splat=, ztol=, quant=, min_cover=), TemporalFilter's own
    keywords passed through (temporal.py; not in the reference; splat="bilinear": the sub-pixel splat), for a filter that fuses the
    depth of every push that was given imu_tx with what the earlier ones left (nextFrameDepth).
    post: None, or dict(consistency=tol, fill=True | levels, median=k | (k, sigma), temporal=dict(tol=, wmax=, decay=, gain=, bias=, splat=,
    ztol=, quant=, min_cover=)): the post-processing chain inside the stream object (include/dfe.h: dfe_stream_create_post,
    dfe_stream_push_post_*; stream_post above) -- the forward-backward check, hole filling, the guided weighted median and the temporal
    filter with its state on the device, without Python between the stages.  post["temporal"] and temporal= exclude each other."""

    def __init__(self, geometry, filter, K, distP=None, calibration=None, rectify="features", u8Scale=1.0 / 255.0, temporal=None, post=None, **sfm):
        self.geometry, self.filter, self.K, self.distP = geometry, filter, K, distP
        self.kw = dict(sfm, calibration=calibration, rectify=rectify)
        self.u8Scale = float(u8Scale)
        self.handle, self.ctx, self.shape, self.params, self._keep = None, None, None, None, None
        self.last = {}
        self.temporal = None
        self.post = None if post is None else stream_post(post)
        if self.post is not None and self.post.temporal and temporal is not None:
            raise ValueError("DepthEstimationAPI: post[\"temporal\"] and temporal= are two forms of one filter: give one")
        if temporal is not None:
            from .temporal import TemporalFilter

            self.temporal = TemporalFilter(**temporal)

    def _open(self, frame):
        Cc, H, W = frame.shape
        self.params, self._keep = stream_params(self.geometry, self.filter, self.K, self.distP, Cc, H, W, **self.kw)
        self.ctx = get_ctx(frame)
        h = C.c_void_p()
        if self.post is None:
            self.ctx.check(lib().dfe_stream_create(self.ctx.handle, C.byref(self.params), C.byref(h)))
        else:
            self.ctx.check(lib().dfe_stream_create_post(self.ctx.handle, C.byref(self.params), C.byref(self.post), C.byref(h)))
        self.handle, self.shape = h, (Cc, H, W)

    def nextFrameDepth(self, frame, imu_tx=None):
        """frame: float32 or uint8 C x H x W device tensor -> None for the first frame, else (im_scaled, xflow, mask) (:196).  self.last
        holds status (0 first frame, 1 result, 2 bad image: zero flow and mask), im_scaled, yflow, R, T, nFound, nInliers, and with imu_tx
        depth / depth_conf (ARdroneAPI::computeDepthMapFromFlow on the x-flow and the mask).  With temporal= a result that was given imu_tx
        also has depth_fused, depth_fused_weight, depth_fused_flag: the filter's push of depth[None], depth_conf and the flow planes with
        rectify = (K_small, R), K_small = diag(wImg / Wsrc, hImg / Hsrc, 1) K; the first frame, a bad image (no usable pose: the grid cannot
        be carried), a push without imu_tx (no depth) and reset() reset the filter.  With post= a result also has flow_post [2][h][w],
        weight_post, consistent (consistency on), with imu_tx depth_post / depth_post_conf, and with post["temporal"] (imu_tx required:
        ValueError without) depth_fused, depth_fused_weight, depth_fused_flag, all computed inside the stream."""
        if frame.dim() != 3 or frame.dtype not in (torch.float32, torch.uint8):
            raise TypeError("nextFrameDepth: a float32 or uint8 C x H x W tensor expected")
        frame = frame.contiguous()
        if self.handle is None:
            self._open(frame)
        if tuple(frame.shape) != self.shape:
            raise DfeError(-2, "nextFrameDepth: frame %s, the stream was opened for %s" % (tuple(frame.shape), self.shape))
        if get_ctx(frame) is not self.ctx:
            raise DfeError(-1, "nextFrameDepth: the frame is on another device or stream than the first one")
        if self.post is not None and self.post.temporal and imu_tx is None:
            raise ValueError("nextFrameDepth: post[\"temporal\"] fuses depth: imu_tx is required")
        p, dev = self.params, frame.device
        ims = torch.empty((p.C, p.hImg, p.wImg), dtype=torch.float32, device=dev)
        flow = torch.empty((2, p.hImg, p.wImg), dtype=torch.float32, device=dev)
        mask = torch.empty((p.hImg, p.wImg), dtype=torch.float32, device=dev)
        depth = torch.empty_like(mask) if imu_tx is not None else None
        dconf = torch.empty_like(mask) if imu_tx is not None else None
        R, T, nf, ni, st = (C.c_double * 9)(), (C.c_double * 3)(), C.c_int(), C.c_int(), C.c_int()
        head = (float(imu_tx or 0.0), ptr(ims), ptr(flow), ptr(mask), ptr(depth), ptr(dconf))
        tail = (R, T, C.byref(nf), C.byref(ni), C.byref(st))
        posted = {}
        if self.post is not None:
            posted = dict(flow_post=torch.empty_like(flow), weight_post=torch.empty_like(mask))
            if self.post.consistency_tol > 0:
                posted["consistent"] = torch.empty_like(mask)
            if imu_tx is not None:
                posted.update(depth_post=torch.empty_like(mask), depth_post_conf=torch.empty_like(mask))
            if self.post.temporal:
                posted.update(depth_fused=torch.empty_like(mask), depth_fused_weight=torch.empty_like(mask), depth_fused_flag=torch.empty_like(mask))
            po = StreamPostOut()
            for k, t in posted.items():
                setattr(po, {"depth_fused_weight": "fused_weight", "depth_fused_flag": "fused_flag"}.get(k, k), ptr(t))
            head += (C.byref(po),)
            push_u8, push_f32 = lib().dfe_stream_push_post_u8, lib().dfe_stream_push_post_f32
        else:
            push_u8, push_f32 = lib().dfe_stream_push_u8, lib().dfe_stream_push_f32
        if frame.dtype == torch.uint8:
            self.ctx.check(push_u8(self.handle, ptr(frame), self.u8Scale, *head, *tail))
        else:
            self.ctx.check(push_f32(self.handle, ptr(frame), *head, *tail))
        self.last = dict(status=st.value, im_scaled=ims, nFound=nf.value, nInliers=ni.value)
        if self.temporal is not None and (st.value != 1 or imu_tx is None):   # nothing to carry the state with: it starts over
            self.temporal.reset()
        if st.value == 0:
            return None
        self.last.update(yflow=flow[0], xflow=flow[1], mask=mask, R=torch.tensor(R[:], dtype=torch.float64).reshape(3, 3), T=torch.tensor(T[:], dtype=torch.float64))
        self.last.update(posted)
        if imu_tx is not None:
            self.last.update(depth=depth, depth_conf=dconf)
            if self.temporal is not None and st.value == 1:
                fused, weight, flag = self.temporal.push(depth[None], dconf, flow, rectify=(self.K_small(), self.last["R"]))
                self.last.update(depth_fused=fused[0], depth_fused_weight=weight, depth_fused_flag=flag)
        return ims, flow[1], mask

    def K_small(self):
        """diag(wImg / Wsrc, hImg / Hsrc, 1) K as a float64 3 x 3 tensor: the camera matrix at the session's working size (include/dfe.h)"""
        p = self.params
        k = torch.tensor(list(p.K), dtype=torch.float64).reshape(3, 3).clone()
        k[0] *= float(p.wImg) / float(p.Wsrc)
        k[1] *= float(p.hImg) / float(p.Hsrc)
        return k

    def reset(self):
        """forget the previous frame: the next nextFrameDepth returns None again"""
        if self.handle is not None:
            self.ctx.check(lib().dfe_stream_reset(self.handle))
        if self.temporal is not None:
            self.temporal.reset()
        self.last = {}

    def close(self):
        if self.handle is not None:
            lib().dfe_stream_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            if self.ctx is not None and self.ctx.handle:   # (a stream must go before its ctx)
                self.close()
        except Exception:
            pass
