"""The slice of the un-vendored `sfm2` package the hot path's callers use (next-row N4), with its names:
undistortImage, removeEgoMotion, getEgoMotion / getEgoMotion2 (relative pose R, T by parallel RANSAC on the device; the
correspondences are the library's own corner tracks between the two images -- findCorners, trackPoints --, the caller's tracks, or
samples of the matcher's dense flow), getEpipole (e2 = K T
scaled, radial/radial_opticalflow_data.lua:218-220) and -- not in the reference -- getFOEFromFlow (focus of expansion of a
dense flow field, an estimator of this library for the pure-translation case).
Restated from the call sites (radial/radial_opticalflow_data.lua:24,211-231, depth_estimation_api.lua:139-147,
test_opticalflow.lua:280-284); `sfm2` itself is not in the reference repository, so parity is unpinned."""
import ctypes as C

import torch

from ._lib import TrackerParams, lib
from .context import get_ctx, ptr


def _d(vals, n):
    v = [float(x) for x in (vals.reshape(-1).tolist() if hasattr(vals, "reshape") else vals)]
    if len(v) != n:
        raise ValueError("expected %d numbers, got %d" % (n, len(v)))
    return (C.c_double * n)(*v)


def undistortImage(img, K, distP):
    """sfm2.undistortImage(img, K, distP): img C x H x W FloatTensor, K 3 x 3, distP = (k1, k2, p1, p2, k3)."""
    img = img.contiguous()
    Cc, H, W = img.shape
    out = torch.empty_like(img)
    ctx = get_ctx(img)
    ctx.check(lib().dfe_undistort_image_f32(ctx.handle, ptr(img), Cc, H, W, _d(K, 9), _d(distP, 5), ptr(out)))
    return out


def removeEgoMotion(img, K, R, mode="bilinear", inverse=False):
    """sfm2.removeEgoMotion(img, K, R, 'bilinear') -> warped, mask: the rotation R between the two frames is undone by the
    homography K R K^-1 (inverse=True: R^T); mask is 1 where the warped pixel has a source inside the frame."""
    if mode != "bilinear":
        raise NotImplementedError("removeEgoMotion: the reference uses 'bilinear'")
    img = img.contiguous()
    Cc, H, W = img.shape
    out = torch.empty_like(img)
    mask = torch.empty((H, W), dtype=torch.float32, device=img.device)
    ctx = get_ctx(img)
    ctx.check(lib().dfe_remove_ego_motion_f32(ctx.handle, ptr(img), Cc, H, W, _d(K, 9), _d(R, 9), int(inverse), ptr(out), ptr(mask)))
    return out, mask


def getEpipole(K, T, scale=1.0):
    """e2 = K * T; e2 = e2 / e2[3]; e2 = e2 * scale (radial/radial_opticalflow_data.lua:218-220) -> (x, y)"""
    e = (C.c_double * 2)()
    rc = lib().dfe_epipole(_d(K, 9), _d(T, 3), float(scale), e)
    if rc != 0:
        raise ValueError("getEpipole: translation parallel to the image plane (epipole at infinity)")
    return e[0], e[1]


def getFOEFromFlow(flow, confidences=None, min_flow=0.5, iterations=2):
    """Focus of expansion (x, y) of a dense flow field 2 x H x W (plane 0 = y, plane 1 = x, the layout of processOutput's
    `full`): the point closest to all flow lines, Huber re-weighted `iterations` times.  Also returns the weight sum.  Skipped:
    vectors shorter than min_flow, of non-finite or zero length, and pixels whose confidence is <= 0 or NaN."""
    flow = flow.contiguous()
    _, H, W = flow.shape
    conf = confidences.contiguous() if confidences is not None else None
    out, n = (C.c_double * 2)(), C.c_double()
    ctx = get_ctx(flow)
    ctx.check(lib().dfe_foe_from_flow_f32(ctx.handle, ptr(flow[0]), ptr(flow[1]), ptr(conf) if conf is not None else None, H, W, float(min_flow),
                                          int(iterations), out, C.byref(n)))
    return (out[0], out[1]), n.value


# the .cal files' sfm table (radial/*.cal, version2/rectified_gopro.cal): sfm{max_points=1000, points_min_dist=30, points_quality=1e-4,
# tracker_win_size=21, ransac2_max_dist}; the pyramid depth, step count and thresholds are this library's own
SFM_DEFAULTS = dict(max_points=1000, points_quality=1e-4, points_min_dist=30.0, tracker_win_size=21, tracker_levels=3, tracker_max_iters=30,
                    tracker_eps=0.01, tracker_min_eig=1e-4, tracker_max_err=0.0, ransac2_max_dist=1.0)


def _sfm(calibration, key, given):
    """a keyword that was given wins, then the calibration dict's sfm table (torch7_io.load_calibration), then SFM_DEFAULTS"""
    if given is not None:
        return given
    table = calibration.get("sfm", calibration) if isinstance(calibration, dict) else None
    if isinstance(table, dict) and key in table:
        return table[key]
    return SFM_DEFAULTS.get(key)


def _tracker_params(maxPoints, pointsQuality, pointsMinDistance, winSize, levels, maxIters, eps, minEig, maxErr):
    """the host half of the library's argument checks (the same limits as include/dfe.h), so that a wrong value is refused without a device"""
    p = TrackerParams(int(maxPoints), float(pointsQuality), float(pointsMinDistance), int(winSize), int(levels), int(maxIters), float(eps), float(minEig),
                      float(maxErr))
    if not 1 <= p.max_points <= 4096:
        raise ValueError("maxPoints = %d: 1 .. 4096" % p.max_points)
    if not 0 <= p.quality <= 1:
        raise ValueError("pointsQuality = %g: 0 .. 1" % p.quality)
    if not p.min_dist >= 1:
        raise ValueError("pointsMinDistance = %g: >= 1" % p.min_dist)
    if not (3 <= p.win <= 31 and p.win % 2 == 1):
        raise ValueError("winSize = %d: odd, 3 .. 31" % p.win)
    if not 1 <= p.levels <= 8:
        raise ValueError("levels = %d: 1 .. 8" % p.levels)
    if not 1 <= p.max_iters <= 64:
        raise ValueError("maxIters = %d: 1 .. 64" % p.max_iters)
    if not p.eps >= 0:
        raise ValueError("eps = %g: >= 0" % p.eps)
    return p


def _luminance(img, name):
    """H x W, 1 x H x W or 3 x H x W float tensor -> (contiguous tensor, C, H, W)"""
    if img.dim() == 2:
        img = img.unsqueeze(0)
    if img.dim() != 3 or img.shape[0] not in (1, 3):
        raise ValueError("%s must be H x W, 1 x H x W or 3 x H x W, got %s" % (name, tuple(img.shape)))
    img = img.to(torch.float32).contiguous()
    return img, img.shape[0], img.shape[1], img.shape[2]


def _gray(img, name):
    img, Cc, H, W = _luminance(img, name)
    if Cc == 3:
        y = torch.empty((1, H, W), dtype=torch.float32, device=img.device)
        ctx = get_ctx(img)
        ctx.check(lib().dfe_rgb2y_f32(ctx.handle, ptr(img), H, W, ptr(y)))
        img = y
    return img, H, W


def cornerResponse(img):
    """Smaller eigenvalue of the 3 x 3 structure tensor of central-difference gradients (dfe_corner_response_f32) -> H x W."""
    img, H, W = _gray(img, "img")
    out = torch.empty((H, W), dtype=torch.float32, device=img.device)
    ctx = get_ctx(img)
    ctx.check(lib().dfe_corner_response_f32(ctx.handle, ptr(img), H, W, ptr(out)))
    return out


def selectCorners(resp, maxPoints=None, pointsQuality=None, pointsMinDistance=None, calibration=None):
    """dfe_select_corners_f32 on a response map H x W -> (pts n x 2 = (x, y), responses n), best first."""
    p = _tracker_params(_sfm(calibration, "max_points", maxPoints), _sfm(calibration, "points_quality", pointsQuality),
                        _sfm(calibration, "points_min_dist", pointsMinDistance), 21, 1, 1, 0, 0, 0)
    if resp.dim() != 2:
        raise ValueError("selectCorners: the response map must be H x W, got %s" % (tuple(resp.shape),))
    resp = resp.to(torch.float32).contiguous()
    H, W = resp.shape
    pts = torch.empty((p.max_points, 2), dtype=torch.float32, device=resp.device)
    val = torch.empty((p.max_points,), dtype=torch.float32, device=resp.device)
    n = C.c_int()
    ctx = get_ctx(resp)
    ctx.check(lib().dfe_select_corners_f32(ctx.handle, ptr(resp), H, W, p.quality, p.min_dist, p.max_points, ptr(pts), ptr(val), C.byref(n)))
    return pts[: n.value], val[: n.value]


def findCorners(img, maxPoints=None, pointsQuality=None, pointsMinDistance=None, calibration=None):
    """The corners sfm2 tracks: at most maxPoints points of img (H x W, 1 x H x W or RGB 3 x H x W) whose corner response is at least
    pointsQuality x the frame's largest, pairwise more than pointsMinDistance pixels apart, best first -> n x 2 (x, y).  Defaults: the
    .cal files' sfm table (`calibration` = torch7_io.load_calibration's dict, or SFM_DEFAULTS)."""
    return selectCorners(cornerResponse(img), maxPoints, pointsQuality, pointsMinDistance, calibration)[0]


def pyrDown(img):
    """One pyramid step (dfe_pyr_down_f32): H x W -> (H+1)/2 x (W+1)/2, (1 4 6 4 1)/16 separable, reflected borders."""
    if img.dim() != 2:
        raise ValueError("pyrDown: H x W, got %s" % (tuple(img.shape),))
    img = img.to(torch.float32).contiguous()
    H, W = img.shape
    out = torch.empty(((H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=img.device)
    ctx = get_ctx(img)
    ctx.check(lib().dfe_pyr_down_f32(ctx.handle, ptr(img), H, W, ptr(out)))
    return out


def trackPoints(im1, im2, pts, winSize=None, levels=None, maxIters=None, eps=None, minEig=None, maxErr=None, calibration=None):
    """Pyramidal Lucas-Kanade (dfe_track_points_lk_f32): pts N x 2 (x, y) in im1 -> (pts2 N x 2, status N int32 (1 = tracked), err N).
    Lost points keep their position and err = 0."""
    p = _tracker_params(1, 0, 1, _sfm(calibration, "tracker_win_size", winSize), _sfm(calibration, "tracker_levels", levels),
                        _sfm(calibration, "tracker_max_iters", maxIters), _sfm(calibration, "tracker_eps", eps), _sfm(calibration, "tracker_min_eig", minEig),
                        _sfm(calibration, "tracker_max_err", maxErr))
    if pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError("trackPoints: pts must be N x 2, got %s" % (tuple(pts.shape),))
    a, H, W = _gray(im1, "im1")
    b, H2, W2 = _gray(im2, "im2")
    if (H, W) != (H2, W2):
        raise ValueError("trackPoints: the frames differ in size, %d x %d and %d x %d" % (H, W, H2, W2))
    pts = pts.to(torch.float32).contiguous()
    N = pts.shape[0]
    out = torch.empty_like(pts)
    status = torch.empty((N,), dtype=torch.int32, device=pts.device)
    err = torch.empty((N,), dtype=torch.float32, device=pts.device)
    ctx = get_ctx(a)
    ctx.check(lib().dfe_track_points_lk_f32(ctx.handle, ptr(a), ptr(b), H, W, ptr(pts), N, C.byref(p), ptr(out), ptr(status), ptr(err)))
    return out, status, err


def getEgoMotion2(K, flow=None, confidences=None, pts1=None, pts2=None, weights=None, maxPoints=None, ransacMaxDist=None, iterations=512, seed=0, im1=None,
                  im2=None, pointsQuality=None, pointsMinDistance=None, trackerWinSize=None, trackerLevels=None, trackerMaxIters=None, trackerEps=None,
                  trackerMinEig=None, trackerMaxErr=None, calibration=None, returnTracks=False):
    """sfm2.getEgoMotion2{im1, im2, K, maxPoints, pointsQuality, ransacMaxDist, pointsMinDistance} -> R, T, nFound, nInliers, fundmat
    (radial/radial_opticalflow_data.lua:211-217; getEgoMotion: depth_estimation_api.lua:141).  Three sources of correspondences:
    `im1` / `im2` (H x W, 1 x H x W or RGB 3 x H x W: the reference's way -- corners of im1 by findCorners' rule, tracked into im2 by
    trackPoints' rule, one library call; nFound = corners tracked; defaults from the .cal files' sfm table through `calibration` =
    torch7_io.load_calibration's dict, else SFM_DEFAULTS; returnTracks=True appends (pts1, pts2, status)), or `flow` (2 x H x W, plane 0 = y,
    1 = x: the matcher's dense flow from frame 1 to frame 2, sampled on a regular grid of at most maxPoints (default 400) points,
    `confidences` <= 0 or non-finite flow skipped) or `pts1` / `pts2` (N x 2 (x, y) pixel positions, `weights` <= 0 skipped).  The RANSAC
    draws are taken among the valid correspondences only, however few of the N they are.  Returns R (3 x 3 float64 tensor), T (3,
    |T| = 1), nFound, nInliers, fundmat (3 x 3) with x2 ~ R x1 + T: getEpipole(K, T) is the FOE in the current frame and
    removeEgoMotion(prev, K, R, inverse=True) takes the rotation out of the previous frame."""
    R, T, F = (C.c_double * 9)(), (C.c_double * 3)(), (C.c_double * 9)()
    nf, ni = C.c_int(), C.c_int()
    tracks = None
    ransacMaxDist = _sfm(calibration, "ransac2_max_dist", ransacMaxDist)
    if im1 is not None or im2 is not None:
        if im1 is None or im2 is None or flow is not None or pts1 is not None or pts2 is not None:
            raise ValueError("getEgoMotion2: give im1 and im2, or the dense flow, or two point lists")
        p = _tracker_params(_sfm(calibration, "max_points", maxPoints), _sfm(calibration, "points_quality", pointsQuality),
                            _sfm(calibration, "points_min_dist", pointsMinDistance), _sfm(calibration, "tracker_win_size", trackerWinSize),
                            _sfm(calibration, "tracker_levels", trackerLevels), _sfm(calibration, "tracker_max_iters", trackerMaxIters),
                            _sfm(calibration, "tracker_eps", trackerEps), _sfm(calibration, "tracker_min_eig", trackerMinEig),
                            _sfm(calibration, "tracker_max_err", trackerMaxErr))
        a, Cc, H, W = _luminance(im1, "im1")
        b, Cb, Hb, Wb = _luminance(im2, "im2")
        if (Cc, H, W) != (Cb, Hb, Wb):
            raise ValueError("getEgoMotion2: the frames differ in shape, %s and %s" % (tuple(a.shape), tuple(b.shape)))
        o1 = torch.zeros((p.max_points, 2), dtype=torch.float32, device=a.device)
        o2 = torch.zeros((p.max_points, 2), dtype=torch.float32, device=a.device)
        st = torch.zeros((p.max_points,), dtype=torch.int32, device=a.device)
        nc = C.c_int()
        ctx = get_ctx(a)
        ctx.check(lib().dfe_ego_motion_from_images_f32(ctx.handle, ptr(a), ptr(b), Cc, H, W, _d(K, 9), C.byref(p), float(ransacMaxDist), int(iterations), int(seed), R,
                                                       T, C.byref(nf), C.byref(ni), F, ptr(o1), ptr(o2), ptr(st), C.byref(nc)))
        tracks = (o1[: nc.value], o2[: nc.value], st[: nc.value])
    elif flow is not None:
        flow = flow.contiguous()
        _, H, W = flow.shape
        conf = confidences.contiguous() if confidences is not None else None
        ctx = get_ctx(flow)
        ctx.check(lib().dfe_ego_motion_from_flow_f32(ctx.handle, ptr(flow[0]), ptr(flow[1]), ptr(conf) if conf is not None else None, H, W, _d(K, 9),
                                                     int(400 if maxPoints is None else maxPoints), float(ransacMaxDist), int(iterations), int(seed), R, T, C.byref(nf),
                                                     C.byref(ni), F))
    else:
        if pts1 is None or pts2 is None:
            raise ValueError("getEgoMotion2: give the dense flow or two point lists")
        pts1, pts2 = pts1.to(torch.float32).contiguous(), pts2.to(torch.float32).contiguous()
        if pts1.dim() != 2 or pts1.shape[1] != 2 or tuple(pts1.shape) != tuple(pts2.shape):
            raise ValueError("getEgoMotion2: pts1 / pts2 must both be N x 2, got %s / %s" % (tuple(pts1.shape), tuple(pts2.shape)))
        w = weights.to(torch.float32).contiguous() if weights is not None else None
        ctx = get_ctx(pts1)
        ctx.check(lib().dfe_ego_motion_from_points_f32(ctx.handle, ptr(pts1), ptr(pts2), ptr(w) if w is not None else None, pts1.shape[0], _d(K, 9),
                                                       float(ransacMaxDist), int(iterations), int(seed), R, T, C.byref(ni), F))
        nf.value = int((w > 0).sum()) if w is not None else pts1.shape[0]
    out = (torch.tensor(R[:], dtype=torch.float64).reshape(3, 3), torch.tensor(T[:], dtype=torch.float64), nf.value, ni.value,
           torch.tensor(F[:], dtype=torch.float64).reshape(3, 3))
    return out + tracks if returnTracks and tracks is not None else out


def getEgoMotion(im1, im2=None, K=None, maxPoints=None, **kw):
    """sfm2.getEgoMotion(im1, im2, K, maxPoints) -> R, T, nFound, nInliers (depth_estimation_api.lua:141, test_opticalflow.lua:282).  Also
    takes the reference's table style, as one dict or as keywords: getEgoMotion{im1=, im2=, K=, maxPoints=, pointsQuality=,
    pointsMinDistance=, ransacMaxDist=, ...}; the remaining keywords are getEgoMotion2's."""
    if isinstance(im1, dict):
        kw = dict(im1, **kw)
        im1, im2, K, maxPoints = kw.pop("im1"), kw.pop("im2"), kw.pop("K"), kw.pop("maxPoints", maxPoints)
    if im2 is None or K is None:
        raise ValueError("getEgoMotion: im1, im2 and K are needed")
    return getEgoMotion2(K, im1=im1, im2=im2, maxPoints=maxPoints, **kw)[:4]
