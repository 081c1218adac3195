"""GPU suite (-m gpu), part 12: the stream layer -- dfe_image_scale_f32 / _u8 against the float64 reference written from the definition
(tests/stream_ref64.py), dfe_mask_paste_mul_f32 against numpy, and the stream object (dfe_stream_*: nextFrameDepth() of
depth_estimation_api.lua:134-198) against the composition of the public ops it replaces, bit for bit, through the first frame, a result,
a second result that needs the right frame kept, the bad-image gate and a reset -- at 240 x 320 frames with square layers and windows, and
at an asymmetric case with odd plane sizes, other plane counts and other stack depths.  Outputs are written into buffers pre-filled with -7
that are 64 elements longer than the result: the tail must keep its -7.  Every figure a test bounds is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import stream_ref64 as sr
from tests import tracker_ref64 as tr
from tests.egomotion_cases import ARDRONE_DIST

pytestmark = pytest.mark.gpu

FILL, TAIL = -7.0, 64
E_ARG, E_SHAPE = -1, -2                                           # DFE_E_ARG, DFE_E_SHAPE (include/dfe.h)


def T(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def guarded(n, cuda):
    return torch.full((n + TAIL,), FILL, device=cuda, dtype=torch.float32)


def unguard(buf, shape, what, written=True):
    b, n = buf.cpu().numpy(), int(np.prod(shape))
    assert (b[n:] == FILL).all(), "%s: wrote behind the output" % what
    if written:
        assert not (b[:n] == np.float32(FILL)).any(), "%s: left elements unwritten" % what
    return b[:n].reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------- 1. scale
def scale(dfe, cuda, img, Hd, Wd, u8_scale=None):
    Cc, Hs, Ws = img.shape
    ctx, out, src = dfe.get_ctx(0), guarded(Cc * Hd * Wd, cuda), T(img, cuda)   # (src stays alive until the result has been copied back)
    if img.dtype == np.uint8:
        ctx.check(dfe.lib().dfe_image_scale_u8(ctx.handle, src.data_ptr(), u8_scale, Cc, Hs, Ws, Hd, Wd, out.data_ptr()))
    else:
        ctx.check(dfe.lib().dfe_image_scale_f32(ctx.handle, src.data_ptr(), Cc, Hs, Ws, Hd, Wd, out.data_ptr()))
    return unguard(out, (Cc, Hd, Wd), "scale")


SCALE_CASES = [((1, 1), (1, 1)), ((1, 1), (4, 6)), ((1, 7), (1, 3)), ((7, 1), (2, 1)), ((37, 53), (23, 71)), ((23, 71), (37, 53)), ((67, 129), (33, 64)),
               ((240, 320), (120, 160))]


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("src,dst", SCALE_CASES, ids=["%dx%d->%dx%d" % (s + d) for s, d in SCALE_CASES])
def test_scale_against_float64(dfe, cuda, Cc, src, dst):
    """|out - scale64| <= 2^-20 x max |in|: at most seven fp32 roundings of values no larger than 2 max |in|, contracted or not.  The same
    frame as bytes with scale 1 / 255, against the reference fed float32(src) x float32(1 / 255): the same bound on those values."""
    rng = np.random.default_rng(src[0] * 977 + src[1] + Cc)
    img = (rng.random((Cc,) + src) * 255).astype(np.float32)
    got, bound = scale(dfe, cuda, img, *dst), 2.0 ** -20 * np.abs(img).max()
    err = np.abs(got - sr.scale64(img, *dst)).max()
    print("scale %s C=%d: max |out - scale64| = %.3e (bound %.3e)" % ((src, dst), Cc, err, bound))
    assert err <= bound
    assert np.array_equal(dfe.imageScale(T(img, cuda), dst[1], dst[0]).cpu().numpy(), got)
    b = rng.integers(0, 256, (Cc,) + src).astype(np.uint8)
    conv = b.astype(np.float32) * np.float32(1.0 / 255.0)
    got8, bound8 = scale(dfe, cuda, b, *dst, u8_scale=1.0 / 255.0), 2.0 ** -20 * np.abs(conv).max()
    err8 = np.abs(got8 - sr.scale64(conv, *dst)).max()
    print("scale %s C=%d, bytes / 255: max |out - scale64| = %.3e (bound %.3e)" % ((src, dst), Cc, err8, bound8))
    assert err8 <= bound8


def test_scale_exact_cases(dfe, cuda):
    """Equal sizes give a bit copy (negative zeros, infinities and a NaN included); (64, 130) -> (32, 65) on integer frames 0..255 is the
    2 x 2 mean bit for bit; bytes with scale 1 equal the f32 call on the same values bit for bit."""
    rng = np.random.default_rng(7)
    img = ((rng.random((3, 37, 53)) - 0.5) * 255).astype(np.float32)
    img[0, 0, :4] = (-0.0, np.inf, -np.inf, np.nan)
    ctx, out, src = dfe.get_ctx(0), guarded(img.size, cuda), T(img, cuda)
    ctx.check(dfe.lib().dfe_image_scale_f32(ctx.handle, src.data_ptr(), 3, 37, 53, 37, 53, out.data_ptr()))
    got = out.cpu().numpy()
    assert (got[img.size:] == FILL).all() and np.array_equal(got[: img.size].view(np.uint32), img.reshape(-1).view(np.uint32))
    ints = rng.integers(0, 256, (3, 64, 130)).astype(np.uint8)
    f = ints.astype(np.float32)
    mean = (f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2]) / np.float32(4)
    assert np.array_equal(scale(dfe, cuda, f, 32, 65), mean)
    for dst in ((32, 65), (23, 71), (64, 130), (100, 131)):
        assert np.array_equal(scale(dfe, cuda, ints, *dst, u8_scale=1.0), scale(dfe, cuda, f, *dst)), dst


def test_scale_argument_errors(dfe, cuda):
    ctx, buf = dfe.get_ctx(0), guarded(64, cuda)
    for Hs, Ws, Hd, Wd in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (32769, 1, 1, 1), (1, 32769, 1, 1), (1, 1, 32769, 1), (1, 1, 1, 32769)):
        assert dfe.lib().dfe_image_scale_f32(ctx.handle, buf.data_ptr(), 1, Hs, Ws, Hd, Wd, buf.data_ptr()) == E_ARG
        assert dfe.lib().dfe_image_scale_u8(ctx.handle, buf.data_ptr(), 1.0, 1, Hs, Ws, Hd, Wd, buf.data_ptr()) == E_ARG
    assert dfe.lib().dfe_image_scale_f32(ctx.handle, buf.data_ptr(), 0, 4, 4, 4, 4, buf.data_ptr()) == E_ARG
    assert dfe.lib().dfe_image_scale_f32(ctx.handle, None, 1, 4, 4, 4, 4, buf.data_ptr()) == E_ARG
    assert (buf.cpu().numpy() == FILL).all()


# ---------------------------------------------------------------------------------------------------------------------- 2. paste
PASTE_CASES = [((1, 1), (3, 3), (0, 0)), ((1, 1), (3, 3), (0, 2)), ((1, 1), (3, 3), (2, 0)), ((1, 1), (3, 3), (2, 2)), ((1, 1), (3, 3), (1, 1)),
               ((112, 152), (120, 160), (3, 3)), ((112, 152), (120, 160), (4, 4))]


@pytest.mark.parametrize("msz,fsz,off", PASTE_CASES, ids=["%dx%d in %dx%d at %d,%d" % (m + f + o) for m, f, o in PASTE_CASES])
def test_mask_paste_mul_against_numpy(dfe, cuda, msz, fsz, off):
    rng = np.random.default_rng(msz[0] + fsz[1] + 10 * off[0] + off[1])
    mask = (rng.random(msz) > 0.3).astype(np.float32) if msz != (1, 1) else np.ones(msz, np.float32)
    conf = (rng.random(fsz).astype(np.float32) + np.float32(0.5))
    ctx, out, m, c = dfe.get_ctx(0), guarded(fsz[0] * fsz[1], cuda), T(mask, cuda), T(conf, cuda)
    ctx.check(dfe.lib().dfe_mask_paste_mul_f32(ctx.handle, m.data_ptr(), msz[0], msz[1], c.data_ptr(), fsz[0], fsz[1], off[0], off[1], out.data_ptr()))
    got, want = unguard(out, fsz, "paste"), sr.paste_mul(mask, conf, *off)
    assert want.any() and np.array_equal(got, want)


def test_mask_paste_mul_region_leaving_the_frame(dfe, cuda):
    ctx, out, m, c = dfe.get_ctx(0), guarded(9, cuda), T(np.ones((2, 2), np.float32), cuda), T(np.ones((3, 3), np.float32), cuda)
    for oy, ox in ((2, 0), (0, 2), (-1, 0), (0, -1), (3, 3), (2 ** 31 - 1, 0)):
        assert dfe.lib().dfe_mask_paste_mul_f32(ctx.handle, m.data_ptr(), 2, 2, c.data_ptr(), 3, 3, oy, ox, out.data_ptr()) == E_ARG
    assert dfe.lib().dfe_mask_paste_mul_f32(ctx.handle, m.data_ptr(), 4, 2, c.data_ptr(), 3, 3, 0, 0, out.data_ptr()) == E_ARG
    assert (out.cpu().numpy() == FILL).all()
    ctx.check(dfe.lib().dfe_mask_paste_mul_f32(ctx.handle, m.data_ptr(), 2, 2, c.data_ptr(), 3, 3, 1, 1, out.data_ptr()))
    assert np.array_equal(unguard(out, (3, 3), "paste"), sr.paste_mul(np.ones((2, 2)), np.ones((3, 3)), 1, 1))


# --------------------------------------------------------------------------------------------------------------------- 3. stream
LAYERS = [(3, 5, 5, 4), (4, 5, 5, 4)]
GAINS = (0.9, 1.0, 1.1)                                           # the per-channel gains of test_gpu_tracker.py's RGB case
_shared = {}


def frames(cuda, size=(240, 320), planes=3):
    """(im0, im1, flat, K): C x H x W device tensors of the two-view pair of that size and its planted K; made once per size and plane
    count.  Three planes: the luminance pair times the per-channel GAINS; one plane: the pair as two_view_pair gives it."""
    key = ("frames", tuple(size), planes)
    if key not in _shared:
        tv = tr.two_view_pair(*size)
        w = torch.tensor(GAINS if planes == 3 else (1.0,), device=cuda).reshape(planes, 1, 1)
        im0, im1 = (T(tv["im0"], cuda).unsqueeze(0) * w).contiguous(), (T(tv["im1"], cuda).unsqueeze(0) * w).contiguous()
        _shared[key] = (im0, im1, torch.full_like(im0, 100.0), tv["K"])
    return _shared[key]


def sfm_kw(**over):
    q = tr.ROUTE
    kw = dict(maxPoints=q["max_points"], pointsQuality=q["quality"], pointsMinDistance=q["min_dist"], trackerWinSize=q["win"], trackerLevels=q["levels"],
              trackerMaxIters=q["max_iters"], trackerEps=q["eps"], trackerMinEig=q["min_eig"], ransacMaxDist=q["ransac"], iterations=q["iterations"], seed=q["seed"])
    kw.update(over)
    return kw


def make_filter(dfe, cuda, gain=1.0 / 128, layers=LAYERS, peak=10.0):
    """getFilter with seeded weights; the first layer is scaled down so that frames of 0..255 do not saturate its tanh, and the last one up
    so that the matching costs differ enough between cells for the soft-max to peak (confidences need a probability above 0.11).  An
    empty layer list gives None: the raw frames are the features (stream_params' filter=None, nlayers == 0)."""
    if not layers:
        return None
    filt = dfe.getFilter(dict(layers=list(layers)), device=cuda, generator=torch.Generator().manual_seed(11))
    filt.modules[0].weight.mul_(gain)
    filt.modules[-1].weight.mul_(peak)
    return filt


def features(filt, x):
    """the filter stack's output on a frame, in a tensor of its own; filt None: the frame is its own feature map"""
    return x if filt is None else filt.forward(x).clone()


class Config:
    """win: the window's side, or (maxh, maxw); layers: geometry.layers, () for raw frames; shape: the camera frames' (C, Hsrc, Wsrc)"""

    def __init__(self, hImg, wImg, win, method="max", threshold=None, rectify="features", dist=None, fix=False, ratio=0.2, sfm=None, gain=1.0 / 128, layers=LAYERS,
                 shape=(3, 240, 320), peak=10.0):
        self.peak = peak                                          # the last layer's gain (make_filter)
        maxh, maxw = win if isinstance(win, tuple) else (win, win)
        self.geometry = dict(hImg=hImg, wImg=wImg, maxh=maxh, maxw=maxw, layers=list(layers), output_extraction_method=method)
        self.threshold, self.rectify, self.dist, self.fix, self.ratio, self.sfm, self.gain = threshold, rectify, dist, fix, ratio, sfm or sfm_kw(), gain
        self.layers, self.shape = tuple(layers), tuple(shape)

    def frames(self, cuda):
        return frames(cuda, self.shape[1:], self.shape[0])

    def filter(self, dfe, cuda):
        return make_filter(dfe, cuda, self.gain, self.layers, self.peak)

    def extra(self):
        return dict(self.sfm, rectify=self.rectify, threshold=self.threshold, fixMaskOffset=self.fix, minInlierRatio=self.ratio)


OUTPUTS = ("im_scaled", "flow", "mask", "depth", "dconf")         # the device outputs of a push, in the ABI's order


class Stream:
    """the C ABI driven directly, every device output in a guarded buffer"""

    def __init__(self, dfe, cuda, cfg, filt, K, tweak=None):
        self.dfe, self.cuda, self.ctx = dfe, cuda, dfe.get_ctx(0)
        self.p, self.keep = dfe.stream.stream_params(cfg.geometry, filt, K, cfg.dist, *cfg.shape, **cfg.extra())
        if tweak:                                                 # (a value the Python layer would refuse on the host)
            tweak(self.p)
        self.h = C.c_void_p()
        self.ctx.check(dfe.lib().dfe_stream_create(self.ctx.handle, C.byref(self.p), C.byref(self.h)))

    def push(self, frame, imu_tx=1.0, u8_scale=None, expect=0, want=OUTPUTS):
        """one push; `want` names the device outputs that get a buffer, the others are passed as NULL"""
        p, cuda = self.p, self.cuda
        n = p.hImg * p.wImg
        shapes = dict(im_scaled=(p.C, p.hImg, p.wImg), flow=(2, p.hImg, p.wImg), mask=(p.hImg, p.wImg), depth=(p.hImg, p.wImg), dconf=(p.hImg, p.wImg))
        bufs = {k: guarded(int(np.prod(shapes[k])), cuda) for k in want}
        R, Tt, nf, ni, st = (C.c_double * 9)(*([-7.0] * 9)), (C.c_double * 3)(*([-7.0] * 3)), C.c_int(-7), C.c_int(-7), C.c_int(-7)
        tail = (imu_tx,) + tuple(bufs[k].data_ptr() if k in bufs else None for k in OUTPUTS) + (R, Tt, C.byref(nf), C.byref(ni), C.byref(st))
        if frame is None or frame.dtype != torch.uint8:
            rc = self.dfe.lib().dfe_stream_push_f32(self.h, None if frame is None else frame.data_ptr(), *tail)
        else:
            rc = self.dfe.lib().dfe_stream_push_u8(self.h, frame.data_ptr(), u8_scale, *tail)
        assert rc == expect, (rc, self.dfe.lib().dfe_last_error(self.ctx.handle))
        if rc:
            assert all((bufs[k] == FILL).all() for k in bufs if k != "im_scaled") and st.value == -7, "a refused push wrote a result"
            return None
        first = st.value == 0
        out = dict(status=st.value, nf=nf.value, ni=ni.value, R=np.array(R[:]).reshape(3, 3), T=np.array(Tt[:]))
        for k in want:                                            # (-7 is a flow value: every flow element is compared with the composition's)
            out[k] = unguard(bufs[k], shapes[k], k, k == "im_scaled" or (k != "flow" and not first))
        if first:                                                 # the first frame writes im_scaled only
            assert all((out[k] == FILL).all() for k in want if k != "im_scaled")
        elif "flow" in out:
            assert np.isfinite(out["flow"]).all()
        return out

    def close(self):
        self.dfe.lib().dfe_stream_destroy(self.h)


def composition(dfe, cfg, filt, K, prev, cur, imu_tx=1.0):
    """what a caller had to stitch before the stream existed, from the public ops, in the reference's order"""
    g = cfg.geometry
    h, w = g["hImg"], g["wImg"]
    if cfg.dist is not None:
        prev, cur = dfe.sfm2.undistortImage(prev, K, cfg.dist), dfe.sfm2.undistortImage(cur, K, cfg.dist)
    R, Tt, nf, ni = dfe.sfm2.getEgoMotion2(K, im1=prev, im2=cur, **cfg.sfm)[:4]
    ps, cs = dfe.imageScale(prev, w, h), dfe.imageScale(cur, w, h)
    Ks = np.array(K, np.float64).copy()
    Ks[0] *= w / prev.shape[2]
    Ks[1] *= h / prev.shape[1]
    fcur = features(filt, cs)
    if cfg.rectify == "features":
        wprev, mask = dfe.sfm2.removeEgoMotion(features(filt, ps), Ks, R, inverse=True)
    else:
        wimg, mask = dfe.sfm2.removeEgoMotion(ps, Ks, R, inverse=True)
        wprev = features(filt, wimg)
    model = dfe.getModel(dict(g, prefilter=True), True, True, device=cs.device)
    po = model.forwardFlow([wprev, fcur], cfg.threshold)
    full, fc = po["full"], po["full_confidences"]
    H1, W1 = po["confidences"].shape
    dfe.enlargeMask(mask, -(-(w - W1) // 2), -(-(h - H1) // 2))
    if cfg.rectify == "features":
        oy, ox = (h - mask.shape[0]) // 2 - (0 if cfg.fix else 1), (w - mask.shape[1]) // 2 - (0 if cfg.fix else 1)
    else:
        oy = ox = 0
    mask2 = torch.zeros((h, w), device=cs.device)
    mask2[oy:oy + mask.shape[0], ox:ox + mask.shape[1]] = mask
    mask2 = mask2 * fc
    depth, dconf = dfe.computeDepthMapFromFlow(full[1], mask2, imu_tx)
    return dict(status=1, nf=nf, ni=ni, R=R.numpy(), T=Tt.numpy(), im_scaled=cs.cpu().numpy(), flow=full.cpu().numpy(), mask=mask2.cpu().numpy(),
                depth=depth.cpu().numpy(), dconf=dconf.cpu().numpy())


def assert_same(got, want, what):
    assert got["status"] == want["status"] and (got["nf"], got["ni"]) == (want["nf"], want["ni"]), (what, got["status"], got["nf"], got["ni"], want["nf"], want["ni"])
    for k in ("R", "T", "im_scaled", "flow", "mask", "depth", "dconf"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs from the composition (%d elements)" % (what, k, (got[k] != want[k]).sum())
    assert want["mask"].any() and want["flow"].any() and want["dconf"].any(), "%s: the composition's result is empty" % what


FUSED = ("feat_matching_flat_kernel+softmax", "feat_matching_flat_mean_kernel")   # the matcher with the per-pixel tail in its epilogue


def run_sequence(dfe, cuda, cfg, fused=False, imu=(1.0, 1.0, 1.0), frame_scale=1.0):
    """[im0, im1, im0] (times frame_scale) through a stream of cfg, push i with imu_tx = imu[i]; pushes 2 and 3 against the composition"""
    im0, im1, _, K = cfg.frames(cuda)
    if frame_scale != 1.0:
        im0, im1 = im0 * np.float32(frame_scale), im1 * np.float32(frame_scale)
    filt = cfg.filter(dfe, cuda)
    s = Stream(dfe, cuda, cfg, filt, K)
    try:
        r1 = s.push(im0, imu_tx=imu[0])
        assert r1["status"] == 0 and (r1["nf"], r1["ni"]) == (0, 0)
        assert np.array_equal(r1["im_scaled"], dfe.imageScale(im0 if cfg.dist is None else dfe.sfm2.undistortImage(im0, K, cfg.dist), s.p.wImg, s.p.hImg).cpu().numpy())
        r2 = s.push(im1, imu_tx=imu[1])
        assert (dfe.get_ctx(0).last_kernel() in FUSED) == fused, dfe.get_ctx(0).last_kernel()   # (nothing behind the matcher's step names a kernel)
        r3 = s.push(im0, imu_tx=imu[2])
    finally:
        s.close()
    assert_same(r2, composition(dfe, cfg, filt, K, im0, im1, imu[1]), "push 2")
    assert_same(r3, composition(dfe, cfg, filt, K, im1, im0, imu[2]), "push 3 (im1 -> im0: the stream must have kept im1 and ITS features)")
    assert not np.array_equal(r2["flow"], r3["flow"])
    print("stream %s %s: push 2 %d / %d inliers, push 3 %d / %d; mask keeps %d and %d pixels" % (cfg.geometry["output_extraction_method"], cfg.rectify, r2["ni"], r2["nf"],
                                                                                              r3["ni"], r3["nf"], int(r2["mask"].sum()), int(r3["mask"].sum())))
    return r2, r3


CASES_A = [
    ("max features", dict(method="max")),
    ("max threshold features fixed offset", dict(method="max", threshold=0.11, fix=True)),
    ("mean features undistorted", dict(method="mean", dist=ARDRONE_DIST)),
    ("max image", dict(method="max", rectify="image")),
    ("max threshold image", dict(method="max", threshold=0.11, rectify="image")),
    ("mean image", dict(method="mean", rectify="image")),
]


@pytest.mark.parametrize("name,kw", CASES_A, ids=[c[0] for c in CASES_A])
def test_stream_equals_composition_half_size(dfe, cuda, name, kw):
    """Case A: geometry 120 x 160 from 240 x 320 frames, two 5 x 5 layers, a 16 x 16 window: the map is under 253 columns, so the matcher
    goes through the stand-alone ops.  im_scaled, both flow planes, mask, R, T, n_found, n_inliers and depth (imu_tx = 1) equal the
    composition bit for bit on pushes 2 and 3 of [im0, im1, im0]."""
    run_sequence(dfe, cuda, Config(120, 160, 16, **kw))


def test_stream_offsets_shipped_and_fixed_differ(dfe, cuda):
    """the shipped paste offset is one pixel up and left of the fixed one: the same masks, shifted -- and nothing else changes"""
    a, _ = run_sequence(dfe, cuda, Config(120, 160, 16))
    b, _ = run_sequence(dfe, cuda, Config(120, 160, 16, fix=True))
    assert np.array_equal(a["flow"], b["flow"]) and not np.array_equal(a["mask"], b["mask"])


@pytest.mark.parametrize("method", ["max", "mean"])
def test_stream_equals_composition_full_size(dfe, cuda, method):
    """Case B: geometry 240 x 320 (scale 1 : 1), the same layers, a 17 x 17 window: the map is 312 columns wide, so the matcher's fused
    soft-max / soft-arg-max epilogue runs and the volume is never written."""
    run_sequence(dfe, cuda, Config(240, 320, 17, method=method), fused=True)


# ---- off the 240 x 320, square-window case.  In cases A and B x and y are interchangeable (hImg - H1 == wImg - W1, so ix == iy and ox == oy),
# every plane is a multiple of 256 floats, C is 3 and the stack has two layers.  The asymmetric case: camera frames 3 x 149 x 203 (90741
# bytes, odd), geometry 67 x 93 (n = 6231, odd; scale ratios 2.22 and 2.18), a stack whose kernel is 7 rows by 9 columns and a window of
# 10 rows by 17 columns.  By the reference's rules (depth_estimation_api.lua:172-179; tests/test_stream_cpu.py pins them on the host):
# Hf, Wf = 61, 85; H1, W1 = 52, 69; oy, ox = 2, 3 (3, 4 with fix_mask_offset; 0, 0 in image mode); ix, iy = 12, 8.
ASYM_SHAPE, ASYM_LAYERS, ASYM_WIN = (3, 149, 203), ((3, 3, 5, 4), (4, 7, 3, 4)), (10, 17)
ASYM_SHAPES = dict(Hf=61, Wf=85, H1=52, W1=69, oy=2, ox=3, ix=12, iy=8)
MONO_SHAPE, MONO_LAYERS = (1, 149, 203), ((1, 5, 5, 4), (4, 5, 5, 4))
# The last layer's gain at this geometry is 40, not make_filter's 10.  With 10 the soft-max over the window's 170 cells stays flat on these
# frames: no probability passes 0.11 (the composition's thresholded mask is empty), and the 'mean' flows stay under 2.5 px, so that every
# depth is the far value 100 whatever imu_tx is.  With 40 the thresholded mask keeps about 2550 pixels, the 'mean' flows reach 6 to 7.6 px
# and are not integers (from 80 on they are: the soft-max is one-hot), and some 550 to 1000 depths lie below 100.
ASYM_PEAK = 40.0


def asym(**kw):
    kw = dict(dict(layers=ASYM_LAYERS, shape=ASYM_SHAPE, peak=ASYM_PEAK), **kw)
    return Config(67, 93, ASYM_WIN, **kw)


CASES_ASYM = [
    ("max features", dict(method="max"), dict()),
    ("max threshold features fixed offset", dict(method="max", threshold=0.11, fix=True), dict(oy=3, ox=4)),
    ("mean image", dict(method="mean", rectify="image"), dict(oy=0, ox=0)),
    ("mean features undistorted", dict(method="mean", dist=ARDRONE_DIST), dict()),
]


@pytest.mark.parametrize("name,kw,off", CASES_ASYM, ids=[c[0] for c in CASES_ASYM])
def test_stream_equals_composition_asymmetric(dfe, cuda, name, kw, off):
    """The asymmetric case: no two of the x / y pairs (Hf, Wf), (H1, W1), (oy, ox), (ix, iy) are equal, so an exchanged pair in the
    enlargeMask or the paste call changes the mask; n is odd, so the second flow plane starts at an odd element."""
    cfg = asym(**kw)
    p, keep = dfe.stream.stream_params(cfg.geometry, cfg.filter(dfe, cuda), cfg.frames(cuda)[3], cfg.dist, *cfg.shape, **cfg.extra())
    assert dfe.stream.stream_shapes(p) == dict(ASYM_SHAPES, **off)
    run_sequence(dfe, cuda, cfg)


@pytest.mark.parametrize("rectify", ["features", "image"])
def test_stream_one_plane(dfe, cuda, rectify):
    """C = 1: the luminance pair as two_view_pair gives it, a stack whose first layer reads one plane, the asymmetric window"""
    run_sequence(dfe, cuda, asym(method="mean", rectify=rectify, layers=MONO_LAYERS, shape=MONO_SHAPE))


# Raw frames are matched pixel by pixel on their 0..255 values.  RAW_SCALE multiplies the frames (and RAW_SCALE^2 the tracker's eigenvalue
# floor, as in test_stream_u8_push_and_reset): 1.0 unless the soft-max saturated on raw bytes and left the composition's mask empty
RAW_SCALE = 1.0
RAW_CASES = [(r, planes, m) for r in ("image", "features") for planes in (3, 1) for m in ("max", "mean")]


def raw_config(rectify, planes, method):
    return Config(67, 93, ASYM_WIN, method=method, rectify=rectify, fix=rectify == "features", layers=(), shape=(planes, 149, 203),
                  sfm=sfm_kw(trackerMinEig=tr.ROUTE["min_eig"] * RAW_SCALE ** 2))


@pytest.mark.parametrize("rectify,planes,method", RAW_CASES, ids=["%s C=%d %s" % c for c in RAW_CASES])
def test_stream_raw_frames(dfe, cuda, rectify, planes, method):
    """filter=None, nlayers == 0: the scaled frame is its own feature map (feat[i] is scaled[i]), in image mode the matcher reads the
    rectified frame itself, and the features' offset is zero, which the reference's offset (-1) cannot express: fix_mask_offset"""
    cfg = raw_config(rectify, planes, method)
    assert cfg.filter(dfe, cuda) is None
    run_sequence(dfe, cuda, cfg, frame_scale=RAW_SCALE)


DEPTHS = [("one layer", ((3, 5, 5, 4),)), ("three layers", ((3, 3, 3, 4), (4, 3, 3, 4), (4, 3, 3, 6)))]


@pytest.mark.parametrize("rectify", ["features", "image"])
@pytest.mark.parametrize("name,layers", DEPTHS, ids=[d[0] for d in DEPTHS])
def test_stream_stack_depths(dfe, cuda, name, layers, rectify):
    """one layer: the stack writes straight into the feature map and the stream carves no intermediate planes; three layers: both of
    them are in use, and the last layer's plane count (6) is not the intermediate ones' (4)"""
    run_sequence(dfe, cuda, asym(method="mean", rectify=rectify, layers=layers))


def test_stream_three_wide_layers_full_size(dfe, cuda):
    """Three layers of ten planes at 240 x 320 (case B's frames, window and fused matcher).  At 67 x 93 a layer is a few dozen blocks that
    all stage their input before any of them stores, so a stack that read and wrote ONE intermediate buffer would still come out right;
    here the middle layer is 900 blocks of the batched convolution, each holding 54 KB of LDS, more than the device keeps resident at
    once, and the later ones would read rows that the earlier ones have overwritten.  ('max': behind these 3 x 3 layers the soft-max is
    too flat for 'mean' to call any pixel confident, and the composition's mask would be empty.)"""
    run_sequence(dfe, cuda, Config(240, 320, 17, method="max", layers=((3, 3, 3, 10), (10, 3, 3, 10), (10, 3, 3, 4))), fused=True)


def test_stream_imu_tx(dfe, cuda):
    """imu_tx = 1.0, 0.5 and 2.0 on the three pushes: each pair's depth is the composition's with that pair's value, and the value
    matters (on the composition alone: the depth of push 2 at 0.5 is not the depth at 1.0)"""
    cfg = asym(method="mean")
    im0, im1, _, K = cfg.frames(cuda)
    filt = cfg.filter(dfe, cuda)
    a, b = composition(dfe, cfg, filt, K, im0, im1, 0.5), composition(dfe, cfg, filt, K, im0, im1, 1.0)
    assert a["dconf"].any() and not np.array_equal(a["depth"], b["depth"])
    run_sequence(dfe, cuda, cfg, imu=(1.0, 0.5, 2.0))


def u8_push_and_reset(dfe, cuda, cfg):
    """the rule of test_stream_u8_push_and_reset on cfg's frames"""
    im0, im1, _, K = cfg.frames(cuda)
    b0, b1 = (im0 / np.float32(GAINS[2])).round().clamp(0, 255).to(torch.uint8), (im1 / np.float32(GAINS[2])).round().clamp(0, 255).to(torch.uint8)
    f0, f1 = b0.to(torch.float32) * np.float32(1.0 / 255.0), b1.to(torch.float32) * np.float32(1.0 / 255.0)
    filt = cfg.filter(dfe, cuda)
    s8, sf = Stream(dfe, cuda, cfg, filt, K), Stream(dfe, cuda, cfg, filt, K)
    try:
        for i, (b, f) in enumerate(((b0, f0), (b1, f1), (b0, f0))):
            r8, rf = s8.push(b, u8_scale=1.0 / 255.0), sf.push(f)
            assert r8["status"] == rf["status"] == (0 if i == 0 else 1)
            for k in r8:
                assert np.array_equal(r8[k], rf[k]), (i, k)
        want = composition(dfe, cfg, filt, K, f1, f0)
        assert_same(r8, want, "u8 push 3")
        assert dfe.lib().dfe_stream_reset(s8.h) == 0
        r = s8.push(b1, u8_scale=1.0 / 255.0)
        assert r["status"] == 0
        assert_same(s8.push(b0, u8_scale=1.0 / 255.0), want, "the pair after the reset")
    finally:
        s8.close()
        sf.close()


@pytest.mark.parametrize("dist", [None, ARDRONE_DIST], ids=["as it is", "undistorted"])
def test_stream_u8_push_odd_byte_count(dfe, cuda, dist):
    """the rule of test_stream_u8_push_and_reset on the asymmetric case's frames: 3 x 149 x 203 = 90741 bytes, so the conversion's last
    group of bytes is a partial one"""
    assert int(np.prod(ASYM_SHAPE)) % 2 == 1
    u8_push_and_reset(dfe, cuda, asym(method="mean", dist=dist, sfm=sfm_kw(trackerMinEig=tr.ROUTE["min_eig"] / 255.0 ** 2), gain=255.0 / 128))


@pytest.mark.parametrize("dist", [None, ARDRONE_DIST], ids=["as it is", "undistorted"])
def test_stream_u8_push_and_reset(dfe, cuda, dist):
    """bytes round(255 frame) with scale 1 / 255 (frame in 0..1) give what the f32 push on float32(byte) x float32(1 / 255) gives, bit for
    bit -- converted straight into the frame's slot, or with `has_dist` into the staging buffer in front of the undistortion; after a
    reset a push returns status 0 again, and the pair after it is computed from the frames pushed after it.  The frames are 255 times
    darker than the other tests', so the tracker's eigenvalue floor goes down by 255^2, and the first layer's gain up by 255."""
    u8_push_and_reset(dfe, cuda, Config(120, 160, 16, method="mean", dist=dist, sfm=sfm_kw(trackerMinEig=tr.ROUTE["min_eig"] / 255.0 ** 2), gain=255.0 / 128))


SUBSETS = [("depth",), ("dconf",), ("mask",), ("flow",), ("flow", "depth"), ("mask", "dconf"), ()]


@pytest.mark.parametrize("rectify", ["features", "image"])
def test_stream_optional_outputs(dfe, cuda, rectify):
    """every device output may be NULL: whatever subset is asked for equals the same output of the push that asks for all five, bit for
    bit.  Depth without flow or mask goes through the stream's own flow and mask planes, one of depth / depth_conf through its spare
    plane; a push that asks for nothing still returns the pose and the counts, and advances the state."""
    im0, im1, _, K = frames(cuda)
    cfg = Config(120, 160, 16, method="mean", rectify=rectify)
    filt = make_filter(dfe, cuda)
    full = Stream(dfe, cuda, cfg, filt, K)
    try:
        full.push(im0)
        want2, want3 = full.push(im1), full.push(im0)
    finally:
        full.close()
    assert want2["status"] == want3["status"] == 1 and want2["depth"].any() and want2["dconf"].any()
    for sub in SUBSETS:
        s = Stream(dfe, cuda, cfg, filt, K)
        try:
            assert s.push(im0, want=sub)["status"] == 0
            r2, r3 = s.push(im1, want=sub), s.push(im0, want=sub)
        finally:
            s.close()
        for got, want in ((r2, want2), (r3, want3)):
            assert set(got) == set(sub) | {"status", "nf", "ni", "R", "T"}
            for k in got:
                assert np.array_equal(got[k], want[k]), (sub, k)


def zeros_of(r):
    return all(not r[k].any() for k in ("flow", "mask", "depth", "dconf"))


def test_stream_bad_image_no_corners_then_recovers(dfe, cuda):
    """[flat frame, im0, im1]: push 2 finds no corner in the previous frame -- status 2, return code 0, flow, mask and depth all zero,
    n_found what the pose step saw (0) -- and the state advances through the gate: push 3 is the composition on (im0, im1)."""
    im0, im1, flat, K = frames(cuda)
    cfg = Config(120, 160, 16, method="mean")
    filt = make_filter(dfe, cuda)
    s = Stream(dfe, cuda, cfg, filt, K)
    try:
        assert s.push(flat)["status"] == 0
        r2 = s.push(im0)
        assert r2["status"] == 2 and (r2["nf"], r2["ni"]) == (0, 0) and zeros_of(r2)
        assert (r2["R"] == -7).all() and (r2["T"] == -7).all()       # no pose: not written
        assert np.array_equal(r2["im_scaled"], dfe.imageScale(im0, 160, 120).cpu().numpy())
        r3 = s.push(im1)
    finally:
        s.close()
    assert_same(r3, composition(dfe, cfg, filt, K, im0, im1), "push 3 behind a bad image")


def test_stream_bad_image_inlier_ratio(dfe, cuda):
    """min_inlier_ratio = 1.01 can never be met: [im0, im1] gives status 2 with all outputs zero and the pose step's own counts and pose;
    the state advanced: with the gate open again (another stream) nothing else differs"""
    im0, im1, _, K = frames(cuda)
    cfg = Config(120, 160, 16, ratio=1.01)
    filt = make_filter(dfe, cuda)
    s = Stream(dfe, cuda, cfg, filt, K)
    try:
        assert s.push(im0)["status"] == 0
        r = s.push(im1)
    finally:
        s.close()
    R, Tt, nf, ni = dfe.sfm2.getEgoMotion2(K, im1=im0, im2=im1, **cfg.sfm)[:4]
    assert r["status"] == 2 and zeros_of(r) and (r["nf"], r["ni"]) == (nf, ni) and nf >= 8
    assert np.array_equal(r["R"], R.numpy()) and np.array_equal(r["T"], Tt.numpy())


def test_stream_argument_errors_leave_the_state(dfe, cuda):
    """Creation refuses a window that does not fit and the reference's negative offset.  A refused push leaves the state as it was: after
    im0, a push without a frame is refused, and so is a flat frame that the pose step refuses for its arguments -- late, with the flat
    frame already scaled and filtered into the slots the push writes; the push of im1 behind them equals the composition on (im0, im1).
    Had either refused push advanced the state, the previous frame would be the flat one and that push a bad image.  (The pose step's
    arguments are the stream's own, fixed at creation, so the late refusal is lifted on a second stream fed the same frames, whose state
    the first stream's refusals must not disturb either: both work on one ctx.)"""
    im0, im1, flat, K = frames(cuda)
    ctx, filt = dfe.get_ctx(0), make_filter(dfe, cuda)
    cfg = Config(120, 160, 16)
    p, keep = dfe.stream.stream_params(cfg.geometry, filt, K, None, 3, 240, 320, **sfm_kw())
    h = C.c_void_p()
    p.maxh = 200
    assert dfe.lib().dfe_stream_create(ctx.handle, C.byref(p), C.byref(h)) == E_SHAPE and not h.value
    p.maxh, p.nlayers = 16, 0
    assert dfe.lib().dfe_stream_create(ctx.handle, C.byref(p), C.byref(h)) == E_ARG and not h.value
    good = Stream(dfe, cuda, cfg, filt, K)
    bad = Stream(dfe, cuda, cfg, filt, K, tweak=lambda q: setattr(q.tracker, "win", 4))   # an even window: refused by the pose step, at the second push
    try:
        assert good.push(im0)["status"] == 0 and bad.push(im0)["status"] == 0
        assert good.push(None, expect=E_ARG) is None
        assert bad.push(flat, expect=E_ARG) is None                # the late refusal
        assert bad.push(im1, expect=E_ARG) is None
        r = good.push(im1)
        assert dfe.lib().dfe_stream_reset(bad.h) == 0 and bad.push(flat)["status"] == 0 and bad.push(im1, expect=E_ARG) is None
    finally:
        good.close()
        bad.close()
    assert_same(r, composition(dfe, cfg, filt, K, im0, im1), "the push behind refused ones")
    none = [None] * 9
    assert dfe.lib().dfe_stream_push_f32(None, im0.data_ptr(), 1.0, *none, None) == E_ARG
    assert dfe.lib().dfe_stream_push_u8(None, im0.data_ptr(), 1.0, 1.0, *none, None) == E_ARG
    assert dfe.lib().dfe_stream_reset(None) == E_ARG


# --------------------------------------------------------------------------------------------------------------------- 4. Python
def test_python_next_frame_depth(dfe, cuda):
    """nextFrameDepth returns None, then (im_scaled, xflow, mask) equal to the C ABI's outputs; api.last is filled; a frame of another
    size raises DfeError; reset() starts over."""
    im0, im1, _, K = frames(cuda)
    cfg = Config(120, 160, 16, method="mean")
    filt = make_filter(dfe, cuda)
    s = Stream(dfe, cuda, cfg, filt, K)
    try:
        s.push(im0)
        want = s.push(im1)
    finally:
        s.close()
    api = dfe.DepthEstimationAPI(cfg.geometry, filt, K, u8Scale=1.0, **cfg.extra())
    assert api.nextFrameDepth(im0) is None and api.last["status"] == 0
    got = api.nextFrameDepth(im1, imu_tx=1.0)
    assert isinstance(got, tuple) and len(got) == 3
    ims, xflow, mask = (t.cpu().numpy() for t in got)
    assert np.array_equal(ims, want["im_scaled"]) and np.array_equal(xflow, want["flow"][1]) and np.array_equal(mask, want["mask"])
    last = api.last
    assert last["status"] == 1 and (last["nFound"], last["nInliers"]) == (want["nf"], want["ni"])
    assert np.array_equal(last["yflow"].cpu().numpy(), want["flow"][0]) and np.array_equal(last["R"].numpy(), want["R"]) and np.array_equal(last["T"].numpy(), want["T"])
    assert np.array_equal(last["depth"].cpu().numpy(), want["depth"]) and np.array_equal(last["depth_conf"].cpu().numpy(), want["dconf"])
    with pytest.raises(dfe.DfeError):
        api.nextFrameDepth(im0[:, :200])
    with pytest.raises(dfe.DfeError):
        api.nextFrameDepth(im0[:1].contiguous())
    got2 = api.nextFrameDepth(im0)                                 # the refused frames changed nothing: this is the pair (im1, im0)
    assert got2 is not None and api.last["status"] == 1 and not np.array_equal(got2[1].cpu().numpy(), xflow)
    api.reset()
    assert api.nextFrameDepth(im0) is None
    again = api.nextFrameDepth(im1)
    assert np.array_equal(again[1].cpu().numpy(), xflow) and np.array_equal(again[2].cpu().numpy(), mask)
    b = im0.round().clamp(0, 255).to(torch.uint8)
    assert api.nextFrameDepth(b) is not None and api.last["status"] == 1     # a uint8 frame is taken too (here with u8Scale = 1: the same range)
    api.close()
