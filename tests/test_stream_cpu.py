"""CPU suite: the stream layer's host side -- the float64 reference of image.scale against torch's bilinear interpolation, and
dfe_stream_shapes (host only, no device)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import stream_ref64 as sr

E_ARG, E_SHAPE = -1, -2                                           # DFE_E_ARG, DFE_E_SHAPE (include/dfe.h)


@pytest.mark.parametrize("src,dst", [((1, 1), (3, 5)), ((7, 5), (7, 5)), ((37, 53), (23, 71)), ((64, 64), (32, 32)), ((5, 300), (9, 17))])
def test_scale_reference_is_torch_bilinear(src, dst):
    """The definition's mapping -- taps and unrounded weights, scale64(weights="exact") -- is that of torch.nn.functional.interpolate(
    float64, bilinear, align_corners=False): within 1e-12 x max |in|.  The definition then rounds each weight to float32 (what scale64
    computes by default, and what the kernel is held to): that moves a result by at most 2^-24 x 2 max |in| through wx (top and bot are
    combined convexly) plus as much through wy, 2^-22 x max |in| together -- so a float64 interpolation cannot agree with it to 1e-12, and
    the default form is held to that bound here."""
    rng = np.random.default_rng(src[0] * 1000 + src[1])
    img = rng.random((3,) + src) * 255.0
    ref = torch.nn.functional.interpolate(torch.from_numpy(img)[None], size=dst, mode="bilinear", align_corners=False)[0].numpy()
    m = np.abs(img).max()
    e_exact, e_f32 = np.abs(sr.scale64(img, *dst, weights="exact") - ref).max(), np.abs(sr.scale64(img, *dst) - ref).max()
    print("scale64 %s -> %s: |exact weights - torch| = %.3e (bound %.3e), |float32 weights - torch| = %.3e (bound %.3e)" % (src, dst, e_exact, 1e-12 * m, e_f32,
                                                                                                                          2.0 ** -22 * m))
    assert e_exact <= 1e-12 * m
    assert e_f32 <= 2.0 ** -22 * m


def test_scale_reference_consequences():
    """equal sizes copy; a 2 x reduction of integer frames is the 2 x 2 mean; both exactly"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (2, 64, 130)).astype(np.float64)
    assert np.array_equal(sr.scale64(img, 64, 130), img)
    mean = (img[:, 0::2, 0::2] + img[:, 0::2, 1::2] + img[:, 1::2, 0::2] + img[:, 1::2, 1::2]) / 4
    assert np.array_equal(sr.scale64(img, 32, 65), mean)


def params(dfe, hImg=240, wImg=320, layers=((3, 5, 5, 4), (4, 5, 5, 4), (4, 5, 5, 10)), win=(16, 16), rectify=0, fix=0, Hsrc=480, Wsrc=640):
    """dfe_stream_params with geometry.layers-style tuples (nIn, kW, kH, nOut); the weights are never read by dfe_stream_shapes, so any
    non-NULL address stands in for them"""
    from depth_estimation_amd._lib import FilterLayer, StreamParams

    p = StreamParams()
    p.C, p.Hsrc, p.Wsrc, p.hImg, p.wImg = 3, Hsrc, Wsrc, hImg, wImg
    p.K = (C.c_double * 9)(300, 0, 320, 0, 300, 240, 0, 0, 1)
    arr = (FilterLayer * max(len(layers), 1))()
    dummy = (C.c_float * 1)()
    for L, (nin, kw, kh, nout) in zip(arr, layers):
        L.nIn, L.nOut, L.kH, L.kW, L.weight = nin, nout, kh, kw, C.addressof(dummy)
    p.layers, p.nlayers = (C.cast(arr, C.POINTER(FilterLayer)) if layers else None), len(layers)
    p.maxh, p.maxw = win
    p.rectify, p.fix_mask_offset = rectify, fix
    p.iterations, p.ransac_max_dist, p.min_inlier_ratio = 512, 1.0, 0.2
    return p, (arr, dummy)


def shapes(dfe, p):
    v = [C.c_int(-99) for _ in range(8)]
    rc = dfe.lib().dfe_stream_shapes(C.byref(p), *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def test_stream_shapes_vga_to_half(dfe):
    p, keep = params(dfe)
    assert shapes(dfe, p) == (0, (228, 308, 213, 293, 5, 5, 14, 14))               # Hf, Wf, H1, W1, oy, ox, ix, iy
    p, keep = params(dfe, fix=1)
    assert shapes(dfe, p) == (0, (228, 308, 213, 293, 6, 6, 14, 14))
    assert dfe.stream.stream_shapes(p) == dict(Hf=228, Wf=308, H1=213, W1=293, oy=6, ox=6, ix=14, iy=14)


# The asymmetric geometry of the GPU suites (tests/test_gpu_stream.py, ASYM): 67 x 93 from 149 x 203 frames, a stack whose kernel is 7 rows
# by 9 columns, a window of 10 rows by 17 columns.  The numbers are the reference's rules (depth_estimation_api.lua:172-179) worked by
# hand: Hf, Wf = 67 - 6, 93 - 8; H1, W1 = 61 - 9, 85 - 16; oy, ox = floor(6 / 2) - 1, floor(8 / 2) - 1; ix, iy = ceil(24 / 2), ceil(15 / 2).
# No two of the x / y pairs are equal, so a swap anywhere in stream_shapes shows.
ASYM = dict(hImg=67, wImg=93, layers=((3, 3, 5, 4), (4, 7, 3, 4)), win=(10, 17), Hsrc=149, Wsrc=203)
ASYM_T = dict(hImg=93, wImg=67, layers=((3, 5, 3, 4), (4, 3, 7, 4)), win=(17, 10), Hsrc=203, Wsrc=149)   # x and y exchanged


def test_stream_shapes_asymmetric(dfe):
    p, keep = params(dfe, **ASYM)
    assert shapes(dfe, p) == (0, (61, 85, 52, 69, 2, 3, 12, 8))                    # Hf, Wf, H1, W1, oy, ox, ix, iy
    assert dfe.stream.stream_shapes(p) == dict(Hf=61, Wf=85, H1=52, W1=69, oy=2, ox=3, ix=12, iy=8)
    p, keep = params(dfe, fix=1, **ASYM)
    assert shapes(dfe, p) == (0, (61, 85, 52, 69, 3, 4, 12, 8))
    assert dfe.stream.stream_shapes(p) == dict(Hf=61, Wf=85, H1=52, W1=69, oy=3, ox=4, ix=12, iy=8)
    for fix in (0, 1):
        p, keep = params(dfe, rectify=1, fix=fix, **ASYM)
        assert shapes(dfe, p) == (0, (61, 85, 52, 69, 0, 0, 12, 8))
    assert dfe.stream.stream_shapes(p) == dict(Hf=61, Wf=85, H1=52, W1=69, oy=0, ox=0, ix=12, iy=8)


def test_stream_shapes_asymmetric_transposed(dfe):
    """frame, geometry, every layer's kernel and the window with x and y exchanged: every pair of the tuple comes out exchanged"""
    def swap(t):
        Hf, Wf, H1, W1, oy, ox, ix, iy = t
        return (Wf, Hf, W1, H1, ox, oy, iy, ix)

    for kw in (dict(), dict(fix=1), dict(rectify=1)):
        p, keep = params(dfe, **dict(ASYM, **kw))
        q, keep2 = params(dfe, **dict(ASYM_T, **kw))
        rc, t = shapes(dfe, p)
        assert rc == 0 and shapes(dfe, q) == (0, swap(t)), kw
    q, keep2 = params(dfe, **ASYM_T)
    assert shapes(dfe, q) == (0, (85, 61, 69, 52, 3, 2, 8, 12))
    assert dfe.stream.stream_shapes(q) == dict(Hf=85, Wf=61, H1=69, W1=52, oy=3, ox=2, ix=8, iy=12)


def test_stream_shapes_image_mode_offset_is_zero(dfe):
    for fix in (0, 1):
        p, keep = params(dfe, rectify=1, fix=fix)
        assert shapes(dfe, p) == (0, (228, 308, 213, 293, 0, 0, 14, 14))
    p, keep = params(dfe, layers=(), rectify=1)                                   # raw frames: still no offset to go negative
    assert shapes(dfe, p) == (0, (240, 320, 225, 305, 0, 0, 8, 8))


def test_stream_shapes_reference_offset_negative_without_layers(dfe):
    p, keep = params(dfe, layers=())
    rc, _ = shapes(dfe, p)
    assert rc == E_ARG and b"fix_mask_offset" in dfe.lib().dfe_last_error(None)
    p, keep = params(dfe, layers=(), fix=1)
    assert shapes(dfe, p) == (0, (240, 320, 225, 305, 0, 0, 8, 8))
    with pytest.raises(dfe.DfeError):
        dfe.stream.stream_shapes(params(dfe, layers=())[0])


def test_stream_shapes_window_larger_than_the_feature_map(dfe):
    p, keep = params(dfe, hImg=28, wImg=320)                                      # Hf = 16: a 17-row window does not fit, 16 rows do
    p.maxh = 17
    assert shapes(dfe, p)[0] == E_SHAPE
    p.maxh = 16
    assert shapes(dfe, p) == (0, (16, 308, 1, 293, 5, 5, 14, 14))
    p, keep = params(dfe, hImg=12, wImg=320)                                      # the filter alone does not fit
    assert shapes(dfe, p)[0] == E_SHAPE


def test_stream_shapes_argument_errors(dfe):
    for edit in (lambda p: setattr(p, "C", 2), lambda p: setattr(p, "Hsrc", 0), lambda p: setattr(p, "wImg", 32769), lambda p: setattr(p, "extraction", 3),
                 lambda p: setattr(p, "rectify", 2), lambda p: setattr(p, "maxw", 0), lambda p: setattr(p, "nlayers", 9)):
        p, keep = params(dfe)
        edit(p)
        assert shapes(dfe, p)[0] == E_ARG
    assert dfe.lib().dfe_stream_shapes(None, *([None] * 8)) == E_ARG
    p, keep = params(dfe, layers=((1, 5, 5, 4),))                                  # the stack's first layer reads another number of planes than C
    assert shapes(dfe, p)[0] == E_SHAPE
