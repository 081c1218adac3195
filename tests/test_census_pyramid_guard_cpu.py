"""The census pyramid kernels (csrc/census_pyramid.hip) inside the register file: the three forms of the signature
kernel (k = 3, 5, 7), the staged route's multiply and the twelve forms of the volume kernel (agg 1 / 3 / 5 by 1 .. 4 channels), 0 bytes of
scratch, 0 SGPR spills and at most 168 VGPRs -- a thread's patch columns, a lane's frame-0 signatures and its column of Hamming distances
are arrays indexed by unrolled constants, and a form that indexed them at run time would move them to scratch.  And the argument checks
of the Python wrappers, which need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_pyramid_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "census_pyramid.hip"),
                          "census_pyramid_"], capture_output=True, text=True).stdout
    rows = re.findall(r"^(census_pyramid_\w+)(?:<([^>]*)>)?\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out, flags=re.M)
    want = sorted([("census_pyramid_volume_kernel", "%d, %d" % (a, c)) for a in (1, 3, 5) for c in (1, 2, 3, 4)]
                  + [("census_pyramid_sig_kernel", "%d" % k) for k in (3, 5, 7)] + [("census_pyramid_scale_kernel", "")])
    assert sorted(r[:2] for r in rows) == want and len(rows) == len(re.findall(r"^census_pyramid_", out, flags=re.M)), out
    for name, form, vgpr, scratch, spill in rows:
        text = "%s<%s>: %s VGPRs, %s B scratch, %s SGPR spills" % (name, form, vgpr, scratch, spill)
        assert int(scratch) == 0 and int(spill) == 0, text
        assert int(vgpr) <= 168, text + ": below 3 waves a SIMD"


def _model(d, k=7, kw=None, maxh=8, maxw=8, ratios=(1, 2, 4), **kwargs):
    geo = dict(maxh=maxh, maxw=maxw, ratios=list(ratios), multiscale=True, hKernel=k, wKernel=k if kw is None else kw, hImg=32, wImg=48,
               output_extraction_method="max")
    return d.MultiscaleModel(geo, **kwargs)


def test_census_pyramid_argument_checks_need_no_device():
    import depth_estimation_amd as d

    img = torch.zeros((3, 32, 48))
    byte = torch.zeros((3, 32, 48), dtype=torch.uint8)
    m = _model(d)
    vol = lambda *a, **k: d.censusPyramidScaleVolume(img, img, *a, **k)
    # the values are accepted; the CPU tensor is not
    for call in (lambda: m.forwardFlow([img, img], census=True), lambda: m.forwardFlow([img, img], census=dict(agg=5, beta=0.01), one_call=False),
                 lambda: m.forwardFlow([byte, byte], census=dict(agg=1)), lambda: m.forwardFlow([img, img], census={}, process_full=False),
                 lambda: _model(d, k=3, maxh=5, maxw=7, ratios=(1,)).forwardFlow([img[:2], img[:2]], census=dict(beta=1)),
                 lambda: vol(1, 7, 8, 8), lambda: vol(2, 5, 4, 8, agg=5, beta=0.5), lambda: vol(4, 3, 16, 4, 1, 2)):
        with pytest.raises(TypeError):
            call()
    # a wrong dtype, two dtypes
    for call in (lambda: m.forwardFlow([img.double(), img.double()], census=True), lambda: m.forwardFlow([img, byte], census=True),
                 lambda: m.forwardFlow([img.int(), img.int()], census=True), lambda: d.censusPyramidScaleVolume(byte, byte, 1, 7, 8, 8),
                 lambda: d.censusPyramidScaleVolume(img, img.double(), 1, 7, 8, 8)):
        with pytest.raises(TypeError):
            call()
    # agg outside {1, 3, 5}, beta not finite and positive, a census argument of another kind
    for agg in (0, 2, 4, 7, 3.0, True, None):
        for call in (lambda: m.forwardFlow([img, img], census=dict(agg=agg)), lambda: vol(1, 7, 8, 8, agg)):
            with pytest.raises(ValueError):
                call()
    for beta in (0, 0.0, -0.25, float("inf"), float("nan"), "1", True):
        for call in (lambda: m.forwardFlow([img, img], census=dict(beta=beta)), lambda: vol(1, 7, 8, 8, 3, beta)):
            with pytest.raises(ValueError):
                call()
    for census in (3, "agg", (3, 0.1), dict(agg=3, gamma=1.0), [3]):
        with pytest.raises(ValueError):
            m.forwardFlow([img, img], census=census)
    # the patch: odd, 3 .. 7, square
    for k in (1, 4, 6, 9, 11):
        with pytest.raises(ValueError):
            _model(d, k=k).forwardFlow([img, img], census=True)
    for k in (1, 4, 6, 9, 7.0, True, (7, 7)):
        with pytest.raises(ValueError):
            vol(1, k, 8, 8)
    with pytest.raises(ValueError):
        _model(d, k=7, kw=5).forwardFlow([img, img], census=True)
    # what census is not combined with: fp16 volumes, the refinement, learned filters, prefiltered features
    for kw in (dict(f16_scale=1.0), dict(subpixel=True), dict(f16_scale=0.5, one_call=False), dict(subpixel=True, one_call=False)):
        with pytest.raises(ValueError):
            m.forwardFlow([img, img], census=True, **kw)
    with pytest.raises(ValueError):
        _model(d, prefiltered=True).forwardFlow([img, img], census=True)
    geo = dict(maxh=8, maxw=8, ratios=[1, 2], multiscale=True, layers=[[3, 5, 5, 4]], share_filters=True, hImg=32, wImg=48, output_extraction_method="max")
    with pytest.raises(ValueError):
        d.getModelMultiscale(geo, device="cpu").forwardFlow([img, img], census=True)
    # channels, shapes, the staged entry's own arguments
    big = torch.zeros((5, 32, 48))
    for call in (lambda: m.forwardFlow([big, big], census=True), lambda: m.forwardFlow([img, img[:, 1:]], census=True), lambda: m.forwardFlow([img[0], img[0]], census=True),
                 lambda: d.censusPyramidScaleVolume(big, big, 1, 7, 8, 8), lambda: d.censusPyramidScaleVolume(img, img[:, :, 1:], 1, 7, 8, 8),
                 lambda: vol(0, 7, 8, 8), lambda: vol(5, 7, 8, 8), lambda: vol(3, 7, 8, 8), lambda: vol(2.0, 7, 8, 8), lambda: vol(1, 7, 0, 8),
                 lambda: vol(1, 7, 8, True), lambda: vol(1, 7, 40, 40)):
        with pytest.raises(ValueError):
            call()
    # census=None and census=False ask for the SSD pyramid: its own refusal of a CPU tensor, as before
    for census in (None, False):
        with pytest.raises(d.DfeError):
            m.forwardFlow([img, img], census=census)
