"""The census refinement kernels (csrc/census_subpixel.hip) inside the register file: the three forms of each of
the two kernels (agg 1 / 3 / 5), 0 bytes of scratch and 0 SGPR spills -- a lane's frame-0 box and its row of frame-1 signatures are arrays
indexed by unrolled constants, and a form that indexed them at run time would move them to scratch.  And the new keyword's checks in the
Python wrappers, which need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cenfit_kernels_have_no_scratch_and_no_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "census_subpixel.hip"),
                          "cenfit_"], capture_output=True, text=True).stdout
    rows = re.findall(r"^(cenfit_\w+)(?:<([^>]*)>)?\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out, flags=re.M)
    want = sorted((name, "%d" % a) for name in ("cenfit_refine_kernel", "cenfit_pyramid_refine_kernel") for a in (1, 3, 5))
    assert sorted(r[:2] for r in rows) == want and len(rows) == len(re.findall(r"^cenfit_", out, flags=re.M)), out
    # every __global__ function of the file carries the prefix the search above goes by
    src = open(os.path.join(ROOT, "depth-estimation_amd", "csrc", "census_subpixel.hip")).read()
    assert sorted(set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src))) == ["cenfit_pyramid_refine_kernel", "cenfit_refine_kernel"]
    for name, form, vgpr, scratch, spill in rows:
        text = "%s<%s>: %s VGPRs, %s B scratch, %s SGPR spills" % (name, form, vgpr, scratch, spill)   # (as built: 48 / 74 / 118 and 52 / 77 / 127 VGPRs)
        assert int(scratch) == 0 and int(spill) == 0, text
        assert int(vgpr) <= 128, text + ": below 4 waves a SIMD"


def test_refine_keyword_of_the_single_scale_wrappers():
    import depth_estimation_amd as d

    img = torch.zeros((3, 40, 60))
    byte = img.to(torch.uint8)
    sig = torch.zeros((3, 34, 54), dtype=torch.int64)
    idx = torch.ones((24, 44), dtype=torch.int64)          # 34 - 9 + 1 - 3 + 1 by 54 - 9 + 1 - 3 + 1
    foe = (30.0, 20.0)
    # the values are accepted; the CPU tensor is not
    for call in (lambda: d.censusFlow(sig, sig, 48, 9, 9, refine=True), lambda: d.censusFlow(sig, sig, 48, 9, 9, agg=5, refine=False),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx), lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx[:22, :42], agg=5),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, flow_y=torch.zeros((30, 50)), flow_x=torch.zeros((30, 50)), pad_t=6, pad_l=6),
                 lambda: d.censusFlowDepthPair(img, img, 7, 9, 9, foe, refine=True), lambda: d.censusFlowDepthPair(byte, byte, 7, 9, 9, foe, agg=5, refine=True),
                 lambda: d.censusFlowDepthPair(img, img, 7, 9, 9, foe, refine=True, consistency=1.0, gate=True, fill=True, median=5)):
        with pytest.raises(TypeError):
            call()
    # refine=True refines on the raw cost: with sgm= the message points to subpixel=True
    for sgm in ((1.0, 2.0), dict(P1=1.0, P2=2.0, min_unique=0.2)):
        with pytest.raises(ValueError, match="subpixel=True"):
            d.censusFlowDepthPair(img, img, 7, 9, 9, foe, refine=True, sgm=sgm)
        with pytest.raises(ValueError, match="subpixel=True"):
            d.censusFlowDepthPair(img, img, 7, 9, 9, foe, refine=True, sgm=sgm, subpixel=True)
    # subpixel=True without sgm stays the refusal it is, with and without refine
    for kw in (dict(subpixel=True), dict(subpixel=True, refine=True)):
        with pytest.raises(ValueError, match="needs sgm="):
            d.censusFlowDepthPair(img, img, 7, 9, 9, foe, **kw)
    # the stand-alone call's own arguments
    for call in (lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx[1:]), lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, agg=2),
                 lambda: d.censusRefineSubpixel(sig, sig, 33, 9, idx), lambda: d.censusRefineSubpixel(sig, sig[:, 1:], 9, 9, idx),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, pad_t=-1), lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, pad_l=1.0),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, flow_y=torch.zeros((24, 44))),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, flow_y=torch.zeros((24, 44)), flow_x=torch.zeros((24, 45))),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, flow_y=torch.zeros((24, 44)), flow_x=torch.zeros((24, 44)), pad_l=1),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, flow_y=torch.zeros((24, 88))[:, ::2], flow_x=torch.zeros((24, 88))[:, ::2])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx.int()), lambda: d.censusRefineSubpixel(sig.float(), sig.float(), 9, 9, idx),
                 lambda: d.censusRefineSubpixel(sig, sig, 9, 9, idx, flow_y=torch.zeros((24, 44)).double(), flow_x=torch.zeros((24, 44)).double())):
        with pytest.raises(TypeError):
            call()


def _model(d, k=7, maxh=8, maxw=8, ratios=(1, 2, 4), **kwargs):
    geo = dict(maxh=maxh, maxw=maxw, ratios=list(ratios), multiscale=True, hKernel=k, wKernel=k, hImg=32, wImg=48, output_extraction_method="max")
    return d.MultiscaleModel(geo, **kwargs)


def test_refine_key_of_the_pyramids_census_argument():
    import depth_estimation_amd as d

    img = torch.zeros((3, 32, 48))
    byte = img.to(torch.uint8)
    m = _model(d)
    # the values are accepted; the CPU tensor is not
    for call in (lambda: m.forwardFlow([img, img], census=dict(refine=True)), lambda: m.forwardFlow([img, img], census=dict(agg=3, beta=None, refine=True)),
                 lambda: m.forwardFlow([byte, byte], census=dict(agg=5, refine=True)), lambda: m.forwardFlow([img, img], census=dict(refine=True), one_call=False),
                 lambda: m.forwardFlow([img, img], census=dict(refine=False), process_full=False)):
        with pytest.raises(TypeError):
            call()
    # unknown keys stay refused, refine has to be a bool, and census= with subpixel=True stays the refusal it is
    for census in (dict(agg=3, gamma=1.0), dict(refine=True, gamma=1.0), dict(refine=1), dict(refine="yes"), dict(refine=None)):
        with pytest.raises(ValueError):
            m.forwardFlow([img, img], census=census)
    for kw in (dict(subpixel=True), dict(subpixel=True, one_call=False)):
        with pytest.raises(ValueError, match="subpixel=True"):
            m.forwardFlow([img, img], census=dict(refine=True), **kw)
    with pytest.raises(ValueError):
        m.forwardFlow([img, img], census=dict(refine=True), f16_scale=1.0)
    with pytest.raises(ValueError):
        m.forwardFlow([img, img], census=dict(refine=True, agg=2))
