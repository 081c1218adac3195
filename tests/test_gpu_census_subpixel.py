"""Sub-pixel flow on the raw census cost on the device (csrc/census_subpixel.hip; include/dfe.h) against its
numpy restatement (tests/census_subpixel_ref.py) BIT FOR BIT: the costs are integers and the fit is one float32 division, so there is no
tolerance anywhere.  Every output is pre-filled with a sentinel and has a guard band behind or around it.

The cases are chosen by the definition's edges (a region of 1 x 1, of one row, windows of one row, one column, 2 x 2, even and odd, a
winner on the window's border, constant frames, frames full of ties, class maps of another producer) and by the kernel's shape: a wave is
64 pixels of a row and a workgroup four rows, so the regions are 63, 65 and 127 wide and up to 22 high; the three box sizes are three
instantiations, the channels a loop."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import census_pyramid_ref as cp
from tests import census_ref as cr
from tests import census_subpixel_ref as sr
from tests import refpath as rp

pytestmark = pytest.mark.gpu
FILL = -7.0

# name: (C, H, W, k, hWin, wWin, agg, kind of frames)
CASES = {
    "1x1": (1, 7, 7, 3, 3, 3, 3, "random"),                 # Ha = Wa = 1
    "1xW": (2, 9, 130, 3, 3, 3, 5, "moved"),                # Ha = 1, Wa = 122
    "w63-1x9": (3, 20, 79, 7, 1, 9, 3, "moved"),            # Wa = 63, a window of one row
    "w65-9x1": (1, 24, 69, 5, 9, 1, 1, "moved"),            # Wa = 65, a window of one column, no box
    "w127-2x2": (4, 12, 130, 3, 2, 2, 1, "random"),         # Wa = 127, Ha = 9: three workgroups down, nothing to refine
    "8x8-ties": (2, 30, 50, 7, 8, 8, 3, "ties"),            # the even window
    "9x9": (3, 40, 60, 7, 9, 9, 5, "moved"),                # Ha = 22
    "33x33": (2, 37, 40, 3, 33, 33, 3, "moved"),            # the headline window on the smallest frame that holds it: Ha = 1, Wa = 4
    "border": (1, 30, 70, 7, 9, 9, 3, "moved44"),           # the winner on the window's corner
    "constant": (1, 30, 70, 7, 9, 9, 3, "constant"),
    "two-cell-ties": (1, 20, 70, 3, 5, 5, 1, "bits"),       # 8 bits a pixel: minima side by side
    "C4-k5": (4, 26, 48, 5, 3, 3, 5, "random"),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _frames(name):
    Cc, H, W, k, hWin, wWin, agg, kind = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    if kind == "constant":
        return np.full((Cc, H, W), 17, np.uint8), np.full((Cc, H, W), 200, np.uint8)
    if kind == "ties":
        return rng.randint(0, 4, size=(Cc, H, W)).astype(np.uint8), rng.randint(0, 4, size=(Cc, H, W)).astype(np.uint8)
    if kind == "bits":
        return rng.randint(0, 2, size=(Cc, H, W)).astype(np.uint8), rng.randint(0, 2, size=(Cc, H, W)).astype(np.uint8)
    f0 = rng.randint(0, 256, size=(Cc, H, W)).astype(np.float64)
    for _ in range(2):                                      # a little smoothing: neighbouring cells cost alike, the fit has something to do
        f0 = (f0 + np.roll(f0, 1, 1) + np.roll(f0, 1, 2) + np.roll(f0, (1, 1), (1, 2))) / 4.0
    f0 = np.floor(f0).astype(np.uint8)
    if kind == "random":
        return f0, rng.randint(0, 256, size=(Cc, H, W)).astype(np.uint8)
    move = (4, -4) if kind == "moved44" else (1, -1)
    f1 = np.roll(f0, move, (1, 2)).astype(np.float64) * 0.5 + 40 + rng.normal(0, 2, size=(Cc, H, W))   # moved, darker, noisy
    return f0, np.clip(np.floor(f1), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """the case's signatures, cost, integer flow and refined flow by the definition: computed once, read by every test"""
    Cc, H, W, k, hWin, wWin, agg, _ = CASES[name]
    f0, f1 = _frames(name)
    s0, s1 = cr.signature(f0, k, k), cr.signature(f1, k, k)
    cost = cr.cost_volume(s0, s1, hWin, wWin, agg)
    idx, best = cr.arg_best(cost)
    iy, ix = cr.decode(idx, hWin, wWin)
    fy, fx = sr.refine(cost, idx)
    out = dict(s0=s0, s1=s1, cost=cost, idx=idx, best=best.astype(np.float32), match=cr.match_score(best, k * k - 1, Cc, agg), int_y=iy, int_x=ix, flow_y=fy,
               flow_x=fx)
    for a in out.values():
        a.setflags(write=False)
    return out


def _dev_sig(s, cuda):
    return torch.from_numpy(np.array(s).view(np.int64)).to(cuda)      # (a copy: the reference's arrays are read-only)


def _refine_alone(dfe, cuda, s0, s1, hWin, wWin, agg, idx, pad_t=0, pad_l=0, extra_h=0, extra_w=0):
    """dfe_census_refine_subpixel_f32 into sentinel planes of (pad_t + Ha + extra_h) x (pad_l + Wa + extra_w): (fy, fx) as numpy"""
    Ha, Wa = idx.shape
    Cc, Hp, Wp = s0.shape
    fy = torch.full((pad_t + Ha + extra_h, pad_l + Wa + extra_w), FILL, device=cuda)
    fx = torch.full_like(fy, FILL)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    ctx.check(lib.dfe_census_refine_subpixel_f32(ctx.handle, s0.data_ptr(), s1.data_ptr(), Cc, Hp, Wp, hWin, wWin, agg, idx.data_ptr(), fy.data_ptr(), fx.data_ptr(),
                                                 fy.shape[1], pad_t, pad_l))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "cenfit_refine_kernel"
    return fy.cpu().numpy(), fx.cpu().numpy()


# ---- the refinement alone and censusFlow(refine=True) ----
@pytest.mark.parametrize("name", list(CASES))
def test_refine_alone_and_censusFlow_equal_the_definition(dfe, cuda, name):
    Cc, H, W, k, hWin, wWin, agg, kind = CASES[name]
    ref = _ref(name)
    Ha, Wa = ref["idx"].shape
    s0, s1 = _dev_sig(ref["s0"], cuda), _dev_sig(ref["s1"], cuda)
    # what the case is there for, on the reference
    off_y, off_x = ref["flow_y"] - ref["int_y"], ref["flow_x"] - ref["int_x"]
    assert np.abs(off_y).max() <= 0.5 and np.abs(off_x).max() <= 0.5
    if name == "1x1":
        assert (Ha, Wa) == (1, 1)
    if name in ("1xW", "33x33"):
        assert Ha == 1
    if name == "w127-2x2":
        assert Wa == 127 and not off_y.any() and not off_x.any()
    if name == "w63-1x9":
        assert Wa == 63 and not off_y.any() and off_x.any()
    if name == "w65-9x1":
        assert Wa == 65 and off_y.any() and not off_x.any()
    if name == "border":
        assert ((ref["int_y"] == 4) & (ref["int_x"] == -4)).mean() > 0.9 and not off_y[ref["int_y"] == 4].any() and not off_x[ref["int_x"] == -4].any()
    if name == "constant":
        assert not ref["cost"].any() and (ref["idx"] == cr.middle_index(hWin, wWin)).all() and not ref["flow_y"].any() and not ref["flow_x"].any()
    if name == "two-cell-ties":
        assert (np.abs(off_x) == 0.5).sum() >= 10 and (np.abs(off_y) == 0.5).sum() >= 10
    if name in ("9x9", "w63-1x9"):
        assert ((off_x != 0) & (np.abs(off_x) < 0.5)).mean() > 0.5               # most pixels get a fit of their own

    # the sweep with refine=True: idx, best and match are the sweep's, the flow is the refined one
    plain = dfe.censusFlow(s0, s1, k * k - 1, hWin, wWin, agg)
    res = dfe.censusFlow(s0, s1, k * k - 1, hWin, wWin, agg, refine=True)
    assert sorted(res) == ["best", "flow_x", "flow_y", "idx", "match"]
    assert np.array_equal(res["idx"].cpu().numpy(), ref["idx"])
    for key in ("idx", "best", "match"):
        assert torch.equal(res[key], plain[key]), key
    assert np.array_equal(plain["flow_y"].cpu().numpy(), ref["int_y"]) and np.array_equal(plain["flow_x"].cpu().numpy(), ref["int_x"])
    for key in ("flow_y", "flow_x", "match", "best"):
        assert np.array_equal(_bits(res[key].cpu().numpy()), _bits(ref[key])), key

    # the entry alone, at a pitch and pads other than the region's own: the region bit for bit, the sentinel everywhere else
    idx = torch.from_numpy(ref["idx"].copy()).to(cuda)
    for pt, pl, eh, ew in ((0, 0, 0, 0), (2, 3, 1, 5)):
        gy, gx = _refine_alone(dfe, cuda, s0, s1, hWin, wWin, agg, idx, pt, pl, eh, ew)
        for g, key in ((gy, "flow_y"), (gx, "flow_x")):
            want = np.full(g.shape, FILL, np.float32)
            want[pt:pt + Ha, pl:pl + Wa] = ref[key]
            assert np.array_equal(_bits(g), _bits(want)), (key, pt, pl)
    fy, fx = dfe.censusRefineSubpixel(s0, s1, hWin, wWin, idx, agg)
    assert torch.equal(fy, res["flow_y"]) and torch.equal(fx, res["flow_x"])


@pytest.mark.parametrize("name", ["9x9", "8x8-ties", "w65-9x1", "C4-k5", "33x33"])
def test_class_map_of_another_producer(dfe, cuda, name):
    """any class of the window at every pixel -- c0 is rarely the minimum: the clamp and the m > 0 test -- and, sprinkled in, ids that are
    no class (0, hWin wWin + 1, a negative one), whose pixels keep the sentinel"""
    Cc, H, W, k, hWin, wWin, agg, _ = CASES[name]
    ref = _ref(name)
    Ha, Wa = ref["idx"].shape
    rng = np.random.RandomState(3)
    idx = rng.randint(1, hWin * wWin + 1, size=(Ha, Wa)).astype(np.int64)
    bad = rng.uniform(size=(Ha, Wa)) < 0.2
    idx[bad] = rng.choice([0, hWin * wWin + 1, -5], size=int(bad.sum()))
    idx[0, 0], idx[-1, -1] = 0, hWin * wWin + 1
    want_y, want_x = sr.refine(ref["cost"], idx, np.full((Ha, Wa), FILL, np.float32), np.full((Ha, Wa), FILL, np.float32))
    assert (want_y[idx < 1] == FILL).all() and (want_x[idx > hWin * wWin] == FILL).all() and want_y[0, 0] == FILL and want_x[-1, -1] == FILL
    ok = (idx >= 1) & (idx <= hWin * wWin)
    iy, ix = cr.decode(idx, hWin, wWin)
    if name == "9x9":
        assert (np.abs(want_x - ix)[ok] == 0.5).mean() > 0.2                      # the clamp is at work
    gy, gx = _refine_alone(dfe, cuda, _dev_sig(ref["s0"], cuda), _dev_sig(ref["s1"], cuda), hWin, wWin, agg, torch.from_numpy(idx).to(cuda))
    assert np.array_equal(_bits(gy), _bits(want_y)) and np.array_equal(_bits(gx), _bits(want_x))


# ---- the one call ----
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("name", ["9x9", "8x8-ties", "w65-9x1", "1x1"])
def test_one_call_equals_the_staged_calls_and_the_paste(dfe, cuda, name, dtype):
    Cc, H, W, k, hWin, wWin, agg, _ = CASES[name]
    ref = _ref(name)
    f0, f1 = (torch.from_numpy(f).to(cuda) for f in _frames(name))
    if dtype == "f32":
        f0, f1 = f0.float() * 0.5, f1.float() * 0.5
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    cx, cy = W / 2 - 3.5, H / 2 + 1.25

    def call(stem, depth_too=True):
        flow = torch.full((2 * H * W + 64,), FILL, device=cuda)
        match, depth, conf = (torch.full((H * W + 64,), FILL, device=cuda) for _ in range(3))
        dp, cp_ = (depth.data_ptr(), conf.data_ptr()) if depth_too else (None, None)
        if dtype == "u8":
            rc = getattr(lib, stem + "u8")(ctx.handle, f0.data_ptr(), f1.data_ptr(), Cc, H, W, k, hWin, wWin, agg, cx, cy, 0.25, flow.data_ptr(), match.data_ptr(), dp, cp_)
        else:
            rc = getattr(lib, stem + "f32")(ctx.handle, f0.data_ptr(), f1.data_ptr(), Cc, H, W, k, hWin, wWin, agg, cx, cy, flow.data_ptr(), match.data_ptr(), dp, cp_)
        ctx.check(rc)
        torch.cuda.synchronize()
        for t in (flow, match) + ((depth, conf) if depth_too else ()):
            assert (t[-64:] == FILL).all(), "wrote behind an output"
        return flow[:-64].view(2, H, W), match[:-64].view(H, W), depth[:-64].view(H, W), conf[:-64].view(H, W)

    flow, match, depth, conf = call("dfe_census_flow_depth_pair_subpixel_")
    assert ctx.last_kernel() == "cenfit_refine_kernel"
    pflow, pmatch, pdepth, pconf = call("dfe_census_flow_depth_pair_")
    pt, pl, Ha, Wa = cr.region(H, W, k, k, hWin, wWin, agg)
    # the plain one call is what it was: the definition's integer flow and score
    assert np.array_equal(pflow[0].cpu().numpy(), cr.paste(ref["int_y"], H, W, pt, pl)) and np.array_equal(pflow[1].cpu().numpy(), cr.paste(ref["int_x"], H, W, pt, pl))
    assert np.array_equal(_bits(pmatch.cpu().numpy()), _bits(cr.paste(ref["match"], H, W, pt, pl)))
    # match and the border are the plain call's
    assert torch.equal(match.view(torch.int32), pmatch.view(torch.int32))
    border = torch.ones((H, W), dtype=torch.bool, device=cuda)
    border[pt:pt + Ha, pl:pl + Wa] = False
    assert not flow[:, border].any() and torch.equal(flow[:, border], pflow[:, border])
    # the staged composition: two transforms, the sweep, the refinement alone into the pasted planes, the paste of the score, the depth
    s0, s1 = dfe.censusTransform(f0, k), dfe.censusTransform(f1, k)
    r = dfe.censusFlow(s0, s1, k * k - 1, hWin, wWin, agg)
    eflow = torch.zeros((2, H, W), device=cuda)
    dfe.censusRefineSubpixel(s0, s1, hWin, wWin, r["idx"], agg, flow_y=eflow[0], flow_x=eflow[1], pad_t=pt, pad_l=pl)
    assert torch.equal(flow.view(torch.int32), eflow.view(torch.int32))
    # ... and the definition
    assert np.array_equal(_bits(flow[0].cpu().numpy()), _bits(cr.paste(ref["flow_y"], H, W, pt, pl)))
    assert np.array_equal(_bits(flow[1].cpu().numpy()), _bits(cr.paste(ref["flow_x"], H, W, pt, pl)))
    # depth from the refined flow, as the step makes it from its own
    ed, ec = torch.empty((H, W), device=cuda), torch.empty((H, W), device=cuda)
    ctx.check(lib.dfe_flow_to_depth_cartesian(ctx.handle, flow.contiguous().data_ptr(), H, W, cx, cy, 0, ed.data_ptr(), ec.data_ptr()))
    assert torch.equal(depth.view(torch.int32), ed.view(torch.int32)) and torch.equal(conf, ec)
    if name == "9x9":
        assert not torch.equal(depth, pdepth)
    # depth and depth_conf may both be NULL; the wrapper returns the same planes
    flow2, match2, _, _ = call("dfe_census_flow_depth_pair_subpixel_", depth_too=False)
    assert torch.equal(flow2.view(torch.int32), flow.view(torch.int32)) and torch.equal(match2, match)
    res = dfe.censusFlowDepthPair(f0, f1, k, hWin, wWin, (cx, cy), agg=agg, refine=True)
    assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], match) and torch.equal(res["depth"], depth) and torch.equal(res["depth_conf"], conf)


def test_consistency_gate_fill_and_median_on_the_refined_flow(dfe, cuda):
    f0, f1 = (torch.from_numpy(f).to(cuda) for f in sr.scene(1, (2.3, -2.6), 3))
    k, win, foe = 7, 9, (36.0, 28.0)
    R = cr.region(56, 72, k, k, win, win, 3)
    fwd = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, refine=True)
    back = dfe.censusFlowDepthPair(f1, f0, k, win, win, foe, agg=3, refine=True)
    plain = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3)
    assert torch.equal(fwd["scores"], plain["scores"]) and not torch.equal(fwd["flow"], plain["flow"]) and (fwd["flow"] - plain["flow"]).abs().max() <= 0.5
    inner = fwd["flow"][:, R[0]:R[0] + R[2], R[1]:R[1] + R[3]].cpu().numpy()
    whole = plain["flow"][:, R[0]:R[0] + R[2], R[1]:R[1] + R[3]].cpu().numpy()
    assert sr.median_epe(inner[0], inner[1], (2.3, -2.6)) < 0.5 * sr.median_epe(whole[0], whole[1], (2.3, -2.6))
    res = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, refine=True, consistency=1.0, fill=True, median=5)
    ref = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, consistency=1.0, fill=True, median=5)
    assert sorted(res) == sorted(ref) and all(res[key].shape == ref[key].shape and res[key].dtype == ref[key].dtype for key in res)
    assert torch.equal(res["flow"], fwd["flow"]) and torch.equal(res["flow_bw"], back["flow"])              # both directions refined
    mask, err = dfe.flowConsistency(fwd["flow"], back["flow"], 1.0, R)
    assert torch.equal(res["consistent"], mask) and torch.equal(res["consistency_err"].view(torch.int32), err.view(torch.int32))
    dense, filled = dfe.fillHoles(fwd["flow"], (fwd["scores"] > 0).float() * mask, R, 0)
    assert torch.equal(res["flow_dense"].view(torch.int32), dense.view(torch.int32)) and torch.equal(res["filled"], filled)
    gated = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, refine=True, consistency=1.0, gate=True)
    assert torch.equal(gated["scores"], fwd["scores"] * mask) and torch.equal(gated["depth_conf"], fwd["depth_conf"] * mask)


def test_refusals_come_before_any_launch(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    sig = torch.zeros((5, 40, 60), dtype=torch.int64, device=cuda)
    idx = torch.ones((40, 60), dtype=torch.int64, device=cuda)
    out = torch.full((2, 40, 60), FILL, device=cuda)

    def refine(Cc=1, Hp=40, Wp=60, hWin=9, wWin=9, agg=3, pitch=60, pt=0, pl=0, s0=sig, i=idx, fy=out[0]):
        return lib.dfe_census_refine_subpixel_f32(ctx.handle, s0.data_ptr() if s0 is not None else None, sig.data_ptr(), Cc, Hp, Wp, hWin, wWin, agg,
                                                  i.data_ptr() if i is not None else None, fy.data_ptr() if fy is not None else None, out[1].data_ptr(), pitch, pt, pl)

    assert refine() == 0
    for kw in (dict(Cc=0), dict(Cc=5), dict(agg=2), dict(agg=0), dict(hWin=0), dict(s0=None), dict(i=None), dict(fy=None)):
        assert refine(**kw) == -1, kw                                                   # DFE_E_ARG
    assert refine(hWin=34, wWin=33) == -5                                               # DFE_E_UNSUPPORTED
    for kw in (dict(Hp=0), dict(Hp=10), dict(Wp=32769), dict(pitch=49), dict(pt=-1), dict(pl=11)):
        assert refine(**kw) == -2, kw                                                   # DFE_E_SHAPE (the region is 30 x 50)
    f = torch.zeros((3, 40, 60), device=cuda)
    for kw in (dict(C=5), dict(k=4), dict(agg=7), dict(hWin=40), dict(flow=None), dict(depth=None)):
        a = dict(C=3, k=7, hWin=9, agg=3, flow=out, depth=out[0])
        a.update(kw)
        rc = lib.dfe_census_flow_depth_pair_subpixel_f32(ctx.handle, f.data_ptr(), f.data_ptr(), a["C"], 40, 60, a["k"], a["hWin"], 9, a["agg"], 30.0, 20.0,
                                                         a["flow"].data_ptr() if a["flow"] is not None else None, out[1].data_ptr(),
                                                         a["depth"].data_ptr() if a["depth"] is not None else None, out[1].data_ptr())
        assert rc < 0, kw
    assert lib.dfe_census_flow_depth_pair_subpixel_u8(ctx.handle, f.data_ptr(), f.data_ptr(), 3, 40, 60, 7, 9, 9, 3, 30.0, 20.0, 0.0, out.data_ptr(), out[1].data_ptr(),
                                                      None, None) == -1


# ---- the pyramid ----
# name: (ratios, maxh, maxw, k, C, H, W, max planted flow, agg)
PYRAMID = {
    "8x8-124": ([1, 2, 4], 8, 8, 7, 3, 64, 96, 14, 3),       # the one-launch volume kernel, three scales
    "8x8-12-ragged": ([1, 2], 8, 8, 7, 3, 34, 42, 7, 3),     # W % 8 = 2, H / 2 odd (row 3 of census_pyramid_ref's table)
    "8x8-C1-nobox": ([1, 2], 8, 8, 7, 1, 32, 48, 7, 1),
    "16x4-124": ([1, 2, 4], 16, 4, 7, 3, 64, 88, 14, 3),     # the staged volume kernels (row 5)
    "4x8-k5-a5": ([1, 2], 4, 8, 5, 4, 40, 56, 6, 5),         # maxh = 2 d: empty side blocks; the widest box, four channels
    "5x7-one-scale": ([1], 5, 7, 3, 2, 19, 23, 2, 3),        # nothing aligned (row 8)
}


@functools.lru_cache(maxsize=None)
def _pyr(name):
    """the case's frames (byte-valued, frame 1 darker and offset), the reference chain's class map, the integer volumes, and the
    refinement of that class map by the definition: computed once, shared read-only"""
    ratios, mh, mw, k, Cc, H, W, mf, a = PYRAMID[name]
    f0, f1, _, _ = rp.synth_pair(H, W, C=Cc, seed=1, max_flow=mf, noise_sigma=2.0)
    f1 = np.floor(f1 * np.float32(cp.GAIN) + np.float32(cp.OFFSET)).astype(np.float32)
    ch = cp.chain(f0, f1, k, mh, mw, ratios, a, cp.default_beta(Cc, a))
    vols = [cp.scale_volume(f0, f1, r, k, mh, mw, a, 1.0) for r in ratios]      # beta = 1: the integer costs as exact floats
    flow, scale = sr.pyramid_refine(vols, ch["idx"], mh, mw, ratios)
    out = dict(f0=f0, f1=f1, idx=ch["idx"], y=ch["y"], x=ch["x"], vols=vols, flow=flow, scale=scale)
    for v in [f0, f1, out["idx"], flow, scale] + vols:
        v.setflags(write=False)
    return out


def _rr(ratios):
    from depth_estimation_amd._lib import ratios_array

    return ratios_array(ratios)


def _pyr_refine_alone(dfe, cuda, t0, t1, k, mh, mw, ratios, a, idx):
    Cc, H, W = t0.shape
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    rr, n = _rr(ratios)
    flow = torch.full((2 * H * W + 64,), FILL, device=cuda)
    ti = torch.from_numpy(np.array(idx)).to(cuda)
    ctx.check(lib.dfe_multiscale_census_refine_subpixel_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, a, ti.data_ptr(), flow.data_ptr()))
    torch.cuda.synchronize()
    g = flow.cpu().numpy()
    assert (g[2 * H * W:] == FILL).all(), "wrote behind the flow"
    return g[:2 * H * W].reshape(2, H, W)


def _pyr_one_call(dfe, cuda, t0, t1, k, mh, mw, ratios, a, beta, stem, with_idx=True):
    Cc, H, W = t0.shape
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    rr, n = _rr(ratios)
    flow = torch.full((2 * H * W + 64,), FILL, device=cuda)
    idx = torch.full((H * W + 64,), -7, dtype=torch.int64, device=cuda)
    fn = getattr(lib, stem + ("u8" if t0.dtype == torch.uint8 else "f32"))
    ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, a, beta, flow.data_ptr(), idx.data_ptr() if with_idx else None))
    torch.cuda.synchronize()
    g, gi = flow.cpu().numpy(), idx.cpu().numpy()
    assert (g[2 * H * W:] == FILL).all() and (gi[H * W:] == -7).all(), "wrote behind an output"
    assert with_idx or (gi == -7).all()
    return g[:2 * H * W].reshape(2, H, W), gi[:H * W].reshape(H, W), ctx.multiscale_last_path()


@pytest.mark.parametrize("name", list(PYRAMID))
def test_pyramid_refinement_equals_the_definition(dfe, cuda, name):
    ratios, mh, mw, k, Cc, H, W, mf, a = PYRAMID[name]
    ref = _pyr(name)
    beta = cp.default_beta(Cc, a)
    t0, t1 = torch.from_numpy(ref["f0"].copy()).to(cuda), torch.from_numpy(ref["f1"].copy()).to(cuda)
    rho = np.array(ratios)[np.maximum(ref["scale"], 0)]
    # on the reference: every pixel has a class, a coarse scale wins some of them inside the ring geometry, the fit stays within rho / 2
    assert (ref["scale"] >= 0).all()
    if len(ratios) > 1:
        assert all((ref["scale"] == s).sum() >= 50 for s in range(1, len(ratios))), [(ref["scale"] == s).sum() for s in range(len(ratios))]
        coarse = ref["scale"] >= 1
        assert (ref["flow"][:, coarse] != np.stack([ref["y"], ref["x"]])[:, coarse]).any()      # ... and is refined there
    assert (np.abs(ref["flow"][0] - ref["y"]) <= rho / 2).all() and (np.abs(ref["flow"][1] - ref["x"]) <= rho / 2).all()

    # the refinement alone on the reference's class map
    got = _pyr_refine_alone(dfe, cuda, t0, t1, k, mh, mw, ratios, a, ref["idx"])
    assert np.array_equal(_bits(got), _bits(ref["flow"]))

    # the one call: the matcher unchanged, its flow refined in place from its own signatures
    pflow, pidx, ppath = _pyr_one_call(dfe, cuda, t0, t1, k, mh, mw, ratios, a, beta, "dfe_multiscale_census_flow_pair_")
    flow, idx, path = _pyr_one_call(dfe, cuda, t0, t1, k, mh, mw, ratios, a, beta, "dfe_multiscale_census_flow_pair_subpixel_")
    assert path == ppath and path.split()[-1] == ("census_pyramid_volume_kernel" if (mh, mw) == (8, 8) else "census_volume_kernel")
    assert np.array_equal(idx, pidx)
    want, scale = sr.pyramid_refine(ref["vols"], idx, mh, mw, ratios)
    assert np.array_equal(_bits(flow), _bits(want)), "one call against the definition on its own class map"
    assert np.array_equal(_bits(flow), _bits(_pyr_refine_alone(dfe, cuda, t0, t1, k, mh, mw, ratios, a, idx))), "one call against the refinement alone"
    rho = np.array(ratios)[scale]
    assert (np.abs(flow - pflow) <= rho / 2).all()
    # without idx, and the byte entry on the same values
    flow2, _, _ = _pyr_one_call(dfe, cuda, t0, t1, k, mh, mw, ratios, a, beta, "dfe_multiscale_census_flow_pair_subpixel_", with_idx=False)
    assert np.array_equal(_bits(flow2), _bits(flow))
    b0, b1 = t0.to(torch.uint8), t1.to(torch.uint8)
    bflow, bidx, _ = _pyr_one_call(dfe, cuda, b0, b1, k, mh, mw, ratios, a, beta, "dfe_multiscale_census_flow_pair_subpixel_")
    assert np.array_equal(_bits(bflow), _bits(flow)) and np.array_equal(bidx, idx)

    # ids that are no class keep what flow held
    foreign = idx.copy()
    foreign[::3, ::5] = 0
    foreign[1::4, 2::7] = int(dfe.lib().dfe_multi_nclasses(mh, mw, _rr(ratios)[0], len(ratios))) + 1
    want, _ = sr.pyramid_refine(ref["vols"], foreign, mh, mw, ratios, flow=np.full((2, H, W), FILL, np.float32))
    assert (want[:, ::3, ::5] == FILL).all()
    assert np.array_equal(_bits(_pyr_refine_alone(dfe, cuda, t0, t1, k, mh, mw, ratios, a, foreign)), _bits(want))


@pytest.mark.parametrize("name", ["8x8-124", "16x4-124"])
def test_pyramid_python_key(dfe, cuda, name):
    ratios, mh, mw, k, Cc, H, W, mf, a = PYRAMID[name]
    ref = _pyr(name)
    t0, t1 = torch.from_numpy(ref["f0"].copy()).to(cuda), torch.from_numpy(ref["f1"].copy()).to(cuda)
    geo = dict(maxh=mh, maxw=mw, ratios=list(ratios), multiscale=True, hKernel=k, wKernel=k, hImg=H, wImg=W, output_extraction_method="max")
    m = dfe.MultiscaleModel(geo)
    plain = m.forwardFlow([t0, t1], census=dict(agg=a))
    one = m.forwardFlow([t0, t1], census=dict(agg=a, refine=True))
    staged = m.forwardFlow([t0, t1], census=dict(agg=a, refine=True), one_call=False)
    assert "y_sub" not in plain
    want, _ = sr.pyramid_refine(ref["vols"], one["index"].cpu().numpy(), mh, mw, ratios)
    for res in (one, staged):
        assert sorted(res) == sorted(list(plain) + ["y_sub", "x_sub"])
        for key in ("index", "y", "x", "confidences"):
            assert torch.equal(res[key], plain[key]), key
        assert np.array_equal(_bits(res["y_sub"].cpu().numpy()), _bits(want[0])) and np.array_equal(_bits(res["x_sub"].cpu().numpy()), _bits(want[1]))
        assert torch.equal(res["full"], torch.stack([res["y_sub"], res["x_sub"]]))
    byte = m.forwardFlow([t0.to(torch.uint8), t1.to(torch.uint8)], census=dict(agg=a, refine=True))
    assert torch.equal(byte["y_sub"], one["y_sub"]) and torch.equal(byte["x_sub"], one["x_sub"])
