"""The census matcher on the device (include/dfe.h: dfe_census_*) against the numpy restatement of its definition
(tests/census_ref.py) BIT FOR BIT: everything up to the match score is integer arithmetic and the score is two rounded fp32 operations, so
there is no tolerance anywhere.  Every output is pre-filled with a sentinel.

The sweep's cases, beyond the shapes the definition's edges ask for (a single row of output, an even window, a non-square patch, a region
smaller than a tile, constant frames, frames full of ties), are chosen by the paths its launcher can take: the window staged whole, its
rows in several bands (33 x 33 with one channel and with four, 16 x 16 with three), a very wide window in bands of columns (2 x 200 with
four channels) and both at once (12 x 80); tiles of 8 rows (one and two channels) and of 4; several hundred tiles; windows with fewer
cells in a row than the workgroup has waves."""
import functools

import numpy as np
import pytest
import torch

from tests import census_ref as cr

pytestmark = pytest.mark.gpu
DFE_E_ARG, DFE_E_SHAPE, DFE_E_UNSUPPORTED = -1, -2, -5
FILL = -7.0

# name: (C, H, W, kh, kw, hWin, wWin, agg, kind of frames)
CASES = {
    "A": (1, 48, 80, 7, 7, 9, 9, 3, "moved"),
    "B": (3, 41, 83, 7, 7, 16, 16, 1, "random"),
    "C": (1, 45, 109, 7, 7, 33, 33, 3, "moved"),          # Ha = 5, Wa = 69: the headline window on a region smaller than any tile
    "D": (1, 13, 90, 5, 5, 5, 12, 5, "random"),            # Ha = 1
    "E": (2, 40, 75, 9, 7, 8, 15, 3, "moved"),
    "F": (1, 30, 70, 7, 7, 9, 9, 3, "constant"),
    "G": (2, 33, 75, 5, 5, 7, 8, 3, "ties"),
    "many-tiles": (2, 150, 400, 3, 3, 3, 2, 3, "moved"),     # 29 x 19 tiles, a window of fewer rows than a workgroup has waves
    "row-bands": (4, 45, 96, 3, 3, 33, 33, 3, "moved"),
    "column-bands": (4, 10, 225, 3, 3, 2, 200, 5, "random"),
    "both-bands": (4, 19, 115, 3, 3, 12, 80, 5, "random"),
}


# how the launcher bands the window of a case (40 KB of LDS: 40 / C rows of 128 signatures): the others stage it whole
PATHS = {"B": ", row bands", "C": ", row bands", "row-bands": ", row bands", "column-bands": ", column bands", "both-bands": ", row and column bands"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _frames(name):
    C, H, W, kh, kw, hWin, wWin, agg, kind = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    if kind == "constant":
        return np.full((C, H, W), 17, np.uint8), np.full((C, H, W), 200, np.uint8)
    if kind == "ties":
        return rng.randint(0, 4, size=(C, H, W)).astype(np.uint8), rng.randint(0, 4, size=(C, H, W)).astype(np.uint8)
    f0 = rng.randint(0, 256, size=(C, H, W)).astype(np.uint8)
    if kind == "random":
        return f0, rng.randint(0, 256, size=(C, H, W)).astype(np.uint8)
    f1 = np.roll(f0, (1, -1), (1, 2)).astype(np.float64) * 0.5 + 40 + rng.normal(0, 2, size=(C, H, W))   # moved, darker, noisy
    return f0, np.clip(np.floor(f1), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """the case's signatures, volume and flow by the definition: computed once, read by every test"""
    C, H, W, kh, kw, hWin, wWin, agg, _ = CASES[name]
    f0, f1 = _frames(name)
    s0, s1 = cr.signature(f0, kh, kw), cr.signature(f1, kh, kw)
    cost = cr.cost_volume(s0, s1, hWin, wWin, agg)
    idx, best = cr.arg_best(cost)
    fy, fx = cr.decode(idx, hWin, wWin)
    return dict(s0=s0, s1=s1, cost=cost, idx=idx, best=best.astype(np.float32), match=cr.match_score(best, kh * kw - 1, C, agg), flow_y=fy, flow_x=fx)


def _sig(t):
    return t.cpu().numpy().view(np.uint64)


def _dev_sig(s, cuda):
    return torch.from_numpy(np.ascontiguousarray(s).view(np.int64)).to(cuda)


# ---- the transform ----
TRANSFORMS = [(1, 7, 7, 7, 7), (3, 19, 70, 7, 7), (1, 12, 67, 3, 5), (2, 13, 66, 9, 7), (4, 9, 130, 5, 5), (1, 24, 66, 21, 3), (1, 5, 90, 3, 21)]


@pytest.mark.parametrize("C,H,W,kh,kw", TRANSFORMS, ids=["%dx%dx%d-k%dx%d" % t for t in TRANSFORMS])
def test_transform_f32_and_u8_equal_the_definition(dfe, cuda, C, H, W, kh, kw):
    f = np.random.RandomState(C * H + W).randint(0, 256, size=(C, H, W)).astype(np.uint8)
    want = cr.signature(f, kh, kw)
    su = _sig(dfe.censusTransform(torch.from_numpy(f).to(cuda), (kh, kw)))
    sf = _sig(dfe.censusTransform(torch.from_numpy(f.astype(np.float32) * 0.37).to(cuda), (kh, kw)))
    assert su.shape == want.shape and np.array_equal(su, want), "u8"
    assert np.array_equal(sf, want), "f32"


def test_transform_compares_strictly_and_false_with_a_nan(dfe, cuda):
    f = np.random.RandomState(5).randint(0, 4, size=(2, 20, 71)).astype(np.uint8)   # equal neighbours everywhere
    want = cr.signature(f, 7, 7)
    assert np.array_equal(_sig(dfe.censusTransform(torch.from_numpy(f).to(cuda), 7)), want)
    assert np.array_equal(_sig(dfe.censusTransform(torch.from_numpy(f).to(cuda).float(), 7)), want)
    g = np.random.RandomState(6).uniform(-1, 1, size=(1, 15, 40)).astype(np.float32)
    g[0, 7, 20] = np.nan
    g[0, 0, 0] = np.inf
    want = cr.signature(g, 5, 5)
    assert int(want[0, 5, 18]) == 0                                                  # the patch whose centre is the NaN
    assert np.array_equal(_sig(dfe.censusTransform(torch.from_numpy(g).to(cuda), 5)), want)


# ---- the staged volume and the fused sweep ----
@pytest.mark.parametrize("name", list(CASES))
def test_volume_and_fused_flow_equal_the_definition(dfe, cuda, name):
    C, H, W, kh, kw, hWin, wWin, agg, _ = CASES[name]
    ref = _ref(name)
    s0, s1 = _dev_sig(ref["s0"], cuda), _dev_sig(ref["s1"], cuda)
    Ha, Wa = ref["idx"].shape
    vol = dfe.censusCostVolume(s0, s1, hWin, wWin, agg)
    assert tuple(vol.shape) == (Ha, Wa, hWin, wWin)
    assert np.array_equal(vol.cpu().numpy(), ref["cost"].astype(np.float32)), "volume"

    ctx, lib = dfe.get_ctx(0), dfe.lib()
    out = {k: torch.full((Ha, Wa), FILL, device=cuda) for k in ("best", "match", "flow_y", "flow_x")}
    idx = torch.full((Ha, Wa), -7, dtype=torch.int64, device=cuda)
    ctx.check(lib.dfe_census_flow_f32(ctx.handle, s0.data_ptr(), s1.data_ptr(), C, ref["s0"].shape[1], ref["s0"].shape[2], kh * kw - 1, hWin, wWin, agg,
                                      idx.data_ptr(), out["best"].data_ptr(), out["match"].data_ptr(), out["flow_y"].data_ptr(), out["flow_x"].data_ptr()))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "census_sweep_kernel" + PATHS.get(name, "")
    assert np.array_equal(idx.cpu().numpy(), ref["idx"]), "idx"
    for k, t in out.items():
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(ref[k])), k
    if name == "F":
        assert (ref["idx"] == cr.middle_index(hWin, wWin)).all() and not ref["best"].any() and (ref["match"] == 1).all()

    # the fused sweep is the existing arg-min and decode on the staged volume
    P, N = Ha * Wa, hWin * wWin
    aidx = torch.full((P,), -7, dtype=torch.int64, device=cuda)
    abest = torch.full((P,), FILL, device=cuda)
    ctx.check(lib.dfe_argbest_center(ctx.handle, vol.data_ptr(), P, N, dfe.getMiddleIndex(dict(maxh=hWin, maxw=wWin)), 0, aidx.data_ptr(), abest.data_ptr()))
    y, x = torch.empty_like(aidx), torch.empty_like(aidx)
    ctx.check(lib.dfe_x2yx(ctx.handle, aidx.data_ptr(), P, hWin, wWin, y.data_ptr(), x.data_ptr()))
    assert torch.equal(aidx.view(Ha, Wa), idx) and torch.equal(abest.view(Ha, Wa), out["best"])
    assert torch.equal(y.view(Ha, Wa).float(), out["flow_y"]) and torch.equal(x.view(Ha, Wa).float(), out["flow_x"])

    # any output may be NULL; the wrapper returns the same planes
    ctx.check(lib.dfe_census_flow_f32(ctx.handle, s0.data_ptr(), s1.data_ptr(), C, ref["s0"].shape[1], ref["s0"].shape[2], kh * kw - 1, hWin, wWin, agg,
                                      None, None, None, None, None))
    res = dfe.censusFlow(s0, s1, kh * kw - 1, hWin, wWin, agg)
    assert sorted(res) == ["best", "flow_x", "flow_y", "idx", "match"]
    assert torch.equal(res["idx"], idx) and all(torch.equal(res[k], out[k]) for k in out)


# ---- the one call ----
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_one_call_equals_the_staged_calls_and_the_paste(dfe, cuda, name, dtype):
    C, H, W, k, _, hWin, wWin, agg, _ = CASES[name]
    ref = _ref(name)
    f0, f1 = (torch.from_numpy(f).to(cuda) for f in _frames(name))
    if dtype == "f32":
        f0, f1 = f0.float() * 0.5, f1.float() * 0.5
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    flow = torch.full((2, H, W), FILL, device=cuda)
    match, depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(3))
    cx, cy = W / 2 - 3.5, H / 2 + 1.25
    if dtype == "u8":
        rc = lib.dfe_census_flow_depth_pair_u8(ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, agg, cx, cy, 0.25, flow.data_ptr(),
                                               match.data_ptr(), depth.data_ptr(), conf.data_ptr())
    else:
        rc = lib.dfe_census_flow_depth_pair_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, agg, cx, cy, flow.data_ptr(),
                                                match.data_ptr(), depth.data_ptr(), conf.data_ptr())
    ctx.check(rc)
    torch.cuda.synchronize()
    # the staged public calls, pasted by hand
    r = dfe.censusFlow(dfe.censusTransform(f0, k), dfe.censusTransform(f1, k), k * k - 1, hWin, wWin, agg)
    pt, pl, Ha, Wa = cr.region(H, W, k, k, hWin, wWin, agg)
    eflow = torch.zeros((2, H, W), device=cuda)
    ematch = torch.zeros((H, W), device=cuda)
    eflow[0, pt:pt + Ha, pl:pl + Wa], eflow[1, pt:pt + Ha, pl:pl + Wa], ematch[pt:pt + Ha, pl:pl + Wa] = r["flow_y"], r["flow_x"], r["match"]
    assert torch.equal(flow, eflow) and torch.equal(match.view(torch.int32), ematch.view(torch.int32))
    # ... and the definition
    assert np.array_equal(flow[0].cpu().numpy(), cr.paste(ref["flow_y"], H, W, pt, pl)) and np.array_equal(flow[1].cpu().numpy(), cr.paste(ref["flow_x"], H, W, pt, pl))
    assert np.array_equal(_bits(match.cpu().numpy()), _bits(cr.paste(ref["match"], H, W, pt, pl)))
    # depth as the single-scale step makes it from its pasted flow
    ed, ec = torch.empty((H, W), device=cuda), torch.empty((H, W), device=cuda)
    ctx.check(lib.dfe_flow_to_depth_cartesian(ctx.handle, flow.data_ptr(), H, W, cx, cy, 0, ed.data_ptr(), ec.data_ptr()))
    assert torch.equal(depth.view(torch.int32), ed.view(torch.int32)) and torch.equal(conf, ec)
    # depth and depth_conf may both be NULL
    flow2 = torch.full((2, H, W), FILL, device=cuda)
    match2 = torch.full((H, W), FILL, device=cuda)
    res = dfe.censusFlowDepthPair(f0, f1, k, hWin, wWin, (cx, cy), agg=agg)
    assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], match) and torch.equal(res["depth"], depth) and torch.equal(res["depth_conf"], conf)
    if dtype == "f32":
        ctx.check(lib.dfe_census_flow_depth_pair_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, agg, cx, cy, flow2.data_ptr(),
                                                     match2.data_ptr(), None, None))
        assert torch.equal(flow2, flow) and torch.equal(match2, match)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exposure_scene_through_the_one_call(dfe, cuda, seed):
    f0, f1 = cr.scene(seed)
    k, win = cr.SCENE["k"], cr.SCENE["win"]
    res = dfe.censusFlowDepthPair(torch.from_numpy(f0).to(cuda), torch.from_numpy(f1).to(cuda), k, win, win, (52.0, 36.0), agg=3)
    eflow, ematch = cr.pair(f0, f1, k, win, win, 3)
    assert np.array_equal(res["flow"].cpu().numpy(), eflow) and np.array_equal(_bits(res["scores"].cpu().numpy()), _bits(ematch))
    pt, pl, Ha, Wa = cr.region(72, 104, k, k, win, win, 3)
    inner = res["flow"][:, pt:pt + Ha, pl:pl + Wa].cpu().numpy()
    assert cr.share_wrong(inner[0], inner[1]) <= 0.01
    assert (res["scores"][pt:pt + Ha, pl:pl + Wa] > 0).all()


def test_consistency_fill_and_median_return_the_keys_of_flowDepthPair(dfe, cuda):
    f0, f1 = (torch.from_numpy(f).to(cuda) for f in cr.scene(1))
    k, win, foe = 7, 9, (52.0, 36.0)
    res = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, consistency=1.0, fill=True, median=5)
    ssd = dfe.flowDepthPair(f0, f1, k, win, win, foe, consistency=1.0, fill=True, median=5)
    assert sorted(res) == sorted(ssd)
    assert all(res[key].shape == ssd[key].shape and res[key].dtype == ssd[key].dtype for key in res)
    R = cr.region(72, 104, k, k, win, win, 3)
    plain = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3)
    back = dfe.censusFlowDepthPair(f1, f0, k, win, win, foe, agg=3)
    assert torch.equal(res["flow"], plain["flow"]) and torch.equal(res["scores"], plain["scores"]) and torch.equal(res["flow_bw"], back["flow"])
    mask, err = dfe.flowConsistency(plain["flow"], back["flow"], 1.0, R)
    assert torch.equal(res["consistent"], mask) and torch.equal(res["consistency_err"].view(torch.int32), err.view(torch.int32))
    dense, filled = dfe.fillHoles(plain["flow"], (plain["scores"] > 0).float() * mask, R, 0)
    assert torch.equal(res["flow_dense"].view(torch.int32), dense.view(torch.int32)) and torch.equal(res["filled"], filled)
    gated = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, consistency=1.0, gate=True)
    assert torch.equal(gated["scores"], plain["scores"] * mask) and torch.equal(gated["depth_conf"], plain["depth_conf"] * mask)


def test_refusals_come_before_any_launch(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    f = torch.zeros((5, 40, 60), device=cuda)
    sig = torch.full((5, 40, 60), -7, dtype=torch.int64, device=cuda)
    out = torch.full((4, 40, 60), FILL, device=cuda)

    def transform(C=1, H=40, W=60, kh=7, kw=7):
        return lib.dfe_census_transform_f32(ctx.handle, f.data_ptr(), C, H, W, kh, kw, sig.data_ptr())

    def sweep(C=1, Hp=34, Wp=54, nbits=48, hWin=9, wWin=9, agg=3):
        return lib.dfe_census_flow_f32(ctx.handle, sig.data_ptr(), sig.data_ptr(), C, Hp, Wp, nbits, hWin, wWin, agg, None, out.data_ptr(), None, None, None)

    def volume(C=1, Hp=34, Wp=54, hWin=9, wWin=9, agg=3):
        return lib.dfe_census_cost_volume_f32(ctx.handle, sig.data_ptr(), sig.data_ptr(), C, Hp, Wp, hWin, wWin, agg, out.data_ptr())

    def pair(C=1, H=40, W=60, k=7, hWin=9, wWin=9, agg=3):
        return lib.dfe_census_flow_depth_pair_f32(ctx.handle, f.data_ptr(), f.data_ptr(), C, H, W, k, hWin, wWin, agg, 30.0, 20.0, out.data_ptr(),
                                                  out[2].data_ptr(), None, None)

    for bad in (dict(kh=6), dict(kw=1), dict(kh=9, kw=9), dict(kh=-3), dict(C=5), dict(C=0)):
        assert transform(**bad) == DFE_E_ARG, bad
    assert transform(H=6) == DFE_E_SHAPE and transform(W=40000) == DFE_E_SHAPE
    for fn in (sweep, volume, pair):
        for bad in (dict(agg=2), dict(agg=7), dict(agg=0), dict(C=5), dict(hWin=0)):
            assert fn(**bad) == DFE_E_ARG, (fn.__name__, bad)
        assert fn(hWin=33, wWin=34) == DFE_E_UNSUPPORTED
    assert sweep(Hp=10) == DFE_E_SHAPE and volume(Wp=10) == DFE_E_SHAPE and pair(H=16) == DFE_E_SHAPE and pair(H=3) == DFE_E_SHAPE
    assert sweep(nbits=0) == DFE_E_ARG and sweep(nbits=64) == DFE_E_ARG
    assert pair(k=8) == DFE_E_ARG and pair(k=9) == DFE_E_ARG
    torch.cuda.synchronize()
    assert (sig == -7).all() and (out == FILL).all(), "a refused call wrote something"
