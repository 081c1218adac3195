"""Semi-global aggregation on the two-dimensional label plane on the device (include/dfe.h: dfe_sgm_plane_aggregate_f32 and
dfe_census_flow_depth_pair_sgm_*) against the numpy restatement of its definition (tests/sgm_plane_ref.py) BIT FOR
BIT -- the definition fixes every operation and the order of the sum, so there is no tolerance -- on random non-integer volumes, so that
the order of the sum shows.  Every output is pre-filled with a sentinel.

The windows are chosen by the kernel's forms (cells a lane 1, 2, 5, 9, 18): one cell, one row and one column of cells, 64 cells exactly
and 65, 9 x 9, 16 x 16 (256 = 4 a lane exactly), 17 x 17, 33 x 33 and 8 x 137, the ceiling of 1096.  The planes: a pixel, a row, a column,
planes much wider than high and the reverse (the diagonal restarts at the sides) and 33 x 40 (lines longer than one prefetch window)."""
import numpy as np
import pytest
import torch

from tests import census_ref as cr
from tests import sgm_plane_ref as pr

pytestmark = pytest.mark.gpu
DFE_E_ARG, DFE_E_SHAPE, DFE_E_UNSUPPORTED = -1, -2, -5
FILL = -7.0
F = np.float32
WINDOWS = ((1, 1), (1, 9), (9, 1), (3, 3), (8, 8), (5, 13), (9, 9), (16, 16), (17, 17), (33, 33), (8, 137))
PLANES = ((1, 1), (1, 12), (12, 1), (3, 70), (70, 3), (33, 40))
PATHS = (0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x0f, 0xf0, 0x05, 0xff)
PENALTIES = ((0.5, 4.0), (2.25, 16.5), (3.0, 3.0), (0.0, 1.5))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _volume(shape, seed):
    return np.random.default_rng(seed).uniform(-3, 9, size=shape).astype(F)


def aggregate(dfe, cuda, vol, P1, P2, paths, want=("agg", "idx", "flow_y", "flow_x")):
    """the raw call: every output as numpy, the sentinel where it was not given"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, hWin, wWin = vol.shape
    tv = torch.from_numpy(vol).to(cuda)
    out = dict(agg=torch.full(vol.shape, FILL, device=cuda), idx=torch.full((H, W), -7, dtype=torch.int64, device=cuda),
               flow_y=torch.full((H, W), FILL, device=cuda), flow_x=torch.full((H, W), FILL, device=cuda))
    p = [out[k].data_ptr() if k in want else None for k in ("agg", "idx", "flow_y", "flow_x")]
    ctx.check(lib.dfe_sgm_plane_aggregate_f32(ctx.handle, tv.data_ptr(), H, W, hWin, wWin, P1, P2, paths, *p))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "sgmp_path_kernel"
    assert torch.equal(tv.cpu(), torch.from_numpy(vol)), "the volume is an input"
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sum(single, paths):
    want = None
    for r in range(8):
        if paths >> r & 1:
            want = single[r] if want is None else (want + single[r]).astype(F)
    return want


def _check(got, want_agg, tag, want=("agg", "idx", "flow_y", "flow_x")):
    idx, fy, fx = pr.arg_best(want_agg)
    ref = dict(agg=want_agg, idx=idx, flow_y=fy, flow_x=fx)
    for k in ("agg", "idx", "flow_y", "flow_x"):
        if k not in want:
            assert (got[k] == FILL).all(), tag + ": %s was not given" % k
        elif k == "idx":
            assert np.array_equal(got[k], ref[k]), tag + ": idx"
        else:
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), tag + ": " + k


@pytest.mark.parametrize("i,win", list(enumerate(WINDOWS)), ids=["%dx%d" % w for w in WINDOWS])
def test_every_window_equals_the_definition_bit_for_bit(dfe, cuda, i, win):
    P1, P2 = PENALTIES[i % 4]
    for n, (H, W) in enumerate(((5, 7), (7, 5))):
        vol = _volume((H, W) + win, 10 * i + n)
        single = [pr.plane_path(vol, r, P1, P2) for r in range(8)]
        for paths in (0xff, 1 << (i + 4 * n) % 8, (0x0f, 0xf0)[n]):
            tag = "%dx%d window %dx%d paths 0x%02x P (%g, %g)" % (H, W, win[0], win[1], paths, P1, P2)
            _check(aggregate(dfe, cuda, vol, P1, P2, paths), _sum(single, paths), tag)


@pytest.mark.parametrize("i,plane", list(enumerate(PLANES)), ids=["%dx%d" % p for p in PLANES])
def test_every_plane_equals_the_definition_bit_for_bit(dfe, cuda, i, plane):
    P1, P2 = PENALTIES[(i + 1) % 4]
    vol = _volume(plane + (9, 9), 200 + i)
    single = [pr.plane_path(vol, r, P1, P2) for r in range(8)]
    for paths in (0xff, 0xf0, 0x05, 0x40, 0x80):
        tag = "%dx%d window 9x9 paths 0x%02x P (%g, %g)" % (plane[0], plane[1], paths, P1, P2)
        _check(aggregate(dfe, cuda, vol, P1, P2, paths), _sum(single, paths), tag)


def test_every_path_set_and_every_choice_of_outputs(dfe, cuda):
    vol = _volume((6, 9, 5, 13), 300)
    single = [pr.plane_path(vol, r, 0.5, 4.0) for r in range(8)]
    for paths in PATHS:
        _check(aggregate(dfe, cuda, vol, 0.5, 4.0, paths), _sum(single, paths), "paths 0x%02x" % paths)
    every = ("agg", "idx", "flow_y", "flow_x")
    for paths in (0xff, 0x08):                   # several directions; a single one, whose L goes straight into agg when agg is given
        for want in [every] + [tuple(k for k in every if k != drop) for drop in every] + [("agg",), ("idx",), ("flow_y",), ("flow_x",)]:
            _check(aggregate(dfe, cuda, vol, 0.5, 4.0, paths, want), _sum(single, paths), "paths 0x%02x outputs %s" % (paths, want), want)
    for r in range(8):                           # a single direction written straight into agg is that direction's L
        got = aggregate(dfe, cuda, vol, 0.5, 4.0, 1 << r, ("agg",))
        assert np.array_equal(_bits(got["agg"]), _bits(single[r])), r


def test_flat_pixels_take_the_centre_class(dfe, cuda):
    for hWin, wWin in ((3, 3), (4, 6), (9, 9), (8, 137)):
        got = aggregate(dfe, cuda, np.full((5, 7, hWin, wWin), 3.0, F), 1.0, 2.0, 0xff)
        assert (got["idx"] == cr.middle_index(hWin, wWin)).all(), (hWin, wWin)
    vol = _volume((6, 8, 9, 9), 7)
    vol[2:4] = 2.0                               # flat pixels among others, no penalty: every class of theirs ties
    got = aggregate(dfe, cuda, vol, 0.0, 0.0, 0x0f)
    _check(got, pr.plane_sum(vol, 0.0, 0.0, 0x0f), "flat rows")
    assert (got["idx"][2:4] == 41).all() and not got["flow_y"][2:4].any() and not got["flow_x"][2:4].any()


def test_a_census_volume_with_integer_penalties_gives_integers(dfe, cuda):
    vol = np.ascontiguousarray(pr.band_volume(0)[10:30, 20:60])      # many exact ties: the first-minimum rule shows
    for paths in (0x0f, 0xff):
        got = aggregate(dfe, cuda, vol, 144.0, 864.0, paths)
        _check(got, pr.plane_sum(vol, 144.0, 864.0, paths), "census volume, paths 0x%02x" % paths)
        assert np.array_equal(got["agg"], np.rint(got["agg"]))


def test_argument_errors(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, hWin, wWin = 5, 7, 3, 4
    vol = torch.zeros((H, W, 1097), device=cuda)
    agg = torch.full((H, W, 1097), FILL, device=cuda)
    idx = torch.full((H, W), -7, dtype=torch.int64, device=cuda)
    fy, fx = torch.full((H, W), FILL, device=cuda), torch.full((H, W), FILL, device=cuda)
    pv, outs = vol.data_ptr(), (agg.data_ptr(), idx.data_ptr(), fy.data_ptr(), fx.data_ptr())
    fn = lib.dfe_sgm_plane_aggregate_f32
    nan, inf = float("nan"), float("inf")
    assert fn(None, pv, H, W, hWin, wWin, 1.0, 2.0, 0x0f, *outs) == DFE_E_ARG
    assert fn(ctx.handle, None, H, W, hWin, wWin, 1.0, 2.0, 0x0f, *outs) == DFE_E_ARG
    assert fn(ctx.handle, pv, H, W, hWin, wWin, 1.0, 2.0, 0x0f, None, None, None, None) == DFE_E_ARG
    assert fn(ctx.handle, pv, H, W, hWin, wWin, 1.0, 2.0, 0x0f, pv, *outs[1:]) == DFE_E_ARG          # agg == volume
    for paths in (0, 256, 0x10f):
        assert fn(ctx.handle, pv, H, W, hWin, wWin, 1.0, 2.0, paths, *outs) == DFE_E_ARG, paths
    for P1, P2 in ((-1.0, 2.0), (3.0, 2.0), (nan, 2.0), (1.0, nan), (1.0, inf), (inf, inf), (-0.5, -0.25)):
        assert fn(ctx.handle, pv, H, W, hWin, wWin, P1, P2, 0x0f, *outs) == DFE_E_ARG, (P1, P2)
    for h, w in ((0, W), (H, 0), (-1, W), (65536, 65536)):
        assert fn(ctx.handle, pv, h, w, hWin, wWin, 1.0, 2.0, 0x0f, *outs) == DFE_E_SHAPE, (h, w)
    for wh, ww in ((0, 4), (3, 0), (-1, -1)):
        assert fn(ctx.handle, pv, H, W, wh, ww, 1.0, 2.0, 0x0f, *outs) == DFE_E_SHAPE, (wh, ww)
    for wh, ww in ((1, 1097), (1097, 1), (33, 34), (40000, 40000)):
        assert fn(ctx.handle, pv, H, W, wh, ww, 1.0, 2.0, 0x0f, *outs) == DFE_E_UNSUPPORTED, (wh, ww)
    torch.cuda.synchronize()
    assert (agg == FILL).all() and (idx == -7).all() and (fy == FILL).all() and (fx == FILL).all(), "a refused call writes nothing"
    assert fn(ctx.handle, pv, H, W, 8, 137, 0.0, 0.0, 0xff, *outs) == 0
    assert fn(ctx.handle, pv, H, W, hWin, wWin, 2.0, 2.0, 0x01, None, None, None, outs[3]) == 0
    torch.cuda.synchronize()


def test_semiGlobalAggregatePlane_equals_the_raw_call(dfe, cuda):
    vol = _volume((12, 20, 5, 13), 5)
    tv = torch.from_numpy(vol).to(cuda)
    for paths in (0x0f, 0xff, 0x40):
        raw = aggregate(dfe, cuda, vol, 0.5, 4.0, paths)
        res = dfe.semiGlobalAggregatePlane(tv, 0.5, 4.0, paths=paths)
        assert sorted(res) == ["aggregate", "flow_x", "flow_y", "idx"]
        assert tuple(res["aggregate"].shape) == vol.shape and res["idx"].dtype == torch.int64 and tuple(res["idx"].shape) == (12, 20)
        assert np.array_equal(_bits(res["aggregate"].cpu().numpy()), _bits(raw["agg"])) and np.array_equal(res["idx"].cpu().numpy(), raw["idx"])
        assert np.array_equal(res["flow_y"].cpu().numpy(), raw["flow_y"]) and np.array_equal(res["flow_x"].cpu().numpy(), raw["flow_x"])
        lean = dfe.semiGlobalAggregatePlane(tv, 0.5, 4.0, paths=paths, want_volume=False)
        assert lean["aggregate"] is None and all(torch.equal(lean[k], res[k]) for k in ("idx", "flow_y", "flow_x"))
    res = dfe.semiGlobalAggregatePlane(tv, 0.5, 4.0)              # the default: 4 paths
    assert np.array_equal(_bits(res["aggregate"].cpu().numpy()), _bits(aggregate(dfe, cuda, vol, 0.5, 4.0, 0x0f)["agg"]))
    res = dfe.semiGlobalAggregatePlane(tv.permute(1, 0, 2, 3), 0.5, 4.0)      # a view: made contiguous
    assert np.array_equal(_bits(res["aggregate"].cpu().numpy()), _bits(aggregate(dfe, cuda, np.ascontiguousarray(vol.transpose(1, 0, 2, 3)), 0.5, 4.0, 0x0f)["agg"]))
    for bad in (dict(paths=0), dict(paths=256), dict(paths=1.0), dict(paths=True), dict(P1=-1.0), dict(P1=5.0), dict(P2=float("nan")), dict(P1="a")):
        with pytest.raises(ValueError):
            dfe.semiGlobalAggregatePlane(tv, **{**dict(P1=0.5, P2=4.0), **bad})
    with pytest.raises(TypeError):
        dfe.semiGlobalAggregatePlane(tv.double(), 0.5, 4.0)
    for badvol in (tv[0], torch.zeros((3, 4, 33, 34), device=cuda), torch.zeros((0, 4, 5, 5), device=cuda)):
        with pytest.raises(ValueError):
            dfe.semiGlobalAggregatePlane(badvol, 0.5, 4.0)


# ---- the one calls ----
def _three_channel_pair():
    rng = np.random.RandomState(11)
    f0 = rng.randint(0, 256, size=(3, 40, 60)).astype(np.uint8)
    f1 = np.roll(f0, (1, -1), (1, 2)).astype(np.float64) * 0.5 + 40 + rng.normal(0, 2, size=f0.shape)   # moved, darker, noisy
    return f0, np.clip(np.floor(f1), 0, 255).astype(np.uint8)


# name: (frames, k, hWin, wWin, agg, P1, P2, paths)
ONE_CALLS = {
    "band": (lambda: pr.band_scene(0), 7, 9, 9, 3, 144.0, 864.0, 0xff),
    "band-4": (lambda: pr.band_scene(1), 7, 9, 9, 3, 144.0, 864.0, 0x0f),
    "three-channel": (_three_channel_pair, 5, 7, 9, 1, 8.0, 48.0, 0xff),
}


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("name", list(ONE_CALLS))
def test_one_call_equals_the_staged_calls_and_the_definition(dfe, cuda, name, dtype):
    frames, k, hWin, wWin, agg, P1, P2, paths = ONE_CALLS[name]
    n0, n1 = frames()
    C, H, W = n0.shape
    f0, f1 = torch.from_numpy(n0).to(cuda), torch.from_numpy(n1).to(cuda)
    if dtype == "f32":
        f0, f1 = f0.float() * 0.5, f1.float() * 0.5
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    flow = torch.full((2, H, W), FILL, device=cuda)
    match, depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(3))
    cx, cy = W / 2 - 3.5, H / 2 + 1.25
    head = (ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, agg, cx, cy)
    tail = (P1, P2, paths, flow.data_ptr(), match.data_ptr(), depth.data_ptr(), conf.data_ptr())
    ctx.check(lib.dfe_census_flow_depth_pair_sgm_u8(*head, 0.25, *tail) if dtype == "u8" else lib.dfe_census_flow_depth_pair_sgm_f32(*head, *tail))
    torch.cuda.synchronize()
    # the staged public calls: two transforms, the volume, the aggregate, then gather, score and paste by hand
    vol = dfe.censusCostVolume(dfe.censusTransform(f0, k), dfe.censusTransform(f1, k), hWin, wWin, agg)
    r = dfe.semiGlobalAggregatePlane(vol, P1, P2, paths=paths, want_volume=False)
    pt, pl, Ha, Wa = cr.region(H, W, k, k, hWin, wWin, agg)
    raw = vol.view(Ha, Wa, -1).gather(2, (r["idx"] - 1).unsqueeze(-1)).squeeze(-1)
    score = 1.0 - raw / torch.tensor(float((k * k - 1) * C * agg * agg), device=cuda)
    eflow, ematch = torch.zeros((2, H, W), device=cuda), torch.zeros((H, W), device=cuda)
    eflow[0, pt:pt + Ha, pl:pl + Wa], eflow[1, pt:pt + Ha, pl:pl + Wa], ematch[pt:pt + Ha, pl:pl + Wa] = r["flow_y"], r["flow_x"], score
    assert torch.equal(flow, eflow) and torch.equal(match.view(torch.int32), ematch.view(torch.int32))
    # ... and the definition: the flow of the aggregate, the match score of the RAW cost at the chosen class
    cost = cr.cost_volume(cr.signature(n0, k, k), cr.signature(n1, k, k), hWin, wWin, agg)
    assert np.array_equal(vol.cpu().numpy(), cost.astype(F))
    ref = pr.plane_aggregate(cost.astype(F), P1, P2, paths)
    assert np.array_equal(flow[0].cpu().numpy(), cr.paste(ref["flow_y"], H, W, pt, pl)) and np.array_equal(flow[1].cpu().numpy(), cr.paste(ref["flow_x"], H, W, pt, pl))
    rmatch = cr.match_score(pr.raw_at(cost, ref["idx"]), k * k - 1, C, agg)
    assert np.array_equal(_bits(match.cpu().numpy()), _bits(cr.paste(rmatch, H, W, pt, pl)))
    # depth as the single-scale step makes it from its pasted flow
    ed, ec = torch.empty((H, W), device=cuda), torch.empty((H, W), device=cuda)
    ctx.check(lib.dfe_flow_to_depth_cartesian(ctx.handle, flow.data_ptr(), H, W, cx, cy, 0, ed.data_ptr(), ec.data_ptr()))
    assert torch.equal(depth.view(torch.int32), ed.view(torch.int32)) and torch.equal(conf, ec)
    # the wrapper; depth and depth_conf may both be NULL
    res = dfe.censusFlowDepthPair(f0, f1, k, hWin, wWin, (cx, cy), agg=agg, sgm=dict(P1=P1, P2=P2, paths=paths))
    assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], match) and torch.equal(res["depth"], depth) and torch.equal(res["depth_conf"], conf)
    flow2, match2 = torch.full((2, H, W), FILL, device=cuda), torch.full((H, W), FILL, device=cuda)
    tail2 = (P1, P2, paths, flow2.data_ptr(), match2.data_ptr(), None, None)
    ctx.check(lib.dfe_census_flow_depth_pair_sgm_u8(*head, 0.25, *tail2) if dtype == "u8" else lib.dfe_census_flow_depth_pair_sgm_f32(*head, *tail2))
    assert torch.equal(flow2, flow) and torch.equal(match2, match)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_band_scene_through_the_one_call(dfe, cuda, seed):
    f0, f1 = pr.band_scene(seed)
    k, win = cr.SCENE["k"], cr.SCENE["win"]
    pt, pl, Ha, Wa = cr.region(72, 104, k, k, win, win, 3)
    plain = dfe.censusFlowDepthPair(torch.from_numpy(f0).to(cuda), torch.from_numpy(f1).to(cuda), k, win, win, (52.0, 36.0), agg=3)
    inner = plain["flow"][:, pt:pt + Ha, pl:pl + Wa].cpu().numpy()
    assert cr.share_wrong(inner[0], inner[1]) == pr.band_share_wrong(seed, 0)
    for paths in (0x0f, 0xff):
        res = dfe.censusFlowDepthPair(torch.from_numpy(f0).to(cuda), torch.from_numpy(f1).to(cuda), k, win, win, (52.0, 36.0), agg=3,
                                      sgm=dict(P1=pr.BAND["P1"], P2=pr.BAND["P2"], paths=paths))
        inner = res["flow"][:, pt:pt + Ha, pl:pl + Wa].cpu().numpy()
        _, fy, fx = pr.band_flow(seed, paths)
        assert np.array_equal(inner[0], fy) and np.array_equal(inner[1], fx)
        assert cr.share_wrong(inner[0], inner[1]) == pr.band_share_wrong(seed, paths)      # (follows from the bits)
        assert (res["scores"][pt:pt + Ha, pl:pl + Wa] > 0).all()


def test_censusFlowDepthPair_sgm_keyword(dfe, cuda):
    f0, f1 = (torch.from_numpy(f).to(cuda) for f in pr.band_scene(1))
    k, win, foe = 7, 9, (52.0, 36.0)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    # sgm=None is today's call, bit for bit
    flow, match, depth, conf = torch.empty((2, 72, 104), device=cuda), *(torch.empty((72, 104), device=cuda) for _ in range(3))
    ctx.check(lib.dfe_census_flow_depth_pair_u8(ctx.handle, f0.data_ptr(), f1.data_ptr(), 1, 72, 104, k, win, win, 3, foe[0], foe[1], 1.0, flow.data_ptr(),
                                                match.data_ptr(), depth.data_ptr(), conf.data_ptr()))
    for res in (dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3), dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, sgm=None)):
        assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], match) and torch.equal(res["depth"].view(torch.int32), depth.view(torch.int32))
        assert torch.equal(res["depth_conf"], conf)
    # with a value both directions of consistency= are aggregated; fill and median follow unchanged
    res = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, consistency=1.0, fill=True, median=5, sgm=(144, 864))
    wta = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, consistency=1.0, fill=True, median=5)
    assert sorted(res) == sorted(wta)
    assert all(res[key].shape == wta[key].shape and res[key].dtype == wta[key].dtype for key in res)
    fw = dfe.censusFlowDepthPair(f0, f1, k, win, win, foe, agg=3, sgm=dict(P1=144, P2=864, paths=0x0f))
    bw = dfe.censusFlowDepthPair(f1, f0, k, win, win, foe, agg=3, sgm=(144.0, 864.0))
    assert torch.equal(res["flow"], fw["flow"]) and torch.equal(res["scores"], fw["scores"]) and torch.equal(res["flow_bw"], bw["flow"])
    assert not torch.equal(fw["flow"], flow), "the aggregation changes the band's labels"
    mask, err = dfe.flowConsistency(fw["flow"], bw["flow"], 1.0, cr.region(72, 104, k, k, win, win, 3))
    assert torch.equal(res["consistent"], mask) and torch.equal(res["consistency_err"].view(torch.int32), err.view(torch.int32))


def test_one_call_refusals_come_before_any_launch(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    f = torch.zeros((5, 40, 60), device=cuda)
    out = torch.full((4, 40, 60), FILL, device=cuda)

    def pair(C=1, H=40, W=60, k=7, hWin=9, wWin=9, agg=3, P1=1.0, P2=2.0, paths=0x0f):
        return lib.dfe_census_flow_depth_pair_sgm_f32(ctx.handle, f.data_ptr(), f.data_ptr(), C, H, W, k, hWin, wWin, agg, 30.0, 20.0, P1, P2, paths,
                                                      out.data_ptr(), out[2].data_ptr(), None, None)

    for bad in (dict(agg=2), dict(agg=0), dict(C=5), dict(hWin=0), dict(k=8), dict(k=9), dict(paths=0), dict(paths=256), dict(P1=3.0), dict(P1=-1.0),
                dict(P2=float("inf")), dict(P1=float("nan"))):
        assert pair(**bad) == DFE_E_ARG, bad
    assert pair(hWin=33, wWin=34) == DFE_E_UNSUPPORTED
    assert pair(H=16) == DFE_E_SHAPE and pair(H=3) == DFE_E_SHAPE
    assert lib.dfe_census_flow_depth_pair_sgm_u8(ctx.handle, f.data_ptr(), f.data_ptr(), 1, 40, 60, 7, 9, 9, 3, 30.0, 20.0, 0.0, 1.0, 2.0, 0x0f, out.data_ptr(),
                                                 out[2].data_ptr(), None, None) == DFE_E_ARG
    torch.cuda.synchronize()
    assert (out == FILL).all(), "a refused call wrote something"
