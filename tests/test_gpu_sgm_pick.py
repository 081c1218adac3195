"""The pick operator and its one calls on the device (include/dfe.h: dfe_sgm_plane_pick_f32, dfe_flow_depth_pair_sgm_*,
dfe_census_flow_depth_pair_sgm2_*) against the numpy restatement of the definition (tests/sgm_pick_ref.py) BIT FOR
BIT -- the definition fixes every operation and the order of the sum, so there is no tolerance.  Every output is pre-filled with a sentinel.

The windows: few or no far cells and missing neighbours (1 x 1, 1 x 9, 9 x 1, 3 x 3), 4 x 6, 64 cells (one a lane exactly), 65 (the first
cell of a lane's second round), 17 x 17, 33 x 33 and 8 x 137, the ceiling of 1096.  Winners are planted at the corners, on the edges and
at cells 63 / 64, where the winner and its neighbours straddle a lane round."""
import itertools

import numpy as np
import pytest
import torch

from tests import census_ref as cr
from tests import sgm_pick_ref as kr
from tests import sgm_plane_ref as pr

pytestmark = pytest.mark.gpu
DFE_E_ARG, DFE_E_SHAPE, DFE_E_UNSUPPORTED = -1, -2, -5
FILL = -7.0
F = np.float32
WINDOWS = ((1, 1), (1, 9), (9, 1), (3, 3), (4, 6), (8, 8), (5, 13), (17, 17), (33, 33), (8, 137))
PATHS = (0, 0x01, 0x80, 0x0f, 0xff)
MIN_UNIQUE = (0.0, 0.2, 1.0)
PENALTIES = ((0.5, 4.0), (2.25, 16.5), (3.0, 3.0), (0.0, 1.5))
OUTS = ("agg", "idx", "flow_y", "flow_x", "best", "second", "unique")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _volume(shape, seed, lo=-3.0):
    return np.random.default_rng(seed).uniform(lo, 9, size=shape).astype(F)


def pick_call(dfe, cuda, vol, P1, P2, paths, subpixel=0, min_unique=0.0, want=OUTS):
    """the raw call: every output as numpy, the sentinel where it was not given"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, hWin, wWin = vol.shape
    tv = torch.from_numpy(vol).to(cuda)
    out = dict(agg=torch.full(vol.shape, FILL, device=cuda), idx=torch.full((H, W), -7, dtype=torch.int64, device=cuda))
    for k in OUTS[2:]:
        out[k] = torch.full((H, W), FILL, device=cuda)
    p = [out[k].data_ptr() if k in want else None for k in OUTS]
    ctx.check(lib.dfe_sgm_plane_pick_f32(ctx.handle, tv.data_ptr(), H, W, hWin, wWin, P1, P2, paths, subpixel, min_unique, *p))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "sgpk_pick_kernel"
    assert torch.equal(tv.cpu(), torch.from_numpy(vol)), "the volume is an input"
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sum(vol, single, paths):
    if paths == 0:
        return vol
    want = None
    for r in range(8):
        if paths >> r & 1:
            want = single[r] if want is None else (want + single[r]).astype(F)
    return want


def _check(got, want_agg, subpixel, min_unique, tag, want=OUTS):
    ref = dict(kr.pick(want_agg, bool(subpixel), min_unique), agg=want_agg)
    for k in OUTS:
        if k not in want:
            assert (got[k] == (-7 if k == "idx" else FILL)).all(), tag + ": %s was not given" % k
        elif k == "idx":
            assert np.array_equal(got[k], ref[k]), tag + ": idx"
        else:
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), tag + ": " + k


@pytest.mark.parametrize("i,win", list(enumerate(WINDOWS)), ids=["%dx%d" % w for w in WINDOWS])
def test_every_window_equals_the_definition_bit_for_bit(dfe, cuda, i, win):
    P1, P2 = PENALTIES[i % 4]
    for n, (H, W) in enumerate(((5, 7), (7, 5))):
        vol = _volume((H, W) + win, 10 * i + n, lo=(-3.0, 1.0)[n])     # costs of mixed sign (second <= 0 happens), then positive ones
        single = [pr.plane_path(vol, r, P1, P2) for r in range(8)]
        for j, (paths, subpixel) in enumerate(itertools.product(PATHS, (0, 1))):
            mu = MIN_UNIQUE[(i + n + j) % 3]
            tag = "%dx%d window %dx%d paths 0x%02x P (%g, %g) subpixel %d min_unique %g" % (H, W, win[0], win[1], paths, P1, P2, subpixel, mu)
            _check(pick_call(dfe, cuda, vol, P1, P2, paths, subpixel, mu), _sum(vol, single, paths), subpixel, mu, tag)


def _planted(win, cells, seed):
    """one pixel per planted cell: costs in 5 .. 9, the planted cell at 1, its 3 x 3 neighbours in 2 .. 4 (so both parabolas bend)"""
    hWin, wWin = win
    rng = np.random.default_rng(seed)
    vol = rng.uniform(5, 9, size=(len(cells), 1, hWin, wWin)).astype(F)
    for p, c in enumerate(cells):
        r, s = divmod(c, wWin)
        for rr in range(max(r - 1, 0), min(r + 2, hWin)):
            for ss in range(max(s - 1, 0), min(s + 2, wWin)):
                vol[p, 0, rr, ss] = rng.uniform(2, 4)
        vol[p, 0, r, s] = 1.0
    return vol


@pytest.mark.parametrize("win", [(8, 8), (5, 13), (9, 9), (17, 17), (8, 137)], ids=lambda w: "%dx%d" % w)
def test_planted_winners_at_corners_edges_and_lane_rounds(dfe, cuda, win):
    hWin, wWin = win
    n = hWin * wWin
    cells = [0, wWin - 1, n - wWin, n - 1, wWin // 2, n - 1 - wWin // 2, (hWin // 2) * wWin, (hWin // 2) * wWin + wWin - 1]
    cells += [c for c in (62, 63, 64, 65, 127, 128) if c < n]
    vol = _planted(win, cells, 7)
    for paths, P in ((0, (1.0, 2.0)), (0xff, (0.0, 0.0)), (0x05, (0.0, 0.0))):     # without penalties L = C: the planted cell stays the winner
        want = kr.plane_pick(vol, P[0], P[1], paths)["agg"]
        got = pick_call(dfe, cuda, vol, P[0], P[1], paths, 1, 0.2)
        _check(got, want, 1, 0.2, "window %dx%d paths 0x%02x" % (hWin, wWin, paths))
        assert np.array_equal(got["idx"][:, 0], np.asarray(cells) + 1)
        assert (got["unique"] > 0.2).all() and (np.abs(got["flow_x"] - np.rint(got["flow_x"])) <= 0.5).all()
    inner = [p for p, c in enumerate(cells) if 0 < c % wWin < wWin - 1 and 0 < c // wWin < hWin - 1]
    if inner:
        assert (got["flow_x"][inner, 0] != np.rint(got["flow_x"][inner, 0])).any(), "an interior winner moves off the grid"


def test_every_subset_of_outputs(dfe, cuda):
    vol = _volume((5, 7, 5, 13), 300, lo=1.0)
    single = [pr.plane_path(vol, r, 0.5, 4.0) for r in range(8)]
    for m in range(1, 1 << len(OUTS)):
        want = tuple(k for b, k in enumerate(OUTS) if m >> b & 1)
        _check(pick_call(dfe, cuda, vol, 0.5, 4.0, 0x0f, 1, 0.2, want), _sum(vol, single, 0x0f), 1, 0.2, "outputs %s" % (want,), want)
    for paths in (0x08, 0):                      # a single direction, whose L goes straight into agg when agg is given; no direction at all
        for want in (OUTS, ("agg",), ("agg", "unique"), ("second",), ("flow_x", "best"), OUTS[1:]):
            _check(pick_call(dfe, cuda, vol, 0.5, 4.0, paths, 1, 0.0, want), _sum(vol, single, paths), 1, 0.0, "paths 0x%02x outputs %s" % (paths, want), want)


def test_a_census_volume_with_many_exact_ties(dfe, cuda):
    vol = np.ascontiguousarray(pr.band_volume(0)[10:30, 20:60])
    for paths in (0, 0x0f, 0xff):
        for subpixel in (0, 1):
            want = kr.plane_pick(vol, 144.0, 864.0, paths)["agg"]
            got = pick_call(dfe, cuda, vol, 144.0, 864.0, paths, subpixel, 0.2)
            _check(got, want, subpixel, 0.2, "census volume, paths 0x%02x subpixel %d" % (paths, subpixel))
            assert np.array_equal(got["agg"], np.rint(got["agg"]))


def test_idx_agg_and_integer_flow_are_the_aggregation_s_own(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    for win, seed in (((5, 13), 1), ((17, 17), 2), ((8, 137), 3)):
        vol = _volume((6, 9) + win, seed)
        tv = torch.from_numpy(vol).to(cuda)
        for paths in (0x01, 0x80, 0x0f, 0xf0, 0xff):
            agg = torch.full(vol.shape, FILL, device=cuda)
            idx = torch.full((6, 9), -7, dtype=torch.int64, device=cuda)
            fy, fx = torch.full((6, 9), FILL, device=cuda), torch.full((6, 9), FILL, device=cuda)
            ctx.check(lib.dfe_sgm_plane_aggregate_f32(ctx.handle, tv.data_ptr(), 6, 9, win[0], win[1], 0.5, 4.0, paths, agg.data_ptr(), idx.data_ptr(),
                                                      fy.data_ptr(), fx.data_ptr()))
            torch.cuda.synchronize()
            for subpixel in (0, 1):
                got = pick_call(dfe, cuda, vol, 0.5, 4.0, paths, subpixel, 0.2)
                assert np.array_equal(_bits(got["agg"]), _bits(agg.cpu().numpy())) and np.array_equal(got["idx"], idx.cpu().numpy()), (win, paths)
                if not subpixel:
                    assert np.array_equal(_bits(got["flow_y"]), _bits(fy.cpu().numpy())) and np.array_equal(_bits(got["flow_x"]), _bits(fx.cpu().numpy()))


def test_semiGlobalPick_equals_the_raw_call(dfe, cuda):
    vol = _volume((12, 20, 5, 13), 5, lo=1.0)
    tv = torch.from_numpy(vol).to(cuda)
    for paths, subpixel, mu in ((0, False, 0.0), (0x0f, True, 0.2), (0xff, True, 0.0), (0x40, False, 1.0)):
        raw = pick_call(dfe, cuda, vol, 0.5, 4.0, paths, int(subpixel), mu)
        res = dfe.semiGlobalPick(tv, 0.5, 4.0, paths=paths, subpixel=subpixel, min_unique=mu, want_volume=True)
        assert sorted(res) == ["aggregate", "best", "flow_x", "flow_y", "idx", "second", "unique"]
        assert np.array_equal(_bits(res["aggregate"].cpu().numpy()), _bits(raw["agg"])) and np.array_equal(res["idx"].cpu().numpy(), raw["idx"])
        for k in OUTS[2:]:
            assert np.array_equal(_bits(res[k].cpu().numpy()), _bits(raw[k])), k
        lean = dfe.semiGlobalPick(tv, 0.5, 4.0, paths=paths, subpixel=subpixel, min_unique=mu)
        assert lean["aggregate"] is None and all(torch.equal(lean[k], res[k]) for k in OUTS[1:])
    res = dfe.semiGlobalPick(tv)                                     # the defaults: winner-takes-all on the volume itself
    assert np.array_equal(_bits(res["best"].cpu().numpy()), _bits(vol.reshape(12, 20, -1).min(-1)))


# ---- the one calls ----
def _three_channel_pair():
    rng = np.random.RandomState(11)
    f0 = rng.randint(0, 256, size=(3, 40, 60)).astype(np.uint8)
    f1 = np.roll(f0, (1, -1), (1, 2)).astype(np.float64) + rng.normal(0, 6, size=f0.shape)   # moved and noisy
    return f0, np.clip(np.floor(f1), 0, 255).astype(np.uint8)


# name: (frames, k, hWin, wWin, P1, P2, paths, subpixel, min_unique)
SSD_CALLS = {
    "three-channel": (_three_channel_pair, 5, 7, 9, 400.0, 3200.0, 0xff, 1, 0.2),
    "wide-band": (lambda: kr.wide_band_scene(0), 7, 9, 9, kr.WIDE["P1"], kr.WIDE["P2"], 0xff, 1, 0.2),
    "wide-band-4": (lambda: kr.wide_band_scene(0), 7, 9, 9, kr.WIDE["P1"], kr.WIDE["P2"], 0x0f, 0, 0.0),
}


def _paste(plane, H, W, pt, pl):
    out = torch.zeros((H, W), device=plane.device)
    out[pt:pt + plane.shape[0], pl:pl + plane.shape[1]] = plane
    return out


def _depth(dfe, flow, cx, cy):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    _, H, W = flow.shape
    ed, ec = torch.empty((H, W), device=flow.device), torch.empty((H, W), device=flow.device)
    ctx.check(lib.dfe_flow_to_depth_cartesian(ctx.handle, flow.data_ptr(), H, W, cx, cy, 0, ed.data_ptr(), ec.data_ptr()))
    return ed, ec


def _ssd_volume(dfe, f0, f1, k, hWin, wWin):
    """dfe_ssd_cost_volume_f32 of float frames on the device"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C, H, W = f0.shape
    vol = torch.empty((H - k + 1 - hWin + 1, W - k + 1 - wWin + 1, hWin, wWin), device=f0.device)
    ctx.check(lib.dfe_ssd_cost_volume_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, k, hWin, wWin, vol.data_ptr()))
    return vol


@pytest.mark.parametrize("dtype", ["f32", "u8", "u8-half"])
@pytest.mark.parametrize("name", list(SSD_CALLS))
def test_ssd_one_call_equals_the_staged_calls_and_the_definition(dfe, cuda, name, dtype):
    frames, k, hWin, wWin, P1, P2, paths, subpixel, mu = SSD_CALLS[name]
    n0, n1 = frames()
    C, H, W = n0.shape
    scale = 0.5 if dtype in ("f32", "u8-half") else 1.0
    b0, b1 = torch.from_numpy(n0).to(cuda), torch.from_numpy(n1).to(cuda)
    f0, f1 = b0.float() * scale, b1.float() * scale
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    flow = torch.full((2, H, W), FILL, device=cuda)
    scores, depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(3))
    cx, cy = W / 2 - 3.5, H / 2 + 1.25

    def call(out_flow, out_scores, out_depth, out_conf):
        tail = (P1, P2, paths, subpixel, mu, out_flow.data_ptr(), out_scores.data_ptr(), out_depth, out_conf)
        if dtype == "f32":
            return lib.dfe_flow_depth_pair_sgm_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, cx, cy, *tail)
        return lib.dfe_flow_depth_pair_sgm_u8(ctx.handle, b0.data_ptr(), b1.data_ptr(), C, H, W, k, hWin, wWin, cx, cy, scale, *tail)

    ctx.check(call(flow, scores, depth.data_ptr(), conf.data_ptr()))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "sgpk_pick_kernel"
    # the staged public calls: the volume, the pick, then paste by hand
    vol = _ssd_volume(dfe, f0, f1, k, hWin, wWin)
    r = dfe.semiGlobalPick(vol, P1, P2, paths=paths, subpixel=bool(subpixel), min_unique=mu)
    Ho, Wo = vol.shape[:2]
    pt, pl = (H - Ho) // 2, (W - Wo) // 2
    eflow = torch.stack([_paste(r["flow_y"], H, W, pt, pl), _paste(r["flow_x"], H, W, pt, pl)])
    assert torch.equal(flow.view(torch.int32), eflow.view(torch.int32))
    assert torch.equal(scores.view(torch.int32), _paste(r["unique"], H, W, pt, pl).view(torch.int32))
    # ... and the definition
    cost = kr.ssd_volume(n0, n1, k, hWin, wWin, scale)
    assert np.array_equal(_bits(vol.cpu().numpy()), _bits(cost))
    ref = kr.plane_pick(cost, P1, P2, paths, bool(subpixel), mu)
    assert np.array_equal(_bits(flow[0].cpu().numpy()), _bits(cr.paste(ref["flow_y"], H, W, pt, pl)))
    assert np.array_equal(_bits(flow[1].cpu().numpy()), _bits(cr.paste(ref["flow_x"], H, W, pt, pl)))
    assert np.array_equal(_bits(scores.cpu().numpy()), _bits(cr.paste(ref["unique"], H, W, pt, pl)))
    # depth as the single-scale step makes it from its pasted flow
    ed, ec = _depth(dfe, flow, cx, cy)
    assert torch.equal(depth.view(torch.int32), ed.view(torch.int32)) and torch.equal(conf, ec)
    # the wrapper; depth and depth_conf may both be NULL
    res = dfe.flowDepthPair(f0 if dtype == "f32" else b0, f1 if dtype == "f32" else b1, k, hWin, wWin, (cx, cy), threshold=0.9, subpixel=bool(subpixel), scale=scale,
                            sgm=dict(P1=P1, P2=P2, paths=paths, min_unique=mu))
    assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], scores) and torch.equal(res["depth"], depth) and torch.equal(res["depth_conf"], conf)
    flow2, scores2 = torch.full((2, H, W), FILL, device=cuda), torch.full((H, W), FILL, device=cuda)
    ctx.check(call(flow2, scores2, None, None))
    assert torch.equal(flow2, flow) and torch.equal(scores2, scores)


def test_wide_band_scene_through_the_ssd_one_call(dfe, cuda):
    f0, f1 = (torch.from_numpy(f).to(cuda) for f in kr.wide_band_scene(0))
    k, win = cr.SCENE["k"], cr.SCENE["win"]
    pt, pl, Ho, Wo = cr.region(72, 104, k, k, win, win, 1)
    res = dfe.flowDepthPair(f0, f1, k, win, win, (52.0, 36.0), sgm=dict(P1=kr.WIDE["P1"], P2=kr.WIDE["P2"], paths=0xff, min_unique=kr.WIDE["min_unique"]))
    ref = kr.wide_pick(0, 0xff)
    inner = res["flow"][:, pt:pt + Ho, pl:pl + Wo].cpu().numpy()
    assert np.array_equal(inner[0], ref["flow_y"]) and np.array_equal(inner[1], ref["flow_x"])
    assert np.array_equal(_bits(res["scores"][pt:pt + Ho, pl:pl + Wo].cpu().numpy()), _bits(ref["unique"]))
    assert float(np.mean(kr.wrong(dict(flow_y=inner[0], flow_x=inner[1])))) == float(kr.wrong(ref).mean())      # (follows from the bits)


def _census_pair():
    rng = np.random.RandomState(11)
    f0 = rng.randint(0, 256, size=(3, 40, 60)).astype(np.uint8)
    f1 = np.roll(f0, (1, -1), (1, 2)).astype(np.float64) * 0.5 + 40 + rng.normal(0, 2, size=f0.shape)   # moved, darker, noisy
    return f0, np.clip(np.floor(f1), 0, 255).astype(np.uint8)


# name: (frames, k, hWin, wWin, agg, P1, P2, paths)
CENSUS_CALLS = {
    "wide-band": (lambda: kr.wide_band_scene(0), 7, 9, 9, 3, 144.0, 864.0, 0xff),
    "three-channel": (_census_pair, 5, 7, 9, 1, 8.0, 48.0, 0x0f),
}


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("name", list(CENSUS_CALLS))
def test_census_sgm2_equals_the_staged_calls_the_definition_and_the_sgm_entry(dfe, cuda, name, dtype):
    frames, k, hWin, wWin, agg, P1, P2, paths = CENSUS_CALLS[name]
    n0, n1 = frames()
    C, H, W = n0.shape
    f0, f1 = torch.from_numpy(n0).to(cuda), torch.from_numpy(n1).to(cuda)
    if dtype == "f32":
        f0, f1 = f0.float() * 0.5, f1.float() * 0.5
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    cx, cy = W / 2 - 3.5, H / 2 + 1.25
    head = (ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, agg, cx, cy)
    fn2 = (lambda *t: lib.dfe_census_flow_depth_pair_sgm2_u8(*head, 0.25, *t)) if dtype == "u8" else (lambda *t: lib.dfe_census_flow_depth_pair_sgm2_f32(*head, *t))
    fn1 = (lambda *t: lib.dfe_census_flow_depth_pair_sgm_u8(*head, 0.25, *t)) if dtype == "u8" else (lambda *t: lib.dfe_census_flow_depth_pair_sgm_f32(*head, *t))
    vol = dfe.censusCostVolume(dfe.censusTransform(f0, k), dfe.censusTransform(f1, k), hWin, wWin, agg)
    cost = cr.cost_volume(cr.signature(n0, k, k), cr.signature(n1, k, k), hWin, wWin, agg).astype(F)
    assert np.array_equal(vol.cpu().numpy(), cost)
    pt, pl, Ha, Wa = cr.region(H, W, k, k, hWin, wWin, agg)
    for subpixel, mu in ((1, 0.2), (0, 0.0)):
        flow = torch.full((2, H, W), FILL, device=cuda)
        match, unique, depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(4))
        ctx.check(fn2(P1, P2, paths, subpixel, mu, flow.data_ptr(), match.data_ptr(), unique.data_ptr(), depth.data_ptr(), conf.data_ptr()))
        torch.cuda.synchronize()
        # the staged public calls plus the paste
        r = dfe.semiGlobalPick(vol, P1, P2, paths=paths, subpixel=bool(subpixel), min_unique=mu)
        raw = vol.view(Ha, Wa, -1).gather(2, (r["idx"] - 1).unsqueeze(-1)).squeeze(-1)
        score = 1.0 - raw / torch.tensor(float((k * k - 1) * C * agg * agg), device=cuda)
        eflow = torch.stack([_paste(r["flow_y"], H, W, pt, pl), _paste(r["flow_x"], H, W, pt, pl)])
        assert torch.equal(flow.view(torch.int32), eflow.view(torch.int32))
        assert torch.equal(match.view(torch.int32), _paste(score, H, W, pt, pl).view(torch.int32))
        assert torch.equal(unique.view(torch.int32), _paste(r["unique"], H, W, pt, pl).view(torch.int32))
        # the definition
        ref = kr.plane_pick(cost, P1, P2, paths, bool(subpixel), mu)
        for got, key in ((flow[0], "flow_y"), (flow[1], "flow_x"), (unique, "unique")):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(cr.paste(ref[key], H, W, pt, pl))), key
        rmatch = cr.match_score(pr.raw_at(cost, ref["idx"]), k * k - 1, C, agg)
        assert np.array_equal(_bits(match.cpu().numpy()), _bits(cr.paste(rmatch, H, W, pt, pl)))
        ed, ec = _depth(dfe, flow, cx, cy)
        assert torch.equal(depth.view(torch.int32), ed.view(torch.int32)) and torch.equal(conf, ec)
        # the wrapper
        res = dfe.censusFlowDepthPair(f0, f1, k, hWin, wWin, (cx, cy), agg=agg, scale=0.25, subpixel=bool(subpixel), sgm=dict(P1=P1, P2=P2, paths=paths, min_unique=mu))
        assert sorted(res) == ["depth", "depth_conf", "flow", "scores", "unique"]
        assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], match) and torch.equal(res["unique"], unique) and torch.equal(res["depth"], depth)
    # subpixel = 0 and unique = NULL: the existing sgm entry, bit for bit
    old = [torch.full((2, H, W), FILL, device=cuda)] + [torch.full((H, W), FILL, device=cuda) for _ in range(3)]
    new = [torch.full((2, H, W), FILL, device=cuda)] + [torch.full((H, W), FILL, device=cuda) for _ in range(3)]
    ctx.check(fn1(P1, P2, paths, *(t.data_ptr() for t in old)))
    ctx.check(fn2(P1, P2, paths, 0, 0.0, new[0].data_ptr(), new[1].data_ptr(), None, new[2].data_ptr(), new[3].data_ptr()))
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(old, new))
    assert "unique" not in dfe.censusFlowDepthPair(f0, f1, k, hWin, wWin, (cx, cy), agg=agg, sgm=(P1, P2))      # the old keyword, the old entry


def test_flowDepthPair_sgm_with_fill_and_median_is_the_composition_of_public_ops(dfe, cuda):
    n0, n1 = kr.wide_band_scene(1)
    f0, f1 = torch.from_numpy(n0).to(cuda), torch.from_numpy(n1).to(cuda)
    k, win, foe = 7, 9, (52.0, 36.0)
    H, W = 72, 104
    sgm = dict(P1=kr.WIDE["P1"], P2=kr.WIDE["P2"], paths=0xff, min_unique=0.2)
    res = dfe.flowDepthPair(f0, f1, k, win, win, foe, sgm=sgm, subpixel=True, fill=True, median=(7, 30.0))
    assert sorted(res) == sorted(["flow", "scores", "depth", "depth_conf", "flow_dense", "filled", "depth_dense", "flow_median", "median_valid", "depth_median"])
    vol = _ssd_volume(dfe, f0.float(), f1.float(), k, win, win)
    r = dfe.semiGlobalPick(vol, sgm["P1"], sgm["P2"], paths=0xff, subpixel=True, min_unique=0.2)
    pt, pl, Ho, Wo = cr.region(H, W, k, k, win, win, 1)
    R = (pt, pl, Ho, Wo)
    flow = torch.stack([_paste(r["flow_y"], H, W, pt, pl), _paste(r["flow_x"], H, W, pt, pl)])
    scores = _paste(r["unique"], H, W, pt, pl)
    depth, conf = _depth(dfe, flow, *foe)
    wgt = (scores > 0).float()
    assert 0 < float(wgt[pt:pt + Ho, pl:pl + Wo].mean()) < 1, "the gate rejects some pixels and keeps others"
    dense, filled = dfe.fillHoles(flow, wgt, R, 0)
    med, valid = dfe.weightedMedian(dense, torch.where(wgt > 0, filled, 0.25 * filled), f0.float(), 7, 30.0, R)
    want = dict(flow=flow, scores=scores, depth=depth, depth_conf=conf, flow_dense=dense, filled=filled, depth_dense=_depth(dfe, dense, *foe)[0],
                flow_median=med, median_valid=valid, depth_median=_depth(dfe, med, *foe)[0])
    for key, t in want.items():
        assert torch.equal(res[key].view(torch.int32), t.view(torch.int32)), key
    assert (res["flow"] != torch.round(res["flow"])).any(), "subpixel=True moves the flow off the grid"
    with pytest.raises(ValueError):
        dfe.flowDepthPair(f0, f1, k, win, win, foe, sgm=sgm, consistency=1.0)


def test_refusals_come_before_any_launch(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    nan, inf = float("nan"), float("inf")
    # the operator
    H, W, hWin, wWin = 5, 7, 3, 4
    vol = torch.zeros((H, W, 1097), device=cuda)
    agg = torch.full((H, W, 1097), FILL, device=cuda)
    idx = torch.full((H, W), -7, dtype=torch.int64, device=cuda)
    planes = [torch.full((H, W), FILL, device=cuda) for _ in range(5)]
    pv, outs = vol.data_ptr(), (agg.data_ptr(), idx.data_ptr()) + tuple(t.data_ptr() for t in planes)
    fn = lib.dfe_sgm_plane_pick_f32

    def op(h=H, w=W, wh=hWin, ww=wWin, P1=1.0, P2=2.0, paths=0x0f, mu=0.2, v=pv, o=outs):
        return fn(ctx.handle, v, h, w, wh, ww, P1, P2, paths, 1, mu, *o)

    assert fn(None, pv, H, W, hWin, wWin, 1.0, 2.0, 0x0f, 1, 0.2, *outs) == DFE_E_ARG
    assert op(v=None) == DFE_E_ARG and op(o=(None,) * 7) == DFE_E_ARG and op(o=(pv,) + outs[1:]) == DFE_E_ARG
    assert "dfe_sgm_plane_pick_f32" in ctx.last_error()
    for bad in (dict(paths=256), dict(paths=0x10f), dict(P1=-1.0), dict(P1=3.0), dict(P1=nan), dict(P2=inf), dict(paths=0, P1=3.0), dict(paths=0, P2=nan),
                dict(mu=-0.1), dict(mu=1.5), dict(mu=nan)):
        assert op(**bad) == DFE_E_ARG, bad
        assert "dfe_sgm_plane_pick_f32" in ctx.last_error()
    for bad in (dict(h=0), dict(w=0), dict(h=-1), dict(h=65536, w=65536), dict(wh=0), dict(ww=0), dict(wh=-1, ww=-1)):
        assert op(**bad) == DFE_E_SHAPE, bad
    for wh, ww in ((1, 1097), (1097, 1), (33, 34), (40000, 40000)):
        assert op(wh=wh, ww=ww) == DFE_E_UNSUPPORTED, (wh, ww)
    torch.cuda.synchronize()
    assert (agg == FILL).all() and (idx == -7).all() and all((t == FILL).all() for t in planes), "a refused call writes nothing"
    assert op(wh=8, ww=137, P1=0.0, P2=0.0, paths=0xff) == 0 and op(paths=0) == 0
    assert fn(ctx.handle, pv, H, W, hWin, wWin, 2.0, 2.0, 0x01, 0, 0.0, None, None, None, None, None, None, outs[6]) == 0
    torch.cuda.synchronize()
    # the one calls
    f = torch.zeros((5, 40, 60), device=cuda)
    b = torch.zeros((5, 40, 60), dtype=torch.uint8, device=cuda)
    out = torch.full((5, 40, 60), FILL, device=cuda)

    def ssd(C=1, H=40, W=60, k=7, hWin=9, wWin=9, P1=1.0, P2=2.0, paths=0x0f, mu=0.2, flow=out.data_ptr(), depth=None, scale=None):
        tail = (P1, P2, paths, 1, mu, flow, out[2].data_ptr(), depth, None)
        if scale is None:
            return lib.dfe_flow_depth_pair_sgm_f32(ctx.handle, f.data_ptr(), f.data_ptr(), C, H, W, k, hWin, wWin, 30.0, 20.0, *tail)
        return lib.dfe_flow_depth_pair_sgm_u8(ctx.handle, b.data_ptr(), b.data_ptr(), C, H, W, k, hWin, wWin, 30.0, 20.0, scale, *tail)

    for scale, name in ((None, "dfe_flow_depth_pair_sgm_f32"), (1.0, "dfe_flow_depth_pair_sgm_u8")):
        for bad in (dict(C=0), dict(k=0), dict(hWin=0), dict(flow=None), dict(depth=out[3].data_ptr()), dict(paths=0), dict(paths=256), dict(P1=3.0), dict(P1=-1.0),
                    dict(P2=inf), dict(P1=nan), dict(mu=1.5), dict(mu=nan)):
            assert ssd(scale=scale, **bad) == DFE_E_ARG, bad
            assert name in ctx.last_error(), ctx.last_error()
        assert ssd(scale=scale, hWin=33, wWin=34, H=80, W=80) == DFE_E_UNSUPPORTED
        assert ssd(scale=scale, H=14) == DFE_E_SHAPE and ssd(scale=scale, W=14) == DFE_E_SHAPE
    assert ssd(scale=0.0) == DFE_E_ARG and ssd(scale=-1.0) == DFE_E_ARG

    def census(C=1, H=40, W=60, k=7, hWin=9, wWin=9, agg=3, P1=1.0, P2=2.0, paths=0x0f, mu=0.2):
        return lib.dfe_census_flow_depth_pair_sgm2_f32(ctx.handle, f.data_ptr(), f.data_ptr(), C, H, W, k, hWin, wWin, agg, 30.0, 20.0, P1, P2, paths, 1, mu,
                                                       out.data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None, None)

    for bad in (dict(agg=2), dict(agg=0), dict(C=5), dict(hWin=0), dict(k=8), dict(k=9), dict(paths=0), dict(paths=256), dict(P1=3.0), dict(P1=-1.0),
                dict(P2=inf), dict(P1=nan), dict(mu=-0.5), dict(mu=2.0)):
        assert census(**bad) == DFE_E_ARG, bad
        assert "dfe_census_flow_depth_pair_sgm2_f32" in ctx.last_error()
    assert census(hWin=33, wWin=34) == DFE_E_UNSUPPORTED
    assert census(H=16) == DFE_E_SHAPE and census(H=3) == DFE_E_SHAPE
    assert lib.dfe_census_flow_depth_pair_sgm2_u8(ctx.handle, b.data_ptr(), b.data_ptr(), 1, 40, 60, 7, 9, 9, 3, 30.0, 20.0, 0.0, 1.0, 2.0, 0x0f, 1, 0.2,
                                                  out.data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None, None) == DFE_E_ARG
    torch.cuda.synchronize()
    assert (out == FILL).all(), "a refused call wrote something"
