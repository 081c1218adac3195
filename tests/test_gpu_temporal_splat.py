"""The four-tap splat of the temporal depth filter on the device (include/dfe.h: dfe_forward_splat_f32, dfe_temporal_step_splat_f32; DESIGN
section 4.36) against the numpy restatement of its definition (tests/temporal_splat_ref.py), bit for bit, through the C ABI with every
output pre-filled with NaN and guard elements behind it.  Every case runs both forms of the accumulate pass (option splat_lds = 0 and 1)
and each of them twice: the sums are integers, so all four runs must give the reference's bits.  The shapes are small on purpose: a
13 x 19 region inside a 17 x 23 frame has a partial 64-wide tile, a partial 4-row and a partial 8-row tile, and with flows of up to 6
pixels against the LDS window's margin of 3 its taps land inside the window, outside it and outside the region."""
import numpy as np
import pytest
import torch

from tests.temporal_ref import SCENE_TOL, SCENE_WMAX
from tests.temporal_splat_ref import TemporalFilterSplatRef, forward_splat_ref, temporal_step_splat_ref
from tests.test_gpu_temporal import E_ARG, E_SHAPE, F, P, T, floats, guarded, run_fuse, same, unguard, untouched

pytestmark = pytest.mark.gpu

H, W, REGION = 17, 23, (2, 2, 13, 19)


# ------------------------------------------------------------------------------------------------------------------------- runners
def run_splat(dfe, cuda, lds, v, w, flow, key=None, region=None, gain=None, bias=None, decay=1.0, ztol=0.0, quant=1024.0, min_cover=0.0, want_cover=True):
    Cc, h, wd = v.shape
    ctx, reg = dfe.get_ctx(0), (0, 0, h, wd) if region is None else region
    tv, tw, tf, tk = T(v, cuda), T(w, cuda), T(flow, cuda), T(key, cuda)
    out, wout, cover = guarded(Cc * h * wd, cuda), guarded(h * wd, cuda), guarded(h * wd, cuda)
    ctx.set_option("splat_lds", lds)
    try:
        ctx.check(dfe.lib().dfe_forward_splat_f32(ctx.handle, P(tv), Cc, h, wd, P(tw), P(tf), P(tk), *reg, floats(gain), floats(bias), decay, ztol, quant,
                                                 min_cover, P(out), P(wout), P(cover) if want_cover else None))
        torch.cuda.synchronize()
    finally:
        ctx.set_option("splat_lds", None)
    assert want_cover or untouched(cover)
    return unguard(out, (Cc, h, wd), "out"), unguard(wout, (h, wd), "wout"), unguard(cover, (h, wd), "cover") if want_cover else None


STEP_OUTS = ("out", "wout", "flag", "prior", "wprior", "cover")


def run_step(dfe, cuda, lds, v, w, flow, m, wm, tol, wmax, key, region, gain, bias, decay, ztol, quant, min_cover, want=("flag", "prior", "wprior", "cover")):
    Cc, h, wd = v.shape
    ctx, reg = dfe.get_ctx(0), (0, 0, h, wd) if region is None else region
    ins = [T(a, cuda) for a in (v, w, flow, key, m, wm)]
    shapes = dict(out=(Cc, h, wd), wout=(h, wd), flag=(h, wd), prior=(Cc, h, wd), wprior=(h, wd), cover=(h, wd))
    bufs = {k: guarded(int(np.prod(s)), cuda) for k, s in shapes.items()}
    given = {k: P(bufs[k]) if k in want or k in ("out", "wout") else None for k in shapes}
    ctx.set_option("splat_lds", lds)
    try:
        ctx.check(dfe.lib().dfe_temporal_step_splat_f32(ctx.handle, P(ins[0]), Cc, h, wd, P(ins[1]), P(ins[2]), P(ins[3]), *reg, floats(gain), floats(bias), decay,
                                                       ztol, quant, min_cover, P(ins[4]), P(ins[5]), tol, wmax, *[given[k] for k in STEP_OUTS]))
        torch.cuda.synchronize()
    finally:
        ctx.set_option("splat_lds", None)
    for k in shapes:
        assert given[k] is not None or untouched(bufs[k]), k
    return {k: unguard(bufs[k], shapes[k], k) for k in shapes if given[k] is not None}


def check_splat(dfe, cuda, what, v, w, flow, key=None, region=None, **kw):
    """both forms, each twice, against the reference; returns the reference with its integer planes"""
    want = forward_splat_ref(v, w, flow, key, region, sums=True, **kw)
    assert want[3]["taps"].max() <= 256, "the case is outside the definition"
    for lds in (0, 1):
        for again in (0, 1):
            got = run_splat(dfe, cuda, lds, v, w, flow, key, region, **kw)
            for g, r, name in zip(got, want, ("out", "wout", "cover")):
                same(g, r, "%s splat_lds=%d run %d %s" % (what, lds, again, name))
    return want


# -------------------------------------------------------------------------------------------------------------------------- inputs
def inputs(Cc, seed, region=REGION, h=H, wd=W, layers=False):
    """a state with holes (weights 0 and 1e-7, a NaN under some zero weights and over some weights), a fractional flow of up to 6 pixels
    with a third of its components on exact .5 fractions and a tenth on integers, negative ones, NaN and Inf, and on each side of the
    region a line of sources whose taps straddle the bound; layers: two depth layers, 3 and 7, that move against each other"""
    rng = np.random.default_rng(seed)
    y0, x0, Ho, Wo = region
    v = (rng.normal(size=(Cc, h, wd)) * 3).astype(F)
    w = rng.choice(np.array([0, 1e-7, 1e-6, 0.004, 0.5, 1, 2.5, 7, 300], F), (h, wd), p=[0.08, 0.04, 0.04, 0.04, 0.2, 0.3, 0.15, 0.1, 0.05])
    flow = rng.uniform(-6, 6, (2, h, wd)).astype(F)
    half = rng.random((2, h, wd)) < 0.33
    flow[half] = (np.floor(flow[half]) + F(0.5)).astype(F)
    whole = rng.random((2, h, wd)) < 0.1
    flow[whole] = np.floor(flow[whole])
    yy, xx = np.mgrid[0:h, 0:wd].astype(F)
    edge = np.array([-1.5, -1.0, -0.5, -0.25, 0.0, 0.25], F)       # around the bound: both taps out, one in, both in
    flow[0, y0, :] = rng.choice(edge, wd)
    flow[1, :, x0] = rng.choice(edge, h)
    flow[0, y0 + Ho - 1, :] = -rng.choice(edge, wd)
    flow[1, :, x0 + Wo - 1] = -rng.choice(edge, h)
    if layers:
        near = rng.random((h, wd)) < 0.4
        v[0] = np.where(near, 3, 7) + rng.normal(size=(h, wd)).astype(F) * F(0.05)
        flow[1] = np.where(near, F(1.25), F(-1.5))
        flow[0] = rng.uniform(-0.5, 0.5, (h, wd)).astype(F)
    key = (np.abs(v[0]) + 1).astype(F) if not layers else v[0].copy()
    hole = (w == 0) & (rng.random((h, wd)) < 0.5)
    v[:, hole] = np.nan
    for a, share in ((v, 0.02), (flow, 0.03), (key, 0.02)):
        hit = rng.random(a.shape) < share
        a[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(hit.sum()))
    return v, w.astype(F), flow, key


GB = [(None, None), ((1.5, -2.0, 0.25, 3.0), None), (None, (0.5, -1.0, 2.0, 0.0)), ((2.0, -0.5, 1.0, 0.75), (0.25, 1.0, -3.0, 0.0))]


# --------------------------------------------------------------------------------------------------------------------------- splat
@pytest.mark.parametrize("Cc", [1, 4])
@pytest.mark.parametrize("gb", range(4), ids=["plain", "gain", "bias", "gain-bias"])
def test_splat_random_flow_gain_bias_decay(dfe, cuda, Cc, gb):
    v, w, flow, key = inputs(Cc, 10 * Cc + gb)
    gain, bias = (None if g is None else g[:Cc] for g in GB[gb])
    for decay in (1.0, 0.75):
        want = check_splat(dfe, cuda, "decay %g" % decay, v, w, flow, key, REGION, gain=gain, bias=bias, decay=decay, ztol=0.5, quant=1024.0, min_cover=0.0)
        inside = want[2][2:15, 2:21]
        assert 0 < (inside > 0).sum() < inside.size and (inside > 1).any() and ((inside > 0) & (inside < 1)).any()   # holes, over- and under-covered targets
        assert want[3]["taps"].max() >= 3
    fin = flow[np.isfinite(flow)]
    assert fin.size < flow.size and (fin - np.floor(fin) == 0.5).any() and (fin < 0).any()


def test_splat_without_key_and_without_cover(dfe, cuda):
    for Cc in (1, 4):
        v, w, flow, _ = inputs(Cc, 3 + Cc)
        want = check_splat(dfe, cuda, "no key", v, w, flow, None, REGION, ztol=0.0, quant=512.0, min_cover=0.0)
        for lds in (0, 1):
            out, wout, none = run_splat(dfe, cuda, lds, v, w, flow, None, REGION, quant=512.0, want_cover=False)
            same(out, want[0], "out without cover")
            same(wout, want[1], "wout without cover")


@pytest.mark.parametrize("Cc", [1, 4])
def test_two_depth_layers_collide(dfe, cuda, Cc):
    """ztol = 0: only the taps whose key equals the front's; ztol = 0.5: the near layer's own spread (0.05) passes, the far layer (4
    behind) does not; ztol = 10: everything mixes"""
    v, w, flow, key = inputs(Cc, 40 + Cc, layers=True)
    res = [check_splat(dfe, cuda, "ztol %g" % z, v, w, flow, key, REGION, ztol=z, quant=1024.0, min_cover=0.0) for z in (0.0, 0.5, 10.0)]
    t0, t1, t2 = (r[3]["taps"] for r in res)
    assert (t0 <= t1).all() and (t1 <= t2).all() and (t0 < t1).any() and (t1 < t2).any()
    mixed = (res[2][0][0] > 3.5) & (res[2][0][0] < 6.5) & (res[2][1] > 0)
    assert mixed.any() and not ((res[1][0][0] > 3.5) & (res[1][0][0] < 6.5) & (res[1][1] > 0)).any()


@pytest.mark.parametrize("Cc", [1, 4])
def test_min_cover(dfe, cuda, Cc):
    v, w, flow, key = inputs(Cc, 50 + Cc)
    a = check_splat(dfe, cuda, "min_cover 0", v, w, flow, key, REGION, ztol=0.5, min_cover=0.0)
    b = check_splat(dfe, cuda, "min_cover 0.5", v, w, flow, key, REGION, ztol=0.5, min_cover=0.5)
    dropped = (a[2] > 0) & (b[2] == 0)
    assert dropped.any() and (a[2][dropped] < 0.5).all() and (b[2][b[2] > 0] >= 0.5).all()
    c = check_splat(dfe, cuda, "min_cover 1", v, w, flow, key, REGION, ztol=0.5, min_cover=1.0)
    assert (c[2][c[2] > 0] >= 1).all()


def test_sources_outside_the_quant_range_are_dropped_whole(dfe, cuda):
    v, w, flow, key = inputs(4, 60)
    v[:, 5, 7] = v[:, 8, 9] = v[:, 9, 9] = 1
    v[2, 5, 7], v[0, 8, 9], v[3, 9, 9] = 16385.0, -20000.0, 16384.0  # x 1024: above 2^24, below -2^24, 2^24 itself (stays)
    w[5, 7] = w[8, 9] = w[9, 9] = 1
    flow[:, 5, 7] = flow[:, 8, 9] = flow[:, 9, 9] = 0.25
    key[5, 7] = key[8, 9] = key[9, 9] = 0.5                        # in front of everything: they would own their targets
    want = check_splat(dfe, cuda, "quant range", v, w, flow, key, REGION, ztol=0.0, quant=1024.0)
    assert want[0][3, 9, 9] == 16384.0 and abs(want[0][2, 5, 7]) < 100 and abs(want[0][0, 8, 9]) < 100
    check_splat(dfe, cuda, "quant 1", v, w, flow, key, REGION, ztol=0.5, quant=1.0)           # coarse values: nothing dropped
    check_splat(dfe, cuda, "quant 3e6", v, w, flow, key, REGION, ztol=0.5, quant=3e6)        # most sources dropped


@pytest.mark.parametrize("Cc", [1, 4])
def test_256_taps_on_one_target_the_stated_bound(dfe, cuda, Cc):
    """16 x 16 sources sent to one pixel by an integer flow, every value at the top of the range (2^24 on the quant grid) and every weight
    above the cap: A = 256 2^14 2^16 2^24 = 2^62, the largest sum the definition allows"""
    h, wd, region = 17, 23, (0, 0, 16, 16)
    yy, xx = np.mgrid[0:h, 0:wd].astype(F)
    flow = np.stack((F(5) - yy, F(9) - xx)).astype(F)
    v = np.full((Cc, h, wd), 16384.0, F)
    if Cc > 1:
        v[1], v[3] = -16384.0, np.where((yy + xx) % 2 == 0, 16384.0, -16384.0)
    w = np.full((h, wd), 300.0, F)
    want = check_splat(dfe, cuda, "256 taps", v, w, flow, None, region, quant=1024.0)
    assert want[3]["taps"][5, 9] == 256 and want[3]["taps"].sum() == 256 and int(want[3]["A"][0, 5, 9]) == 2 ** 62
    assert want[0][0, 5, 9] == 16384.0 and want[1][5, 9] == 256.0 and want[2][5, 9] == 256.0
    check_splat(dfe, cuda, "256 taps, keyed", v, w, flow, np.full((h, wd), 2.0, F), region, quant=1024.0)


def test_regions_at_the_frame_corners_one_by_one_and_the_whole_frame(dfe, cuda):
    for Cc, region in ((1, (0, 0, 13, 19)), (4, (4, 4, 13, 19)), (1, (0, 0, 17, 23)), (4, (8, 11, 1, 1)), (1, (16, 22, 1, 1)), (1, (3, 0, 9, 23))):
        v, w, flow, key = inputs(Cc, 70 + region[0], region=region)
        if region[2] == 1:                                          # something must land on the one pixel
            w[region[0], region[1]], flow[:, region[0], region[1]], key[region[0], region[1]] = 1, 0.25, 1
            v[:, region[0], region[1]] = 2
        want = check_splat(dfe, cuda, "region %s" % (region,), v, w, flow, key, region, ztol=0.5)
        assert (want[1] > 0).any()
    v, w, flow, key = inputs(1, 80, region=(0, 0, 1, 1), h=1, wd=1)
    v[:], w[:], flow[:], key[:] = 1.5, 2, 0, 1
    want = check_splat(dfe, cuda, "1 x 1 frame", v, w, flow, key, None)
    assert want[0][0, 0, 0] == 1.5 and want[1][0, 0] == 2 and want[2][0, 0] == 1


def test_several_tiles(dfe, cuda):
    """more than one workgroup of either form in both directions, the LDS form's windows side by side: 37 x 150 in 40 x 155, a flow that
    expands about a point (the window follows the tile's centre) with a part that is thrown 40 pixels away (past every window)"""
    h, wd, region = 40, 155, (2, 3, 37, 150)
    for Cc in (1, 2, 3):
        v, w, flow, key = inputs(Cc, 90 + Cc, region=region, h=h, wd=wd)
        yy, xx = np.mgrid[0:h, 0:wd].astype(F)
        smooth = np.stack((F(0.06) * (yy - 20) + F(2.5), F(0.06) * (xx - 70) - F(7.25))).astype(F)
        far = np.random.default_rng(Cc).random((h, wd)) < 0.1
        smooth[1][far] += 40
        flow = np.where(np.isfinite(flow), smooth + flow * F(0.1), flow).astype(F)
        want = check_splat(dfe, cuda, "tiles C=%d" % Cc, v, w, flow, key, region, ztol=0.5, min_cover=0.25)
        assert (want[1] > 0).mean() > 0.25 and want[3]["taps"].max() >= 4


# ------------------------------------------------------------------------------------------------------------------------ one call
@pytest.mark.parametrize("Cc", [1, 4])
def test_one_call_equals_the_staged_pair_and_the_reference(dfe, cuda, Cc):
    v, w, flow, key = inputs(Cc, 100 + Cc)
    rng = np.random.default_rng(Cc)
    m = (np.nan_to_num(v, nan=0, posinf=0, neginf=0) + rng.normal(size=v.shape) * rng.choice([0.3, 3.0], (H, W))).astype(F)
    wm = rng.choice(np.array([0, 1e-7, 0.5, 1, 1, 2, 20], F), (H, W))
    m[:, (wm == 0) & (rng.random((H, W)) < 0.5)] = np.nan
    gain, bias, decay, tol, wmax = [1.0, 0.5, 2.0, -1.0][:Cc], [0.25, 0.0, -1.0, 1.0][:Cc] if Cc > 1 else None, 0.75, 1.5, 6.0
    sp = dict(ztol=0.5, quant=1024.0, min_cover=0.25)
    want = temporal_step_splat_ref(v, w, flow, m, wm, tol, wmax, key, REGION, gain, bias, decay, **sp)
    assert len(np.unique(want["flag"])) >= 5
    for lds in (0, 1):
        prior, wprior, cover = run_splat(dfe, cuda, lds, v, w, flow, key, REGION, gain, bias, decay, **sp)
        out, wout, flag = run_fuse(dfe, cuda, prior, wprior, m, wm, tol, wmax, REGION)
        staged = dict(out=out, wout=wout, flag=flag, prior=prior, wprior=wprior, cover=cover)
        got = run_step(dfe, cuda, lds, v, w, flow, m, wm, tol, wmax, key, REGION, gain, bias, decay, want=STEP_OUTS[2:], **sp)
        for k in STEP_OUTS:
            same(staged[k], want[k], "staged %s splat_lds=%d" % (k, lds))
            same(got[k], want[k], "one call %s splat_lds=%d" % (k, lds))
        for leave in STEP_OUTS[2:]:                                # each optional output NULL in turn
            lean = run_step(dfe, cuda, lds, v, w, flow, m, wm, tol, wmax, key, REGION, gain, bias, decay, want=[k for k in STEP_OUTS[2:] if k != leave], **sp)
            for k in lean:
                same(lean[k], want[k], "%s without %s" % (k, leave))
        lean = run_step(dfe, cuda, lds, v, w, flow, m, wm, tol, wmax, None, REGION, gain, bias, decay, want=(), **sp)
        ref = temporal_step_splat_ref(v, w, flow, m, wm, tol, wmax, None, REGION, gain, bias, decay, **sp)
        same(lean["out"], ref["out"], "out alone, no key")
        same(lean["wout"], ref["wout"], "wout alone, no key")


# -------------------------------------------------------------------------------------------------------------------------- errors
def test_errors_are_refused_before_any_launch(dfe, cuda):
    lib, ctx = dfe.lib(), dfe.get_ctx(0)
    Cc, h, wd, n = 2, 6, 8, 48
    v, w, flow, key, m, wm = (torch.ones(k * n, device=cuda) for k in (2, 1, 2, 1, 2, 1))
    nan, inf = float("nan"), float("inf")

    def outputs():
        return dict(out=guarded(2 * n, cuda), wout=guarded(n, cuda), flag=guarded(n, cuda), prior=guarded(2 * n, cuda), wprior=guarded(n, cuda),
                    cover=guarded(n, cuda), joint=guarded(3 * n, cuda))

    def ptr(o, k):
        return k if k is None or isinstance(k, int) else P(o[k])

    def splat(o, v=v, C_=Cc, H_=h, W_=wd, w=w, flow=flow, key=key, reg=(0, 0, h, wd), gain=None, bias=None, decay=1.0, ztol=0.5, quant=1024.0, min_cover=0.25,
              out="out", wout="wout", cover="cover"):
        return lib.dfe_forward_splat_f32(ctx.handle, P(v), C_, H_, W_, P(w), P(flow), P(key), *reg, floats(gain), floats(bias), decay, ztol, quant, min_cover,
                                         ptr(o, out), ptr(o, wout), ptr(o, cover))

    def step(o, v=v, C_=Cc, H_=h, W_=wd, w=w, flow=flow, key=key, reg=(0, 0, h, wd), gain=None, bias=None, decay=1.0, ztol=0.5, quant=1024.0, min_cover=0.25,
             m=m, wm=wm, tol=1.0, wmax=8.0, out="out", wout="wout", flag="flag", prior="prior", wprior="wprior", cover="cover"):
        return lib.dfe_temporal_step_splat_f32(ctx.handle, P(v), C_, H_, W_, P(w), P(flow), P(key), *reg, floats(gain), floats(bias), decay, ztol, quant,
                                               min_cover, P(m), P(wm), tol, wmax, ptr(o, out), ptr(o, wout), ptr(o, flag), ptr(o, prior), ptr(o, wprior),
                                               ptr(o, cover))

    regions = [(0, 0, 0, 8), (0, 0, 6, 0), (-1, 0, 6, 8), (0, -1, 6, 8), (1, 0, 6, 8), (0, 1, 6, 8), (0, 0, 7, 8), (0, 0, 6, 9)]
    both = [(E_ARG, dict(C_=0)), (E_ARG, dict(C_=5)), (E_ARG, dict(v=None)), (E_ARG, dict(w=None)), (E_ARG, dict(flow=None)), (E_ARG, dict(out=None)),
            (E_ARG, dict(wout=None)), (E_ARG, dict(decay=0.0)), (E_ARG, dict(decay=-0.5)), (E_ARG, dict(decay=1.25)), (E_ARG, dict(decay=nan)),
            (E_ARG, dict(gain=(1.0, nan))), (E_ARG, dict(gain=(inf, 1.0))), (E_ARG, dict(bias=(0.0, -inf))), (E_ARG, dict(bias=(nan, 0.0))),
            (E_ARG, dict(ztol=-0.5)), (E_ARG, dict(ztol=nan)), (E_ARG, dict(ztol=inf)), (E_ARG, dict(quant=0.0)), (E_ARG, dict(quant=-1.0)),
            (E_ARG, dict(quant=nan)), (E_ARG, dict(quant=inf)), (E_ARG, dict(min_cover=-0.1)), (E_ARG, dict(min_cover=1.5)), (E_ARG, dict(min_cover=nan)),
            (E_ARG, dict(H_=65536, W_=32768, reg=(0, 0, 1, 1))), (E_SHAPE, dict(H_=0)), (E_SHAPE, dict(W_=-3))] + [(E_SHAPE, dict(reg=r)) for r in regions]
    fusion = [(E_ARG, dict(tol=-1.0)), (E_ARG, dict(tol=nan)), (E_ARG, dict(wmax=inf)), (E_ARG, dict(wmax=nan)), (E_ARG, dict(wmax=5e-7)), (E_ARG, dict(m=None)),
              (E_ARG, dict(wm=None))]
    cases = [("dfe_forward_splat_f32", splat, rc, kw) for rc, kw in both] + [("dfe_temporal_step_splat_f32", step, rc, kw) for rc, kw in both + fusion]
    # overlaps: an output on an input, and two outputs on each other (the joint buffer holds the one and, half a plane in, the other)
    for fn, name in ((splat, "dfe_forward_splat_f32"), (step, "dfe_temporal_step_splat_f32")):
        for kw in (dict(v=None, out="v"), dict(w=None, wout="w"), dict(flow=None, cover="flow"), dict(key=None, wout="key"), dict(out="joint", wout="joint+"),
                   dict(out="joint", cover="joint+")):
            cases.append((name, fn, E_ARG, dict(kw, overlap=True)))
    for kw in (dict(prior="joint", wprior="joint+"), dict(flag="joint", cover="joint+"), dict(m=None, prior="m"), dict(wm=None, cover="wm")):
        cases.append(("dfe_temporal_step_splat_f32", step, E_ARG, dict(kw, overlap=True)))
    inputs_ = dict(v=v, w=w, flow=flow, key=key, m=m, wm=wm)
    for name, fn, rc, kw in cases:
        o = outputs()
        if kw.pop("overlap", False):                              # an output placed on an input's memory or on the joint buffer
            kw = dict(kw)
            for k, val in list(kw.items()):
                if val is None:
                    del kw[k]
                elif val in inputs_:
                    kw[k] = inputs_[val].data_ptr() + 4
                elif val == "joint+":
                    kw[k] = o["joint"].data_ptr() + 4 * (n // 2)
        before = {k: t.clone() for k, t in inputs_.items()}
        got = fn(o, **kw)
        torch.cuda.synchronize()
        assert got == rc, (name, kw, got, lib.dfe_last_error(ctx.handle))
        assert lib.dfe_last_error(ctx.handle).startswith(name.encode()), (name, kw, lib.dfe_last_error(ctx.handle))
        assert all(untouched(t) for t in o.values()), (name, kw)
        assert all(torch.equal(before[k], inputs_[k]) for k in inputs_), (name, kw)


def test_python_checks_raise_before_any_device_work(dfe, cuda):
    v, w, f = torch.zeros((2, 6, 8), device=cuda), torch.ones((6, 8), device=cuda), torch.zeros((2, 6, 8), device=cuda)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(ztol=-1.0), dict(ztol=nan), dict(ztol=inf), dict(quant=0.0), dict(quant=inf), dict(quant=nan), dict(min_cover=-0.5), dict(min_cover=2.0),
               dict(min_cover=nan), dict(decay=0.0), dict(gain=(1.0,))):
        with pytest.raises(ValueError):
            dfe.forwardSplat(v, w, f, **kw)
        with pytest.raises(ValueError):
            dfe.temporalStep(v, w, f, v, w, 1.0, splat="bilinear", **kw)
        if "decay" not in kw and "gain" not in kw:
            with pytest.raises(ValueError):
                dfe.TemporalFilter(1.0, splat="bilinear", **kw)
    for call in (lambda: dfe.temporalStep(v, w, f, v, w, 1.0, splat="cubic"), lambda: dfe.TemporalFilter(1.0, splat="cubic"), lambda: dfe.TemporalFilter(-1.0, splat="bilinear")):
        with pytest.raises(ValueError):
            call()
    r = dfe.temporalStep(v, w, f, v, w, 1.0, splat="bilinear", want_prior=True)
    assert set(r) == {"out", "wout", "flag", "prior", "wprior", "cover"}
    assert set(dfe.temporalStep(v, w, f, v, w, 1.0, want_prior=True)) == {"out", "wout", "flag", "prior", "wprior", "src"}   # the default: the nearest warp


# -------------------------------------------------------------------------------------------------------------------------- filter
def test_filter_bilinear_over_four_frames_equals_the_reference_loop(dfe, cuda):
    from tests.test_temporal_splat_ref_cpu import subpixel_scene

    ref = TemporalFilterSplatRef(SCENE_TOL, SCENE_WMAX, decay=0.75, key_channel=0)
    f = dfe.TemporalFilter(SCENE_TOL, SCENE_WMAX, decay=0.75, splat="bilinear")
    assert (f.ztol, f.quant, f.min_cover) == (SCENE_TOL, 1024.0, 0.25)
    region = (2, 3, 40, 56)
    for t, (truth, meas, weight, flow) in enumerate(subpixel_scene(0, frames=4)):
        want = ref.push(meas, weight, flow, region)
        got = f.push(T(meas, cuda), T(weight, cuda), T(flow, cuda), region=region)
        for g, r, what in zip(got, want, ("state", "weight", "flag")):
            same(g.cpu().numpy(), r, "frame %d %s" % (t, what))
    assert set(np.unique(want[2])) >= {1, 3, 5}                    # (a prior without holes: hardly a pixel with the measurement alone)
    out, wout, cover = dfe.forwardSplat(got[0], got[1], T(flow, cuda), got[0][0], region, decay=0.75, ztol=SCENE_TOL, min_cover=0.25)
    rs = forward_splat_ref(want[0], want[1], flow, want[0][0], region, decay=0.75, ztol=SCENE_TOL, min_cover=0.25)
    for g, r, what in zip((out, wout, cover), rs, ("out", "wout", "cover")):
        same(g.cpu().numpy(), r, "forwardSplat " + what)


def test_filter_bilinear_with_rectify_equals_the_composition(dfe, cuda):
    from tests.test_temporal_splat_ref_cpu import subpixel_scene

    K = np.array([[60.0, 0, 32], [0, 60.0, 24], [0, 0, 1]])
    a = 0.02
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    f = dfe.TemporalFilter(SCENE_TOL, SCENE_WMAX, decay=0.75, gain=(1.0,), bias=(0.125,), splat="bilinear", ztol=0.5, quant=512.0, min_cover=0.5)
    frames = [tuple(T(x, cuda) for x in fr[1:]) for fr in subpixel_scene(1, frames=3)]
    region = (2, 3, 40, 56)
    state, weight, flag = f.push(*frames[0], region=region)
    for t in (1, 2):
        prior, wprior, _ = dfe.forwardSplat(state, weight, frames[t - 1][2], state[0], region, (1.0,), (0.125,), 0.75, 0.5, 512.0, 0.5)
        warped, mask = dfe.sfm2.removeEgoMotion(torch.cat((prior, wprior[None])), K, R, inverse=True)
        want = dfe.temporalFuse(warped[:1].contiguous(), warped[1] * mask, frames[t][0], frames[t][1], SCENE_TOL, SCENE_WMAX, region)
        state, weight, flag = f.push(*frames[t], region=region, rectify=(K, R))
        for g, r, what in zip((state, weight, flag), want, ("state", "weight", "flag")):
            assert torch.equal(g, r), "frame %d %s" % (t, what)
        assert (flag == 3).any() and (mask == 0).any()
