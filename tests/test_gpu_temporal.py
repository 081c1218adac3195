"""The temporal depth filter on the device (include/dfe.h): dfe_forward_warp_f32, dfe_temporal_fuse_f32 and
dfe_temporal_step_f32 against the numpy restatement of their definitions (tests/temporal_ref.py), bit for bit, through the C ABI with
every output pre-filled (NaN / -7) and guard elements behind it; TemporalFilter against the reference loop and against the hand-written
composition of its stages; and the video session's temporal= keyword."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.temporal_ref import (SCENE_TOL, SCENE_WMAX, TemporalFilterRef, forward_warp_ref, scene, temporal_fuse_ref, temporal_step_ref)

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 64
E_ARG, E_SHAPE = -1, -2                                           # DFE_E_ARG, DFE_E_SHAPE (include/dfe.h)


def T(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def P(t):
    return None if t is None else t.data_ptr()


def guarded(n, cuda, dtype=torch.float32):
    """n elements and a tail, all NaN (float) or -7 (int)"""
    return torch.full((n + TAIL,), float("nan") if dtype == torch.float32 else -7, device=cuda, dtype=dtype)


def untouched(buf):
    b = buf.cpu().numpy()
    return bool(np.isnan(b).all()) if b.dtype == F else bool((b == -7).all())


def unguard(buf, shape, what):
    b, n = buf.cpu().numpy(), int(np.prod(shape))
    assert untouched(buf[n:]), "%s: wrote behind the output" % what
    assert not (np.isnan(b[:n]).any() if b.dtype == F else (b[:n] == -7).any()), "%s: left elements unwritten" % what
    return b[:n].reshape(shape)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, len(bad), got.size, i, got[i], want[i]))


def floats(v):
    return None if v is None else (C.c_float * len(v))(*v)


# ------------------------------------------------------------------------------------------------------------------------- runners
def run_warp(dfe, cuda, v, w, flow, key=None, region=None, gain=None, bias=None, decay=1.0, want_src=True):
    Cc, H, W = v.shape
    ctx, reg = dfe.get_ctx(0), (0, 0, H, W) if region is None else region
    tv, tw, tf, tk = T(v, cuda), T(w, cuda), T(flow, cuda), T(key, cuda)
    out, wout, src = guarded(Cc * H * W, cuda), guarded(H * W, cuda), guarded(H * W, cuda, torch.int32)
    ctx.check(dfe.lib().dfe_forward_warp_f32(ctx.handle, P(tv), Cc, H, W, P(tw), P(tf), P(tk), *reg, floats(gain), floats(bias), decay, P(out), P(wout),
                                            P(src) if want_src else None))
    torch.cuda.synchronize()
    assert want_src or untouched(src)
    return unguard(out, (Cc, H, W), "out"), unguard(wout, (H, W), "wout"), unguard(src, (H, W), "src") if want_src else None


def run_fuse(dfe, cuda, z, wp, m, wm, tol, wmax=8.0, region=None, want_flag=True):
    Cc, H, W = z.shape
    ctx, reg = dfe.get_ctx(0), (0, 0, H, W) if region is None else region
    tz, twp, tm, twm = T(z, cuda), T(wp, cuda), T(m, cuda), T(wm, cuda)
    out, wout, flag = guarded(Cc * H * W, cuda), guarded(H * W, cuda), guarded(H * W, cuda)
    ctx.check(dfe.lib().dfe_temporal_fuse_f32(ctx.handle, P(tz), P(twp), P(tm), P(twm), Cc, H, W, *reg, tol, wmax, P(out), P(wout), P(flag) if want_flag else None))
    torch.cuda.synchronize()
    assert want_flag or untouched(flag)
    return unguard(out, (Cc, H, W), "out"), unguard(wout, (H, W), "wout"), unguard(flag, (H, W), "flag") if want_flag else None


def run_step(dfe, cuda, v, w, flow, m, wm, tol, wmax=8.0, key=None, region=None, gain=None, bias=None, decay=1.0, want=("flag", "prior", "wprior", "src")):
    Cc, H, W = v.shape
    ctx, reg = dfe.get_ctx(0), (0, 0, H, W) if region is None else region
    ins = [T(a, cuda) for a in (v, w, flow, key, m, wm)]
    shapes = dict(out=(Cc, H, W), wout=(H, W), flag=(H, W), prior=(Cc, H, W), wprior=(H, W), src=(H, W))
    bufs = {k: guarded(int(np.prod(s)), cuda, torch.int32 if k == "src" else torch.float32) for k, s in shapes.items()}
    given = {k: P(bufs[k]) if k in want or k in ("out", "wout") else None for k in shapes}
    ctx.check(dfe.lib().dfe_temporal_step_f32(ctx.handle, P(ins[0]), Cc, H, W, P(ins[1]), P(ins[2]), P(ins[3]), *reg, floats(gain), floats(bias), decay, P(ins[4]),
                                             P(ins[5]), tol, wmax, *[given[k] for k in ("out", "wout", "flag", "prior", "wprior", "src")]))
    torch.cuda.synchronize()
    for k in shapes:
        assert given[k] is not None or untouched(bufs[k]), k
    return {k: unguard(bufs[k], shapes[k], k) for k in shapes if given[k] is not None}


# -------------------------------------------------------------------------------------------------------------------------- inputs
WEIGHTS = np.array([0, 1e-7, 1e-6, 0.5, 7, 1, 2.5], F)
POISON = np.array([np.nan, np.inf, -np.inf], F)


def poison(rng, a, share=0.03):
    hit = rng.random(a.shape) < share
    a[hit] = rng.choice(POISON, int(hit.sum()))


def warp_inputs(Cc, H, W, seed, flow_kind="int", key_kind="depth", poisoned=True, region=None):
    rng = np.random.default_rng(seed)
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else region
    v = (rng.normal(size=(Cc, H, W)) * 3).astype(F)
    w = rng.choice(WEIGHTS, (H, W), p=[0.08, 0.05, 0.1, 0.2, 0.2, 0.27, 0.1])
    yy, xx = np.mgrid[0:H, 0:W].astype(F)
    if flow_kind == "int":                                         # +-4: many collisions
        flow = rng.integers(-4, 5, (2, H, W)).astype(F)
    elif flow_kind == "sub":                                       # sub-pixel, a third on exact .5 fractions; the first row and column aim at
        flow = rng.uniform(-3, 3, (2, H, W)).astype(F)             # coordinates around -0.5 (just below: outside; -0.5 itself: pixel 0)
        half = rng.random((2, H, W)) < 0.33
        flow[half] = (np.floor(flow[half]) + F(0.5)).astype(F)
        edge = np.array([np.nextafter(F(-0.5), F(-1)), F(-0.5), F(-0.25), np.nextafter(F(-0.5), F(0))], F)
        flow[0, y0, :] = rng.choice(edge, W)
        flow[1, :, x0] = rng.choice(edge, H)
    elif flow_kind == "one":                                       # every source of R to one target
        flow = np.stack((F(y0 + Ho // 2) - yy, F(x0 + Wo // 3) - xx)).astype(F)
    else:                                                          # "leave": half of the sources leave the region, on every side
        flow = rng.integers(-1, 2, (2, H, W)).astype(F)
        side = rng.integers(0, 8, (H, W))
        flow[0][side == 0], flow[0][side == 1] = -(yy[side == 0] - y0 + 1), (y0 + Ho - yy[side == 1])
        flow[1][side == 2], flow[1][side == 3] = -(xx[side == 2] - x0 + 1), (x0 + Wo - xx[side == 3])
    if key_kind is None:
        key = None
    elif key_kind == "depth":
        key = rng.uniform(1, 10, (H, W)).astype(F)
    elif key_kind == "neg":
        key = (rng.normal(size=(H, W)) * 4).astype(F)
    elif key_kind == "zeros":                                      # -0.0 against +0.0: equal keys, the smaller index wins
        key = rng.choice(np.array([-0.0, 0.0], F), (H, W))
    elif key_kind == "few":                                        # many ties between negative and positive values
        key = rng.choice(np.array([-2.5, -0.0, 0.0, 1e-30, 3], F), (H, W))
    else:                                                          # "equal"
        key = np.full((H, W), 3, F)
    if poisoned:
        for a in (v, w, flow) + (() if key is None else (key,)):
            poison(rng, a)
    return v, w.astype(F), flow, key


def fuse_inputs(Cc, H, W, seed, integer=False):
    rng = np.random.default_rng(seed)
    if integer:                                                    # |d|^2 hits tol^2 = 4 exactly
        z, m = rng.integers(0, 4, (Cc, H, W)).astype(F), rng.integers(0, 4, (Cc, H, W)).astype(F)
    else:
        z = (rng.normal(size=(Cc, H, W)) * 2).astype(F)
        m = (z + rng.normal(size=(Cc, H, W)) * rng.choice([0.3, 3.0], (H, W))).astype(F)
    ws = np.array([0, 1e-7, 1e-6, 0.5, 1, 1, 2, 3, 7, 20], F)      # holes on either side and on both, a == b, weights above wmax
    wp, wm = rng.choice(ws, (H, W)), rng.choice(ws, (H, W))
    for val, wt in ((z, wp), (m, wm)):                             # a NaN under a zero weight, and one over a weight (a hole by the rule)
        hole = (wt == 0) & (rng.random((H, W)) < 0.5)
        val[:, hole] = np.nan
        poison(rng, val, 0.02)
        poison(rng, wt, 0.02)
    return z, wp, m, wm


SHAPES = [("1x1", 1, 1, None), ("3x5", 3, 5, None), ("37x67", 37, 67, None), ("64x256", 64, 256, None), ("37x67 inner", 37, 67, (3, 5, 29, 50))]


# ---------------------------------------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("name,H,W,region", SHAPES, ids=[s[0] for s in SHAPES])
def test_warp_shapes(dfe, cuda, name, H, W, region, Cc):
    for flow_kind, key_kind in (("int", "depth"), ("sub", "neg")):
        v, w, flow, key = warp_inputs(Cc, H, W, 7 * Cc + H, flow_kind, key_kind, poisoned=H > 1, region=region)
        gain, bias = ([1.5, -2.0, 0.25, 3.0][:Cc], None) if Cc % 2 else (None, [0.5, -1.0, 2.0, 0.0][:Cc])
        got = run_warp(dfe, cuda, v, w, flow, key, region, gain, bias, 0.75 if Cc > 2 else 1.0)
        want = forward_warp_ref(v, w, flow, key, region, gain, bias, 0.75 if Cc > 2 else 1.0)
        for g, r, what in zip(got, want, ("out", "wout", "src")):
            same(g, r, "%s %s C=%d %s" % (name, flow_kind, Cc, what))
        if H > 3 and flow_kind == "int":
            assert (want[2] >= 0).sum() > 0.2 * (want[2].size if region is None else region[2] * region[3])   # the case is not empty


FLOW_CASES = [(f, k, gb, d, reg) for f in ("int", "sub", "leave") for k, gb, d, reg in (
    ("depth", (None, None), 1.0, None), ("neg", ((2.0, -0.5), (0.25, 1.0)), 0.75, (3, 5, 29, 50)), ("zeros", ((1.0, 3.0), None), 1.0, None),
    ("few", (None, (1.0, -1.0)), 0.75, None), ("equal", (None, None), 0.75, (3, 5, 29, 50)), (None, ((-1.0, 0.5), (0.0, 0.0)), 1.0, None))]


@pytest.mark.parametrize("flow_kind,key_kind,gb,decay,region", FLOW_CASES, ids=["%s-%s-%s" % (c[0], c[1], "inner" if c[4] else "frame") for c in FLOW_CASES])
def test_warp_flows_keys_and_value_models(dfe, cuda, flow_kind, key_kind, gb, decay, region):
    v, w, flow, key = warp_inputs(2, 37, 67, len(flow_kind) + 3 * len(str(key_kind)), flow_kind, key_kind, region=region)
    got = run_warp(dfe, cuda, v, w, flow, key, region, gb[0], gb[1], decay)
    want = forward_warp_ref(v, w, flow, key, region, gb[0], gb[1], decay)
    for g, r, what in zip(got, want, ("out", "wout", "src")):
        same(g, r, what)
    inside = want[2] if region is None else want[2][region[0]:region[0] + region[2], region[1]:region[1] + region[3]]
    assert 0 < (inside >= 0).sum() < inside.size                   # targets with a winner and targets without
    out2, wout2, none = run_warp(dfe, cuda, v, w, flow, key, region, gb[0], gb[1], decay, want_src=False)
    same(out2, want[0], "out without src")
    same(wout2, want[1], "wout without src")


@pytest.mark.parametrize("key_kind", ["depth", "equal", None])
def test_warp_every_source_on_one_target_is_reproducible(dfe, cuda, key_kind):
    """2479 contenders on one word: the integer minimum does not depend on who arrives first"""
    v, w, flow, key = warp_inputs(3, 37, 67, 5, "one", key_kind, poisoned=False)
    w[:] = 1
    want = forward_warp_ref(v, w, flow, key)
    assert (want[2] >= 0).sum() == 1 and want[2][18, 22] == (int(np.argmin(key)) if key_kind == "depth" else 0)
    first = run_warp(dfe, cuda, v, w, flow, key)
    second = run_warp(dfe, cuda, v, w, flow, key)
    for g, g2, r, what in zip(first, second, want, ("out", "wout", "src")):
        same(g, r, what)
        same(g2, r, what + " (second call)")


def test_warp_weights_are_not_clipped_and_small_ones_are_holes(dfe, cuda):
    w = np.array([[0, 1e-7, 1e-6, 0.5, 7]], F)
    v = np.arange(1, 6, dtype=F).reshape(1, 1, 5)
    out, wout, src = run_warp(dfe, cuda, v, w, np.zeros((2, 1, 5), F), decay=1.0)
    assert src[0].tolist() == [-1, -1, 2, 3, 4] and wout[0].tolist() == [0, 0, F(1e-6), 0.5, 7] and out[0, 0].tolist() == [0, 0, 3, 4, 5]
    same(run_warp(dfe, cuda, v, w, np.zeros((2, 1, 5), F), decay=0.75)[1], forward_warp_ref(v, w, np.zeros((2, 1, 5), F), decay=0.75)[1], "decayed")


# ---------------------------------------------------------------------------------------------------------------------------- fuse
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("name,H,W,region", SHAPES, ids=[s[0] for s in SHAPES])
def test_fuse_shapes(dfe, cuda, name, H, W, region, Cc):
    for integer, tol, wmax in ((True, 2.0, 8.0), (False, 1.0, 6.0)):
        z, wp, m, wm = fuse_inputs(Cc, H, W, 11 * Cc + W, integer)
        got = run_fuse(dfe, cuda, z, wp, m, wm, tol, wmax, region)
        want = temporal_fuse_ref(z, wp, m, wm, tol, wmax, region)
        for g, r, what in zip(got, want, ("out", "wout", "flag")):
            same(g, r, "%s C=%d integer=%s %s" % (name, Cc, integer, what))
        if H * W > 100:
            assert set(np.unique(want[2])) == {0, 1, 2, 3, 4, 5}   # every row of the table
            if integer and Cc == 1:
                d2 = (np.nan_to_num(z[0], posinf=0, neginf=0) - np.nan_to_num(m[0], posinf=0, neginf=0)) ** 2
                assert ((want[2] == 3) & (d2 == 4)).any()            # the boundary d2 == tol^2 agrees
    same(run_fuse(dfe, cuda, z, wp, m, wm, tol, wmax, region, want_flag=False)[0], want[0], "out without flag")


def test_fuse_in_place(dfe, cuda):
    z, wp, m, wm = fuse_inputs(2, 37, 67, 3)
    region = (3, 5, 29, 50)
    want = temporal_fuse_ref(z, wp, m, wm, 1.0, 6.0, region)
    ctx = dfe.get_ctx(0)
    for over in ("prior", "meas"):
        tz, twp, tm, twm = T(z, cuda), T(wp, cuda), T(m, cuda), T(wm, cuda)
        out, wout = (tz, twp) if over == "prior" else (tm, twm)
        flag = guarded(37 * 67, cuda)
        ctx.check(dfe.lib().dfe_temporal_fuse_f32(ctx.handle, P(tz), P(twp), P(tm), P(twm), 2, 37, 67, *region, 1.0, 6.0, P(out), P(wout), P(flag)))
        same(out.cpu().numpy(), want[0], "out = " + over)
        same(wout.cpu().numpy(), want[1], "wout over " + over)
        same(unguard(flag, (37, 67), "flag"), want[2], "flag")


# ------------------------------------------------------------------------------------------------------------------------ one call
STEP_CASES = [(Cc, f, k, reg) for Cc, f, k, reg in ((1, "int", "depth", None), (2, "sub", "neg", (3, 5, 29, 50)), (3, "leave", "few", None), (4, "int", None, (3, 5, 29, 50)),
                                                    (2, "one", "equal", None))]


@pytest.mark.parametrize("Cc,flow_kind,key_kind,region", STEP_CASES, ids=["C%d-%s-%s" % c[:3] for c in STEP_CASES])
def test_one_call_equals_the_staged_pair_and_the_reference(dfe, cuda, Cc, flow_kind, key_kind, region):
    v, w, flow, key = warp_inputs(Cc, 37, 67, 20 + Cc, flow_kind, key_kind, region=region)
    _, _, m, wm = fuse_inputs(Cc, 37, 67, 30 + Cc)
    m = (m * F(0.5) + np.nan_to_num(v, nan=0, posinf=0, neginf=0)).astype(F)        # near the state: agreements and dissents
    gain, bias, decay, tol, wmax = [1.0, 0.5, 2.0, -1.0][:Cc], [0.25, 0.0, -1.0, 1.0][:Cc] if Cc > 1 else None, 0.75, 1.5, 6.0
    want = temporal_step_ref(v, w, flow, m, wm, tol, wmax, key, region, gain, bias, decay)
    prior, wprior, src = run_warp(dfe, cuda, v, w, flow, key, region, gain, bias, decay)
    out, wout, flag = run_fuse(dfe, cuda, prior, wprior, m, wm, tol, wmax, region)
    staged = dict(out=out, wout=wout, flag=flag, prior=prior, wprior=wprior, src=src)
    got = run_step(dfe, cuda, v, w, flow, m, wm, tol, wmax, key, region, gain, bias, decay)
    for k in ("out", "wout", "flag", "prior", "wprior", "src"):
        same(staged[k], want[k], "staged " + k)
        same(got[k], want[k], "one call " + k)
    assert len(np.unique(want["flag"])) >= 4 or flow_kind == "one"
    lean = run_step(dfe, cuda, v, w, flow, m, wm, tol, wmax, key, region, gain, bias, decay, want=())
    same(lean["out"], want["out"], "out alone")
    same(lean["wout"], want["wout"], "wout alone")


# -------------------------------------------------------------------------------------------------------------------------- errors
def test_errors_are_refused_before_any_launch(dfe, cuda):
    lib, ctx = dfe.lib(), dfe.get_ctx(0)
    Cc, H, W, n = 2, 6, 8, 48
    v, w, flow, key, m, wm = (torch.ones(k * n, device=cuda) for k in (2, 1, 2, 1, 2, 1))
    nan, inf = float("nan"), float("inf")

    def outputs():
        return dict(out=guarded(2 * n, cuda), wout=guarded(n, cuda), flag=guarded(n, cuda), prior=guarded(2 * n, cuda), wprior=guarded(n, cuda),
                    src=guarded(n, cuda, torch.int32), joint=guarded(3 * n, cuda))

    def warp(o, v=v, C_=Cc, H_=H, W_=W, w=w, flow=flow, key=key, reg=(0, 0, H, W), gain=None, bias=None, decay=1.0, out="out", wout="wout", src="src"):
        ptr = lambda k: k if k is None or isinstance(k, int) else P(o[k])
        return lib.dfe_forward_warp_f32(ctx.handle, P(v), C_, H_, W_, P(w), P(flow), P(key), *reg, floats(gain), floats(bias), decay, ptr(out), ptr(wout), ptr(src))

    def fuse(o, z=v, wp=w, m=m, wm=wm, C_=Cc, reg=(0, 0, H, W), tol=1.0, wmax=8.0, out="out", wout="wout"):
        ptr = lambda k: None if k is None else P(o[k])
        return lib.dfe_temporal_fuse_f32(ctx.handle, P(z), P(wp), P(m), P(wm), C_, H, W, *reg, tol, wmax, ptr(out), ptr(wout), P(o["flag"]))

    def step(o, v=v, C_=Cc, H_=H, W_=W, w=w, flow=flow, key=key, reg=(0, 0, H, W), gain=None, bias=None, decay=1.0, m=m, wm=wm, tol=1.0, wmax=8.0, out="out",
             wout="wout", flag="flag", prior="prior", wprior="wprior", src="src"):
        ptr = lambda k: k if k is None or isinstance(k, int) else P(o[k])
        return lib.dfe_temporal_step_f32(ctx.handle, P(v), C_, H_, W_, P(w), P(flow), P(key), *reg, floats(gain), floats(bias), decay, P(m), P(wm), tol, wmax,
                                         ptr(out), ptr(wout), ptr(flag), ptr(prior), ptr(wprior), ptr(src))

    regions = [(0, 0, 0, 8), (0, 0, 6, 0), (-1, 0, 6, 8), (0, -1, 6, 8), (1, 0, 6, 8), (0, 1, 6, 8), (0, 0, 7, 8), (0, 0, 6, 9)]
    both = [(E_ARG, dict(C_=0)), (E_ARG, dict(C_=5)), (E_ARG, dict(v=None)), (E_ARG, dict(w=None)), (E_ARG, dict(flow=None)), (E_ARG, dict(out=None)),
            (E_ARG, dict(wout=None)), (E_ARG, dict(decay=0.0)), (E_ARG, dict(decay=-0.5)), (E_ARG, dict(decay=1.25)), (E_ARG, dict(decay=nan)),
            (E_ARG, dict(gain=(1.0, nan))), (E_ARG, dict(gain=(inf, 1.0))), (E_ARG, dict(bias=(0.0, -inf))), (E_ARG, dict(bias=(nan, 0.0))),
            (E_ARG, dict(H_=65536, W_=32768, reg=(0, 0, 1, 1))), (E_SHAPE, dict(H_=0)), (E_SHAPE, dict(W_=-3))] + [(E_SHAPE, dict(reg=r)) for r in regions]
    fusion = [(E_ARG, dict(tol=-1.0)), (E_ARG, dict(tol=nan)), (E_ARG, dict(wmax=inf)), (E_ARG, dict(wmax=nan)), (E_ARG, dict(wmax=5e-7)), (E_ARG, dict(m=None)),
              (E_ARG, dict(wm=None))]
    cases = [("dfe_forward_warp_f32", warp, rc, kw) for rc, kw in both]
    cases += [("dfe_temporal_step_f32", step, rc, kw) for rc, kw in both + fusion]
    cases += [("dfe_temporal_fuse_f32", fuse, rc, kw) for rc, kw in fusion + [(E_ARG, dict(C_=0)), (E_ARG, dict(C_=5)), (E_ARG, dict(z=None)), (E_ARG, dict(wp=None)),
                                                                             (E_ARG, dict(out=None)), (E_ARG, dict(wout=None))] + [(E_SHAPE, dict(reg=r)) for r in regions]]
    # overlaps: an output on an input, and two outputs on each other (the joint buffer holds the one and, half a plane in, the other)
    for fn, name in ((warp, "dfe_forward_warp_f32"), (step, "dfe_temporal_step_f32")):
        for kw in (dict(v=None, out="v"), dict(w=None, wout="w"), dict(flow=None, out="flow"), dict(key=None, wout="key"), dict(out="joint", wout="joint+"),
                   dict(out="joint", src="joint+")):
            cases.append((name, fn, E_ARG, dict(kw, overlap=True)))
    for kw in (dict(prior="joint", wprior="joint+"), dict(flag="joint", src="joint+"), dict(m=None, prior="m"), dict(wm=None, flag="wm")):
        cases.append(("dfe_temporal_step_f32", step, E_ARG, dict(kw, overlap=True)))
    inputs = dict(v=v, w=w, flow=flow, key=key, m=m, wm=wm)
    for name, fn, rc, kw in cases:
        o = outputs()
        if kw.pop("overlap", False):                              # an output placed on an input's memory or on the joint buffer
            kw = dict(kw)
            for k, val in list(kw.items()):
                if val is None:
                    del kw[k]
                elif val in inputs:
                    kw[k] = inputs[val].data_ptr() + 4
                elif val == "joint+":
                    kw[k] = o["joint"].data_ptr() + 4 * (n // 2)
        before = {k: t.clone() for k, t in inputs.items()}
        got = fn(o, **kw)
        torch.cuda.synchronize()
        assert got == rc, (name, kw, got, lib.dfe_last_error(ctx.handle))
        assert lib.dfe_last_error(ctx.handle).startswith(name.encode()), (name, kw, lib.dfe_last_error(ctx.handle))
        assert all(untouched(t) for t in o.values()), (name, kw)
        assert all(torch.equal(before[k], inputs[k]) for k in inputs), (name, kw)


# -------------------------------------------------------------------------------------------------------------------------- filter
def test_filter_over_the_scene_equals_the_reference_loop(dfe, cuda):
    ref, f = TemporalFilterRef(SCENE_TOL, SCENE_WMAX, key_channel=0), dfe.TemporalFilter(SCENE_TOL, SCENE_WMAX)
    frames = scene(0)
    for t, (truth, meas, weight, flow) in enumerate(frames):
        want = ref.push(meas, weight, flow)
        got = f.push(T(meas, cuda), T(weight, cuda), T(flow, cuda))
        for g, r, what in zip(got, want, ("state", "weight", "flag")):
            same(g.cpu().numpy(), r, "frame %d %s" % (t, what))
    assert set(np.unique(want[2])) >= {1, 2, 3}
    f.reset()                                                      # starts over: the first frame's flags are 0 / 2 again
    ref.reset()
    truth, meas, weight, flow = frames[0]
    got, want = f.push(T(meas, cuda), T(weight, cuda), T(flow, cuda)), ref.push(meas, weight, flow)
    same(got[2].cpu().numpy(), want[2], "flag after reset")
    assert set(np.unique(want[2])) == {0, 2}
    with pytest.raises(ValueError):                                # a changed shape raises
        f.push(T(meas[:, :40], cuda), T(weight[:40], cuda), T(flow[:, :40], cuda))
    got = f.push(T(frames[1][1], cuda), T(frames[1][2], cuda), T(frames[1][3], cuda))   # and changed nothing
    same(got[0].cpu().numpy(), ref.push(*frames[1][1:])[0], "state after the refused push")


def test_filter_with_rectify_equals_the_composition(dfe, cuda):
    K = np.array([[60.0, 0, 32], [0, 60.0, 24], [0, 0, 1]])
    a = 0.02
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    f = dfe.TemporalFilter(SCENE_TOL, SCENE_WMAX, decay=0.75, gain=(1.0,), bias=(0.125,), key_channel=0)
    frames = [tuple(T(x, cuda) for x in fr[1:]) for fr in scene(1)[:3]]
    region = (2, 3, 40, 56)
    state, weight, flag = f.push(*frames[0], region=region)
    zero = torch.zeros_like(frames[0][0])
    for g, r in zip((state, weight, flag), dfe.temporalFuse(zero, zero[0], frames[0][0], frames[0][1], SCENE_TOL, SCENE_WMAX, region)):
        assert torch.equal(g, r)
    for t in (1, 2):
        prior, wprior, _ = dfe.forwardWarp(state, weight, frames[t - 1][2], state[0], region, (1.0,), (0.125,), 0.75)
        warped, mask = dfe.sfm2.removeEgoMotion(torch.cat((prior, wprior[None])), K, R, inverse=True)
        want = dfe.temporalFuse(warped[:1].contiguous(), warped[1] * mask, frames[t][0], frames[t][1], SCENE_TOL, SCENE_WMAX, region)
        state, weight, flag = f.push(*frames[t], region=region, rectify=(K, R))
        for g, r, what in zip((state, weight, flag), want, ("state", "weight", "flag")):
            assert torch.equal(g, r), "frame %d %s" % (t, what)
        assert (flag == 3).any() and (mask == 0).any()


# ------------------------------------------------------------------------------------------------------------------------- session
def test_session_temporal_keyword(dfe, cuda):
    """three pushes with imu_tx: depth_fused and its weight equal a TemporalFilter driven by hand from the session's own outputs, and what
    the session returned before is bit-identical to a session without temporal="""
    from tests.test_gpu_stream import Config, frames, make_filter

    im0, im1, _, K = frames(cuda)
    cfg = Config(120, 160, 16, method="mean")
    filt = make_filter(dfe, cuda)
    plain = dfe.DepthEstimationAPI(cfg.geometry, filt, K, u8Scale=1.0, **cfg.extra())
    api = dfe.DepthEstimationAPI(cfg.geometry, filt, K, u8Scale=1.0, temporal=dict(tol=0.5, wmax=4.0), **cfg.extra())
    hand = dfe.TemporalFilter(0.5, 4.0)
    Ks = np.array(K, np.float64).reshape(3, 3).copy()
    Ks[0] *= 160.0 / 320.0
    Ks[1] *= 120.0 / 240.0
    for i, im in enumerate((im0, im1, im0)):
        r0, r1 = plain.nextFrameDepth(im, imu_tx=1.0), api.nextFrameDepth(im, imu_tx=1.0)
        assert plain.last["status"] == api.last["status"] == (0 if i == 0 else 1)
        if i == 0:
            assert r0 is None and r1 is None and "depth_fused" not in api.last
            continue
        for a, b in zip(r0, r1):
            assert torch.equal(a, b)
        for k in plain.last:
            a, b = plain.last[k], api.last[k]
            assert torch.equal(a, b) if torch.is_tensor(a) else a == b, k
        assert set(api.last) - set(plain.last) == {"depth_fused", "depth_fused_weight", "depth_fused_flag"}
        assert np.array_equal(api.K_small().numpy(), Ks)
        flow = torch.stack((plain.last["yflow"], plain.last["xflow"]))
        want = hand.push(plain.last["depth"][None], plain.last["depth_conf"], flow, rectify=(Ks, plain.last["R"]))
        assert torch.equal(api.last["depth_fused"], want[0][0]) and torch.equal(api.last["depth_fused_weight"], want[1])
        assert torch.equal(api.last["depth_fused_flag"], want[2])
        print("push %d: flags %s" % (i, torch.unique(want[2], return_counts=True)))
        assert i == 1 or bool(((want[2] == 1) | (want[2] >= 3)).any())   # the second pair's fusion had a prior
    api.reset()
    assert api.temporal.state is None and api.nextFrameDepth(im0, imu_tx=1.0) is None
    api.nextFrameDepth(im1, imu_tx=1.0)
    assert set(torch.unique(api.last["depth_fused_flag"]).tolist()) <= {0.0, 2.0}   # the filter started over with the session
    plain.close()
    api.close()
