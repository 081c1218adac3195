"""The edge-aware semi-global entries on the device (include/dfe.h: dfe_sgm_aggregate_guided_f32, dfe_sgm_plane_pick_guided_f32,
dfe_flow_depth_pair_sgm_guided_*, dfe_census_flow_depth_pair_sgm_guided_*) against the numpy restatement of the
definition (tests/sgm_guided_ref.py) BIT FOR BIT -- the definition fixes every operation, so there is no tolerance.  Every output is
pre-filled with a sentinel.

The guide of the operator tests is made of constant patches, steps larger than sigma and ramps, so that one case has steps with w = 0,
w = 1 and in between; it is not symmetric, so a swap of p and q, or an off-by-one in the plane that opposite directions share, changes
bits.  The windows are the path kernel's forms (1, 2, 5, 9, 18 cells a lane); the planes make diagonal chains start again at the sides and
lines longer than one look-ahead window; the radial label counts are one and two labels a lane, the line counts no multiple of 4."""
import numpy as np
import pytest
import torch

from tests import census_ref as cr
from tests import sgm_guided_ref as gr
from tests import sgm_pick_ref as kr
from tests import sgm_plane_ref as pr

pytestmark = pytest.mark.gpu
DFE_E_ARG, DFE_E_SHAPE, DFE_E_UNSUPPORTED = -1, -2, -5
FILL = -7.0
F = np.float32
WINDOWS = ((1, 1), (1, 9), (3, 3), (8, 8), (5, 13), (9, 9), (17, 17), (33, 33), (8, 137))
PLANES = ((1, 1), (1, 12), (12, 1), (3, 70), (70, 3), (33, 40))
SETS = tuple(1 << r for r in range(8)) + (0x0f, 0xf0, 0x05, 0xff)
OUTS = ("agg", "idx", "flow_y", "flow_x", "best", "second", "unique")
SIGMA = 4.0
P1, P2, P2_EDGE = 0.5, 4.0, 1.25


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _volume(shape, seed, lo=-3.0):
    return np.random.default_rng(seed).uniform(lo, 9, size=shape).astype(F)


def _guide(Cg, H, W, seed):
    """[Cg][H][W]: patches of 2 x 3 pixels at levels 10 apart (steps above sigma: w = 0; inside a patch w = 1), a ramp of 0.9 a column on the
    odd patch rows (in between), a finer ramp in y on channel 1 and noise on channel 2"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    level = rng.integers(0, 3, size=(H // 2 + 1, W // 3 + 1))
    g = np.empty((Cg, H, W), F)
    for c in range(Cg):
        g[c] = 10.0 * np.roll(level, c, 1)[y // 2, x // 3]
    g[0] += np.where((y // 2) % 2 == 1, 0.9 * x, 0.0).astype(F)
    if Cg > 1:
        g[1] += (0.4 * y).astype(F)
    if Cg > 2:
        g[2] += rng.uniform(0, 2, size=(H, W)).astype(F)
    return g


def test_the_guide_has_steps_of_every_kind_and_is_not_symmetric():
    for Cg in (1, 3):
        g = _guide(Cg, 6, 9, 1)
        ys, xs = (a.ravel() for a in np.mgrid[0:6, 1:9])
        pen = gr.penalty(g, ys, xs, ys, xs - 1, SIGMA, P2, P2_EDGE)
        assert (pen == F(P2_EDGE)).any() and ((pen > F(P2_EDGE)) & (pen < F(P2))).any()
        assert (gr.penalty(_guide(1, 6, 9, 1), ys, xs, ys, xs - 1, SIGMA, P2, P2_EDGE) == F(P2)).any()
        assert not np.array_equal(g, g[:, ::-1]) and not np.array_equal(g, g[:, :, ::-1])


# ---- the plane family ----
def pick_call(dfe, cuda, vol, paths, subpixel=0, min_unique=0.0, want=OUTS, guide=None, sigma=SIGMA, P2_edge=P2_EDGE, P=(P1, P2), kernel="sgpk_pick_kernel"):
    """the raw guided call: every output as numpy, the sentinel where it was not given"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, hWin, wWin = vol.shape
    tv = torch.from_numpy(vol).to(cuda)
    tg = None if guide is None else torch.from_numpy(np.ascontiguousarray(guide, F)).to(cuda)
    out = dict(agg=torch.full(vol.shape, FILL, device=cuda), idx=torch.full((H, W), -7, dtype=torch.int64, device=cuda))
    for k in OUTS[2:]:
        out[k] = torch.full((H, W), FILL, device=cuda)
    p = [out[k].data_ptr() if k in want else None for k in OUTS]
    ctx.check(lib.dfe_sgm_plane_pick_guided_f32(ctx.handle, tv.data_ptr(), H, W, hWin, wWin, P[0], P[1], paths, subpixel, min_unique, *p,
                                                None if tg is None else tg.data_ptr(), 0 if tg is None else tg.shape[0], sigma, P2_edge))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == kernel
    assert torch.equal(tv.cpu(), torch.from_numpy(vol)), "the volume is an input"
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sum(single, paths):
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


def _plane_case(dfe, cuda, shape, seed):
    H, W = shape[:2]
    vol = _volume(shape, seed, lo=1.0)
    for Cg in (1, 3):
        g = _guide(Cg, H, W, seed + Cg)
        single = [gr.plane_path(vol, r, P1, P2, g, SIGMA, P2_EDGE) for r in range(8)]
        if H * W > 1 and shape[2] * shape[3] > 1:
            assert not np.array_equal(_bits(_sum(single, 0xff)), _bits(pr.plane_sum(vol, P1, P2, 0xff))), "the guide changes the aggregate"
        for j, paths in enumerate(SETS):
            subpixel, mu = j & 1, (0.0, 0.2)[j >> 1 & 1]
            tag = "%s Cg %d paths 0x%02x subpixel %d" % (shape, Cg, paths, subpixel)
            _check(pick_call(dfe, cuda, vol, paths, subpixel, mu, guide=g), _sum(single, paths), subpixel, mu, tag)


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "%dx%d" % w)
def test_plane_family_every_window_form(dfe, cuda, win):
    _plane_case(dfe, cuda, (6, 9) + win, 10 + win[0] + win[1])


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_plane_family_every_plane(dfe, cuda, plane):
    _plane_case(dfe, cuda, plane + (5, 13), 40 + plane[0])


def test_plane_family_every_subset_of_outputs(dfe, cuda):
    vol = _volume((5, 7, 5, 13), 300, lo=1.0)
    g = _guide(3, 5, 7, 2)
    single = [gr.plane_path(vol, r, P1, P2, g, SIGMA, P2_EDGE) for r in range(8)]
    for m in range(1, 1 << len(OUTS)):
        want = tuple(k for b, k in enumerate(OUTS) if m >> b & 1)
        _check(pick_call(dfe, cuda, vol, 0x0f, 1, 0.2, want, guide=g), _sum(single, 0x0f), 1, 0.2, "outputs %s" % (want,), want)
    for paths in (0x08, 0x10):                   # a single direction, whose L goes straight into agg when agg is given
        for want in (OUTS, ("agg",), ("agg", "unique"), ("second",), ("flow_x", "best"), OUTS[1:]):
            _check(pick_call(dfe, cuda, vol, paths, 1, 0.0, want, guide=g), _sum(single, paths), 1, 0.0, "paths 0x%02x outputs %s" % (paths, want), want)
    # paths = 0 stays the winner-takes-all read: the guide is ignored
    _check(pick_call(dfe, cuda, vol, 0, 1, 0.2, guide=g), vol, 1, 0.2, "paths 0")


def _old_pick(dfe, cuda, vol, paths, subpixel, mu):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, hWin, wWin = vol.shape
    tv = torch.from_numpy(vol).to(cuda)
    out = dict(agg=torch.full(vol.shape, FILL, device=cuda), idx=torch.full((H, W), -7, dtype=torch.int64, device=cuda))
    for k in OUTS[2:]:
        out[k] = torch.full((H, W), FILL, device=cuda)
    ctx.check(lib.dfe_sgm_plane_pick_f32(ctx.handle, tv.data_ptr(), H, W, hWin, wWin, P1, P2, paths, subpixel, mu, *(out[k].data_ptr() for k in OUTS)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, ctx.last_kernel()


def test_plane_family_where_the_guide_says_nothing_the_bits_are_the_existing_entry_s(dfe, cuda):
    for win, seed in (((5, 13), 1), ((17, 17), 2)):
        vol = _volume((6, 9) + win, seed)
        flat = np.full((2, 6, 9), 3.5, F)
        for paths in (0x01, 0x0f, 0xff):
            old, kernel = _old_pick(dfe, cuda, vol, paths, 1, 0.2)
            for kw in (dict(guide=None), dict(guide=_guide(2, 6, 9, 3), sigma=0.0), dict(guide=_guide(2, 6, 9, 3), sigma=float("nan")),
                       dict(guide=_guide(2, 6, 9, 3), sigma=-1.0), dict(guide=flat), dict(guide=flat, P2_edge=P2)):
                got = pick_call(dfe, cuda, vol, paths, 1, 0.2, kernel=kernel, **kw)
                assert all(np.array_equal(_bits(got[k]), _bits(old[k])) for k in OUTS if k != "idx") and np.array_equal(got["idx"], old["idx"]), (win, paths, kw)


def test_plane_family_a_nan_in_the_guide(dfe, cuda):
    vol = _volume((6, 9, 5, 13), 9, lo=1.0)
    g = _guide(3, 6, 9, 4)
    g[1, 2, 4], g[0, 5, 8], g[2, 0, 0] = np.nan, np.inf, -np.inf
    want = gr.plane_sum(vol, P1, P2, 0xff, g, SIGMA, P2_EDGE)
    assert np.isfinite(want).all()
    got = pick_call(dfe, cuda, vol, 0xff, 1, 0.2, guide=g)
    _check(got, want, 1, 0.2, "NaN guide")
    assert np.isfinite(got["agg"]).all()


# ---- the radial family ----
def agg_call(dfe, cuda, vol, paths, ring, guide=None, sigma=SIGMA, P2_edge=P2_EDGE, want=("agg", "flow"), guided=True):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, D = vol.shape
    tv = torch.from_numpy(vol).to(cuda)
    tg = None if guide is None else torch.from_numpy(np.ascontiguousarray(guide, F)).to(cuda)
    agg, flow = torch.full(vol.shape, FILL, device=cuda), torch.full((H, W), FILL, device=cuda)
    head = (ctx.handle, tv.data_ptr(), H, W, D, P1, P2, paths, ring, agg.data_ptr() if "agg" in want else None, flow.data_ptr() if "flow" in want else None)
    if guided:
        ctx.check(lib.dfe_sgm_aggregate_guided_f32(*head, None if tg is None else tg.data_ptr(), 0 if tg is None else tg.shape[0], sigma, P2_edge))
    else:
        ctx.check(lib.dfe_sgm_aggregate_f32(*head))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "sgm_path_kernel"
    return agg.cpu().numpy(), flow.cpu().numpy()


@pytest.mark.parametrize("D", [1, 15, 16, 17, 32])
def test_radial_family_every_plane_ring_and_path_set(dfe, cuda, D):
    for i, (H, W) in enumerate(PLANES):
        vol = _volume((H, W, D), 100 + D + i, lo=1.0)
        Cg = (1, 3)[i & 1]
        g = _guide(Cg, H, W, 7 + i)
        for ring in sorted({0, min(5, W), W}):
            single = [gr.sgm_path(vol, r, P1, P2, ring, g, SIGMA, P2_EDGE) for r in range(8)]
            for j, paths in enumerate(SETS):
                want = (("agg", "flow"), ("flow",), ("agg",))[j % 3]
                agg, flow = agg_call(dfe, cuda, vol, paths, ring, g, want=want)
                ref = _sum(single, paths)
                tag = "%dx%dx%d ring %d paths 0x%02x" % (H, W, D, ring, paths)
                assert np.array_equal(_bits(agg), _bits(ref)) if "agg" in want else (agg == FILL).all(), tag
                assert np.array_equal(flow, np.argmin(ref, -1).astype(F)) if "flow" in want else (flow == FILL).all(), tag


def test_radial_family_the_wrap_pair_has_its_own_penalty(dfe, cuda):
    H, W, D = 5, 9, 17
    vol = _volume((H, W, D), 5, lo=1.0)
    g = np.full((1, H, W), 2.0, F)
    g[0, :, W - 1] = 50.0                      # flat but for the last column: the edges are (W - 2, W - 1) and the wrap pair (W - 1, 0)
    for paths in (0x01, 0x02, 0x10, 0xff):
        on_ring = agg_call(dfe, cuda, vol, paths, W, g)[0]
        assert np.array_equal(_bits(on_ring), _bits(gr.sgm_aggregate(vol, P1, P2, paths, W, g, SIGMA, P2_EDGE)[0]))
        # a guide that is flat but for the wrap pair's penalty gives other bits: column 0's step from column W - 1 read it
        g0 = g.copy()
        g0[0, :, W - 1] = 2.0
        g0[0, :, W - 2] = 50.0                  # the edges are now (W - 3, W - 2) and (W - 2, W - 1): column 0 has none
        other = gr.sgm_aggregate(vol, P1, P2, paths, W, g0, SIGMA, P2_EDGE)[0]
        assert not np.array_equal(_bits(on_ring[:, 0]), _bits(other[:, 0]))
    assert not np.array_equal(_bits(on_ring), _bits(agg_call(dfe, cuda, vol, 0xff, W, guided=False)[0]))


def test_radial_family_where_the_guide_says_nothing_the_bits_are_the_existing_entry_s(dfe, cuda):
    for D in (16, 17):
        vol = _volume((7, 10, D), D)
        flat = np.full((1, 7, 10), -2.0, F)
        for paths, ring in ((0x01, 0), (0x0f, 5), (0xff, 10)):
            old = agg_call(dfe, cuda, vol, paths, ring, guided=False)
            for kw in (dict(guide=None), dict(guide=_guide(3, 7, 10, 1), sigma=0.0), dict(guide=_guide(3, 7, 10, 1), sigma=float("nan")), dict(guide=flat)):
                got = agg_call(dfe, cuda, vol, paths, ring, **kw)
                assert np.array_equal(_bits(got[0]), _bits(old[0])) and np.array_equal(got[1], old[1]), (D, paths, ring, kw)


def test_radial_family_a_nan_in_the_guide(dfe, cuda):
    vol = _volume((6, 9, 17), 9, lo=1.0)
    g = _guide(3, 6, 9, 4)
    g[1, 2, 4], g[0, 5, 8], g[2, 0, 0] = np.nan, np.inf, -np.inf
    for ring in (0, 9):
        want = gr.sgm_aggregate(vol, P1, P2, 0xff, ring, g, SIGMA, P2_EDGE)
        got = agg_call(dfe, cuda, vol, 0xff, ring, g)
        assert np.isfinite(got[0]).all() and np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])


# ---- refusals ----
def test_refusals_come_before_any_launch(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    nan, inf = float("nan"), float("inf")
    H, W = 5, 7
    g = torch.zeros((2, H, W), device=cuda)
    # the radial operator
    vol = torch.zeros((H, W, 8), device=cuda)
    agg, flow = torch.full((H, W, 8), FILL, device=cuda), torch.full((H, W), FILL, device=cuda)

    def rad(P1=1.0, P2=4.0, paths=0x0f, ring=0, D=8, guide=g.data_ptr(), Cg=2, sigma=2.0, pe=2.0, v=vol.data_ptr()):
        return lib.dfe_sgm_aggregate_guided_f32(ctx.handle, v, H, W, D, P1, P2, paths, ring, agg.data_ptr(), flow.data_ptr(), guide, Cg, sigma, pe)

    # the plane operator
    pvol = torch.zeros((H, W, 3, 4), device=cuda)
    pagg = torch.full((H, W, 3, 4), FILL, device=cuda)
    idx = torch.full((H, W), -7, dtype=torch.int64, device=cuda)
    planes = [torch.full((H, W), FILL, device=cuda) for _ in range(5)]

    def pln(P1=1.0, P2=4.0, paths=0x0f, mu=0.2, guide=g.data_ptr(), Cg=2, sigma=2.0, pe=2.0, v=pvol.data_ptr(), wh=3, ww=4):
        return lib.dfe_sgm_plane_pick_guided_f32(ctx.handle, v, H, W, wh, ww, P1, P2, paths, 1, mu, pagg.data_ptr(), idx.data_ptr(), *(t.data_ptr() for t in planes),
                                                 guide, Cg, sigma, pe)

    for op, name in ((rad, "dfe_sgm_aggregate_guided_f32"), (pln, "dfe_sgm_plane_pick_guided_f32")):
        for bad in (dict(pe=0.5), dict(pe=4.5), dict(pe=nan), dict(pe=inf), dict(Cg=0), dict(Cg=-1), dict(P1=-1.0), dict(P1=5.0), dict(P2=inf), dict(paths=256),
                    dict(v=None), dict(pe=0.5, guide=None), dict(pe=0.5, sigma=0.0)):
            assert op(**bad) == DFE_E_ARG, (name, bad)
            assert name in ctx.last_error(), ctx.last_error()
    assert rad(paths=0) == DFE_E_ARG and rad(ring=W + 1) == DFE_E_ARG and rad(D=33) == DFE_E_UNSUPPORTED
    assert pln(mu=1.5) == DFE_E_ARG and pln(wh=33, ww=34) == DFE_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (agg == FILL).all() and (flow == FILL).all() and (pagg == FILL).all() and (idx == -7).all() and all((t == FILL).all() for t in planes)
    assert rad() == 0 and pln() == 0 and pln(paths=0, guide=None, Cg=0) == 0 and rad(guide=None, Cg=0) == 0 and rad(pe=1.0) == 0 and pln(pe=4.0) == 0
    torch.cuda.synchronize()
    # the one calls
    f = torch.zeros((3, 40, 60), device=cuda)
    b = torch.zeros((3, 40, 60), dtype=torch.uint8, device=cuda)
    out = torch.full((6, 40, 60), FILL, device=cuda)

    def ssd(u8, P1=1.0, P2=4.0, paths=0x0f, mu=0.2, sigma=2.0, pe=2.0, C=3):
        tail = (P1, P2, paths, 1, mu, sigma, pe, out.data_ptr(), out[2].data_ptr(), None, None)
        if u8:
            return lib.dfe_flow_depth_pair_sgm_guided_u8(ctx.handle, b.data_ptr(), b.data_ptr(), C, 40, 60, 7, 9, 9, 30.0, 20.0, 1.0, *tail)
        return lib.dfe_flow_depth_pair_sgm_guided_f32(ctx.handle, f.data_ptr(), f.data_ptr(), C, 40, 60, 7, 9, 9, 30.0, 20.0, *tail)

    def cen(u8, P1=1.0, P2=4.0, paths=0x0f, mu=0.2, sigma=2.0, pe=2.0, C=3):
        tail = (P1, P2, paths, 1, mu, sigma, pe, out.data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None, None)
        if u8:
            return lib.dfe_census_flow_depth_pair_sgm_guided_u8(ctx.handle, b.data_ptr(), b.data_ptr(), C, 40, 60, 7, 9, 9, 3, 30.0, 20.0, 1.0, *tail)
        return lib.dfe_census_flow_depth_pair_sgm_guided_f32(ctx.handle, f.data_ptr(), f.data_ptr(), C, 40, 60, 7, 9, 9, 3, 30.0, 20.0, *tail)

    for fn, stem in ((ssd, "dfe_flow_depth_pair_sgm_guided_"), (cen, "dfe_census_flow_depth_pair_sgm_guided_")):
        for u8 in (False, True):
            for bad in (dict(pe=0.5), dict(pe=4.5), dict(pe=nan), dict(paths=0), dict(P1=5.0), dict(mu=1.5), dict(pe=0.5, sigma=0.0)):
                assert fn(u8, **bad) == DFE_E_ARG, (stem, u8, bad)
                assert stem + ("u8" if u8 else "f32") in ctx.last_error(), ctx.last_error()
    torch.cuda.synchronize()
    assert (out == FILL).all(), "a refused call writes nothing"
    assert all(fn(u8) == 0 for fn in (ssd, cen) for u8 in (False, True))
    torch.cuda.synchronize()


# ---- the one calls ----
def _pair(C, seed):
    """two uint8 frames [C][40][60]: smooth texture with a bright block (edges for the guide), moved by (1, -1), noisy"""
    rng = np.random.RandomState(seed)
    t = rng.uniform(size=(C, 44, 64))
    for _ in range(3):
        t = (t + np.roll(t, 1, 1) + np.roll(t, -1, 1) + np.roll(t, 1, 2) + np.roll(t, -1, 2)) / 5.0
    t = (t - t.min()) / (t.max() - t.min()) * 120.0
    t[:, 14:26, 20:27] += 110.0
    f0 = t[:, 2:42, 2:62] + rng.normal(0, 2, size=(C, 40, 60))
    f1 = t[:, 1:41, 3:63] + rng.normal(0, 2, size=(C, 40, 60))
    to_u8 = lambda f: np.clip(np.floor(f), 0, 255).astype(np.uint8)
    return to_u8(f0), to_u8(f1)


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


# name: (C, hWin, wWin, paths, subpixel, min_unique)
ONE_CALLS = {"1ch-9x9-8paths": (1, 9, 9, 0xff, 1, 0.2), "3ch-5x13-4paths": (3, 5, 13, 0x0f, 0, 0.0)}


@pytest.mark.parametrize("dtype", ["f32", "u8", "u8-half"])
@pytest.mark.parametrize("name", list(ONE_CALLS))
def test_ssd_one_call_equals_the_staged_calls_the_definition_and_the_keywords(dfe, cuda, name, dtype):
    C, hWin, wWin, paths, subpixel, mu = ONE_CALLS[name]
    k, p1, p2, pe = 7, 8000.0, 200000.0, (None, 20000.0)[C > 1]
    n0, n1 = _pair(C, 3 + C)
    H, W = n0.shape[1:]
    scale = 0.5 if dtype in ("f32", "u8-half") else 1.0
    sigma = 30.0 * scale
    p1, p2, pe = p1 * scale * scale, p2 * scale * scale, None if pe is None else pe * scale * scale
    b0, b1 = torch.from_numpy(n0).to(cuda), torch.from_numpy(n1).to(cuda)
    f0, f1 = b0.float() * scale, b1.float() * scale
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    flow = torch.full((2, H, W), FILL, device=cuda)
    scores, depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(3))
    cx, cy = W / 2 - 3.5, H / 2 + 1.25
    tail = (p1, p2, paths, subpixel, mu, sigma, p1 if pe is None else pe, flow.data_ptr(), scores.data_ptr(), depth.data_ptr(), conf.data_ptr())
    if dtype == "f32":
        ctx.check(lib.dfe_flow_depth_pair_sgm_guided_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, cx, cy, *tail))
    else:
        ctx.check(lib.dfe_flow_depth_pair_sgm_guided_u8(ctx.handle, b0.data_ptr(), b1.data_ptr(), C, H, W, k, hWin, wWin, cx, cy, scale, *tail))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "sgpk_pick_kernel"
    # the staged public calls: the volume, the guided pick on frame 0's region, then the paste
    Ho, Wo = H - k + 1 - hWin + 1, W - k + 1 - wWin + 1
    pt, pl = (H - Ho) // 2, (W - Wo) // 2
    vol = torch.empty((Ho, Wo, hWin, wWin), device=cuda)
    ctx.check(lib.dfe_ssd_cost_volume_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, k, hWin, wWin, vol.data_ptr()))
    guide = f0[:, pt:pt + Ho, pl:pl + Wo]
    r = dfe.semiGlobalPick(vol, p1, p2, paths=paths, subpixel=bool(subpixel), min_unique=mu, guide=guide, sigma=sigma, P2_edge=pe)
    eflow = torch.stack([_paste(r["flow_y"], H, W, pt, pl), _paste(r["flow_x"], H, W, pt, pl)])
    assert torch.equal(flow.view(torch.int32), eflow.view(torch.int32))
    assert torch.equal(scores.view(torch.int32), _paste(r["unique"], H, W, pt, pl).view(torch.int32))
    # ... and the definition
    cost = kr.ssd_volume(n0, n1, k, hWin, wWin, scale)
    assert np.array_equal(_bits(vol.cpu().numpy()), _bits(cost))
    ng = (n0.astype(F) * F(scale))[:, pt:pt + Ho, pl:pl + Wo]
    ref = gr.plane_pick(cost, p1, p2, paths, bool(subpixel), mu, ng, sigma, p1 if pe is None else pe)
    plain = kr.plane_pick(cost, p1, p2, paths, bool(subpixel), mu)
    assert not np.array_equal(_bits(ref["agg"]), _bits(plain["agg"])), "the guide changes the aggregate"
    assert np.array_equal(_bits(flow[0].cpu().numpy()), _bits(cr.paste(ref["flow_y"], H, W, pt, pl)))
    assert np.array_equal(_bits(flow[1].cpu().numpy()), _bits(cr.paste(ref["flow_x"], H, W, pt, pl)))
    assert np.array_equal(_bits(scores.cpu().numpy()), _bits(cr.paste(ref["unique"], H, W, pt, pl)))
    ed, ec = _depth(dfe, flow, cx, cy)
    assert torch.equal(depth.view(torch.int32), ed.view(torch.int32)) and torch.equal(conf, ec)
    # the keywords
    sgm = dict(P1=p1, P2=p2, paths=paths, min_unique=mu, sigma=sigma)
    if pe is not None:
        sgm["P2_edge"] = pe
    res = dfe.flowDepthPair(f0 if dtype == "f32" else b0, f1 if dtype == "f32" else b1, k, hWin, wWin, (cx, cy), subpixel=bool(subpixel), scale=scale, sgm=sgm)
    assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], scores) and torch.equal(res["depth"], depth) and torch.equal(res["depth_conf"], conf)
    # sigma = 0 in the dict: the guided entry, the unguided bits
    sgm0 = dict(P1=p1, P2=p2, paths=paths, min_unique=mu)
    a = dfe.flowDepthPair(f0 if dtype == "f32" else b0, f1 if dtype == "f32" else b1, k, hWin, wWin, (cx, cy), subpixel=bool(subpixel), scale=scale, sgm=sgm0)
    z = dfe.flowDepthPair(f0 if dtype == "f32" else b0, f1 if dtype == "f32" else b1, k, hWin, wWin, (cx, cy), subpixel=bool(subpixel), scale=scale,
                          sgm=dict(sgm0, sigma=0.0))
    assert all(torch.equal(a[key].view(torch.int32), z[key].view(torch.int32)) for key in a)


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("name", list(ONE_CALLS))
def test_census_one_call_equals_the_staged_calls_the_definition_and_the_keywords(dfe, cuda, name, dtype):
    C, hWin, wWin, paths, subpixel, mu = ONE_CALLS[name]
    k, agg, p1, p2, pe, scale = 7, (3, 1)[C > 1], 144.0, 864.0, (None, 300.0)[C > 1], 0.25
    n0, n1 = _pair(C, 5 + C)
    H, W = n0.shape[1:]
    f0, f1 = torch.from_numpy(n0).to(cuda), torch.from_numpy(n1).to(cuda)
    if dtype == "f32":
        f0, f1 = f0.float() * scale, f1.float() * scale
    sigma = 30.0 * scale                          # (float(byte) * scale for the byte entry: the same guide values either way)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    cx, cy = W / 2 - 3.5, H / 2 + 1.25
    vol = dfe.censusCostVolume(dfe.censusTransform(f0, k), dfe.censusTransform(f1, k), hWin, wWin, agg)
    cost = cr.cost_volume(cr.signature(n0, k, k), cr.signature(n1, k, k), hWin, wWin, agg).astype(F)
    assert np.array_equal(vol.cpu().numpy(), cost)
    pt, pl, Ha, Wa = cr.region(H, W, k, k, hWin, wWin, agg)
    ng = (n0.astype(F) * F(scale))[:, pt:pt + Ha, pl:pl + Wa]
    guide = torch.from_numpy(np.ascontiguousarray(ng)).to(cuda)
    flow = torch.full((2, H, W), FILL, device=cuda)
    match, unique, depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(4))
    head = (ctx.handle, f0.data_ptr(), f1.data_ptr(), C, H, W, k, hWin, wWin, agg, cx, cy)
    tail = (p1, p2, paths, subpixel, mu, sigma, p1 if pe is None else pe, flow.data_ptr(), match.data_ptr(), unique.data_ptr(), depth.data_ptr(), conf.data_ptr())
    if dtype == "u8":
        ctx.check(lib.dfe_census_flow_depth_pair_sgm_guided_u8(*head, scale, *tail))
    else:
        ctx.check(lib.dfe_census_flow_depth_pair_sgm_guided_f32(*head, *tail))
    torch.cuda.synchronize()
    assert ctx.last_kernel() == "sgpk_pick_kernel"
    # the staged public calls plus the paste
    r = dfe.semiGlobalPick(vol, p1, p2, paths=paths, subpixel=bool(subpixel), min_unique=mu, guide=guide, sigma=sigma, P2_edge=pe)
    raw = vol.view(Ha, Wa, -1).gather(2, (r["idx"] - 1).unsqueeze(-1)).squeeze(-1)
    score = 1.0 - raw / torch.tensor(float((k * k - 1) * C * agg * agg), device=cuda)
    eflow = torch.stack([_paste(r["flow_y"], H, W, pt, pl), _paste(r["flow_x"], H, W, pt, pl)])
    assert torch.equal(flow.view(torch.int32), eflow.view(torch.int32))
    assert torch.equal(match.view(torch.int32), _paste(score, H, W, pt, pl).view(torch.int32))
    assert torch.equal(unique.view(torch.int32), _paste(r["unique"], H, W, pt, pl).view(torch.int32))
    # the definition
    ref = gr.plane_pick(cost, p1, p2, paths, bool(subpixel), mu, ng, sigma, p1 if pe is None else pe)
    assert not np.array_equal(_bits(ref["agg"]), _bits(pr.plane_sum(cost, p1, p2, paths))), "the guide changes the aggregate"
    for got, key in ((flow[0], "flow_y"), (flow[1], "flow_x"), (unique, "unique")):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(cr.paste(ref[key], H, W, pt, pl))), key
    rmatch = cr.match_score(pr.raw_at(cost, ref["idx"]), k * k - 1, C, agg)
    assert np.array_equal(_bits(match.cpu().numpy()), _bits(cr.paste(rmatch, H, W, pt, pl)))
    ed, ec = _depth(dfe, flow, cx, cy)
    assert torch.equal(depth.view(torch.int32), ed.view(torch.int32)) and torch.equal(conf, ec)
    # the keywords, with consistency=: the backward direction is guided by ITS first frame
    sgm = dict(P1=p1, P2=p2, paths=paths, min_unique=mu, sigma=sigma)
    if pe is not None:
        sgm["P2_edge"] = pe
    res = dfe.censusFlowDepthPair(f0, f1, k, hWin, wWin, (cx, cy), agg=agg, scale=scale, subpixel=bool(subpixel), sgm=sgm, consistency=1.0)
    assert torch.equal(res["flow"], flow) and torch.equal(res["scores"], match) and torch.equal(res["unique"], unique) and torch.equal(res["depth"], depth)
    bvol = dfe.censusCostVolume(dfe.censusTransform(f1, k), dfe.censusTransform(f0, k), hWin, wWin, agg)
    bg = (n1.astype(F) * F(scale))[:, pt:pt + Ha, pl:pl + Wa]
    bref = gr.plane_pick(bvol.cpu().numpy(), p1, p2, paths, bool(subpixel), mu, bg, sigma, p1 if pe is None else pe)
    assert np.array_equal(_bits(res["flow_bw"][0].cpu().numpy()), _bits(cr.paste(bref["flow_y"], H, W, pt, pl)))
    assert np.array_equal(_bits(res["flow_bw"][1].cpu().numpy()), _bits(cr.paste(bref["flow_x"], H, W, pt, pl)))
    mask, err = dfe.flowConsistency(res["flow"], res["flow_bw"], 1.0, (pt, pl, Ha, Wa))
    assert torch.equal(res["consistent"], mask) and torch.equal(res["consistency_err"].view(torch.int32), err.view(torch.int32))


def test_python_keywords_of_the_operators_equal_the_raw_calls(dfe, cuda):
    vol = _volume((12, 20, 5, 13), 5, lo=1.0)
    g = _guide(3, 12, 20, 6)
    tv, tg = torch.from_numpy(vol).to(cuda), torch.from_numpy(g).to(cuda)
    for paths, subpixel, mu, pe in ((0x0f, True, 0.2, None), (0xff, False, 0.0, 2.0), (0x40, True, 1.0, P2)):
        raw = pick_call(dfe, cuda, vol, paths, int(subpixel), mu, guide=g, P2_edge=P1 if pe is None else pe)
        res = dfe.semiGlobalPick(tv, P1, P2, paths=paths, subpixel=subpixel, min_unique=mu, want_volume=True, guide=tg, sigma=SIGMA, P2_edge=pe)
        assert np.array_equal(_bits(res["aggregate"].cpu().numpy()), _bits(raw["agg"])) and np.array_equal(res["idx"].cpu().numpy(), raw["idx"])
        for k in OUTS[2:]:
            assert np.array_equal(_bits(res[k].cpu().numpy()), _bits(raw[k])), k
        if not subpixel:
            ap = dfe.semiGlobalAggregatePlane(tv, P1, P2, paths=paths, guide=tg, sigma=SIGMA, P2_edge=pe)
            assert sorted(ap) == ["aggregate", "flow_x", "flow_y", "idx"]
            assert all(np.array_equal(_bits(ap[a].cpu().numpy()), _bits(raw[b])) for a, b in (("aggregate", "agg"), ("flow_y", "flow_y"), ("flow_x", "flow_x")))
            assert np.array_equal(ap["idx"].cpu().numpy(), raw["idx"])
    rvol = _volume((12, 20, 17), 6, lo=1.0)
    flow, agg = dfe.semiGlobalAggregate(torch.from_numpy(rvol).to(cuda), P1, P2, paths=0xff, ring=20, guide=tg, sigma=SIGMA, P2_edge=P2_EDGE)
    raw = agg_call(dfe, cuda, rvol, 0xff, 20, g)
    assert np.array_equal(_bits(agg.cpu().numpy()), _bits(raw[0])) and np.array_equal(flow.cpu().numpy(), raw[1])
    flow2, none = dfe.semiGlobalAggregate(torch.from_numpy(rvol).to(cuda), P1, P2, paths=0xff, ring=20, want_volume=False, guide=tg, sigma=SIGMA)
    assert none is None and np.array_equal(flow2.cpu().numpy(), gr.sgm_aggregate(rvol, P1, P2, 0xff, 20, g, SIGMA, P1)[1])


# ---- the bar scene of the quality table: the device has the reference's bits, so its figures carry over ----
def test_bar_scene_through_the_ssd_one_call(dfe, cuda):
    s = gr.BAR
    seed, k, win = s["seeds"][0], s["k"], s["win"]
    n0, n1, _ = gr.bar_scene(seed)
    vol, guide, on_bar, far = gr.bar_case(seed, k)
    pt, pl, Ho, Wo = gr.bar_region(k)
    f0, f1 = torch.from_numpy(n0).to(cuda), torch.from_numpy(n1).to(cuda)
    for paths in (0x0f, 0xff):
        res = dfe.flowDepthPair(f0, f1, k, win, win, (48.0, 32.0), sgm=dict(P1=s["P1"], P2=s["P2"], paths=paths, sigma=s["sigma"]))
        ref = gr.plane_pick(vol, s["P1"], s["P2"], paths, False, 0.0, guide, s["sigma"], s["P1"])
        inner = res["flow"][:, pt:pt + Ho, pl:pl + Wo].cpu().numpy()
        assert np.array_equal(_bits(inner[0]), _bits(ref["flow_y"])) and np.array_equal(_bits(inner[1]), _bits(ref["flow_x"]))
        assert np.array_equal(_bits(res["scores"][pt:pt + Ho, pl:pl + Wo].cpu().numpy()), _bits(ref["unique"]))
        wrong = (inner[0] != s["bar_move"][0]) | (inner[1] != s["bar_move"][1])
        assert float(wrong[on_bar].mean()) == gr.bar_shares(seed, paths, "adaptive", k)[0]      # (follows from the bits)
