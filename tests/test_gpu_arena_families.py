"""The context's scratch under every entry added since tests/test_gpu_arena.py: the contiguous arena, the plain arena and the side buffer
only ever grow and nothing clears them between calls, so a launcher that reads a cell it did not write, holds a carved pointer across a
growth or lays integers over another family's floats is right on a fresh allocation and wrong afterwards.  Every case here calls the raw C
entry on contexts of its own (tests/arena_run.py), into outputs pre-filled with a sentinel:

    grow_and_reuse   new context -> A -> B (every block grows; the old one is freed, a contiguous one goes idle in the process's pool) -> A
                     (B's contents underneath)
    poisoned         both arenas first filled with 1e30 .. 1e33 by two ordinary calls, then A and B inside those bytes (the cases that carve
                     an arena; the driver asserts through capfd that neither call grew one)
    round robin      one context runs every case at A in registry order and back again: one family's uint64 and double layouts land on
                     another's floats, with the int8 verdict ring and the cached coefficient plane in between

and every result must equal, bit for bit, what a context of its own gives for that case alone (its contiguous arena is a block of the
pool with an earlier context's bytes in it, tests/arena_run.py).  Correctness against the definitions stays with
the families' own suites.  A is the smallest frame at which the geometry is valid and more than one block runs, B is larger in both
directions and no multiple of A; the frames are seeded and frame 1 is a rolled copy of frame 0, so that the flow is not trivial."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import tracker_ref64 as tr
from tests.arena_run import SENTINEL, conv_layer, filled, float_pair, fresh, grow_and_reuse, new_context, poisoned, same, u8_pair

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "make A B options arena")
REGISTRY = {}        # name -> Case; make(dfe, cuda) -> run(ctx, case)
_runs, _alone = {}, {}   # per module: the run closures and the fresh-context results, name -> run / name -> {case: outputs}


def register(name, A, B, options=None, arena=True):
    """arena: the entry carves one of the two arenas, so the poisoned sequence applies (the side buffer alone: grow_and_reuse only)"""
    def deco(make):
        assert name not in REGISTRY
        REGISTRY[name] = Case(make, A, B, options, arena)
        return make
    return deco


def row(prefix):
    return [n for n in REGISTRY if n.startswith(prefix + "/")]


def run_of(dfe, cuda, name):
    if name not in _runs:
        _runs[name] = REGISTRY[name].make(dfe, cuda)
    return _runs[name]


def check(dfe, cuda, capfd, name):
    c, run, alone = REGISTRY[name], run_of(dfe, cuda, name), _alone.setdefault(name, {})
    grow_and_reuse(run, c.A, c.B, options=c.options, alone=alone)
    if c.arena:
        poisoned(run, c.A, c.B, options=c.options, capfd=capfd, alone=alone)


def pair_outputs(cuda, H, W, extra=0):
    """flow [2][H][W] and 3 + extra planes [H][W], as every pair entry writes them"""
    return [filled(cuda, 2, H, W)] + [filled(cuda, H, W) for _ in range(3 + extra)]


def ptrs(ts):
    return tuple(t.data_ptr() for t in ts)


def frames_of(cuda, dtype, H, W, seed):
    if dtype == "u8":
        return tuple(t.to(cuda) for t in u8_pair(H, W, seed))
    return float_pair(cuda, H, W, seed)


SMALL, LARGE = (40, 56), (57, 91)       # the census and semi-global one calls: 3 x H x W, k = 7, a 9 x 9 window
K7, WIN9 = 7, 9


# ------------------------------------------------------------------ census, single scale (census.hip:361, census_subpixel.hip:185)
def census_pair(entry, dtype):
    def make(dfe, cuda):
        fn = getattr(dfe.lib(), "%s_%s" % (entry, dtype))

        def run(ctx, case):
            H, W = case
            a, b = frames_of(cuda, dtype, H, W, 21)
            o = pair_outputs(cuda, H, W)
            scale = (1.0,) if dtype == "u8" else ()
            ctx.check(fn(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, K7, WIN9, WIN9, 1, W / 2.0, H / 2.0, *scale, *ptrs(o)))
            return o
        return run
    return make


for _dt in ("f32", "u8"):
    register("census/" + _dt, SMALL, LARGE)(census_pair("dfe_census_flow_depth_pair", _dt))
    register("census_subpixel/" + _dt, SMALL, LARGE)(census_pair("dfe_census_flow_depth_pair_subpixel", _dt))


@pytest.mark.parametrize("name", row("census"))
def test_census_single_scale(dfe, cuda, capfd, name):
    """dfe_census_flow_depth_pair_f32 / _u8: two uint64 signature planes in the arena, read k - 1 cells past the region they serve."""
    check(dfe, cuda, capfd, name)


@pytest.mark.parametrize("name", row("census_subpixel"))
def test_census_subpixel(dfe, cuda, capfd, name):
    """dfe_census_flow_depth_pair_subpixel_f32 / _u8: the signatures and the class map behind them, re-read by the vee fit."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ census one calls through the label plane (sgm_pick.hip:161)
def census_sgm(pick, dtype):
    def make(dfe, cuda):
        fn = getattr(dfe.lib(), "dfe_census_flow_depth_pair_%s_%s" % ("sgm2" if pick else "sgm", dtype))

        def run(ctx, case):
            H, W = case
            a, b = frames_of(cuda, dtype, H, W, 23)
            o = pair_outputs(cuda, H, W, extra=1 if pick else 0)          # (sgm2: unique behind match)
            scale = (1.0,) if dtype == "u8" else ()
            mid = (4.0, 32.0, 0xff) + ((1, 0.05) if pick else ())
            ctx.check(fn(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, K7, WIN9, WIN9, 1, W / 2.0, H / 2.0, *scale, *mid, *ptrs(o)))
            return o
        return run
    return make


for _dt in ("f32", "u8"):
    register("census_sgm/sgm_" + _dt, SMALL, LARGE)(census_sgm(False, _dt))
    register("census_sgm/sgm2_" + _dt, SMALL, LARGE)(census_sgm(True, _dt))


@pytest.mark.parametrize("name", row("census_sgm"))
def test_census_sgm(dfe, cuda, capfd, name):
    """dfe_census_flow_depth_pair_sgm_f32 / _u8 and _sgm2_: signatures, the volume and 8 direction planes in one carve."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ census in the polar matcher (census_radial.hip:336)
RADIAL_FRAME = (180, 320)
RADIAL_A, RADIAL_B = (96, 100), (120, 136)      # the polar sizes of the two smallest parameter blocks of test_gpu_arena.py::test_radial


def census_radial(sgm):
    def make(dfe, cuda):
        from depth_estimation_amd._lib import CensusRadialParams

        lib = dfe.lib()
        a, b = float_pair(cuda, *RADIAL_FRAME, seed=19)

        def run(ctx, case):
            hIn, wIn = case
            hWin, k, agg = 15, 7, 3
            hm = hIn - (k - 1) - (hWin - 1) - (agg - 1)
            hOut, wOut = int(RADIAL_FRAME[0] * (hm / hIn)), int(RADIAL_FRAME[1] * (hm / hIn))
            prm = CensusRadialParams(3, RADIAL_FRAME[0], RADIAL_FRAME[1], hIn, wIn, hWin, k, k, agg, 1.0, 0.65, 0)
            o = [filled(cuda, hm, wIn), filled(cuda, hm, wIn)] + [filled(cuda, hOut, wOut) for _ in range(3)]
            mid = (4.0, 32.0, 0x0f, hWin, 1) if sgm else (0.0, 0.0, 0, 0, 0)
            ctx.check(lib.dfe_census_radial_flow_depth_pair_f32(ctx.handle, C.byref(prm), a.data_ptr(), b.data_ptr(), 171.0, 83.0, *mid, None, None, *ptrs(o)))
            return o
        return run
    return make


register("census_radial/first minimum", RADIAL_A, RADIAL_B)(census_radial(False))
register("census_radial/sgm+subpixel", RADIAL_A, RADIAL_B)(census_radial(True))


@pytest.mark.parametrize("name", row("census_radial"))
def test_census_radial(dfe, cuda, capfd, name):
    """dfe_census_radial_flow_depth_pair_f32: polar frames, double tables, float4 frames and uint64 signatures in one carve; with the
    aggregation its volume, aggregate and direction planes behind them."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ pyramids (census_pyramid.hip:321, multiscale.hip:1577 / 1623 / 1643)
PYR_A, PYR_B = (32, 48), (64, 96)               # ratios (1, 2), 8 x 8 windows: test_gpu_arena.py::test_multiscale's


def census_pyramid(form, dtype="f32"):
    def make(dfe, cuda):
        from depth_estimation_amd._lib import ratios_array

        lib = dfe.lib()
        rr, n = ratios_array([1, 2])
        agg, beta = 3, 0.25 / (3 * 9)

        def run(ctx, case):
            H, W = case
            a, b = frames_of(cuda, dtype, H, W, 17)
            flow, idx = filled(cuda, 2, H, W), filled(cuda, H, W, dtype=torch.int64)
            head = (ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, K7, 8, 8, rr, n)
            if form == "ssd refine":                                   # the SSD pyramid's class map, then its refinement alone
                ctx.check(lib.dfe_multiscale_flow_pair_f32(*head, flow.data_ptr(), idx.data_ptr()))
                fine = flow.clone()
                ctx.check(lib.dfe_multiscale_refine_subpixel_f32(*head, idx.data_ptr(), fine.data_ptr()))
                return [flow, idx, fine]
            if form == "refine":                                       # the census pyramid's class map, then its refinement alone
                ctx.check(lib.dfe_multiscale_census_flow_pair_f32(*head, agg, beta, flow.data_ptr(), idx.data_ptr()))
                fine = flow.clone()
                ctx.check(lib.dfe_multiscale_census_refine_subpixel_f32(*head, agg, idx.data_ptr(), fine.data_ptr()))
                return [flow, idx, fine]
            fn = getattr(lib, "dfe_multiscale_census_flow_pair_%s%s" % ("subpixel_" if form == "subpixel" else "", dtype))
            if form == "subpixel" and dtype == "f32":                  # (without idx: the class map stays in the arena)
                ctx.check(fn(*head, agg, beta, flow.data_ptr(), None))
                return [flow]
            ctx.check(fn(*head, agg, beta, flow.data_ptr(), idx.data_ptr()))
            return [flow, idx]
        return run
    return make


for _form in ("classes", "subpixel"):
    for _dt in ("f32", "u8"):
        register("census_pyramid/%s_%s" % (_form, _dt), PYR_A, PYR_B)(census_pyramid(_form, _dt))
register("census_pyramid/refine", PYR_A, PYR_B)(census_pyramid("refine"))
register("census_pyramid/ssd refine", PYR_A, PYR_B)(census_pyramid("ssd refine"))


@pytest.mark.parametrize("name", row("census_pyramid"))
def test_census_pyramid(dfe, cuda, capfd, name):
    """dfe_multiscale_census_flow_pair_f32 / _u8, their _subpixel_ forms and the two refinements alone: every scale's frames, volumes and
    uint64 signature planes in one carve."""
    check(dfe, cuda, capfd, name)


@register("pyramid_filtered/f32", PYR_A, PYR_B)
def _pyramid_filtered(dfe, cuda):
    from depth_estimation_amd._lib import FilterLayer, ratios_array

    lib = dfe.lib()
    rr, n = ratios_array([1, 2])
    (l1, k1), (l2, k2) = conv_layer(cuda, 3, 4, 5, 1, 1), conv_layer(cuda, 4, 10, 5, 0, 2)
    arr = (FilterLayer * 2)(l1, l2)

    def run(ctx, case, keep=(k1, k2)):
        H, W = case
        a, b = float_pair(cuda, H, W, seed=17)
        flow, idx = filled(cuda, 2, H, W), filled(cuda, H, W, dtype=torch.int64)
        ctx.check(lib.dfe_multiscale_flow_pair_filtered_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, 8, 8, rr, n, arr, 2, 1, 0.0, flow.data_ptr(), idx.data_ptr()))
        return [flow, idx]
    return run


@pytest.mark.parametrize("name", row("pyramid_filtered"))
def test_pyramid_filtered(dfe, cuda, capfd, name):
    """dfe_multiscale_flow_pair_filtered_f32 in the plain arena: a shared stack 3 -> 4 (5 x 5, tanh), 4 -> 10 (5 x 5) on both scales."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ the aggregations on a caller's volume (sgm.hip:227, sgm_plane.hip:229, sgm_pick.hip:202)
def random_volume(cuda, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 8.0).to(cuda)


def sgm_volume(entry, one_direction):
    """flow only: the aggregate stays in the arena; one direction with agg given: it goes straight into agg"""
    def make(dfe, cuda):
        lib = dfe.lib()
        paths = 0x04 if one_direction else 0xff

        def run(ctx, case):
            H, W = case
            if entry == "aggregate":
                vol = random_volume(cuda, (H, W, 15), 31)
                agg, flow = filled(cuda, H, W, 15), filled(cuda, H, W)
                ctx.check(lib.dfe_sgm_aggregate_f32(ctx.handle, vol.data_ptr(), H, W, 15, 0.5, 4.0, paths, 0, agg.data_ptr() if one_direction else None, flow.data_ptr()))
                return [flow] + ([agg] if one_direction else [])
            vol = random_volume(cuda, (H, W, WIN9, WIN9), 33)
            agg, idx = filled(cuda, H, W, WIN9, WIN9), filled(cuda, H, W, dtype=torch.int64)
            o = [filled(cuda, H, W) for _ in range(5 if entry == "pick" else 2)]
            aggp = agg.data_ptr() if one_direction else None
            if entry == "plane":
                ctx.check(lib.dfe_sgm_plane_aggregate_f32(ctx.handle, vol.data_ptr(), H, W, WIN9, WIN9, 0.5, 4.0, paths, aggp, idx.data_ptr(), *ptrs(o)))
            else:
                ctx.check(lib.dfe_sgm_plane_pick_f32(ctx.handle, vol.data_ptr(), H, W, WIN9, WIN9, 0.5, 4.0, paths, 1, 0.05, aggp, idx.data_ptr(), *ptrs(o)))
            return [idx] + o + ([agg] if one_direction else [])
        return run
    return make


SGM_A, SGM_B = (26, 42), (43, 77)               # the regions of SMALL and LARGE
for _entry in ("aggregate", "plane", "pick"):
    register("sgm_volume/%s flow only" % _entry, SGM_A, SGM_B)(sgm_volume(_entry, False))
    register("sgm_volume/%s one direction into agg" % _entry, SGM_A, SGM_B)(sgm_volume(_entry, True))


@pytest.mark.parametrize("name", row("sgm_volume"))
def test_sgm_on_a_volume(dfe, cuda, capfd, name):
    """dfe_sgm_aggregate_f32, dfe_sgm_plane_aggregate_f32, dfe_sgm_plane_pick_f32: the direction planes, summed where no agg is given."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ the learned polar path (radial_pipeline.hip:577)
def radial(form):
    def make(dfe, cuda):
        from depth_estimation_amd._lib import RadialParams
        from depth_estimation_amd.radial import _separable_weights

        lib = dfe.lib()
        blocks = {}
        for hIn, wIn, layers in ((96, 100, [[3, 1, 9, 4], [4, 11, 1, 6]]), (120, 136, [[3, 1, 17, 5], "tanh", [5, 17, 1, 10]])):
            networkp = dict(hImg=RADIAL_FRAME[0], wImg=RADIAL_FRAME[1], hInput=hIn, wInput=wIn, hWin=15, layers=layers)
            net = dfe.getTesterNetwork(networkp, device=cuda, generator=torch.Generator().manual_seed(0))
            blocks[(hIn, wIn)] = (networkp, _separable_weights(net, networkp), net)
        a, b = float_pair(cuda, *RADIAL_FRAME, seed=19)

        def run(ctx, case):
            networkp, (w1, b1, w2, b2, th), _ = blocks[case]
            hIn, wIn = case
            hm, hOut, wOut = dfe.radial_out_shape(networkp)
            prm = RadialParams(3, RADIAL_FRAME[0], RADIAL_FRAME[1], hIn, wIn, 15, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), 1.0, 0.65, 0)
            o = [filled(cuda, hm, wIn)] + [filled(cuda, hOut, wOut) for _ in range(3)]
            head = (ctx.handle, C.byref(prm), a.data_ptr(), b.data_ptr(), 171.0, 83.0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr())
            if form == "subpixel":
                ctx.check(lib.dfe_radial_flow_depth_pair_subpixel_f32(*head, None, *ptrs(o)))
            else:
                ctx.check(lib.dfe_radial_flow_depth_pair_sgm_f32(*head, 0.02, 0.2, 0xff, 15, 1 if form == "sgm+subpixel" else 0, None, None, *ptrs(o)))
            return o
        return run
    return make


for _form in ("sgm", "sgm+subpixel", "subpixel"):
    register("radial/" + _form, RADIAL_A, RADIAL_B)(radial(_form))


@pytest.mark.parametrize("name", row("radial"))
def test_radial_sgm_and_subpixel(dfe, cuda, capfd, name):
    """dfe_radial_flow_depth_pair_sgm_f32 and dfe_radial_flow_depth_pair_subpixel_f32 with volume = NULL: the matcher's volume, the
    aggregate and the direction planes behind the feature maps."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ the single-scale SSD step (flow_step.hip:58 / 116 / 243)
STEP_A, STEP_B = (48, 72), (64, 104)            # 33 x 33: the window of the volume-free sweep and of the int8 kernel


def flow_step(entry, dtype, win):
    def make(dfe, cuda):
        fn = getattr(dfe.lib(), "%s_%s" % (entry, dtype))

        def run(ctx, case):
            H, W = case
            a, b = frames_of(cuda, dtype, H, W, 7)
            o = pair_outputs(cuda, H, W)
            scale = (1.0,) if dtype == "u8" else ()
            ctx.check(fn(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, K7, win, win, W / 2.0, H / 2.0, 0.21, *scale, *ptrs(o)))
            return o
        return run
    return make


register("flow_step/f32", STEP_A, STEP_B)(flow_step("dfe_flow_depth_pair", "f32", 33))
register("flow_step/f32 9x9", SMALL, LARGE)(flow_step("dfe_flow_depth_pair", "f32", WIN9))
register("flow_step/subpixel_f32", STEP_A, STEP_B)(flow_step("dfe_flow_depth_pair_subpixel", "f32", 33))
register("flow_step/subpixel_u8", STEP_A, STEP_B)(flow_step("dfe_flow_depth_pair_subpixel", "u8", 33))
register("flow_step/u8 cv_i8=1", STEP_A, STEP_B, options={"cv_i8": 1})(flow_step("dfe_flow_depth_pair", "u8", 33))
register("flow_step/u8 cv_i8=0", STEP_A, STEP_B, options={"cv_i8": 0})(flow_step("dfe_flow_depth_pair", "u8", 33))


@pytest.mark.parametrize("name", row("flow_step"))
def test_flow_step(dfe, cuda, capfd, name):
    """dfe_flow_depth_pair_f32 on float frames (the records and the fallback plane; at 9 x 9 the banded volume), the _subpixel_ entries,
    and the byte step with the int8 kernel forced on and off."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ operators on their own (tracker.hip:447 / 471, postfilters.hip:158,
#                                                                    single_scale.hip:270, version2.hip:159, ssd_cost_volume.hip:2238)
@register("alone/tracker", (120, 160), (240, 320))
def _tracker(dfe, cuda):
    from depth_estimation_amd._lib import TrackerParams

    lib = dfe.lib()
    q = tr.ROUTE
    prm = TrackerParams(q["max_points"], q["quality"], q["min_dist"], q["win"], q["levels"], q["max_iters"], q["eps"], q["min_eig"], 0.0)

    def run(ctx, case):
        H, W = case
        tv = tr.two_view_pair(H, W)
        y0, y1 = (torch.from_numpy(tv[k].copy()).contiguous().to(cuda) for k in ("im0", "im1"))
        resp, n, mp = filled(cuda, H, W), C.c_int(SENTINEL), prm.max_points
        pts, val = filled(cuda, mp, 2), filled(cuda, mp)
        ctx.check(lib.dfe_corner_response_f32(ctx.handle, y0.data_ptr(), H, W, resp.data_ptr()))
        ctx.check(lib.dfe_select_corners_f32(ctx.handle, resp.data_ptr(), H, W, prm.quality, prm.min_dist, mp, pts.data_ptr(), val.data_ptr(), C.byref(n)))
        assert 8 <= n.value <= mp
        pts1, st, err = filled(cuda, mp, 2), filled(cuda, mp, dtype=torch.int32), filled(cuda, mp)
        ctx.check(lib.dfe_track_points_lk_f32(ctx.handle, y0.data_ptr(), y1.data_ptr(), H, W, pts.data_ptr(), n.value, C.byref(prm), pts1.data_ptr(), st.data_ptr(),
                                              err.data_ptr()))
        torch.cuda.synchronize()
        assert int(st[: n.value].sum()) >= 8
        return [pts, val, pts1, st, err, np.array([n.value])]
    return run


def postprocess(method):
    def make(dfe, cuda):
        lib = dfe.lib()

        def run(ctx, case):
            H, W = case
            g = torch.Generator().manual_seed(41)
            flow = ((torch.rand((2, H, W), generator=g) - 0.5) * 6.0).to(cuda)
            mask = (torch.rand((H, W), generator=g) > 0.3).to(torch.float32).to(cuda)
            out = filled(cuda, 2, H, W)
            ctx.check(lib.dfe_postprocess_image_f32(ctx.handle, flow.data_ptr(), mask.data_ptr(), H, W, 5, method, out.data_ptr()))
            return [out]
        return run
    return make


def matcher(form):
    """9 x 9 windows on K = 6 planes: no matcher without a volume takes them, so the arg-min goes through a volume in the arena, and the
    strided call through a contiguous copy of its view"""
    def make(dfe, cuda):
        lib = dfe.lib()
        K, mh, mw = 6, 9, 9

        def run(ctx, case):
            H1, W1 = case
            H2, W2 = H1 + mh - 1, W1 + mw - 1
            g = torch.Generator().manual_seed(43)
            in2 = torch.rand((K, H2, W2), generator=g).to(cuda)
            wide = torch.roll(in2, (1, -2), dims=(1, 2)).contiguous()
            if form == "argmin":
                in1 = wide[:, 4 : 4 + H1, 4 : 4 + W1].contiguous()
                o = [filled(cuda, H1, W1, dtype=torch.int64), filled(cuda, H1, W1), filled(cuda, H1, W1)]
                ctx.check(lib.dfe_spatial_matching_argmin_f32(ctx.handle, in1.data_ptr(), in2.data_ptr(), K, H1, W1, mh, mw, *ptrs(o)))
                return o
            out = filled(cuda, H1, W1, mh, mw)
            view = wide.data_ptr() + 4 * (4 * W2 + 4)                  # the view wide[:, 4:4 + H1, 4:4 + W1]
            ctx.check(lib.dfe_spatial_matching_strided_f32(ctx.handle, view, W2, H2 * W2, in2.data_ptr(), K, H1, W1, mh, mw, out.data_ptr()))
            torch.cuda.synchronize()
            return [out]
        return run
    return make


@register("alone/cost volume f16 5x7 patch", SMALL, LARGE)
def _volume_f16(dfe, cuda):
    lib = dfe.lib()

    def run(ctx, case):
        H, W = case
        a, b = float_pair(cuda, H, W, seed=47)
        Ho, Wo = H - 5 + 1 - WIN9 + 1, W - 7 + 1 - WIN9 + 1
        out = filled(cuda, Ho, Wo, WIN9, WIN9, dtype=torch.float16)
        ctx.check(lib.dfe_ssd_cost_volume_f16(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, 5, 7, WIN9, WIN9, 1.0, out.data_ptr()))
        return [out]
    return run


register("alone/postprocess max", (37, 53), (64, 104))(postprocess(0))
register("alone/postprocess median", (37, 53), (64, 104), arena=False)(postprocess(1))
register("alone/matcher argmin", (33, 45), (50, 71))(matcher("argmin"))
register("alone/matcher strided", (33, 45), (50, 71))(matcher("strided"))


@pytest.mark.parametrize("name", row("alone"))
def test_operators_on_their_own(dfe, cuda, capfd, name):
    """dfe_select_corners_f32 and dfe_track_points_lk_f32 without the ego-motion call around them, dfe_postprocess_image_f32,
    dfe_spatial_matching_argmin_f32 and dfe_spatial_matching_strided_f32 at a window no volume-free matcher takes, and
    dfe_ssd_cost_volume_f16 at a non-square patch (fp32 bands in the arena, converted)."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ the SSD semi-global one call, plain arena (sgm_pick.hip:118)
def ssd_sgm(dtype):
    def make(dfe, cuda):
        fn = getattr(dfe.lib(), "dfe_flow_depth_pair_sgm_" + dtype)

        def run(ctx, case):
            H, W = case
            a, b = frames_of(cuda, dtype, H, W, 29)
            o = pair_outputs(cuda, H, W)
            mid = (1.0, 1e4, 1e5) if dtype == "u8" else (1.0, 8.0)       # (scale, P1, P2): the bytes' costs are 255^2 times the floats'
            ctx.check(fn(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, K7, WIN9, WIN9, W / 2.0, H / 2.0, *mid, 0xff, 1, 0.05, *ptrs(o)))
            return o
        return run
    return make


for _dt in ("f32", "u8"):
    register("ssd_sgm/" + _dt, SMALL, LARGE)(ssd_sgm(_dt))


@pytest.mark.parametrize("name", row("ssd_sgm"))
def test_ssd_sgm(dfe, cuda, capfd, name):
    """dfe_flow_depth_pair_sgm_f32 / _u8: the whole volume and 8 direction planes carved from the plain arena, then the public
    dfe_ssd_cost_volume_f32 called on the carved pointer."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ the side buffer: consistency, fill, temporal (consistency.hip:87, fill.hip:331,
#                                                                    temporal.hip:139, temporal_splat.hip:313)
FIELD_A, FIELD_B = (37, 53), (64, 104)


@register("consistency/fields", FIELD_A, FIELD_B, arena=False)
def _consistency(dfe, cuda):
    lib = dfe.lib()

    def run(ctx, case):
        H, W = case
        g = torch.Generator().manual_seed(53)
        fw = ((torch.rand((2, H, W), generator=g) - 0.5) * 4.0).round()
        bw = (-torch.roll(fw, (1, -1), dims=(1, 2)) + (torch.rand((2, H, W), generator=g) - 0.5)).contiguous()
        fw, bw = fw.to(cuda), bw.to(cuda)
        mask, err = filled(cuda, H, W), filled(cuda, H, W)
        ctx.check(lib.dfe_flow_consistency_f32(ctx.handle, fw.data_ptr(), bw.data_ptr(), H, W, 1, 2, H - 3, W - 5, 1.0, mask.data_ptr(), err.data_ptr()))
        return [mask, err]
    return run


def pair_fb(dtype):
    def make(dfe, cuda):
        fn = getattr(dfe.lib(), "dfe_flow_depth_pair_fb_" + dtype)

        def run(ctx, case):
            H, W = case
            a, b = frames_of(cuda, dtype, H, W, 59)
            o = pair_outputs(cuda, H, W) + [filled(cuda, H, W), filled(cuda, H, W)]          # ... mask, err; flow_bw = NULL: the side buffer
            scale = (1.0,) if dtype == "u8" else ()
            ctx.check(fn(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, K7, WIN9, WIN9, W / 2.0, H / 2.0, 0.21, *scale, 1 if dtype == "f32" else 0, 1.0,
                         1 if dtype == "f32" else 0, *ptrs(o[:4]), None, *ptrs(o[4:])))
            return o
        return run
    return make


for _dt in ("f32", "u8"):
    register("consistency/fb_" + _dt, FIELD_A, FIELD_B)(pair_fb(_dt))


@pytest.mark.parametrize("name", row("consistency"))
def test_consistency(dfe, cuda, capfd, name):
    """dfe_flow_consistency_f32, and dfe_flow_depth_pair_fb_f32 / _u8 without flow_bw: two flow steps in the arena, the backward flow in the
    side buffer between them."""
    check(dfe, cuda, capfd, name)


def sparse_field(Cc, H, W, seed):
    """values [Cc][H][W] in 1 .. 5, a weight plane with a fifth of the pixels holes, a flow of up to 3 pixels that is no integer"""
    g = torch.Generator().manual_seed(seed + 100 * Cc)
    v = torch.rand((Cc, H, W), generator=g) * 4.0 + 1.0
    w = torch.where(torch.rand((H, W), generator=g) > 0.2, torch.rand((H, W), generator=g) * 3.0 + 0.1, torch.zeros(()))
    flow = (torch.rand((2, H, W), generator=g) - 0.5) * 6.0
    return v, w, flow


def fill(apex):
    def make(dfe, cuda):
        lib = dfe.lib()

        def run(ctx, case):
            H, W = case
            v, w, _ = sparse_field(2, H, W, 61)
            w = torch.where(w > 2.0, torch.ones(()), torch.where(w > 1.5, w - 1.5, torch.zeros(())))      # trusted, partly trusted, holes
            v, w = v.to(cuda), w.to(cuda)
            out, got = filled(cuda, 2, H, W), filled(cuda, H, W)
            ctx.check(lib.dfe_fill_holes_f32(ctx.handle, v.data_ptr(), 2, H, W, w.data_ptr(), 1, 2, H - 3, W - 5, 0, out.data_ptr(), got.data_ptr()))
            return [out, got]
        return run
    return make


for _apex in (0, 1):
    register("fill/fill_apex=%d" % _apex, FIELD_A, FIELD_B, options={"fill_apex": _apex}, arena=False)(fill(_apex))


@pytest.mark.parametrize("name", row("fill"))
def test_fill(dfe, cuda, capfd, name):
    """dfe_fill_holes_f32, both forms: the pyramid's levels in the side buffer."""
    check(dfe, cuda, capfd, name)


TEMPORAL_A, TEMPORAL_B = (1, 24, 40), (4, 37, 67)     # (C, H, W): the splat's accumulator count depends on C


def temporal(entry, keyed):
    """entry: warp, step, splat, step_splat; the region lies inside the frame.  Returns the entry's outputs; the z-buffered forms also
    assert that the warp is no trivial one: many sources win a target, and some targets stay empty"""
    def make(dfe, cuda):
        lib = dfe.lib()

        def run(ctx, case):
            Cc, H, W = case
            v, w, flow = (t.to(cuda) for t in sparse_field(Cc, H, W, 67))
            m, wm, _ = (t.to(cuda) for t in sparse_field(Cc, H, W, 71))
            key = v[0].clone() if keyed else None
            y0, x0, Ho, Wo = 2, 3, H - 5, W - 7
            gain = (C.c_float * Cc)(*[1.0 + 0.01 * c for c in range(Cc)])
            head = (ctx.handle, v.data_ptr(), Cc, H, W, w.data_ptr(), flow.data_ptr(), key.data_ptr() if keyed else None, y0, x0, Ho, Wo, gain, None, 0.9)
            planes = lambda: [filled(cuda, Cc, H, W), filled(cuda, H, W)]
            last = filled(cuda, H, W, dtype=torch.int32) if entry in ("warp", "step") else filled(cuda, H, W)       # src, or cover
            if entry == "warp":
                o = planes() + [last]
                ctx.check(lib.dfe_forward_warp_f32(*head, *ptrs(o)))
            elif entry == "splat":
                o = planes() + [last]
                ctx.check(lib.dfe_forward_splat_f32(*head, 0.5, 1024.0, 0.25, *ptrs(o)))
            else:
                o = planes() + [filled(cuda, H, W)] + planes() + [last]                                         # out, wout, flag, prior, wprior, src / cover
                mid = (0.5, 1024.0, 0.25) if entry == "step_splat" else ()
                fn = lib.dfe_temporal_step_splat_f32 if entry == "step_splat" else lib.dfe_temporal_step_f32
                ctx.check(fn(*head, *mid, m.data_ptr(), wm.data_ptr(), 0.5, 8.0, *ptrs(o)))
            torch.cuda.synchronize()
            inside = last[y0 : y0 + Ho, x0 : x0 + Wo]
            if entry in ("warp", "step"):
                won = inside[inside >= 0]
                assert torch.unique(won).numel() > Ho * Wo // 4 and bool((inside == -1).any()), "the warp is trivial: %d sources won" % torch.unique(won).numel()
            else:
                assert int((inside > 0).sum()) > Ho * Wo // 4, "the splat covers next to nothing"
            return o
        return run
    return make


for _entry in ("warp", "step"):
    for _keyed in (True, False):
        register("temporal/%s %s" % (_entry, "key" if _keyed else "no key"), TEMPORAL_A, TEMPORAL_B, arena=False)(temporal(_entry, _keyed))
for _entry in ("splat", "step_splat"):
    for _keyed in (True, False):
        for _lds in (0, 1):
            register("temporal_splat/%s %s splat_lds=%d" % (_entry, "key" if _keyed else "no key", _lds), TEMPORAL_A, TEMPORAL_B, options={"splat_lds": _lds},
                     arena=False)(temporal(_entry, _keyed))


@pytest.mark.parametrize("name", row("temporal"))
def test_temporal_warp(dfe, cuda, capfd, name):
    """dfe_forward_warp_f32 and dfe_temporal_step_f32: the 64-bit z-buffer in the side buffer, cleared to all ones by every call."""
    check(dfe, cuda, capfd, name)


@pytest.mark.parametrize("name", row("temporal_splat"))
def test_temporal_splat(dfe, cuda, capfd, name):
    """dfe_forward_splat_f32 and dfe_temporal_step_splat_f32, with and without a key, both forms of the passes: C + 2 planes of 64-bit
    sums and the front in the side buffer, cleared by every call."""
    check(dfe, cuda, capfd, name)


# ------------------------------------------------------------------ two streams on one context (stream.hip)
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_two_streams_share_one_context(dfe, cuda, dtype):
    """dfe_stream_push_f32 / _u8: streams of geometry 120 x 160 (16 x 16 window, the stand-alone ops) and 240 x 320 (17 x 17, the fused
    matcher) on ONE context, three frames pushed to each in turn.  Every push equals the same push on a stream that is alone on a context of
    its own: what a stream keeps between pushes is its own, and what it leaves in the context's arenas is nothing the other one reads.
    u8: the frames as bytes with scale 1 / 255, converted on the device into the stream's slot, with the tracker's eigenvalue floor and the
    first layer's gain of tests/test_gpu_stream.py::test_stream_u8_push_and_reset."""
    from tests import test_gpu_stream as gs

    class OwnStream(gs.Stream):
        def __init__(self, ctx, cfg, filt, K):
            self.dfe, self.cuda, self.ctx = dfe, cuda, ctx
            self.p, self.keep = dfe.stream.stream_params(cfg.geometry, filt, K, cfg.dist, 3, 240, 320, **cfg.extra())
            self.h = C.c_void_p()
            ctx.check(dfe.lib().dfe_stream_create(ctx.handle, C.byref(self.p), C.byref(self.h)))

    im0, im1, _, K = gs.frames(cuda)
    if dtype == "u8":
        b0, b1 = ((im / np.float32(gs.GAINS[2])).round().clamp(0, 255).to(torch.uint8) for im in (im0, im1))
        video, push_kw = (b0, b1, b0), dict(u8_scale=1.0 / 255.0)
        cfg_kw = dict(sfm=gs.sfm_kw(trackerMinEig=tr.ROUTE["min_eig"] / 255.0 ** 2), gain=255.0 / 128)
    else:
        video, push_kw, cfg_kw = (im0, im1, im0), {}, {}
    configs = {"A": gs.Config(120, 160, 16, **cfg_kw), "B": gs.Config(240, 320, 17, method="mean", **cfg_kw)}
    filt = gs.make_filter(dfe, cuda, configs["A"].gain)

    def same_push(got, want, what):
        assert sorted(got) == sorted(want)
        for k in got:
            assert np.array_equal(got[k], want[k]), "%s: %s differs from the lone stream's" % (what, k)

    alone = {}
    for name, cfg in configs.items():
        ctx = new_context()
        s = OwnStream(ctx, cfg, filt, K)
        try:
            alone[name] = [s.push(f, **push_kw) for f in video]
        finally:
            s.close()
            ctx.close()
        assert [r["status"] for r in alone[name]] == [0, 1, 1] and alone[name][1]["flow"].any()
    ctx = new_context()
    streams = {name: OwnStream(ctx, cfg, filt, K) for name, cfg in configs.items()}
    try:
        for i, f in enumerate(video):
            for name in ("A", "B"):
                same_push(streams[name].push(f, **push_kw), alone[name][i], "stream %s, push %d" % (name, i + 1))
    finally:
        for s in streams.values():
            s.close()
        ctx.close()


# ------------------------------------------------------------------ every family on one context
def test_round_robin_on_one_context(dfe, cuda):
    """One context runs every registered case at its shape A in registry order, then all of them in reverse order; every output equals the
    case's fresh-context result (the ones the tests above computed, or computed here).  The cases' options are set for their call and
    released behind it."""
    names = list(REGISTRY)
    want = {n: fresh(run_of(dfe, cuda, n), REGISTRY[n].A, REGISTRY[n].options, _alone.setdefault(n, {})) for n in names}
    ctx = new_context()
    differ = []
    for turn, n in enumerate(names + names[::-1]):
        opts = REGISTRY[n].options or {}
        for k, v in opts.items():
            ctx.set_option(k, v)
        got = run_of(dfe, cuda, n)(ctx, REGISTRY[n].A)
        torch.cuda.synchronize()
        for k in opts:
            ctx.set_option(k, -1)
        assert len(got) == len(want[n])
        for j, (g, w) in enumerate(zip(got, want[n])):
            if not same(g, w):
                count = int((g != w).sum())
                differ.append("turn %d (%s): output %d differs from a fresh context's in %d elements" % (turn, n, j, count))
    ctx.close()
    assert not differ, "%d outputs differ:\n%s" % (len(differ), "\n".join(differ))
