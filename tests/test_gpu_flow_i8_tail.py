"""The int8 flow sweep finishes its own pixels (ssd_flow_i8.hip: the finalize inside the wave item) and a gated tail launch writes the
frame's border or, behind the float sweep, runs the record finalize.  Every output of dfe_flow_depth_pair_f32 and dfe_ssd_flow_f32,
pre-filled with -7, must equal the float path's (cv_i8 = 0) byte for byte, whole arrays, border included: below one strip, a shifted
last tile column inside and across a strip, odd row counts, launches that mix two-row and one-row items, partial and empty hit lists,
a focus of expansion outside the frame, and the gate followed by a smaller byte pair on the same context."""
import numpy as np
import pytest
import torch

from tests import refpath as rp

K, WIN = 7, 33
PAD = K + WIN - 2


def _pair(Ho, Wo, seed=5):
    H, W = Ho + PAD, Wo + PAD
    f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=seed, max_flow=min(12, max(1, min(H, W) // 8)), integer=True)
    return f0, f1, foe


def _run(ctx, lib, cuda, f0, f1, foe, thr, i8, slots=None):
    """both entry points with cv_i8 = i8 (and i8_slots = slots); returns (outputs, int8 taken by the pair call, by the flow call)"""
    C, H, W = f0.shape
    Ho, Wo = H - PAD, W - PAD
    t0 = torch.from_numpy(np.ascontiguousarray(f0)).to(cuda)
    t1 = torch.from_numpy(np.ascontiguousarray(f1)).to(cuda)
    with ctx.options(cv_i8=i8, i8_slots=-1 if slots is None else slots):
        flow = torch.full((2, H, W), -7.0, device=cuda)
        sc, dd, cc = (torch.full((H, W), -7.0, device=cuda) for _ in range(3))
        ctx.check(lib.dfe_flow_depth_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, WIN, WIN, foe[0], foe[1], thr, flow.data_ptr(),
                                              sc.data_ptr(), dd.data_ptr(), cc.data_ptr()))
        assert ctx.last_kernel() == "ssd_cv_rowimg_kernel+fused_tail+novol"
        took_pair = ctx.flow_last_path_i8()
        idx = torch.full((Ho, Wo), -7, dtype=torch.int64, device=cuda)
        imx = torch.full((Ho, Wo), -7, dtype=torch.int64, device=cuda)
        best, fy, fx, s2 = (torch.full((Ho, Wo), -7.0, device=cuda) for _ in range(4))
        ctx.check(lib.dfe_ssd_flow_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, K, WIN, WIN, thr, idx.data_ptr(), best.data_ptr(),
                                       fy.data_ptr(), fx.data_ptr(), s2.data_ptr(), imx.data_ptr()))
        took_flow = ctx.flow_last_path_i8()
        torch.cuda.synchronize()
    out = dict(flow=flow, scores=sc, depth=dd, conf=cc, idx=idx, best=best, fy=fy, fx=fx, scores2=s2, imaxs=imx)
    return {k: v.cpu().numpy() for k, v in out.items()}, took_pair, took_flow


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _check(dfe, cuda, f0, f1, foe, thr, slots=None, expect_i8=True):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    ref, rp_, rf_ = _run(ctx, lib, cuda, f0, f1, foe, thr, 0)
    assert not rp_ and not rf_
    new, tp, tf = _run(ctx, lib, cuda, f0, f1, foe, thr, 1, slots)
    assert tp == tf == expect_i8, (tp, tf)
    _same(new, ref)
    return new


def _item_plan(Ho, nstrips, slots, one_row_cost=0.6):
    """(two-row items, one-row items) of csrc/flow_i8_items.h"""
    nrp = (Ho + 1) // 2
    total2, rows = nstrips * nrp, nstrips * Ho
    full = total2 // slots * slots
    r0 = full // nrp * Ho + 2 * (full % nrp)
    n1 = rows - r0
    uniform, rounds1 = -(-total2 // slots), -(-n1 // slots)
    if Ho < 2:
        return 0, rows
    if n1 > 0 and full // slots + one_row_cost * rounds1 < uniform:
        return full, n1
    return total2, 0


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", [(1, 9), (2, 15), (3, 16), (4, 33), (7, 40), (5, 23)])
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_wave_finalize_equals_the_float_path(dfe, cuda, Ho, Wo, thr):
    f0, f1, foe = _pair(Ho, Wo)
    new = _check(dfe, cuda, f0, f1, foe, thr)
    assert (new["scores2"] > 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo,slots", [(9, 48, 12), (7, 40, 10)])
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_wave_finalize_with_two_row_and_one_row_items_in_one_launch(dfe, cuda, Ho, Wo, slots, thr):
    n2, n1 = _item_plan(Ho, -(-Wo // 16), slots)
    assert n2 > 0 and n1 > 0
    f0, f1, foe = _pair(Ho, Wo)
    _check(dfe, cuda, f0, f1, foe, thr, slots=slots)


@pytest.mark.gpu
def test_wave_finalize_partial_and_empty_hit_lists(dfe, cuda, oracle):
    Ho, Wo, M = 9, 48, 4
    rng = np.random.default_rng(17)
    f0 = rng.integers(0, 256, (3, Ho + PAD, Wo + PAD)).astype(np.float32)
    f1 = rng.integers(0, 256, (3, Ho + PAD, Wo + PAD)).astype(np.float32)
    vol = np.asarray(oracle.ssd_cost_volume(f0, f1, K, K, WIN, WIN)).reshape(Ho * Wo, WIN * WIN)
    thr = float(np.floor(np.quantile(vol.max(axis=1), 0.25))) + 0.5   # (costs are integers: no cell lies at the threshold)
    hits = (vol > thr).sum(axis=1)
    assert thr >= 0.2 and (hits < M).mean() > 0.5 and (hits == 0).any() and ((hits > 0) & (hits < M)).any() and (hits >= M).any()
    new = _check(dfe, cuda, f0, f1, (Wo / 2 + 3, Ho / 2), thr)
    none = (hits == 0).reshape(Ho, Wo)
    assert (new["scores2"][none] == -7).all() and (new["imaxs"][none] == -7).all() and (new["scores2"][~none] > 0).all()
    assert (new["scores"][PAD // 2 : PAD // 2 + Ho, PAD // 2 : PAD // 2 + Wo][none] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_wave_finalize_with_the_focus_of_expansion_outside_the_frame(dfe, cuda, thr):
    Ho, Wo = 5, 23
    f0, f1, _ = _pair(Ho, Wo)
    H, W = Ho + PAD, Wo + PAD
    new = _check(dfe, cuda, f0, f1, (-30.5, H + 12.25), thr)
    border = np.ones((H, W), bool)
    border[PAD // 2 : PAD // 2 + Ho, PAD // 2 : PAD // 2 + Wo] = False
    assert (new["depth"][border] == W / 2).all() and (new["conf"][border] == 1).all()   # a pixel at rest: the clamp, confident
    assert not new["flow"][:, border].any() and not new["scores"][border].any()


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), 0.5], ids=["nan", "0.5"])
def test_gate_then_a_smaller_byte_pair_on_the_same_context(dfe, cuda, value):
    lib = dfe.lib()
    f0, f1, foe = _pair(9, 48)
    g0 = f0.copy()
    g0[1, 20, 30] = value
    s0, s1, sfoe = _pair(4, 33, seed=8)
    fresh = dfe.Context(0, torch.cuda.current_stream(0).cuda_stream)
    try:
        want, tp, tf = _run(fresh, lib, cuda, s0, s1, sfoe, 0.21, 1)
        assert tp and tf
    finally:
        fresh.close()
    ctx = dfe.get_ctx(0)
    ref, _, _ = _run(ctx, lib, cuda, g0, f1, foe, 0.21, 0)
    got, tp, tf = _run(ctx, lib, cuda, g0, f1, foe, 0.21, 1)
    assert not tp and not tf
    _same(got, ref)
    got, tp, tf = _run(ctx, lib, cuda, s0, s1, sfoe, 0.21, 1)
    assert tp and tf
    _same(got, want)
