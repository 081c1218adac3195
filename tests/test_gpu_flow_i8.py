"""The single-scale flow step on the int8 matrix cores (option "cv_i8", ssd_flow_i8.hip) against the float sweep (cv_i8 = 0), bit for bit, on
every output of dfe_flow_depth_pair_f32 and dfe_ssd_flow_f32 (outputs pre-filled with -7): strips and rows at their edges, ties (the first
tied minimum in index order, the centre override), extractOutput's fall-back on a flat block, costs at their maximum, the device-side gate
(one value that is not an integer in 0..255 sends the step to the float sweep, and leaves no verdict behind), and the byte entry point.
dfe_flow_last_path tells which kernel produced the result."""
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


def _run(dfe, cuda, f0, f1, foe, thr, i8):
    """both entry points with cv_i8 = i8; returns (outputs, i8 taken by the pair call, i8 taken by the flow call)"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C, H, W = f0.shape
    Ho, Wo = H - PAD, W - PAD
    t0 = torch.from_numpy(np.ascontiguousarray(f0)).to(cuda)
    t1 = torch.from_numpy(np.ascontiguousarray(f1)).to(cuda)
    ctx.set_option("cv_i8", i8)
    try:
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
    finally:
        ctx.set_option("cv_i8", None)
    out = dict(flow=flow, scores=sc, depth=dd, conf=cc, idx=idx, best=best, fy=fy, fx=fx, scores2=s2, imaxs=imx)
    return {k: v.cpu().numpy() for k, v in out.items()}, took_pair, took_flow


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


_REF = {}


def _float_ref(dfe, cuda, key, f0, f1, foe, thr):
    """the float sweep's outputs (cv_i8 = 0), computed once per case"""
    if key not in _REF:
        out, tp, tf = _run(dfe, cuda, f0, f1, foe, thr, 0)
        assert not tp and not tf
        _REF[key] = out
    return _REF[key]


def _check(dfe, cuda, key, f0, f1, foe, thr, expect_i8=True):
    new, tp, tf = _run(dfe, cuda, f0, f1, foe, thr, 1)
    if expect_i8 is not None:
        assert tp == tf == expect_i8, (tp, tf)
    _same(new, _float_ref(dfe, cuda, key, f0, f1, foe, thr))
    return new


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", [(1, 16), (3, 17), (2, 8), (5, 31), (9, 48), (82, 122)])
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_i8_step_equals_the_float_sweep(dfe, cuda, Ho, Wo, thr):
    f0, f1, foe = _pair(Ho, Wo)
    # (2, 8) is less than a strip: handled or declined, the outputs must be equal both ways
    new = _check(dfe, cuda, ("shape", Ho, Wo, thr), f0, f1, foe, thr, expect_i8=None if (Ho, Wo) == (2, 8) else True)
    assert (new["scores2"] > 0).mean() > 0.5


def _texture(H, W):
    rng = np.random.default_rng(11)
    cell = rng.integers(0, 256, size=(3, 6, 8)).astype(np.float32)   # period 8 (x) by 6 (y)
    return np.ascontiguousarray(np.tile(cell, (1, H // 6 + 1, W // 8 + 1))[:, :H, :W])


@pytest.mark.gpu
def test_i8_ties_centre_override_wins_on_a_periodic_texture(dfe, cuda):
    H, W = 9 + PAD, 48 + PAD
    t = _texture(H, W)
    new = _check(dfe, cuda, "tie-centre", t, t.copy(), (W / 2, H / 2), 0.21)
    assert (new["best"] == 0).all() and (new["idx"] == 16 * 33 + 16 + 1).all()


@pytest.mark.gpu
def test_i8_ties_first_minimum_in_index_order_wins(dfe, cuda):
    H, W = 9 + PAD, 48 + PAD
    t = _texture(H, W)
    f0 = np.ascontiguousarray(np.roll(t, (3, -5), axis=(1, 2)))
    new = _check(dfe, cuda, "tie-first", f0, t, (W / 2, H / 2), 0.21)
    # frame0(y, x) = t(y - 3, x + 5): cost 0 at (dy, dx) = (16 - 3, 16 + 5) + multiples of the period (6, 8); the first in index order is
    # dy = 13 - 12 = 1, dx = 21 - 16 = 5, and the centre (cost > 0) must not be chosen
    assert (new["best"] == 0).all() and (new["idx"] == 1 * 33 + 5 + 1).all()


@pytest.mark.gpu
def test_i8_constant_frames_have_no_hits(dfe, cuda):
    H, W = 9 + PAD, 48 + PAD
    f = np.full((3, H, W), 77.0, np.float32)
    new = _check(dfe, cuda, "const", f, f.copy(), (W / 2, H / 2), 0.21)
    assert (new["best"] == 0).all() and (new["scores2"] == -7).all() and (new["imaxs"] == -7).all()
    assert not new["scores"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_i8_flat_block_takes_the_fallback(dfe, cuda, thr):
    f0, f1, foe = _pair(82, 122)
    f0, f1 = f0.copy(), f1.copy()
    v = f1[:, 20, 20].copy()
    f0[:, 30:90, 40:100] = v[:, None, None]
    f1[:, 30:90, 40:100] = v[:, None, None]
    new = _check(dfe, cuda, ("flat", thr), f0, f1, foe, thr)
    # output pixel (yo, xo): frame-0 patch rows yo+16..yo+22, frame-1 patches rows yo..yo+38 (columns alike).  Windows wholly inside the block
    # cost 0 everywhere (flag set, no hit: scores left as they were); at (60, 50) the lead cells are inside (cost 0, flag set) and the lower
    # part of the window is not (hits found by the fall-back)
    assert (new["scores2"][30:52, 40:62] == -7).all()
    assert new["scores2"][60, 50] > 0


@pytest.mark.gpu
def test_i8_costs_at_their_maximum_do_not_wrap(dfe, cuda):
    H, W = 9 + PAD, 48 + PAD
    f0 = np.full((3, H, W), 255.0, np.float32)
    f1 = np.zeros((3, H, W), np.float32)
    new = _check(dfe, cuda, "extreme", f0, f1, (W / 2, H / 2), 0.21)
    assert (new["best"] == 147 * 255.0 ** 2).all()
    new = _check(dfe, cuda, "extreme-swapped", f1, f0, (W / 2, H / 2), 0.21)
    assert (new["best"] == 147 * 255.0 ** 2).all()


@pytest.mark.gpu
@pytest.mark.parametrize("value", [100.5, float("nan"), 256.0, -1.0], ids=["100.5", "nan", "256", "-1"])
@pytest.mark.parametrize("where", ["frame0-top-left", "frame1-bottom-right"])
def test_i8_gate_sends_other_frames_to_the_float_sweep(dfe, cuda, value, where):
    f0, f1, foe = _pair(9, 48)
    g0, g1 = f0.copy(), f1.copy()
    if where == "frame0-top-left":
        g0[0, 16, 16] = value      # the first frame-0 pixel any patch reads
    else:
        g1[2, -1, -1] = value      # the last frame-1 pixel any patch reads
    _check(dfe, cuda, ("gate", where, str(value)), g0, g1, foe, 0.21, expect_i8=False)
    # the untouched pair on the same context: no stale verdict
    _check(dfe, cuda, ("shape", 9, 48, 0.21), f0, f1, foe, 0.21, expect_i8=True)


@pytest.mark.gpu
def test_i8_gate_takes_minus_zero_for_zero(dfe, cuda):
    f0, f1, foe = _pair(9, 48)
    g0, g1 = f0.copy(), f1.copy()
    g0[0, 16, 16] = -0.0
    g1[2, -1, -1] = -0.0
    assert np.signbit(g0[0, 16, 16]) and np.signbit(g1[2, -1, -1])
    _check(dfe, cuda, "minus-zero", g0, g1, foe, 0.21, expect_i8=True)


def _run_u8(dfe, cuda, b0, b1, foe, thr, scale, i8):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C, H, W = b0.shape
    t0, t1 = torch.from_numpy(b0).to(cuda), torch.from_numpy(b1).to(cuda)
    ctx.set_option("cv_i8", i8)
    try:
        flow = torch.full((2, H, W), -7.0, device=cuda)
        sc, dd, cc = (torch.full((H, W), -7.0, device=cuda) for _ in range(3))
        ctx.check(lib.dfe_flow_depth_pair_u8(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, WIN, WIN, foe[0], foe[1], thr, scale, flow.data_ptr(),
                                             sc.data_ptr(), dd.data_ptr(), cc.data_ptr()))
        torch.cuda.synchronize()
    finally:
        ctx.set_option("cv_i8", None)
    return {k: v.cpu().numpy() for k, v in dict(flow=flow, scores=sc, depth=dd, conf=cc).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", [(9, 48), (82, 122)])
def test_i8_byte_entry_point(dfe, cuda, Ho, Wo):
    f0, f1, foe = _pair(Ho, Wo)
    b0, b1 = np.ascontiguousarray(f0.astype(np.uint8)), np.ascontiguousarray(f1.astype(np.uint8))
    assert np.array_equal(b0.astype(np.float32), f0) and np.array_equal(b1.astype(np.float32), f1)
    ref = _float_ref(dfe, cuda, ("shape", Ho, Wo, 0.21), f0, f1, foe, 0.21)
    got = _run_u8(dfe, cuda, b0, b1, foe, 0.21, 1.0, 1)
    _same(got, {k: ref[k] for k in got})
    # any other scale: the float path, whatever cv_i8 says
    thr = 0.21 / 255.0 ** 2
    _same(_run_u8(dfe, cuda, b0, b1, foe, thr, 1.0 / 255.0, 1), _run_u8(dfe, cuda, b0, b1, foe, thr, 1.0 / 255.0, 0))
