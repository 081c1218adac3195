"""The one launch behind the int8 flow kernel (ssd_cv_rowimg_flow_gated_kernel, ssd_cost_volume.hip): it writes the frame's border and, if
the frames were not byte-valued, runs the float sweep and lets every block finalize the pixels of its own tile-row records.  Every output
of dfe_flow_depth_pair_f32 and dfe_ssd_flow_f32, pre-filled with -7, must equal the path without int8 (cv_i8 = 0: the ungated sweep and
the separate finalize launch) byte for byte, whole arrays, border included: one output row, a shifted last tile column, several tile
columns, blocks that hold pieces of two columns, pieces cut mid-column and blocks with an empty range (option sweep_blocks), both
extractOutput list lengths, pixels that take the fallback plane, a focus of expansion outside the frame, and a sequence of gated and byte
steps on one context."""
import numpy as np
import pytest
import torch

from tests import refpath as rp

K, WIN = 7, 33
PAD = K + WIN - 2
SHAPES = [(1, 9), (5, 23), (9, 48), (13, 70)]
# the sweep cuts no piece shorter than 8 rows (kSweepMin), so a cut inside a column needs at least 16 output rows: one shape more for that
SWEEP_SHAPES = SHAPES + [(17, 23)]


def _pair(Ho, Wo, seed=5):
    H, W = Ho + PAD, Wo + PAD
    f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=seed, max_flow=min(12, max(1, min(H, W) // 8)), integer=True)
    return f0, f1, foe


def _spoiled(f0, value, at=None):
    """the pair's first frame with ONE value that is no byte: the pack kernel raises the verdict and the float sweep does the step"""
    g0 = f0.copy()
    y, x = at or (g0.shape[1] // 2, g0.shape[2] // 2)
    g0[1, y, x] = value
    return g0


def _run(ctx, lib, cuda, f0, f1, foe, thr, i8, blocks=None):
    """both entry points with cv_i8 = i8 (and sweep_blocks = blocks); returns (outputs, int8 taken by the pair call, by the flow call)"""
    C, H, W = f0.shape
    Ho, Wo = H - PAD, W - PAD
    t0 = torch.from_numpy(np.ascontiguousarray(f0)).to(cuda)
    t1 = torch.from_numpy(np.ascontiguousarray(f1)).to(cuda)
    with ctx.options(cv_i8=i8, sweep_blocks=-1 if blocks is None else blocks):
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
    assert len(out) == 10
    return {k: v.cpu().numpy() for k, v in out.items()}, took_pair, took_flow


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _check(dfe, cuda, f0, f1, foe, thr, blocks=None, expect_i8=False):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    ref, rp_, rf_ = _run(ctx, lib, cuda, f0, f1, foe, thr, 0, blocks)
    assert not rp_ and not rf_
    new, tp, tf = _run(ctx, lib, cuda, f0, f1, foe, thr, 1, blocks)
    assert tp == tf == expect_i8, (tp, tf)
    _same(new, ref)
    return new


def _cuts(B, ncols, Ho, ovh=9, minr=8):
    """sweep_cut of ssd_cost_volume.hip for b = 0 .. B with the launcher's kSweepOvh and kSweepMin"""
    out = []
    for b in range(B + 1):
        if b >= B:
            out.append(ncols * Ho)
            continue
        Lc = Ho + ovh
        u = Lc * ncols * b // B
        col = u // Lc
        row = u - col * Lc - ovh
        if row < minr:
            row = 0
        elif Ho - row < minr:
            col, row = col + 1, 0
        out.append(col * Ho + row)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", SWEEP_SHAPES)
@pytest.mark.parametrize("blocks", [None, 1, 3, 7, "many"])
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_float_path_through_the_merged_kernel(dfe, cuda, Ho, Wo, blocks, thr):
    ncols = -(-Wo // 8)
    if blocks == "many":
        blocks = ncols * Ho + 5   # more blocks than tile rows: some ranges are empty
    f0, f1, foe = _pair(Ho, Wo)
    new = _check(dfe, cuda, _spoiled(f0, 0.5), f1, foe, thr, blocks)
    assert (new["scores2"] > 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", [(5, 23), (13, 70)])
def test_float_path_with_a_nan(dfe, cuda, Ho, Wo):
    f0, f1, foe = _pair(Ho, Wo)
    _check(dfe, cuda, _spoiled(f0, float("nan")), f1, foe, 0.21, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_float_path_with_the_focus_of_expansion_outside_the_frame(dfe, cuda, thr):
    Ho, Wo = 5, 23
    f0, f1, _ = _pair(Ho, Wo)
    H, W = Ho + PAD, Wo + PAD
    new = _check(dfe, cuda, _spoiled(f0, 0.5), f1, (-30.5, H + 12.25), thr, 3)
    border = np.ones((H, W), bool)
    border[PAD // 2 : PAD // 2 + Ho, PAD // 2 : PAD // 2 + Wo] = False
    assert (new["depth"][border] == W / 2).all() and (new["conf"][border] == 1).all()   # a pixel at rest: the clamp, confident
    assert not new["flow"][:, border].any() and not new["scores"][border].any()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.21, 0.11])
@pytest.mark.parametrize("blocks", [None, 7])
def test_float_path_with_pixels_on_the_fallback_plane(dfe, cuda, thr, blocks):
    Ho, Wo = 13, 70
    f0, f1, foe = _pair(Ho, Wo)
    # both frames constant on a block (as tests/test_gpu_novol.py plants it): pixel (y, x) reads frame 0 at rows y + 16 .. y + 22, columns
    # x + 16 .. x + 22 and, for its eight lead cells, frame 1 at rows y .. y + 6, columns x .. x + 13 -- all inside the block for y <= 8,
    # x <= 38: lead cells of cost 0, none above the threshold, the hits come from further on in the window
    v = f1[:, 40, 90].copy()
    f0[:, :31, :61] = v[:, None, None]
    f1[:, :31, :61] = v[:, None, None]
    new = _check(dfe, cuda, _spoiled(f0, 0.5, at=(45, 100)), f1, foe, thr, blocks)
    assert (new["best"][:9, :39] == 0).all() and (new["scores2"][:9, :39] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", SHAPES)
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_byte_path_border_from_the_merged_kernel(dfe, cuda, Ho, Wo, thr):
    f0, f1, foe = _pair(Ho, Wo)
    new = _check(dfe, cuda, f0, f1, foe, thr, expect_i8=True)
    H, W = Ho + PAD, Wo + PAD
    border = np.ones((H, W), bool)
    border[PAD // 2 : PAD // 2 + Ho, PAD // 2 : PAD // 2 + Wo] = False
    assert not new["flow"][:, border].any() and not new["scores"][border].any() and (new["conf"][border] == 1).all()


def test_the_tested_grids_hold_two_column_blocks_mid_column_cuts_and_empty_ranges():
    """what the shapes and sweep_blocks values above are chosen for, worked out from the cut rule"""
    for Ho, Wo in SWEEP_SHAPES:   # one block: every column of the pair in one range
        assert _cuts(1, -(-Wo // 8), Ho) == [0, -(-Wo // 8) * Ho]
    c = _cuts(7, 3, 17)                       # (17, 23), seven blocks
    assert any(0 < a % 17 for a in c[1:-1])                                           # a cut inside a column
    c = _cuts(3, 9, 13)                       # (13, 70), three blocks
    assert any(a // 13 != (b - 1) // 13 for a, b in zip(c, c[1:]) if b > a)           # a block with pieces of several columns
    c = _cuts(3 * 5 + 5, 3, 5)                # (5, 23), more blocks than tile rows
    assert any(a == b for a, b in zip(c, c[1:])) and c[0] == 0 and c[-1] == 15        # empty ranges, the sequence covered


@pytest.mark.gpu
def test_gated_then_smaller_byte_then_gated_step_on_one_context(dfe, cuda):
    lib = dfe.lib()
    f0, f1, foe = _pair(9, 48)
    g0 = _spoiled(f0, 0.5)
    s0, s1, sfoe = _pair(5, 23, seed=8)
    fresh = dfe.Context(0, torch.cuda.current_stream(0).cuda_stream)
    try:
        want_small, tp, tf = _run(fresh, lib, cuda, s0, s1, sfoe, 0.21, 1)
        assert tp and tf
    finally:
        fresh.close()
    fresh = dfe.Context(0, torch.cuda.current_stream(0).cuda_stream)
    try:
        want_gated, tp, tf = _run(fresh, lib, cuda, g0, f1, foe, 0.21, 1)
        assert not tp and not tf
    finally:
        fresh.close()
    ctx = dfe.get_ctx(0)
    ref, _, _ = _run(ctx, lib, cuda, g0, f1, foe, 0.21, 0)
    _same(want_gated, ref)
    for frames, want, i8 in ((( g0, f1, foe), want_gated, False), ((s0, s1, sfoe), want_small, True), ((g0, f1, foe), want_gated, False)):
        got, tp, tf = _run(ctx, lib, cuda, *frames, 0.21, 1)
        assert tp == tf == i8
        _same(got, want)
