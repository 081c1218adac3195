"""GPU suite (-m gpu): the raw-patch pyramid matcher's launcher switches at its 8 x 8, k = 7, C = 3 corner -- the kernel instantiations
and store paths that only a public setter or a DFE_* variable reaches (csrc/ssd_cost_volume.hip, csrc/multiscale.hip):

    set_cost_volume_tile(2 .. 5)    ssd_cv_tiled_multi_kernel<.., NQ> for NQ = 2, 3, 4, 5 (cv_frames_dispatch_multi)
    fine_nq = 5, mid_nq = 5         launch_cv_fine<5>: ssd_cv_tiled_fine_kernel<.., 5, F16, MID>, fp32 / fp16 x finest / second scale
    xpose = 0                       the multi kernel's plain store path; with half volumes it declines and the caller rounds fp32 volumes
    xpose_nt = 0 / 1                the transposed store path without / with the non-temporal hint, whatever the volumes' size

Every case runs the one call with the launcher's own choice and with the switch forced, into outputs pre-filled with -7 that are 64
elements longer than the result, and requires idx and flow to be equal bit for bit.  One configuration per group also goes against the
oracle chain on row 21 of tests/pyramid_cases.py (tests/test_pyramid_cases_cpu.py pins its tie shares) under assert_matches_oracle's rule.

Every one of these launchers declines silently when its tile does not fit the frame, and the per-scale path then gives the same, correct
answer.  So each case also asserts the observable that tells the forced kernel from that fallback.  The cost-volume launchers bracket
their launches for dfe_profile_read (prep, soft-min, rounding and cascade launches are not bracketed); what ms_run launches, by its plan:

    volumes of the nv = nratios - s0 materialised scales   1 launch (the multi kernel, nv >= 2)    fallback: nv launches, one per scale
    fused finest scale (fine_fuse)                         + 1 (launch_cv_fine)    no plan: + 1 all the same, but last_kernel is not its name
    fused second scale (mid_fuse, >= 3 ratios)             + 1 (launch_cv_fine)    not planned: s0 stays 1 and the count is one lower
    (s0 = 0, 1, 2 for no fused scale, the finest, the finest and the second; nv = 1: the multi kernel does not apply, 1 launch)

so: multi kernel, fine_fuse = 0: 1; multi kernel, fine_fuse = 1, three ratios: 2; fused finest scale with ratios [1] / [1, 2] / [1, 2, 4]:
1 / 2 / 2; both fused, [1, 2, 4]: 3.  ctx.last_kernel() starts with ssd_cv_tiled_fine_kernel only when the fused finest kernel ran, and
is ssd_cv_tiled_multi_kernel_f16 only when the multi kernel wrote halves.  A tile of NQ row groups has 6 NQ - 6 output rows and 32 columns;
the frames' coarsest materialised scale is at least 24 x 34.  The last two tests show that the forced heights really reach the launchers:
a scale lower than the forced tile takes the other path."""
from ctypes import byref, c_double, c_int

import numpy as np
import pytest
import torch

from tests import pyramid_cases as pc

pytestmark = pytest.mark.gpu

FILL, TAIL = -7, 64
FINE = "ssd_cv_tiled_fine_kernel"
MULTI16 = "ssd_cv_tiled_multi_kernel_f16"
ROW = pc.SWITCH_ORACLE                       # 96 x 136, ratios 1, 2, 4: the frames every group uses, and the oracle's
SHAPES = [(96, 136), (136, 200)]             # scales of 24 x 34 and 34 x 50 at ratio 4: ragged last tiles in both directions


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _frames(H, W, ratios):
    if (H, W, ratios) == (ROW.H, ROW.W, ROW.ratios):
        return pc.frames(ROW)
    return pc.frames(pc.Case(0, ratios, 8, 8, 7, 3, H, W, min(14, 4 * ratios[-1] - 2), "switches", None))


def _call(dfe, cuda, f0, f1, ratios, f16):
    """dfe_multiscale_flow_pair_f32 / _f16 (scale 1.0) into guarded buffers with the launch brackets on:
    (idx [H][W], flow [2][H][W], bracketed launches, last_kernel)"""
    from depth_estimation_amd._lib import ratios_array

    Cc, H, W = f0.shape
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    rr, n = ratios_array(ratios)
    idx = torch.full((H * W + TAIL,), FILL, dtype=torch.int64, device=cuda)
    flow = torch.full((2 * H * W + TAIL,), float(FILL), device=cuda)
    t0, t1 = T(f0, cuda), T(f1, cuda)
    ms, cnt = c_double(), c_int()
    ctx.check(lib.dfe_profile_read(ctx.handle, byref(ms), byref(cnt)))          # (nothing left over from an earlier user)
    ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
    try:
        if f16:
            ctx.check(lib.dfe_multiscale_flow_pair_f16(ctx.handle, t0.data_ptr(), t1.data_ptr(), Cc, H, W, 7, 8, 8, rr, n, 1.0, flow.data_ptr(), idx.data_ptr()))
        else:
            ctx.check(lib.dfe_multiscale_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), Cc, H, W, 7, 8, 8, rr, n, flow.data_ptr(), idx.data_ptr()))
        ctx.check(lib.dfe_profile_read(ctx.handle, byref(ms), byref(cnt)))
    finally:
        ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
    gi, gf = idx.cpu().numpy(), flow.cpu().numpy()
    assert (gi[H * W :] == FILL).all() and (gf[2 * H * W :] == FILL).all(), "wrote behind an output"
    assert not (gi[: H * W] == FILL).any(), "left class ids unwritten"
    return gi[: H * W].reshape(H, W), gf[: 2 * H * W].reshape(2, H, W), cnt.value, ctx.last_kernel()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "%s: idx or flow differ from the launcher's own choice" % (what,)


def _oracle(got, f16):
    """row 21 against the oracle chain: assert_matches_oracle's rule; half volumes: the tie rule of test_row_f16_equals_oracle_chain"""
    ref = pc.reference(ROW.no, 1.0 if f16 else None)
    tie = None
    if f16:
        top2 = ref["top2"]
        tie = top2[..., 1] - top2[..., 0] <= 2e-3 * np.maximum(top2[..., 1], 1e-6) + 1e-5
    pc.assert_matches_oracle(got[0], got[1], ref, ROW, tie=tie)


# ---- 1. the multi kernel at every tile height ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("ratios,fuse", [([1, 2], 0), ([1, 2, 4], 0), ([1, 2, 4], 1)], ids=["1_2", "1_2_4", "1_2_4-fused_finest"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_multi_kernel_every_tile_height_equals_own_choice(dfe, cuda, H, W, ratios, fuse, f16):
    """set_cost_volume_tile(2 .. 5) with every scale's volume from the multi kernel (fine_fuse = 0: two or three scales) and with the two
    coarser scales' (fine_fuse = 1), fp32 and half volumes, soft_epilogue 0 and 1: one bracketed launch for the volumes (+ 1 for the fused
    finest scale), bits of the launcher's own choice (4 row groups; 3 beside a fused finest scale).  On the lane <-> pixel path no scale
    leaves the volume launch as probabilities, so the fp32 three-scale volume path also runs with cascade_px = 0, where soft_epilogue
    decides that."""
    f0, f1 = _frames(H, W, ratios)
    ctx = dfe.get_ctx(0)
    count = 2 if fuse else 1
    variants = [(-1, 0), (-1, 1)]                   # (cascade_px, soft_epilogue); -1: released
    if not f16 and not fuse and len(ratios) == 3:
        variants += [(0, 0), (0, 1)]

    def check(what, res):
        assert res[2] == count, "%s: %d bracketed launches, %d expected (%s)" % (what, res[2], count, res[3])
        if fuse:
            assert res[3].startswith(FINE), (what, res[3])
        elif f16:
            assert res[3] == MULTI16, (what, res[3])

    want_px = None
    for px, soft in variants:
        opts = (px, soft)
        with ctx.options(fine_fuse=fuse, cascade_px=px, soft_epilogue=soft):
            want = _call(dfe, cuda, f0, f1, ratios, f16)
            check((opts, 0), want)
            if px == 0:
                assert ctx.multiscale_last_path().endswith("cascade_argmax_kernel<fast>")
            try:
                for nq in (2, 3, 4, 5):
                    ctx.set_cost_volume_tile(nq)
                    got = _call(dfe, cuda, f0, f1, ratios, f16)
                    check((opts, nq), got)
                    _same(got, want, (opts, nq))
            finally:
                ctx.set_cost_volume_tile(0)
        if px != 0:
            if want_px is not None:
                _same(want, want_px, opts)              # (soft_epilogue changes nothing on the lane <-> pixel path)
            want_px = want
    if (H, W, ratios) == (ROW.H, ROW.W, ROW.ratios):
        _oracle(want_px, f16)


# ---- 2. the fused kernels at 5 row groups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("ratios,H,W", [([1], 64, 96), ([1, 2], 96, 128), ([1, 2, 4], 96, 136), ([1, 2, 4], 136, 200)])
def test_fused_kernels_with_five_row_groups_equal_four(dfe, cuda, ratios, H, W, f16):
    """fine_nq = 5 (finest scale fused), mid_nq = 5 and both (second scale fused too, three ratios) against the same plan with the
    launcher's 4 row groups, at the shapes of test_fused_finest_scale_equals_volume_path_bitwise that a 24-row tile fits: the fused
    finest kernel names itself, and the launch count tells a fused second scale (3) from a materialised one (2)."""
    f0, f1 = _frames(H, W, ratios)
    ctx = dfe.get_ctx(0)
    base = {1: 1, 2: 2, 3: 2}[len(ratios)]

    def run(count, **opts):
        with ctx.options(**opts):
            res = _call(dfe, cuda, f0, f1, ratios, f16)
        assert res[3].startswith(FINE) and res[2] == count, (opts, res[2], count, res[3])
        return res

    want = run(base, fine_fuse=1, mid_fuse=0)
    _same(run(base, fine_fuse=1, mid_fuse=0, fine_nq=5), want, "fine_nq = 5")
    if len(ratios) >= 3:
        want_mid = run(3, fine_fuse=1, mid_fuse=1)
        _same(want_mid, want, "mid_fuse = 1")
        _same(run(3, fine_fuse=1, mid_fuse=1, mid_nq=5), want, "mid_nq = 5")
        _same(run(3, fine_fuse=1, mid_fuse=1, fine_nq=5, mid_nq=5), want, "fine_nq = mid_nq = 5")
    if (H, W, ratios) == (ROW.H, ROW.W, ROW.ratios):
        _oracle(run(3, fine_fuse=1, mid_fuse=1, fine_nq=5, mid_nq=5), f16)


# ---- 3. the multi kernel's store paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratios", [[1, 2], [1, 2, 4]], ids=["1_2", "1_2_4"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_untransposed_store_path_equals_transposed(dfe, cuda, H, W, ratios):
    """xpose = 0.  fp32: the multi kernel stores a task row cell by cell instead of through its transpose scratch -- one launch either way,
    same bits.  Half volumes: the multi kernel declines, the fp32 multi kernel runs (one launch, its fp32 name) and the volumes are
    rounded in place -- to the halves the kernel's own store rounds to, so idx and flow are those of the half-volume launch."""
    f0, f1 = _frames(H, W, ratios)
    ctx = dfe.get_ctx(0)
    for f16 in (False, True):
        with ctx.options(fine_fuse=0):
            want = _call(dfe, cuda, f0, f1, ratios, f16)
        with ctx.options(fine_fuse=0, xpose=0):
            got = _call(dfe, cuda, f0, f1, ratios, f16)
        assert want[2] == 1 and got[2] == 1, (f16, want[2], got[2])
        assert want[3] == (MULTI16 if f16 else "ssd_cv_tiled_kernel") and got[3] == "ssd_cv_tiled_kernel", (f16, want[3], got[3])
        _same(got, want, "xpose = 0, f16 %s" % f16)
        if (H, W, ratios) == (ROW.H, ROW.W, ROW.ratios):
            _oracle(got, f16)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_non_temporal_hint_forced_off_and_on(dfe, cuda, H, W, f16):
    """xpose_nt = 0 / 1: the hint of the transposed stores (the launcher turns it on by itself only above 160 MB of volumes) changes no bit"""
    ratios = [1, 2, 4]
    f0, f1 = _frames(H, W, ratios)
    ctx = dfe.get_ctx(0)
    with ctx.options(fine_fuse=0):
        want = _call(dfe, cuda, f0, f1, ratios, f16)
    for nt in (0, 1):
        with ctx.options(fine_fuse=0, xpose_nt=nt):
            got = _call(dfe, cuda, f0, f1, ratios, f16)
        assert got[2] == 1 and got[3] == (MULTI16 if f16 else "ssd_cv_tiled_kernel"), (nt, got[2], got[3])
        _same(got, want, "xpose_nt = %d" % nt)
        if nt == 1 and (H, W) == (ROW.H, ROW.W):
            _oracle(got, f16)


# ---- 4. the forced heights reach the launchers: a scale lower than the tile takes the other path --------------------------------------
def test_multi_kernel_declines_a_scale_lower_than_the_forced_tile(dfe, cuda):
    """ratios 1, 2 on 40 x 72: the second scale has 20 rows -- a tile of 4 row groups (18 rows) fits, one of 5 (24 rows) does not.
    set_cost_volume_tile(4): one launch; (5): one launch per scale.  (The per-scale kernels sum in another order: no bits compared.)"""
    f0, f1 = _frames(40, 72, [1, 2])
    ctx = dfe.get_ctx(0)
    counts = {}
    try:
        for nq in (4, 5):
            ctx.set_cost_volume_tile(nq)
            with ctx.options(fine_fuse=0):
                counts[nq] = _call(dfe, cuda, f0, f1, [1, 2], False)[2]
    finally:
        ctx.set_cost_volume_tile(0)
    assert counts == {4: 1, 5: 2}, counts


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_fused_kernels_decline_a_scale_lower_than_five_row_groups(dfe, cuda, f16):
    """fine_nq = 5 on a 20-row frame: no fused finest kernel, the volume path's bits (the finest scale's sums are exact on these frames).
    mid_nq = 5 on 40 x 136, ratios 1, 2, 4 (second scale 20 rows): the plan keeps the second scale's volume -- the call used to fail with
    'no plan for the fused second scale' -- and the result is that of mid_fuse = 0."""
    ctx = dfe.get_ctx(0)
    f0, f1 = _frames(20, 72, [1])
    with ctx.options(fine_fuse=1):
        want = _call(dfe, cuda, f0, f1, [1], f16)
    with ctx.options(fine_fuse=1, fine_nq=5):
        got = _call(dfe, cuda, f0, f1, [1], f16)
    assert want[3].startswith(FINE) and not got[3].startswith(FINE), (want[3], got[3])
    _same(got, want, "fine_nq = 5 on 20 rows")
    f0, f1 = _frames(40, 136, [1, 2, 4])
    with ctx.options(fine_fuse=1, mid_fuse=0):
        want = _call(dfe, cuda, f0, f1, [1, 2, 4], f16)
    with ctx.options(fine_fuse=1, mid_fuse=1):
        mid = _call(dfe, cuda, f0, f1, [1, 2, 4], f16)
    with ctx.options(fine_fuse=1, mid_fuse=1, mid_nq=5):
        got = _call(dfe, cuda, f0, f1, [1, 2, 4], f16)
    assert want[3].startswith(FINE) and mid[3].startswith(FINE) and got[3].startswith(FINE)
    assert (want[2], mid[2], got[2]) == (3, 3, 3), (want[2], mid[2], got[2])     # the 10-row third scale: no multi kernel, one launch per scale
    _same(mid, want, "mid_fuse = 1 on a 20-row second scale")
    _same(got, want, "mid_nq = 5 on a 20-row second scale")
