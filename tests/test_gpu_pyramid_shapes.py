"""GPU suite (-m gpu): the raw-patch pyramid matcher (csrc/multiscale.hip) off the one corner the rest of the suite runs it at -- k = 7,
C = 3, square 8 x 8 windows, ratios 1, 2, 4, ..., W a multiple of 8.  The rows of tests/pyramid_cases.py take the one-call entries
through the lane <-> cell kernel's generic branch (ratios that are no powers of two, a last group of fewer than 8 pixels), non-square
windows, the slow form (more than 64 cells, more than 5 scales), 8 x 8 windows that must not take the lane <-> pixel path, and the
preparation kernel that makes every scale from one read off its 64-pixel tile grid.

The reference is the oracle chain (rp.multiscale_flow_oracle), computed once per row and shared read-only.  The rule is
_assert_matches_oracle's: indices equal the oracle's except where its two best classes lie within 1e-5, at most 2 % of the pixels
differ, and the decode of whatever index was taken is the codec's, exactly (tests/test_pyramid_cases_cpu.py pins that the rows have
few such ties).  Outputs are written into buffers pre-filled with -7 that are 64 elements longer than the result: the tail keeps its
-7, no class id stays -7 (ids start at 1), and the flow is the decode of the ids (a displacement can be -7 itself).  Every kernel name
the module saw is printed when it is done (-s shows it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import pyramid_cases as pc
from tests import refpath as rp

pytestmark = pytest.mark.gpu

FILL, TAIL = -7, 64
DFE_E_SHAPE = -2
SEEN = set()                # every last_kernel / multiscale_last_path name this module saw
FAST, SLOW, PX = "cascade_argmax_kernel<fast>", "cascade_argmax_kernel<slow>", "cascade_px_kernel"
# the cascade kernel each row is there for (rows 11 and 13: with the lane <-> pixel path on)
CASCADE = {1: FAST, 2: FAST, 3: FAST, 4: FAST, 5: FAST, 6: FAST, 7: SLOW, 8: SLOW, 9: SLOW, 10: FAST, 11: PX, 12: FAST, 13: PX}


@pytest.fixture(scope="module", autouse=True)
def _report_names():
    yield
    print("\nkernel names seen by test_gpu_pyramid_shapes: " + " | ".join(sorted(SEEN)))


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _rr(ratios):
    from depth_estimation_amd._lib import ratios_array

    return ratios_array(ratios)


def _note(ctx):
    SEEN.add("last_kernel=" + ctx.last_kernel())
    path = ctx.multiscale_last_path()
    SEEN.update(path.split())
    return path


def _outputs(cuda, H, W):
    idx = torch.full((H * W + TAIL,), FILL, dtype=torch.int64, device=cuda)
    flow = torch.full((2 * H * W + TAIL,), float(FILL), device=cuda)
    return idx, flow


def _collect(idx, flow, H, W):
    gi, gf = idx.cpu().numpy(), flow.cpu().numpy()
    assert (gi[H * W :] == FILL).all() and (gf[2 * H * W :] == FILL).all(), "wrote behind an output"
    assert not (gi[: H * W] == FILL).any(), "left class ids unwritten"
    return gi[: H * W].reshape(H, W), gf[: 2 * H * W].reshape(2, H, W)


def one_call(dfe, cuda, f0, f1, k, mh, mw, ratios, f16_scale=0.0, u8_scale=0.0, ctx=None):
    """dfe_multiscale_flow_pair_f32 / _f16 / _u8 (u8_scale > 0: the frames hold byte values and go in as bytes at an odd address) into
    guarded buffers; returns (idx [H][W], flow [2][H][W], '<prep> <cascade>')"""
    Cc, H, W = f0.shape
    ctx = ctx or dfe.get_ctx(0)
    lib = dfe.lib()
    rr, n = _rr(ratios)
    idx, flow = _outputs(cuda, H, W)
    if u8_scale:
        m = f0.size
        buf = torch.zeros(2 * m + 2, dtype=torch.uint8, device=cuda)
        buf[1 : m + 1] = T(f0.astype(np.uint8).ravel(), cuda)
        buf[m + 2 :] = T(f1.astype(np.uint8).ravel(), cuda)
        ctx.check(lib.dfe_multiscale_flow_pair_u8(ctx.handle, buf.data_ptr() + 1, buf.data_ptr() + m + 2, Cc, H, W, k, mh, mw, rr, n, u8_scale, f16_scale,
                                                  flow.data_ptr(), idx.data_ptr()))
    else:
        t0, t1 = T(f0, cuda), T(f1, cuda)
        if f16_scale:
            ctx.check(lib.dfe_multiscale_flow_pair_f16(ctx.handle, t0.data_ptr(), t1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, f16_scale, flow.data_ptr(), idx.data_ptr()))
        else:
            ctx.check(lib.dfe_multiscale_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, flow.data_ptr(), idx.data_ptr()))
    ctx.synchronize()
    path = _note(ctx)
    gi, gf = _collect(idx, flow, H, W)
    return gi, gf, path


def run_case(dfe, cuda, c, **kw):
    f0, f1 = pc.frames(c)
    return one_call(dfe, cuda, f0, f1, c.k, c.mh, c.mw, c.ratios, **kw)


# ---- 1. the geometry guard: nothing is launched, nothing is written ------------------------------------------------------------------
@pytest.mark.parametrize("ratios,mh,mw,scale", pc.BAD_RINGS)
def test_every_ring_entry_rejects_a_window_lower_than_twice_its_ring(dfe, cuda, ratios, mh, mw, scale):
    """maxh < 2 d: DFE_E_SHAPE from every entry that uses the ring layout, its outputs (pre-filled with -7) untouched, the message names
    the scale, the window and d.  CascadingAddTable has no ring and still runs these windows."""
    lib = dfe.lib()
    ctx = dfe.get_ctx(0)
    rr, n = _rr(ratios)
    H, W, Cc, k = 4 * ratios[-1], 6 * ratios[-1], 2, 3
    d = pc.ring_widths(ratios, mw)[scale]
    f0 = torch.rand((Cc, H, W), device=cuda)
    f1 = torch.rand((Cc, H, W), device=cuda)
    b0, b1 = (f0 * 255).to(torch.uint8), (f1 * 255).to(torch.uint8)
    probs = [torch.rand((H // r, W // r, mh, mw), device=cuda) for r in ratios]
    parr = (C.c_void_p * n)(*[p.data_ptr() for p in probs])
    ids = torch.ones((H, W), dtype=torch.int64, device=cuda)

    def outs():
        return (torch.full((2, H, W), float(FILL), device=cuda), torch.full((H, W), FILL, dtype=torch.int64, device=cuda),
                torch.full((H, W), float(FILL), device=cuda), torch.full((H, W, 4 * mh * mw), float(FILL), device=cuda))

    fp, ip = lambda o: o[0].data_ptr(), lambda o: o[1].data_ptr()
    entries = {
        "dfe_multiscale_flow_pair_f32": lambda o: lib.dfe_multiscale_flow_pair_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, fp(o), ip(o)),
        "dfe_multiscale_flow_pair_f16": lambda o: lib.dfe_multiscale_flow_pair_f16(ctx.handle, f0.data_ptr(), f1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, 1.0, fp(o), ip(o)),
        "dfe_multiscale_flow_pair_u8": lambda o: lib.dfe_multiscale_flow_pair_u8(ctx.handle, b0.data_ptr(), b1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, 1.0 / 255, 0.0, fp(o), ip(o)),
        "dfe_multiscale_flow_pair_subpixel_f32": lambda o: lib.dfe_multiscale_flow_pair_subpixel_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, fp(o), ip(o)),
        "dfe_multiscale_flow_pair_subpixel_u8": lambda o: lib.dfe_multiscale_flow_pair_subpixel_u8(ctx.handle, b0.data_ptr(), b1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, 1.0 / 255, 0.0, fp(o), ip(o)),
        "dfe_multiscale_refine_subpixel_f32": lambda o: lib.dfe_multiscale_refine_subpixel_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, ids.data_ptr(), fp(o)),
        "dfe_cascade_ring_f32": lambda o: lib.dfe_cascade_ring_f32(ctx.handle, parr, rr, n, H, W, mh, mw, o[3].data_ptr()),
        "dfe_cascade_flow_f32": lambda o: lib.dfe_cascade_flow_f32(ctx.handle, parr, rr, n, H, W, mh, mw, ip(o), o[2].data_ptr(), fp(o), fp(o) + 4 * H * W),
        "dfe_x2yx_multi": lambda o: lib.dfe_x2yx_multi(ctx.handle, mh, mw, rr, n, ids.data_ptr(), H * W, ip(o), o[3].data_ptr(), 0),
        "dfe_x2yx_multi(compat_c)": lambda o: lib.dfe_x2yx_multi(ctx.handle, mh, mw, rr, n, ids.data_ptr(), H * W, ip(o), o[3].data_ptr(), 1),
    }
    for name, call in entries.items():
        o = outs()
        rc = call(o)
        torch.cuda.synchronize()
        assert rc == DFE_E_SHAPE, (name, rc, ctx.last_error())
        msg = ctx.last_error()
        assert "scale %d" % scale in msg and "%dx%d" % (mh, mw) in msg and "d=%d" % d in msg, (name, msg)
        for t in o:
            assert bool((t == FILL).all()), name + " wrote into an output"
    assert lib.dfe_multi_nclasses(mh, mw, rr, n) == -1 and lib.dfe_yx2x_multi(mh, mw, rr, n, 0.0, 0.0) == -1
    # CascadingAddTable itself: no ring, as permissive as CascadingAddTable.lua
    rng = np.random.default_rng(mw)
    ins = [rng.integers(0, 6, (5, mh, mw)).astype(np.float32) / 8 for _ in ratios]
    rc, ref = orc.cascading_add(ins, ratios, mh, mw)
    assert rc == 0
    got = dfe.nn.CascadingAddTable(ratios).forward([T(a, cuda) for a in ins])
    for g, e in zip(got, ref):
        assert np.array_equal(g.cpu().numpy(), e)


# ---- 2. the one-call fp32 entry, row by row --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.CASES, ids=[c.id for c in pc.CASES])
def test_row_equals_oracle_chain(dfe, cuda, c):
    """dfe_multiscale_flow_pair_f32 against the oracle chain; rows 1 to 10 with the soft-min epilogue of the merged volume launch forced off
    and on, rows 11 and 13 with the lane <-> pixel path on and off -- bit-equal both ways; the kernel the row is there for really ran."""
    ref = pc.reference(c.no)
    ctx = dfe.get_ctx(0)
    if c.no in (11, 13):
        variants = [("cascade_px", 1), ("cascade_px", 0)]
    elif c.no <= 10:
        variants = [("soft_epilogue", 0), ("soft_epilogue", 1)]
    else:
        variants = [(None, None)]
    results = []
    for key, v in variants:
        if key:
            ctx.set_option(key, v)
        gi, gf, path = run_case(dfe, cuda, c)
        want = FAST if (key, v) == ("cascade_px", 0) else CASCADE[c.no]
        assert path == "prep_scales_kernel " + want, (c.no, key, v, path)
        pc.assert_matches_oracle(gi, gf, ref, c)
        results.append((gi, gf))
    for gi, gf in results[1:]:
        assert np.array_equal(gi, results[0][0]) and np.array_equal(gf, results[0][1]), "the two variants of row %d differ" % c.no


# ---- 3. fp16 volumes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no", [3, 6, 7, 11])
def test_row_f16_equals_oracle_chain(dfe, cuda, no):
    """dfe_multiscale_flow_pair_f16 (scale 1.0) against the oracle chain with half() applied where the volume is stored: the float-frame
    tie rule of test_one_call_multiscale_f16_equals_oracle_chain -- a cost within an fp32 ulp of a half rounding boundary can round the
    other way on the device, its soft-min moves by up to a half quantum (2^-11 relative on the cost)."""
    c = pc.BY_NO[no]
    ref = pc.reference(no, 1.0)
    gi, gf, path = run_case(dfe, cuda, c, f16_scale=1.0)
    assert path.split()[1] == CASCADE[no], path
    top2 = ref["top2"]
    tie = top2[..., 1] - top2[..., 0] <= 2e-3 * np.maximum(top2[..., 1], 1e-6) + 1e-5
    pc.assert_matches_oracle(gi, gf, ref, c, tie=tie)
    gi32, _, _ = run_case(dfe, cuda, c)
    assert (gi32 == gi).mean() > 0.9


# ---- 4. byte frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no", [3, 10, 12])
def test_row_u8_equals_f32_entry_bitwise(dfe, cuda, no):
    """dfe_multiscale_flow_pair_u8 on byte frames at an odd address, scale 1/255 == the fp32 entry on float(byte) * scale, bit for bit"""
    c = pc.BY_NO[no]
    b0, b1 = pc.frames(c, integer=True)
    assert b0.min() >= 0 and b0.max() <= 255 and np.array_equal(b0, np.round(b0))
    scale = np.float32(1.0 / 255)
    ui, uf, upath = one_call(dfe, cuda, b0, b1, c.k, c.mh, c.mw, c.ratios, u8_scale=float(scale))
    gi, gf, gpath = one_call(dfe, cuda, b0 * scale, b1 * scale, c.k, c.mh, c.mw, c.ratios)
    assert upath == gpath == "prep_scales_kernel " + CASCADE[no]
    assert np.array_equal(ui, gi) and np.array_equal(uf, gf)
    rc, ey, ex = orc.x2yx_multi(c.mh, c.mw, c.ratios, ui)
    assert rc == 0 and np.array_equal(uf[0], ey.astype(np.float32)) and np.array_equal(uf[1], ex.astype(np.float32))
    assert len(np.unique(ui)) > 1                                  # (frames in 0 .. 1: a flat soft-min, but not one class everywhere)


# ---- 5. six scales through the graph path ----------------------------------------------------------------------------------------------
def test_six_scales_graph_replay_equals_direct_launches(dfe, cuda):
    """row 9 with option graphs on a ctx of a real stream (the pattern of test_multiscale_one_call_graph_replay_equals_direct_launches):
    direct, capture + launch, replay, replay -- every call gives the bits of the direct launches on the default stream."""
    c = pc.BY_NO[9]
    ref = pc.reference(9)
    f0, f1 = pc.frames(c)
    want_i, want_f, _ = one_call(dfe, cuda, f0, f1, c.k, c.mh, c.mw, c.ratios)      # default (legacy) stream: cannot be captured
    pc.assert_matches_oracle(want_i, want_f, ref, c)
    rr, n = _rr(c.ratios)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        ctx = dfe.get_ctx(0)                                        # (a new ctx: new stream)
        ctx.set_option("graphs", 1)
        t0, t1 = T(f0, cuda), T(f1, cuda)
        idx, flow = _outputs(cuda, c.H, c.W)
        side.synchronize()
        kernels = []
        for i in range(4):
            idx.fill_(FILL)
            flow.fill_(float(FILL))
            ctx.check(dfe.lib().dfe_multiscale_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), c.C, c.H, c.W, c.k, c.mh, c.mw, rr, n, flow.data_ptr(), idx.data_ptr()))
            ctx.synchronize()
            kernels.append(ctx.last_kernel())
            gi, gf = _collect(idx, flow, c.H, c.W)
            assert np.array_equal(gi, want_i) and np.array_equal(gf, want_f), "call %d" % i
        assert kernels[3] == "multiscale graph", kernels
        assert ctx.multiscale_last_path() == "prep_scales_kernel " + SLOW
        SEEN.add("last_kernel=" + kernels[3])
        ctx.set_option("graphs", 0)
    side.synchronize()


# ---- 6. prep_tiles_kernel off its tile grid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,Cc,ratios,byte", pc.PREP_CASES, ids=["%dx%d-C%d-%s" % (p[0], p[1], p[2], "_".join(map(str, p[3]))) for p in pc.PREP_CASES])
def test_prep_tiles_off_the_tile_grid_equals_per_scale_preparation(dfe, cuda, H, W, Cc, ratios, byte):
    """every scale from ONE read of the frames (prep_tiles_kernel, frames of 1.5 MP and more) == prep_scales_kernel, bit for bit on idx and
    flow: last tiles 8 wide and 8 high, a subset of the ratios with a gap, byte frames; the first shape also against the oracle chain."""
    ctx = dfe.get_ctx(0)
    c = pc.Case(0, ratios, pc.PREP_WIN, pc.PREP_WIN, pc.PREP_K, Cc, H, W, pc.PREP_MF, "prep", None)
    f0, f1 = pc.frames(c, integer=byte)
    kw = dict(u8_scale=float(np.float32(1.0 / 255))) if byte else {}
    res = {}
    for tiles in (1, 0):
        ctx.set_option("prep_tiles", tiles)
        gi, gf, path = one_call(dfe, cuda, f0, f1, c.k, c.mh, c.mw, c.ratios, **kw)
        assert path.split()[0] == ("prep_tiles_kernel" if tiles else "prep_scales_kernel"), path
        res[tiles] = (gi, gf)
    assert np.array_equal(res[1][0], res[0][0]) and np.array_equal(res[1][1], res[0][1])
    if (H, W, Cc, ratios) == (pc.PREP_ORACLE.H, pc.PREP_ORACLE.W, pc.PREP_ORACLE.C, pc.PREP_ORACLE.ratios):
        pc.assert_matches_oracle(res[1][0], res[1][1], pc.reference(0), pc.PREP_ORACLE)
    else:
        rc, ey, ex = orc.x2yx_multi(c.mh, c.mw, c.ratios, res[1][0])
        assert rc == 0 and np.array_equal(res[1][1][0], ey.astype(np.float32)) and np.array_equal(res[1][1][1], ex.astype(np.float32))
