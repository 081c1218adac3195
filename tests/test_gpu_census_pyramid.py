"""The census cost in the pyramid matcher on the device (csrc/census_pyramid.hip, multiscale.hip's census mode)
against its numpy restatement (tests/census_pyramid_ref.py): the staged per-scale volumes bit for bit; the one call bit for bit against
the device-staged composition dfe_census_pyramid_scale_volume_f32 -> dfe_softmin_f32 -> dfe_cascade_flow_f32, its byte entry, and the
route dfe_multiscale_last_path names; the one call against the reference chain under the pyramid's tie rule; the Python key; the
refusals; the exposure scene."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import census_pyramid_ref as cp
from tests import pyramid_cases as pc

pytestmark = pytest.mark.gpu

FILL, TAIL = -7, 64
DFE_E_ARG, DFE_E_SHAPE = -1, -2
FAST_VOLUME, STAGED_VOLUME = "census_pyramid_volume_kernel", "census_volume_kernel"
IDS = [c.id + "-a%d" % c.a for c in cp.CASES]


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _rr(ratios):
    from depth_estimation_amd._lib import ratios_array

    return ratios_array(ratios)


def _one_call(dfe, cuda, f0, f1, k, mh, mw, ratios, a, beta, byte=False):
    """dfe_multiscale_census_flow_pair_f32 / _u8 (the byte frames at an odd address) into guarded buffers: (idx, flow, last path)"""
    Cc, H, W = f0.shape
    ctx = dfe.get_ctx(0)
    lib = dfe.lib()
    rr, n = _rr(ratios)
    idx = torch.full((H * W + TAIL,), FILL, dtype=torch.int64, device=cuda)
    flow = torch.full((2 * H * W + TAIL,), float(FILL), device=cuda)
    if byte:
        m = f0.size
        buf = torch.zeros(2 * m + 2, dtype=torch.uint8, device=cuda)
        buf[1 : m + 1] = T(f0.astype(np.uint8).ravel(), cuda)
        buf[m + 2 :] = T(f1.astype(np.uint8).ravel(), cuda)
        ctx.check(lib.dfe_multiscale_census_flow_pair_u8(ctx.handle, buf.data_ptr() + 1, buf.data_ptr() + m + 2, Cc, H, W, k, mh, mw, rr, n, a, beta,
                                                         flow.data_ptr(), idx.data_ptr()))
    else:
        t0, t1 = T(f0, cuda), T(f1, cuda)
        ctx.check(lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), Cc, H, W, k, mh, mw, rr, n, a, beta, flow.data_ptr(),
                                                          idx.data_ptr()))
    ctx.synchronize()
    path = ctx.multiscale_last_path()
    gi, gf = idx.cpu().numpy(), flow.cpu().numpy()
    assert (gi[H * W :] == FILL).all() and (gf[2 * H * W :] == FILL).all(), "wrote behind an output"
    assert not (gi[: H * W] == FILL).any(), "left class ids unwritten"
    return gi[: H * W].reshape(H, W), gf[: 2 * H * W].reshape(2, H, W), path


def _staged(dfe, cuda, f0, f1, k, mh, mw, ratios, a, beta):
    """the staged composition of the public calls on the device: (volumes, idx, flow)"""
    import depth_estimation_amd as d

    Cc, H, W = f0.shape
    ctx = dfe.get_ctx(0)
    lib = dfe.lib()
    rr, n = _rr(ratios)
    t0, t1 = T(f0, cuda), T(f1, cuda)
    vols = [d.censusPyramidScaleVolume(t0, t1, r, k, mh, mw, a, beta) for r in ratios]
    probs = []
    for v in vols:
        p = torch.empty_like(v)
        ctx.check(lib.dfe_softmin_f32(ctx.handle, v.data_ptr(), v.numel() // (mh * mw), mh * mw, p.data_ptr()))
        probs.append(p)
    idx = torch.empty((H, W), dtype=torch.int64, device=cuda)
    flow = torch.empty((2, H, W), dtype=torch.float32, device=cuda)
    parr = (C.c_void_p * n)(*[p.data_ptr() for p in probs])
    ctx.check(lib.dfe_cascade_flow_f32(ctx.handle, parr, rr, n, H, W, mh, mw, idx.data_ptr(), None, flow[0].data_ptr(), flow[1].data_ptr()))
    ctx.synchronize()
    return [v.cpu().numpy() for v in vols], idx.cpu().numpy(), flow.cpu().numpy()


_dev = {}


def device_row(dfe, cuda, no):
    """row `no` through the one call and through the staged composition, once per process"""
    if no not in _dev:
        c = cp.BY_NO[no]
        f0, f1 = cp.frames(c)
        args = (c.k, c.mh, c.mw, c.ratios, c.a, cp.beta_of(c))
        _dev[no] = dict(one=_one_call(dfe, cuda, f0, f1, *args), staged=_staged(dfe, cuda, f0, f1, *args))
    return _dev[no]


# ---- 1. the staged per-scale volumes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cp.CASES, ids=IDS)
def test_scale_volumes_equal_the_reference_bit_for_bit(dfe, cuda, c):
    ref = cp.reference(c.no)
    vols = device_row(dfe, cuda, c.no)["staged"][0]
    for r, got, want in zip(c.ratios, vols, ref["vols"]):
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "row %d ratio %d: %d cells differ" % (c.no, r, int((got != want).sum()))


# ---- 2. the one call against the staged composition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cp.CASES, ids=IDS)
def test_one_call_equals_the_staged_composition_bit_for_bit(dfe, cuda, c):
    row = device_row(dfe, cuda, c.no)
    gi, gf, path = row["one"]
    _, si, sf = row["staged"]
    assert np.array_equal(gi, si), "row %d: %d class ids differ" % (c.no, int((gi != si).sum()))
    assert np.array_equal(gf.view(np.uint32), sf.view(np.uint32))
    words = path.split()
    assert len(words) == 3 and words[0] in ("prep_scales_kernel", "prep_tiles_kernel"), path
    fast = (c.mh, c.mw) == (8, 8)
    assert words[2] == (FAST_VOLUME if fast else STAGED_VOLUME), path
    if fast and all(r == 1 << s for s, r in enumerate(c.ratios)):
        assert words[1] == "cascade_px_kernel", path
    # the byte entry is the float entry on float(byte)
    f0, f1 = cp.frames(c)
    bi, bf, bpath = _one_call(dfe, cuda, f0, f1, c.k, c.mh, c.mw, c.ratios, c.a, cp.beta_of(c), byte=True)
    assert np.array_equal(bi, gi) and np.array_equal(bf.view(np.uint32), gf.view(np.uint32)) and bpath == path


def test_an_ssd_run_drops_the_census_word(dfe, cuda):
    c = cp.BY_NO[3]
    f0, f1 = cp.frames(c)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    assert len(device_row(dfe, cuda, 3)["one"][2].split()) == 3
    rr, n = _rr(c.ratios)
    t0, t1 = T(f0, cuda), T(f1, cuda)
    idx = torch.empty((c.H, c.W), dtype=torch.int64, device=cuda)
    ctx.check(lib.dfe_multiscale_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), c.C, c.H, c.W, c.k, c.mh, c.mw, rr, n, None, idx.data_ptr()))
    ctx.synchronize()
    assert ctx.multiscale_last_path() == "prep_scales_kernel cascade_px_kernel"


# ---- 3. the one call against the reference chain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cp.FIT, ids=[c.id + "-a%d" % c.a for c in cp.FIT])
def test_one_call_equals_the_reference_chain(dfe, cuda, c):
    """the device may differ from the reference only where its two best classes lie within 1e-5, on at most 2 % of the pixels; the decode
    of whatever class was taken is exact (pyramid_cases.assert_matches_oracle)"""
    gi, gf, _ = device_row(dfe, cuda, c.no)["one"]
    pc.assert_matches_oracle(gi, gf, cp.reference(c.no), c)


# ---- 4. Python ---------------------------------------------------------------------------------------------------------------------------
def _model(d, c):
    geo = dict(maxh=c.mh, maxw=c.mw, ratios=list(c.ratios), multiscale=True, hKernel=c.k, wKernel=c.k, hImg=c.H, wImg=c.W, output_extraction_method="max")
    return d.MultiscaleModel(geo)


@pytest.mark.parametrize("no", [3, 6])
def test_forward_flow_census_key(dfe, cuda, no):
    import depth_estimation_amd as d

    c = cp.BY_NO[no]
    f0, f1 = cp.frames(c)
    t0, t1 = T(f0, cuda), T(f1, cuda)
    m = _model(d, c)
    gi, gf, _ = device_row(dfe, cuda, no)["one"]
    one = m.forwardFlow([t0, t1], census=dict(agg=c.a))
    assert m.volumes is None
    staged = m.forwardFlow([t0, t1], census=dict(agg=c.a, beta=cp.beta_of(c)), one_call=False)
    assert len(m.volumes) == len(c.ratios)
    byte = m.forwardFlow([t0.to(torch.uint8), t1.to(torch.uint8)], census=dict(agg=c.a))
    assert set(one) == set(staged) == set(byte) == {"index", "confidences", "y", "x", "full", "full_confidences"}
    for key in one:
        assert torch.equal(one[key], staged[key]) and torch.equal(one[key], byte[key]), key
    assert np.array_equal(one["index"].cpu().numpy(), gi) and np.array_equal(one["full"].cpu().numpy(), gf)
    assert np.array_equal(one["y"].cpu().numpy(), gf[0].astype(np.int64)) and np.array_equal(one["x"].cpu().numpy(), gf[1].astype(np.int64))
    if c.a == 3:   # (the default box)
        assert torch.equal(m.forwardFlow([t0, t1], census=True)["index"], one["index"])
    # census=None: the SSD pyramid's bits, as from the C entry
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    rr, n = _rr(c.ratios)
    idx = torch.empty((c.H, c.W), dtype=torch.int64, device=cuda)
    flow = torch.empty((2, c.H, c.W), dtype=torch.float32, device=cuda)
    ctx.check(lib.dfe_multiscale_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), c.C, c.H, c.W, c.k, c.mh, c.mw, rr, n, flow.data_ptr(), idx.data_ptr()))
    for census in (None, False):
        plain = m.forwardFlow([t0, t1], census=census)
        assert torch.equal(plain["index"], idx) and torch.equal(plain["full"], flow)
    assert torch.equal(m.forwardFlow([t0, t1])["index"], idx)
    assert not torch.equal(idx, one["index"])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, mh, mw = 16, 24, 8, 8
    rr, n = _rr([1, 2])
    frames = {C_: (torch.rand((C_, H, W), device=cuda), torch.rand((C_, H, W), device=cuda)) for C_ in (3, 5)}
    bytes_ = tuple((f * 255).to(torch.uint8) for f in frames[3])
    good = dict(C=3, k=7, agg=3, beta=0.01)
    bad = [dict(agg=0), dict(agg=2), dict(agg=4), dict(agg=7), dict(agg=-3), dict(beta=0.0), dict(beta=-1.0), dict(beta=float("inf")), dict(beta=float("nan")),
           dict(k=1), dict(k=4), dict(k=6), dict(k=9), dict(C=5)]
    for change in bad:
        a = dict(good, **change)
        f0, f1 = frames[a["C"]]
        entries = {
            "dfe_multiscale_census_flow_pair_f32": lambda o: lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), a["C"], H, W, a["k"], mh, mw,
                                                                                                     rr, n, a["agg"], a["beta"], o[0].data_ptr(), o[1].data_ptr()),
            "dfe_census_pyramid_scale_volume_f32": lambda o: lib.dfe_census_pyramid_scale_volume_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), a["C"], H, W, 2, a["k"], mh, mw,
                                                                                                     a["agg"], a["beta"], o[2].data_ptr()),
        }
        if a["C"] == 3:
            entries["dfe_multiscale_census_flow_pair_u8"] = lambda o: lib.dfe_multiscale_census_flow_pair_u8(ctx.handle, bytes_[0].data_ptr(), bytes_[1].data_ptr(), 3, H, W,
                                                                                                           a["k"], mh, mw, rr, n, a["agg"], a["beta"], o[0].data_ptr(),
                                                                                                           o[1].data_ptr())
        for name, call in entries.items():
            o = (torch.full((2, H, W), float(FILL), device=cuda), torch.full((H, W), FILL, dtype=torch.int64, device=cuda),
                 torch.full((H // 2, W // 2, mh, mw), float(FILL), device=cuda))
            rc = call(o)
            torch.cuda.synchronize()
            assert rc == DFE_E_ARG, (name, change, rc, ctx.last_error())
            assert name in ctx.last_error(), (name, ctx.last_error())
            for t in o:
                assert bool((t == FILL).all()), name + " wrote into an output"
    # the pyramid's own rules still hold: a frame that is no multiple of a ratio, a window with no ring layout
    f0, f1 = frames[3]
    o = (torch.full((2, H, W), float(FILL), device=cuda), torch.full((H, W), FILL, dtype=torch.int64, device=cuda))
    r3, n3 = _rr([1, 5])
    assert lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), 3, H, W, 7, mh, mw, r3, n3, 3, 0.01, o[0].data_ptr(), o[1].data_ptr()) == DFE_E_SHAPE
    ratios, bh, bw, _ = pc.BAD_RINGS[0]
    rb, nb = _rr(ratios)
    assert lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), 3, H, W, 7, bh, bw, rb, nb, 3, 0.01, o[0].data_ptr(), o[1].data_ptr()) == DFE_E_SHAPE
    assert lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), 3, H, W, 7, mh, mw, rr, n, 3, 0.01, None, None) == DFE_E_ARG
    torch.cuda.synchronize()
    for t in o:
        assert bool((t == FILL).all())


# ---- 6. the exposure scene ------------------------------------------------------------------------------------------------------------------
def test_exposure_scene_on_the_device(dfe, cuda):
    """move (9, -11), seed 1: the device takes the reference's classes except inside its ties, so its wrong share is the reference's (1.04 %)
    up to the pixels that differ"""
    move, tol = cp.MOVES[2]
    s = cp.SCENE
    f0, f1 = cp.scene(1, move)
    ref = cp.scene_census(1, move)
    beta = cp.default_beta(s["C"], s["a"])
    gi, gf, path = _one_call(dfe, cuda, f0, f1, s["k"], s["win"], s["win"], list(s["ratios"]), s["a"], beta)
    assert path.split()[1:] == ["cascade_px_kernel", FAST_VOLUME], path
    c = pc.Case(0, list(s["ratios"]), s["win"], s["win"], s["k"], s["C"], s["H"], s["W"], 0, "the exposure scene", None)
    pc.assert_matches_oracle(gi, gf, dict(idx=ref["idx"], top2=pc._top2(ref["joined"]), middle=ref["middle"]), c)
    want = cp.share_wrong(ref["y"], ref["x"], move, tol)
    got = cp.share_wrong(gf[0], gf[1], move, tol)
    b = s["border"]
    differ = float((gi != ref["idx"])[b:-b, b:-b].mean())
    print("exposure scene, move %s: wrong share %.4f on the device, %.4f on the reference, %.4f of the pixels differ" % (move, got, want, differ))
    assert abs(got - want) <= differ
    assert got <= 0.05
