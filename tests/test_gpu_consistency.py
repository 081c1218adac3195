"""Forward-backward flow consistency on the device (include/dfe.h): dfe_flow_consistency_f32 against the float64
restatement of its definition (tests/consistency_ref64.py) on synthetic flows that hold every edge case, and the one-call
dfe_flow_depth_pair_fb_f32 / _u8 against the composition of the public calls it stands for, bit for bit, with every output pre-filled
with a sentinel."""
import numpy as np
import pytest
import torch

from tests.consistency_ref64 import consistency_ref
from tests.test_gpu_subpixel import translation, warped_pair

DFE_E_ARG, DFE_E_SHAPE = -1, -2
FILL = -7.0
H0, W0 = 24, 40
REGIONS = [(0, 0, H0, W0), (3, 5, 17, 29), (11, 19, 1, 1)]


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def consistency(dfe, cuda, fw, bw, region, tol, want_err=True):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    _, H, W = fw.shape
    tf, tb = _dev(cuda, fw), _dev(cuda, bw)
    mask, err = (torch.full((H, W), FILL, device=cuda) for _ in range(2))
    ctx.check(lib.dfe_flow_consistency_f32(ctx.handle, tf.data_ptr(), tb.data_ptr(), H, W, *region, tol, mask.data_ptr(), err.data_ptr() if want_err else None))
    torch.cuda.synchronize()
    return mask.cpu().numpy(), err.cpu().numpy()


# ---- 1. the operator on synthetic flows ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("region", REGIONS)
def test_integer_flows_exact(dfe, cuda, region):
    rng = np.random.default_rng(1)
    fw = rng.integers(-6, 7, size=(2, H0, W0)).astype(np.float32)
    bw = rng.integers(-6, 7, size=(2, H0, W0)).astype(np.float32)
    # a third of the pixels get the backward flow that answers them, so that the mask holds both values
    yy, xx = np.meshgrid(np.arange(H0), np.arange(W0), indexing="ij")
    ty, tx = yy + fw[0].astype(int), xx + fw[1].astype(int)
    ok = (ty >= 0) & (ty < H0) & (tx >= 0) & (tx < W0) & (rng.random((H0, W0)) < 0.33)
    bw[:, ty[ok], tx[ok]] = -fw[:, ok]
    if region[2:] == (1, 1):
        fw[:, region[0], region[1]] = 0   # the only way to stay inside a one-pixel region
        bw[:, region[0], region[1]] = (3, 0)
    for tol in (0.0, 3.0, 5.0):           # 3 and 5: residuals that meet the tolerance exactly (3-4-5 triangles)
        em, ee = consistency_ref(fw, bw, region, tol)
        m, e = consistency(dfe, cuda, fw, bw, region, tol)
        assert np.array_equal(_bits(m), _bits(em)), "mask: %d pixels differ" % np.count_nonzero(m != em)
        assert np.array_equal(np.isinf(e), np.isinf(ee)) and (e[np.isinf(e)] > 0).all()
        fin = np.isfinite(ee)
        assert np.abs(e[fin] - ee[fin]).max() <= 1e-4
        assert np.array_equal(np.rint(e[fin].astype(np.float64) ** 2), np.rint(ee[fin] ** 2)), "err^2 is the integer it should be"
        m2, e2 = consistency(dfe, cuda, fw, bw, region, tol, want_err=False)
        assert np.array_equal(_bits(m2), _bits(em)) and (e2 == FILL).all()
    if region[2:] != (1, 1):
        inR = np.zeros((H0, W0), bool)
        inR[region[0] : region[0] + region[2], region[1] : region[1] + region[3]] = True
        assert 0.05 < consistency_ref(fw, bw, region, 0.0)[0][inR].mean() < 0.9


def subpixel_flows(region, seed=2):
    """random flows in +-6 with, planted inside R, q on and just past every side of R, non-finite fw, and non-finite bw under zero and
    non-zero weight"""
    rng = np.random.default_rng(seed)
    fw = rng.uniform(-6, 6, size=(2, H0, W0)).astype(np.float32)
    bw = rng.uniform(-6, 6, size=(2, H0, W0)).astype(np.float32)
    y0, x0, Ho, Wo = region
    if (Ho, Wo) == (1, 1):
        fw[:, y0, x0] = 0
        return fw, bw
    ym, xm = y0 + Ho // 2, x0 + Wo // 2
    ylast, xlast = y0 + Ho - 1, x0 + Wo - 1
    plant = [  # (pixel, target q), each within 4 of its pixel
        ((ylast - 3, x0 + 1), (ylast, x0 + 2.5)), ((ylast - 3, x0 + 2), (ylast + 0.25, x0 + 2.5)),   # last row: on, just past
        ((y0 + 3, x0 + 3), (y0, x0 + 4.5)), ((y0 + 3, x0 + 4), (y0 - 0.25, x0 + 4.5)),               # first row
        ((y0 + 1, xlast - 3), (y0 + 2.5, xlast)), ((y0 + 2, xlast - 3), (y0 + 2.5, xlast + 0.25)),   # last column
        ((y0 + 5, x0 + 3), (y0 + 5.5, x0)), ((y0 + 6, x0 + 3), (y0 + 5.5, x0 - 0.25)),               # first column
        ((ylast - 2, xlast - 2), (ylast, xlast)),                                                    # the corner, integral
    ]
    for (py, px), (qy, qx) in plant:
        fw[:, py, px] = (qy - py, qx - px)
    fw[0, ym + 2, xm + 2] = np.nan
    fw[1, ym + 2, xm + 3] = np.inf
    fw[0, ym + 2, xm + 4] = -np.inf
    # non-finite bw: the pixel (ym - 2, xm - 3) is NaN; one pixel lands exactly on its neighbour (weight 0 for it), one beside it with weight
    bw[:, ym - 2, xm - 3] = np.nan
    fw[:, ym - 3, xm - 5] = (1.0, 3.0)      # q = (ym - 2, xm - 2): integral, the NaN next door is not a tap
    fw[:, ym - 3, xm - 6] = (1.0, 3.5)      # q = (ym - 2, xm - 2.5): the NaN has weight 1/2
    fw[:, ym - 3, xm - 7] = (0.5, 5.0)      # q = (ym - 2.5, xm - 2): rows ym - 3 and ym - 2 of column xm - 2, finite
    bw[1, ym - 1, xm - 6] = np.inf
    fw[:, ym - 4, xm - 6] = (3.0, 0.0)      # q lands on the Inf
    return fw, bw


@pytest.mark.gpu
@pytest.mark.parametrize("region", REGIONS)
def test_subpixel_flows_against_float64(dfe, cuda, region):
    fw, bw = subpixel_flows(region)
    tol = 4.0
    em, ee = consistency_ref(fw, bw, region, tol)
    m, e = consistency(dfe, cuda, fw, bw, region, tol)
    inR = np.zeros((H0, W0), bool)
    inR[region[0] : region[0] + region[2], region[1] : region[1] + region[3]] = True
    assert np.array_equal(np.isinf(e), np.isinf(ee)) and (e[np.isinf(e)] > 0).all(), "+Inf pixels differ"
    assert not e[~inR].any() and not m[~inR].any(), "border not zero"
    assert not np.isnan(e).any() and np.isin(m, (0.0, 1.0)).all()
    fin = np.isfinite(ee)
    d = np.abs(e[fin].astype(np.float64) - ee[fin])
    print("region %s: %d finite residuals, max |err - err64| = %.3g, max err = %.3g" % (region, fin.sum(), d.max() if d.size else 0, ee[fin].max() if d.size else 0))
    assert d.size == 0 or (d.max() <= 1e-4 and ee[fin].max() < 18)
    sure = ~(np.abs(ee - tol) <= 1e-3)
    assert np.count_nonzero(~sure) <= 0.01 * sure.size, "%d of %d pixels excluded" % (np.count_nonzero(~sure), sure.size)
    assert np.array_equal(m[sure], em[sure]), "mask: %d pixels differ" % np.count_nonzero(m[sure] != em[sure])
    if region[2:] != (1, 1):
        assert 0.05 < em[inR].mean() < 0.95 and np.isinf(ee).sum() >= 12


@pytest.mark.gpu
def test_argument_errors_launch_nothing(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W = H0, W0
    fl = torch.zeros((2, H, W), device=cuda)
    mask, err = (torch.full((H, W), FILL, device=cuda) for _ in range(2))
    f, mp, ep = fl.data_ptr(), mask.data_ptr(), err.data_ptr()
    fn = lib.dfe_flow_consistency_f32
    for reg in ((0, 0, H + 1, W), (0, 0, H, W + 1), (-1, 0, H, W), (0, -1, H, W), (1, 0, H, W), (0, 1, H, W), (0, 0, 0, W), (0, 0, H, 0), (0, 0, H, -3),
                (2**31 - 1, 0, 1, 1), (0, 0, 1, 2**31 - 1)):
        assert fn(ctx.handle, f, f, H, W, *reg, 1.0, mp, ep) == DFE_E_SHAPE, reg
        assert lib.dfe_last_error(ctx.handle).startswith(b"dfe_flow_consistency_f32: region")
    assert fn(ctx.handle, f, f, 0, W, 0, 0, 1, 1, 1.0, mp, ep) == DFE_E_SHAPE
    for tol in (-1e-3, float("nan"), -float("inf")):
        assert fn(ctx.handle, f, f, H, W, 0, 0, H, W, tol, mp, ep) == DFE_E_ARG, tol
        assert b"tol" in lib.dfe_last_error(ctx.handle)
    assert fn(ctx.handle, None, f, H, W, 0, 0, H, W, 1.0, mp, ep) == DFE_E_ARG
    assert fn(ctx.handle, f, None, H, W, 0, 0, H, W, 1.0, mp, ep) == DFE_E_ARG
    assert fn(ctx.handle, f, f, H, W, 0, 0, H, W, 1.0, None, ep) == DFE_E_ARG
    assert fn(None, f, f, H, W, 0, 0, H, W, 1.0, mp, ep) == DFE_E_ARG
    # the one-call: its own arguments, and the step's behind them
    Hf, Wf, k, win = 56, 88, 7, 33
    t = torch.zeros((3, Hf, Wf), device=cuda)
    fl2, bw2 = (torch.full((2, Hf, Wf), FILL, device=cuda) for _ in range(2))
    o = [torch.full((Hf, Wf), FILL, device=cuda) for _ in range(5)]
    p, op = t.data_ptr(), [x.data_ptr() for x in o]
    fb = lib.dfe_flow_depth_pair_fb_f32
    args = lambda **kw: (ctx.handle, kw.get("I0", p), p, 3, kw.get("H", Hf), Wf, k, win, win, 1.0, 1.0, 0.21, 0, kw.get("tol", 1.0), 0,
                         kw.get("flow", fl2.data_ptr()), op[0], op[1], kw.get("conf", op[2]), bw2.data_ptr(), kw.get("mask", op[3]), op[4])
    assert fb(*args(tol=-1.0)) == DFE_E_ARG and fb(*args(tol=float("nan"))) == DFE_E_ARG
    assert fb(*args(mask=None)) == DFE_E_ARG
    assert fb(*args(I0=None)) == DFE_E_ARG and fb(*args(flow=None)) == DFE_E_ARG and fb(*args(conf=None)) == DFE_E_ARG
    assert fb(*args(H=20)) == DFE_E_SHAPE
    b = torch.zeros(3 * Hf * Wf, dtype=torch.uint8, device=cuda).data_ptr()
    fb8 = lib.dfe_flow_depth_pair_fb_u8
    a8 = lambda **kw: (ctx.handle, kw.get("I0", b), b, 3, kw.get("H", Hf), Wf, k, win, win, 1.0, 1.0, 0.21, kw.get("scale", 1.0), 0, kw.get("tol", 1.0), 0,
                       fl2.data_ptr(), op[0], op[1], op[2], bw2.data_ptr(), kw.get("mask", op[3]), op[4])
    assert fb8(*a8(tol=-1.0)) == DFE_E_ARG and fb8(*a8(mask=None)) == DFE_E_ARG and fb8(*a8(I0=None)) == DFE_E_ARG and fb8(*a8(scale=0.0)) == DFE_E_ARG
    assert fb8(*a8(H=20)) == DFE_E_SHAPE
    torch.cuda.synchronize()
    for x in (mask, err, fl2, bw2, *o):
        assert (x == FILL).all(), "a refused call wrote an output"
    with pytest.raises(dfe.DfeError):
        dfe.flowConsistency(fl, fl, -1.0)
    with pytest.raises(ValueError):
        dfe.flowConsistency(fl, fl[:, :5], 1.0)


# ---- 2. the one-call against the composition of the public calls -----------------------------------------------------------------------
KEYS = ("flow", "scores", "depth", "depth_conf", "flow_bw", "mask", "err")


def _frames(case):
    C_, H, W = case["shape"]
    f0, f1 = warped_pair(H, W, translation(1.6, -2.3), C_=C_, seed=21)
    if case.get("half"):
        f0 = f0.copy()
        f0[1, 30, 40] = 0.5      # one value that is not a byte: the device-side gate sends both directions to the float sweep
    return f0, f1


def _step(dfe, cuda, t0, t1, case, sub, outs):
    """the public pair step (its _subpixel_ / _u8 form as the case says) into outs = (flow, scores, depth, conf)"""
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = case["shape"]
    k, hWin, wWin = case["k"], case["win"][0], case["win"][1]
    foe = case["foe"]
    ptrs = [o.data_ptr() for o in outs]
    if case.get("u8"):
        fn = lib.dfe_flow_depth_pair_subpixel_u8 if sub else lib.dfe_flow_depth_pair_u8
        ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, k, hWin, wWin, foe[0], foe[1], 0.21, 1.0, *ptrs))
    else:
        fn = lib.dfe_flow_depth_pair_subpixel_f32 if sub else lib.dfe_flow_depth_pair_f32
        ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, k, hWin, wWin, foe[0], foe[1], 0.21, *ptrs))


def _new(cuda, H, W):
    return [torch.full((2, H, W), FILL, device=cuda)] + [torch.full((H, W), FILL, device=cuda) for _ in range(3)]


def composed(dfe, cuda, t0, t1, case, sub, tol):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = case["shape"]
    k, hWin, wWin = case["k"], case["win"][0], case["win"][1]
    Ho, Wo = H - k + 1 - hWin + 1, W - k + 1 - wWin + 1
    fwd, bwd = _new(cuda, H, W), _new(cuda, H, W)
    _step(dfe, cuda, t0, t1, case, sub, fwd)
    _step(dfe, cuda, t1, t0, case, sub, bwd)
    mask, err = (torch.full((H, W), FILL, device=cuda) for _ in range(2))
    ctx.check(lib.dfe_flow_consistency_f32(ctx.handle, fwd[0].data_ptr(), bwd[0].data_ptr(), H, W, (H - Ho) // 2, (W - Wo) // 2, Ho, Wo, tol, mask.data_ptr(),
                                           err.data_ptr()))
    torch.cuda.synchronize()
    return dict(zip(KEYS, [x.cpu().numpy() for x in (*fwd, bwd[0], mask, err)]))


def one_call(dfe, cuda, t0, t1, case, sub, tol, gate=0, with_bw=True, with_err=True):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = case["shape"]
    k, hWin, wWin = case["k"], case["win"][0], case["win"][1]
    foe = case["foe"]
    outs = _new(cuda, H, W)
    bw = torch.full((2, H, W), FILL, device=cuda)
    mask, err = (torch.full((H, W), FILL, device=cuda) for _ in range(2))
    tail = (int(sub), tol, gate, *[o.data_ptr() for o in outs], bw.data_ptr() if with_bw else None, mask.data_ptr(), err.data_ptr() if with_err else None)
    if case.get("u8"):
        ctx.check(lib.dfe_flow_depth_pair_fb_u8(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, k, hWin, wWin, foe[0], foe[1], 0.21, 1.0, *tail))
    else:
        ctx.check(lib.dfe_flow_depth_pair_fb_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, k, hWin, wWin, foe[0], foe[1], 0.21, *tail))
    took_i8 = ctx.flow_last_path_i8()
    torch.cuda.synchronize()
    return dict(zip(KEYS, [x.cpu().numpy() for x in (*outs, bw, mask, err)])), took_i8


CASES = {
    "i8": dict(shape=(3, 56, 88), k=7, win=(33, 33), foe=(40.0, 30.0), i8=True),
    "half": dict(shape=(3, 56, 88), k=7, win=(33, 33), foe=(40.0, 30.0), half=True, i8=False),
    "volume": dict(shape=(3, 56, 88), k=7, win=(33, 33), foe=(40.0, 30.0), novol=0),
    "u8": dict(shape=(3, 56, 88), k=7, win=(33, 33), foe=(40.0, 30.0), u8=True, i8=True),
    "k5": dict(shape=(1, 40, 48), k=5, win=(9, 9), foe=(20.0, 25.0)),
    "even": dict(shape=(3, 48, 64), k=7, win=(16, 16), foe=(30.0, 20.0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_one_call_equals_the_composition(dfe, cuda, name, sub):
    case = CASES[name]
    ctx = dfe.get_ctx(0)
    f0, f1 = _frames(case)
    C_, H, W = case["shape"]
    if case.get("u8"):
        t0, t1 = _dev(cuda, f0.astype(np.uint8)), _dev(cuda, f1.astype(np.uint8))
    else:
        t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    if "novol" in case:
        ctx.set_option("cv_novol", case["novol"])
    tol = 1.0
    want = composed(dfe, cuda, t0, t1, case, sub, tol)
    got, took_i8 = one_call(dfe, cuda, t0, t1, case, sub, tol)
    if "i8" in case:   # (dfe_flow_last_path speaks of the volume-free route only: the cases that take it say which kernel they expect)
        assert took_i8 == case["i8"], "the step took %s" % ("the int8 kernel" if took_i8 else "the float sweep")
    for key in KEYS:
        assert not (got[key] == FILL).any(), "%s: an element was not written" % key
        assert np.array_equal(_bits(got[key]), _bits(want[key])), "%s: %d elements differ" % (key, np.count_nonzero(_bits(got[key]) != _bits(want[key])))
    k, (hWin, wWin) = case["k"], case["win"]
    Ho, Wo = H - k + 1 - hWin + 1, W - k + 1 - wWin + 1
    inner = want["mask"][(H - Ho) // 2 : (H - Ho) // 2 + Ho, (W - Wo) // 2 : (W - Wo) // 2 + Wo]
    assert 0.5 < inner.mean() < 1.0, "a translation: most of R is consistent, the strip that leaves R is not"
    # the backward flow in the ctx's own scratch, no err
    got2, _ = one_call(dfe, cuda, t0, t1, case, sub, tol, with_bw=False, with_err=False)
    for key in ("flow", "scores", "depth", "depth_conf", "mask"):
        assert np.array_equal(_bits(got2[key]), _bits(want[key])), key
    assert (got2["flow_bw"] == FILL).all() and (got2["err"] == FILL).all()
    # a plain step behind the one-call still gives its bytes (verdict words, scratch)
    plain = _new(cuda, H, W)
    _step(dfe, cuda, t0, t1, case, sub, plain)
    assert "i8" not in case or ctx.flow_last_path_i8() == case["i8"]
    torch.cuda.synchronize()
    for key, x in zip(KEYS, plain):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(want[key])), "plain step after the one-call: %s" % key


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["i8", "k5"])
def test_gate_multiplies_scores_and_confidence(dfe, cuda, name):
    case = CASES[name]
    f0, f1 = _frames(case)
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    free, _ = one_call(dfe, cuda, t0, t1, case, 1, 0.5)
    gated, _ = one_call(dfe, cuda, t0, t1, case, 1, 0.5, gate=1)
    for key in ("flow", "depth", "flow_bw", "mask", "err"):
        assert np.array_equal(_bits(gated[key]), _bits(free[key])), key
    C_, H, W = case["shape"]
    Ho, Wo = H - case["k"] + 1 - case["win"][0] + 1, W - case["k"] + 1 - case["win"][1] + 1
    inR = np.zeros((H, W), bool)
    inR[(H - Ho) // 2 : (H - Ho) // 2 + Ho, (W - Wo) // 2 : (W - Wo) // 2 + Wo] = True
    for key in ("scores", "depth_conf"):   # inside R; the border keeps what the step wrote (score 0, confidence 1 of a zero flow)
        assert np.array_equal(_bits(gated[key]), _bits(np.where(inR, free[key] * free["mask"], free[key]))), key
    assert (free["scores"] * (1 - free["mask"])).any() and (free["depth_conf"] * (1 - free["mask"])).any(), "the gate had nothing to remove"
    # scores and depth_conf NULL: the gate has nothing to multiply
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    flow = torch.full((2, H, W), FILL, device=cuda)
    mask = torch.full((H, W), FILL, device=cuda)
    ctx.check(lib.dfe_flow_depth_pair_fb_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C_, H, W, case["k"], *case["win"], *case["foe"], 0.21, 1, 0.5, 1,
                                             flow.data_ptr(), None, None, None, None, mask.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(flow.cpu().numpy()), _bits(free["flow"])) and np.array_equal(_bits(mask.cpu().numpy()), _bits(free["mask"]))


# ---- 3. Python -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_flow_depth_pair_consistency(dfe, cuda):
    case = CASES["i8"]
    f0, f1 = _frames(case)
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    k, win, foe = case["k"], case["win"][0], case["foe"]
    for sub in (False, True):
        want, _ = one_call(dfe, cuda, t0, t1, case, int(sub), 1.0)
        plain = dfe.flowDepthPair(t0, t1, k, win, win, foe, subpixel=sub, consistency=None)
        assert sorted(plain) == ["depth", "depth_conf", "flow", "scores"]
        got = dfe.flowDepthPair(t0, t1, k, win, win, foe, subpixel=sub, consistency=1.0)
        assert sorted(got) == sorted(["depth", "depth_conf", "flow", "scores", "flow_bw", "consistent", "consistency_err"])
        for key, wk in (("flow", "flow"), ("scores", "scores"), ("depth", "depth"), ("depth_conf", "depth_conf"), ("flow_bw", "flow_bw"), ("consistent", "mask"),
                        ("consistency_err", "err")):
            assert np.array_equal(_bits(got[key].cpu().numpy()), _bits(want[wk])), (sub, key)
        for key in plain:
            assert np.array_equal(_bits(plain[key].cpu().numpy()), _bits(want[key])), (sub, key)
    g8 = dfe.flowDepthPair(_dev(cuda, f0.astype(np.uint8)), _dev(cuda, f1.astype(np.uint8)), k, win, win, foe, consistency=1.0, gate=True)
    w8, _ = one_call(dfe, cuda, t0, t1, case, 0, 1.0, gate=1)
    for key, wk in (("scores", "scores"), ("depth_conf", "depth_conf"), ("consistent", "mask"), ("flow_bw", "flow_bw")):
        assert np.array_equal(_bits(g8[key].cpu().numpy()), _bits(w8[wk])), key


@pytest.mark.gpu
def test_flow_consistency_on_a_pyramid_flow(dfe, cuda):
    H, W, k, win, ratios = 96, 128, 7, 8, (1, 2, 4)
    f0, f1 = warped_pair(H, W, translation(2.3, -4.7), seed=22)
    geo = dict(maxh=win, maxw=win, ratios=list(ratios), multiscale=True, hKernel=k, wKernel=k, hImg=H, wImg=W, output_extraction_method="max")
    model = dfe.getModelMultiscale(geo)
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    fw = model.forwardFlow([t0, t1], True, subpixel=True)["full"]
    bw = model.forwardFlow([t1, t0], True, subpixel=True)["full"]
    assert tuple(fw.shape) == (2, H, W)
    tol = 1.2   # (away from 1 and 1.5: the pyramid's flows are whole cells of a scale where the parabola gives 0, so residuals pile up on integers and halves)
    mask, err = dfe.flowConsistency(fw, bw, tol)
    em, ee = consistency_ref(fw.cpu().numpy(), bw.cpu().numpy(), (0, 0, H, W), tol)
    m, e = mask.cpu().numpy(), err.cpu().numpy()
    assert np.array_equal(np.isinf(e), np.isinf(ee))
    fin = np.isfinite(ee)
    assert np.abs(e[fin] - ee[fin]).max() <= 1e-4
    sure = ~(np.abs(ee - tol) <= 1e-3)
    assert np.count_nonzero(~sure) <= 0.01 * sure.size and np.array_equal(m[sure], em[sure])
    assert em.mean() > 0.5, "a translation: most of the frame is consistent"
    # a region through the Python call
    m2, e2 = dfe.flowConsistency(fw, bw, tol, region=(10, 12, 50, 60))
    em2, ee2 = consistency_ref(fw.cpu().numpy(), bw.cpu().numpy(), (10, 12, 50, 60), tol)
    s2 = ~(np.abs(ee2 - tol) <= 1e-3)
    assert np.array_equal(m2.cpu().numpy()[s2], em2[s2]) and np.array_equal(np.isinf(e2.cpu().numpy()), np.isinf(ee2))
