"""GPU suite (-m gpu), part 9: the batched LDS-tiled convolution, conv_batch_kernel<KW, NT, TANH, NARROW> (csrc/filters.hip), at EVERY
planes-per-thread form the library builds -- KW in {3, 5, 7} x NT in {1, 2, 4, 5, 8, 10} and KW = 17 x NT in {2, 4, 8}, each with and
without the tanh epilogue and in both tile shapes (128 x 8, 64 x 16).  The launcher's own rule gives small frames NT = 1 (2 at 17 wide),
so option conv_nt forces the form and ctx.last_kernel() proves which instantiation ran: nothing falls back unnoticed.

Two references, both independent of the kernel:
  * orc.spatial_convolution, the CPU oracle: bias, then (input plane, ky, kx), multiply and add rounded separately -- the kernel's order,
    compared with np.array_equal;
  * ref64.spatial_convolution64, float64 numpy from the definition: |g - r64| <= (T + 1) 2^-24 (sum|w||x| + |b|), T = nIn kH kW -- the
    standard bound of T + 1 sequentially added, separately rounded terms (the oracle itself uses at most 0.19 of it).
Outputs are written into a buffer pre-filled with -7 that is 64 floats longer than the result: the tail must keep its -7, the inside
must lose every one."""
import math

import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import ref64
from tests import refpath as rp
from tests.test_gpu_multiscale_radial import _assert_matches_oracle, _stack_dicts
from tests.test_gpu_single_scale import _pair, _same

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TANH_ATOL = 2e-7            # the device's tanhf against float64 tanh (test_filter_stack_and_single_scale_model's tolerance)
FILL, TAIL = -7.0, 64
BUILT = [(kw, nt) for kw in (3, 5, 7) for nt in (1, 2, 4, 5, 8, 10)] + [(17, nt) for nt in (2, 4, 8)]
SEEN = set()                # every last_kernel name this module saw (printed when the module is done; -s shows it)


@pytest.fixture(scope="module", autouse=True)
def _report_names():
    yield
    print("\nlast_kernel names seen by test_gpu_conv_batch: " + " ".join(sorted(SEEN)))


def T(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def kernel_name(kW, nt, tanh, narrow):
    """the spelling in the comment above launch_conv_batch"""
    return "conv_batch_kernel<%d,%d>%s%s" % (kW, nt, "+tanh" if tanh else "", "+narrow" if narrow else "")


def auto_nt(ctx, ncu, nOut, kH, kW, Ho, Wo):
    """conv_batch_try's rule, restated: walk {10, 8, 5, 4, 2, 1}, keep the last candidate that divides nOut (and is built for kW), stop
    early once tiles * (nOut / nt) >= 2 * ncu.  Returns (nt, narrow)."""
    o = ctx.get_option("conv_narrow")
    narrow = (kW >= 9 and kH >= 9) if o < 0 else o != 0
    tiles = math.ceil(Wo / (64 if narrow else 128)) * math.ceil(Ho / (16 if narrow else 8))
    nt = 0
    for c in (10, 8, 5, 4, 2, 1):
        if nOut % c or (c == 10 and ctx.get_option("conv_nt10") == 0) or (kW == 17 and c in (10, 5, 1)):
            continue
        nt = c
        if tiles * (nOut // nt) >= 2 * ncu:
            break
    return nt, narrow


def run_conv(dfe, ctx, tx, tw, tb, tanh):
    """dfe_spatial_convolution[_tanh]_f32 through the raw ABI (tb None: bias = NULL) into a guarded buffer; returns (numpy result, kernel name)"""
    nOut, nIn, kH, kW = tw.shape
    _, H, W = tx.shape
    n = nOut * (H - kH + 1) * (W - kW + 1)
    buf = torch.full((n + TAIL,), FILL, device=tx.device)
    fn = dfe.lib().dfe_spatial_convolution_tanh_f32 if tanh else dfe.lib().dfe_spatial_convolution_f32
    ctx.check(fn(ctx.handle, tx.data_ptr(), tw.data_ptr(), tb.data_ptr() if tb is not None else None, nIn, nOut, H, W, kH, kW, buf.data_ptr()))
    name = ctx.last_kernel()
    SEEN.add(name)
    g = buf.cpu().numpy()
    assert (g[n:] == np.float32(FILL)).all(), "wrote behind the output"
    assert not (g[:n] == np.float32(FILL)).any(), "left output elements unwritten"
    return g[:n].reshape(nOut, H - kH + 1, W - kW + 1), name


def device_tanh(dfe, ctx, a, cuda):
    t = T(a, cuda)
    o = torch.empty_like(t)
    ctx.check(dfe.lib().dfe_tanh_f32(ctx.handle, t.data_ptr(), t.numel(), o.data_ptr()))
    return o.cpu().numpy()


def make_case(rng, nIn, nOut, kH, kW, Ho, Wo):
    """standard_normal frame, weights / sqrt(fan-in) (as test_convolution_mfma_equals_fma_oracle), and both references with and without bias"""
    x = rng.standard_normal((nIn, Ho + kH - 1, Wo + kW - 1)).astype(np.float32)
    w = (rng.standard_normal((nOut, nIn, kH, kW)) / np.sqrt(nIn * kH * kW)).astype(np.float32)
    b = rng.standard_normal(nOut).astype(np.float32)
    v64, m64 = ref64.spatial_convolution64(x, w)
    b64 = b.astype(np.float64)[:, None, None]
    refs = {True: (orc.spatial_convolution(x, w, b), v64 + b64, m64 + np.abs(b64)), False: (orc.spatial_convolution(x, w, None), v64, m64)}
    return x, w, b, refs


def check(g, ref, v64, m64, T_, what):
    assert np.array_equal(g, ref), what
    err, bound = np.abs(g.astype(np.float64) - v64), (T_ + 1) * U * m64
    assert (err <= bound).all(), (what, float((err / bound).max()))


def shapes_for(kW):
    """(Ho, Wo, nIn, kH): the smallest output sizes that reach each branch of the kernel"""
    s = [(19, 165, 3, kW),      # ragged both ways in both tile shapes (2 x 3 tiles of 128 x 8, 3 x 2 of 64 x 16): the last tile's staging clamps rows and columns
         (8, 128, 4, kW),       # exactly one 128 x 8 tile, no clamp taken
         (16, 64, 4, kW),       # the same for the narrow shape
         (1, 1, 1, kW),         # a frame no larger than the kernel
         (3, 5, 2, kW),         # one full strip plus one pixel
         (9, 2, 2, kW)]         # a strip cut at 2
    s += [(11, 140, 3, kH) for kH in (1, 3, 9) if kH != kW]   # kH != kW; kH = 1: 8 staged rows per plane, where stage's row / plane carry wraps most often
    return s


@pytest.mark.parametrize("kW,nt", BUILT)
def test_every_instantiation_by_name_against_oracle_and_float64(dfe, cuda, kW, nt):
    """(a) conv_nt = nt on layers of nt and 3 nt planes (one group, several groups), both tile shapes, tanh off and on, bias present and
    NULL: the kernel named is exactly <kW, nt> with the right suffixes; bit-equal to the oracle and inside the float64 bound; with tanh,
    bit-equal to dfe_tanh_f32 of the tanh-free output and within 2e-7 + the bound of float64 tanh (slope <= 1 carries the bound through)."""
    ctx = dfe.get_ctx(0)
    rng = np.random.default_rng(1000 * kW + nt)
    for Ho, Wo, nIn, kH in shapes_for(kW):
        x, w, b, refs = make_case(rng, nIn, 3 * nt, kH, kW, Ho, Wo)
        tx = T(x, cuda)
        T_ = nIn * kH * kW
        for nOut in (nt, 3 * nt):
            tw, tb = T(w[:nOut], cuda), T(b[:nOut], cuda)
            for bias in (True, False):
                ref, v64, m64 = (r[:nOut] for r in refs[bias])
                tanh_of_plain = None
                narrows = (0, 1) + ((-1,) if kH != kW else ())        # -1: the launcher's own rule, narrow for kernels of 9 x 9 and larger
                for narrow in narrows:
                    want_narrow = (kW >= 9 and kH >= 9) if narrow < 0 else bool(narrow)
                    with ctx.options(conv_nt=nt, conv_narrow=narrow):
                        what = (Ho, Wo, nIn, nOut, kH, kW, "bias" if bias else "NULL", "narrow=%d" % narrow)
                        g, name = run_conv(dfe, ctx, tx, tw, tb if bias else None, False)
                        assert name == kernel_name(kW, nt, False, want_narrow), (name, what)
                        check(g, ref, v64, m64, T_, what)
                        gt, name = run_conv(dfe, ctx, tx, tw, tb if bias else None, True)
                        assert name == kernel_name(kW, nt, True, want_narrow), (name, what)
                    if tanh_of_plain is None:
                        tanh_of_plain = device_tanh(dfe, ctx, g, cuda)
                    assert np.array_equal(gt, tanh_of_plain), what
                    err = np.abs(gt.astype(np.float64) - np.tanh(v64))
                    assert (err <= TANH_ATOL + (T_ + 1) * U * m64).all(), (what, float(err.max()))
    assert ctx.get_option("conv_nt") == -1 and ctx.get_option("conv_narrow") == -1


def test_forced_count_leaves_layers_it_does_not_fit_to_the_rule(dfe, cuda):
    """conv_nt = n applies only where nOut % n == 0 and <kW, n> is built: other layers keep the automatic choice (a stack of 4, 4 and 10
    planes runs under one setting), and conv_nt10 = 0 keeps its meaning there."""
    ctx = dfe.get_ctx(0)
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    rng = np.random.default_rng(5)
    for kW, nOut, forced in [(5, 4, 10), (5, 10, 4), (5, 6, 4), (17, 10, 5), (17, 8, 1), (5, 10, 0), (3, 7, 7)]:
        Ho, Wo, nIn = 19, 165, 3
        x, w, b, refs = make_case(rng, nIn, nOut, kW, kW, Ho, Wo)
        for nt10 in (-1, 0):
            with ctx.options(conv_nt=forced, conv_nt10=nt10):
                nt, narrow = auto_nt(ctx, ncu, nOut, kW, kW, Ho, Wo)
                g, name = run_conv(dfe, ctx, T(x, cuda), T(w, cuda), T(b, cuda), False)
            assert nt != forced and name == kernel_name(kW, nt, False, narrow), (name, kW, nOut, forced)
            check(g, *refs[True], nIn * kW * kW, (kW, nOut, forced))
    # forced 10 is taken whatever conv_nt10 says: that switch belongs to the automatic rule
    x, w, b, refs = make_case(rng, 3, 10, 5, 5, 19, 165)
    with ctx.options(conv_nt=10, conv_nt10=0):
        g, name = run_conv(dfe, ctx, T(x, cuda), T(w, cuda), T(b, cuda), False)
    assert name == kernel_name(5, 10, False, False)
    check(g, *refs[True], 75, "forced 10")


def test_lds_limit_is_a_clean_fallback(dfe, cuda):
    """(b) 5 x 5, 128 x 8 tiles: one plane's tile is 12 x 136 x 4 = 6528 B.  10 input planes (65 280 B) are the largest request that fits
    64 KB and run conv_batch_kernel; 11 (71 808 B) run the direct kernels -- conv_kernel, conv_layer_kernel behind the tanh entry -- with
    the same bits.  conv_batch = 0 sends any shape to conv_kernel."""
    ctx = dfe.get_ctx(0)
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    rng = np.random.default_rng(11)
    Ho, Wo, nOut = 12, 136, 4
    for nIn, fits in ((10, True), (11, False)):
        x, w, b, refs = make_case(rng, nIn, nOut, 5, 5, Ho, Wo)
        tx, tw, tb = T(x, cuda), T(w, cuda), T(b, cuda)
        with ctx.options(conv_narrow=0):
            nt, _ = auto_nt(ctx, ncu, nOut, 5, 5, Ho, Wo)
            g, name = run_conv(dfe, ctx, tx, tw, tb, False)
            gt, name_t = run_conv(dfe, ctx, tx, tw, tb, True)
        assert name == (kernel_name(5, nt, False, False) if fits else "conv_kernel"), name
        assert name_t == (kernel_name(5, nt, True, False) if fits else "conv_layer_kernel"), name_t
        check(g, *refs[True], nIn * 25, nIn)
        assert np.array_equal(gt, device_tanh(dfe, ctx, g, cuda))
    for kW, (Ho, Wo, nIn, kH) in [(5, shapes_for(5)[0]), (17, shapes_for(17)[-1]), (3, shapes_for(3)[4])]:
        x, w, b, refs = make_case(rng, nIn, 8, kH, kW, Ho, Wo)
        with ctx.options(conv_batch=0):
            g, name = run_conv(dfe, ctx, T(x, cuda), T(w, cuda), T(b, cuda), False)
            g0, name0 = run_conv(dfe, ctx, T(x, cuda), T(w, cuda), None, False)
        assert name == "conv_kernel" and name0 == "conv_kernel"
        check(g, *refs[True], nIn * kH * kW, (kW, "conv_batch=0"))
        check(g0, *refs[False], nIn * kH * kW, (kW, "conv_batch=0, NULL"))


@pytest.mark.parametrize("nIn,nOut,want", [(3, 4, 4), (4, 10, 10)])
def test_automatic_rule_reaches_the_benchmark_forms(dfe, cuda, nIn, nOut, want):
    """(c) the two layers of the vga-pyramid-learned workload, 3 -> 4 and 4 -> 10 planes of 5 x 5, on the smallest one-tile-column frame
    (Wo = 128) for which the launcher's OWN rule takes NT = 4 / NT = 10 on the device at hand (256 CUs: 512 tile rows, Ho = 4096): the
    name, and the first 3, the last 3 and 3 middle tile rows against the oracle (bit for bit) and the float64 bound."""
    ctx = dfe.get_ctx(0)
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    kH = kW = 5
    Wo = 128
    rows = next(r for r in range(1, 1 << 16) if auto_nt(ctx, ncu, nOut, kH, kW, 8 * r, Wo)[0] == want)
    assert rows == 2 * ncu and auto_nt(ctx, ncu, nOut, kH, kW, 8 * (rows - 1), Wo)[0] != want
    Ho = 8 * rows
    rng = np.random.default_rng(nOut)
    x = rng.standard_normal((nIn, Ho + kH - 1, Wo + kW - 1)).astype(np.float32)
    w = (rng.standard_normal((nOut, nIn, kH, kW)) / np.sqrt(nIn * kH * kW)).astype(np.float32)
    b = rng.standard_normal(nOut).astype(np.float32)
    g, name = run_conv(dfe, ctx, T(x, cuda), T(w, cuda), T(b, cuda), False)
    assert name == kernel_name(kW, want, False, False), name
    for r0 in (0, rows // 2 - 1, rows - 3):
        y0, y1 = 8 * r0, 8 * (r0 + 3)
        xs = x[:, y0 : y1 + kH - 1]                             # a valid convolution is local: these input rows make output rows y0 .. y1
        v64, m64 = ref64.spatial_convolution64(xs, w, b)
        check(g[:, y0:y1], orc.spatial_convolution(xs, w, b), v64, m64, nIn * kH * kW, (r0, name))
    if want == 10:
        # a forced count that does not fit (3) leaves the rule alone, and conv_nt10 = 0 keeps its meaning there: two groups of 5
        with ctx.options(conv_nt=3, conv_nt10=0):
            assert auto_nt(ctx, ncu, nOut, kH, kW, Ho, Wo)[0] == 5
            g5, name = run_conv(dfe, ctx, T(x, cuda), T(w, cuda), T(b, cuda), False)
        assert name == kernel_name(kW, 5, False, False), name
        assert np.array_equal(g5, g)


def _rescale(model):
    """per-scale copies start equal: make them differ so that a mix-up of entries shows (as test_learned_multiscale_one_call_equals_staged_and_oracle)"""
    for i, f in enumerate(model.filters[1:], 1):
        for m in f.modules:
            if getattr(m, "weight", None) is not None:
                m.weight.mul_(1.0 + 0.25 * i)


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("layers,nt", [([(3, 5, 5, 10)], 5), ([(3, 5, 5, 10)], 10), ([(3, 3, 7, 5)], 5)])
def test_pyramid_entries_in_one_launch_at_forced_count(dfe, cuda, layers, nt, share):
    """(d) dfe_filter_layer_forward_batch with six entries (both frames of three scales) under conv_nt: the one call == the staged
    modules bit for bit, the volumes of the tanh-free stack == the oracle's bit for bit, indices and decode against
    rp.multiscale_filtered_oracle."""
    ratios, mh, H, W = [1, 2, 4], 8, 96, 136
    geo = dict(maxh=mh, maxw=mh, ratios=ratios, multiscale=True, layers=layers, share_filters=share, hImg=H, wImg=W, output_extraction_method="max")
    model = dfe.getModelMultiscale(geo, True, False, device=cuda, generator=torch.Generator().manual_seed(17 + nt))
    if not share:
        _rescale(model)
    f0, f1, _, _ = rp.synth_pair(H, W, C=3, seed=H + nt, max_flow=8, noise_sigma=0)
    f0, f1 = f0 / np.float32(255), f1 / np.float32(255)
    ctx = dfe.get_ctx(0)
    with ctx.options(conv_nt=nt):
        one = model.forwardFlow([T(f0, cuda), T(f1, cuda)], False, one_call=True)
        stg = model.forwardFlow([T(f0, cuda), T(f1, cuda)], False, one_call=False)
        # the staged filter modules run the same forced form
        feat = model.filters[0].forward(T(f0, cuda))
        assert ctx.last_kernel() == kernel_name(layers[0][1], nt, False, False), ctx.last_kernel()
        SEEN.add(ctx.last_kernel())
    assert torch.equal(one["index"], stg["index"]) and torch.equal(one["y"], stg["y"]) and torch.equal(one["x"], stg["x"])
    stack = _stack_dicts(model.filters[0])
    assert np.array_equal(feat.cpu().numpy(), orc.spatial_convolution(f0, stack[0]["weight"], stack[0]["bias"]))
    ref = rp.multiscale_filtered_oracle(f0, f1, [_stack_dicts(f) for f in model.filters], mh, mh, ratios)
    for v, rv in zip(model.volumes, ref["vols"]):
        assert np.array_equal(v.cpu().numpy(), rv)
    gi = one["index"].cpu().numpy()
    gflow = np.stack([one["y"].cpu().numpy(), one["x"].cpu().numpy()]).astype(np.float32)
    _assert_matches_oracle(gi, gflow, ref, mh, mh, ratios)
    assert ctx.get_option("conv_nt") == -1


@pytest.mark.parametrize("nt", [4, 8])
def test_single_scale_view_entry_at_forced_count(dfe, cuda, nt):
    """(d) the single-scale one call reads frame 0's narrow in place (dfe_filter_layer_forward_batch_view, two entries); the staged modules
    filter the whole contiguous frames through the plain entry: same results on every key, and the staged feature maps == the oracle."""
    H, W, mh, mw = 64, 300, 16, 16
    geo = dict(layers=[[3, 5, 5, 8]], maxh=mh, maxw=mw, multiscale=False, output_extraction_method="max", hImg=H, wImg=W)
    model = dfe.getModel(geo, True, False, device=cuda, generator=torch.Generator().manual_seed(H + nt))
    f0, f1 = _pair(H, W, H + W, 30.0)
    t0, t1 = T(f0, cuda), T(f1, cuda)
    ctx = dfe.get_ctx(0)
    par = model.modules[0]
    with ctx.options(conv_nt=nt):
        one = model.forwardFlow([t0, t1], None, one_call=True)
        stg = model.forwardFlow([t0, t1], None, one_call=False)
        par.modules[0].forward(t0)
        assert ctx.last_kernel() == kernel_name(5, nt, False, False), ctx.last_kernel()
        SEEN.add(ctx.last_kernel())
        par.modules[1].forward(t1)
    _same(one, stg, None)
    conv = [m for m in par.modules[0].modules if getattr(m, "weight", None) is not None][0]
    w, b = conv.weight.cpu().numpy(), conv.bias.cpu().numpy()
    assert np.array_equal(par.modules[0].output.cpu().numpy(), orc.spatial_convolution(f0, w, b))
    assert np.array_equal(par.modules[1].output.cpu().numpy(), orc.spatial_convolution(f1, w, b))
    assert len(np.unique(one["index"].cpu().numpy())) > 1           # (not a constant: the comparison above compared something)
    assert ctx.get_option("conv_nt") == -1
