"""Semi-global aggregation on the device (include/dfe.h: dfe_sgm_aggregate_f32) against the numpy restatement of its
definition (tests/sgm_ref.py) BIT FOR BIT -- the definition fixes every operation and the order of the sum, so there is no tolerance --
its argument errors, and semiGlobalAggregate against the raw call.  Every output is pre-filled with a sentinel.

A case is one (H x W, D): every shape meets every D.  The other inputs rotate with the case's number:
    paths    three sets a case out of the eight single bits, 0x0f, 0xff, 0x05 and 0xa0
    ring     0, 1, 5, W (clipped to W)
    P1, P2   (0, 0), (0.5, 4), (2, 16), (3, 3)
    values   random floats in -3 .. 9, or byte-valued integers, whose many exact ties test the first-minimum rule
    outputs  agg only, flow only (the aggregate stays in the library's scratch), both.
The shapes: a pixel, a row, a column, a few pixels, a frame of several 4-line waves, and 33 x 130 -- ragged against the 4 lines of a
wave and the 8 steps of the load pipeline in both directions.  D: one label, two, half a row, 12 and 15 (the radial windows), a full row
of 16 lanes, the first D with two labels a lane, and the largest."""
import numpy as np
import pytest
import torch

from tests.sgm_ref import sgm_aggregate, sgm_path

pytestmark = pytest.mark.gpu
DFE_E_ARG, DFE_E_SHAPE, DFE_E_UNSUPPORTED = -1, -2, -5
FILL = -7.0
SHAPES = ((1, 1), (1, 37), (37, 1), (5, 7), (24, 40), (33, 130))
DS = (1, 2, 8, 12, 15, 16, 17, 32)
PATHS = (0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x0f, 0xff, 0x05, 0xa0)
RINGS = (0, 1, 5, None)              # None: W
PENALTIES = ((0.0, 0.0), (0.5, 4.0), (2.0, 16.0), (3.0, 3.0))
CASES = [(i, s, D) for i, (D, s) in enumerate((D, s) for D in DS for s in SHAPES)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _volume(H, W, D, integer, seed):
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(0, 256, size=(H, W, D)).astype(np.float32)
    return rng.uniform(-3, 9, size=(H, W, D)).astype(np.float32)


def aggregate(dfe, cuda, vol, P1, P2, paths, ring, want_agg, want_flow):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, D = vol.shape
    tv = torch.from_numpy(vol).to(cuda)
    agg = torch.full((H, W, D), FILL, device=cuda)
    flow = torch.full((H, W), FILL, device=cuda)
    ctx.check(lib.dfe_sgm_aggregate_f32(ctx.handle, tv.data_ptr(), H, W, D, P1, P2, paths, ring, agg.data_ptr() if want_agg else None,
                                        flow.data_ptr() if want_flow else None))
    torch.cuda.synchronize()
    assert torch.equal(tv.cpu(), torch.from_numpy(vol)), "the volume is an input"
    return agg.cpu().numpy(), flow.cpu().numpy()


@pytest.mark.parametrize("i,shape,D", CASES, ids=["%dx%dx%d" % (s + (D,)) for _, s, D in CASES])
def test_device_equals_the_definition_bit_for_bit(dfe, cuda, i, shape, D):
    H, W = shape
    ring = RINGS[(3 * i + i // 24) % 4]      # (every path set, every shape and every D meet every ring)
    ring = W if ring is None else min(ring, W)
    P1, P2 = PENALTIES[(i + i // 8) % 4]
    integer = (i + i // 6) % 2 == 1
    vol = _volume(H, W, D, integer, i)
    single = [sgm_path(vol, r, P1, P2, ring) for r in range(8)]
    for k in range(3):
        paths = PATHS[(i + i // 6 + 4 * k) % 12]
        mode = (i + k) % 3                       # 0: agg only, 1: flow only, 2: both
        want = None
        for r in range(8):
            if paths >> r & 1:
                want = single[r] if want is None else (want + single[r]).astype(np.float32)
        tag = "%dx%dx%d paths 0x%02x ring %d P (%g, %g) %s mode %d" % (H, W, D, paths, ring, P1, P2, "bytes" if integer else "floats", mode)
        agg, flow = aggregate(dfe, cuda, vol, P1, P2, paths, ring, mode != 1, mode != 0)
        if mode != 1:
            assert np.array_equal(_bits(agg), _bits(want)), tag
        else:
            assert (agg == FILL).all(), tag + ": agg was not given"
        if mode != 0:
            assert np.array_equal(flow, np.argmin(want, axis=-1).astype(np.float32)), tag
        else:
            assert (flow == FILL).all(), tag + ": flow was not given"


def test_the_whole_sum_equals_sgm_aggregate_and_ties_take_the_first_label(dfe, cuda):
    vol = _volume(24, 40, 15, True, 99)
    vol[3:9] = 7.0                                # flat rows: every label ties
    for paths in (0x0f, 0xff):
        want, wflow = sgm_aggregate(vol, 2.0, 16.0, paths, 15)
        agg, flow = aggregate(dfe, cuda, vol, 2.0, 16.0, paths, 15, True, True)
        assert np.array_equal(_bits(agg), _bits(want)) and np.array_equal(flow, wflow)
    agg, flow = aggregate(dfe, cuda, np.full((5, 7, 12), 3.0, np.float32), 1.0, 2.0, 0xff, 0, True, True)
    assert (flow == 0).all()


def test_argument_errors(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, D = 5, 7, 12
    vol = torch.zeros((H, W, 33), device=cuda)
    agg = torch.full((H, W, 33), FILL, device=cuda)
    flow = torch.full((H, W), FILL, device=cuda)
    pv, pa, pf = vol.data_ptr(), agg.data_ptr(), flow.data_ptr()
    fn = lib.dfe_sgm_aggregate_f32
    nan, inf = float("nan"), float("inf")
    assert fn(None, pv, H, W, D, 1.0, 2.0, 0x0f, 0, pa, pf) == DFE_E_ARG
    assert fn(ctx.handle, None, H, W, D, 1.0, 2.0, 0x0f, 0, pa, pf) == DFE_E_ARG
    assert fn(ctx.handle, pv, H, W, D, 1.0, 2.0, 0x0f, 0, None, None) == DFE_E_ARG
    assert fn(ctx.handle, pv, H, W, D, 1.0, 2.0, 0x0f, 0, pv, pf) == DFE_E_ARG          # agg == volume
    for paths in (0, 256, 0x10f):
        assert fn(ctx.handle, pv, H, W, D, 1.0, 2.0, paths, 0, pa, pf) == DFE_E_ARG, paths
    for P1, P2 in ((-1.0, 2.0), (3.0, 2.0), (nan, 2.0), (1.0, nan), (1.0, inf), (inf, inf), (-0.5, -0.25)):
        assert fn(ctx.handle, pv, H, W, D, P1, P2, 0x0f, 0, pa, pf) == DFE_E_ARG, (P1, P2)
    for ring in (-1, W + 1):
        assert fn(ctx.handle, pv, H, W, D, 1.0, 2.0, 0x0f, ring, pa, pf) == DFE_E_ARG, ring
    for h, w, d in ((0, W, D), (H, 0, D), (H, W, 0), (-1, W, D), (65536, 65536, D)):
        assert fn(ctx.handle, pv, h, w, d, 1.0, 2.0, 0x0f, 0, pa, pf) == DFE_E_SHAPE, (h, w, d)
    assert fn(ctx.handle, pv, H, W, 33, 1.0, 2.0, 0x0f, 0, pa, pf) == DFE_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (agg == FILL).all() and (flow == FILL).all(), "a refused call writes nothing"
    assert fn(ctx.handle, pv, H, W, 32, 0.0, 0.0, 0xff, W, pa, pf) == 0
    assert fn(ctx.handle, pv, H, W, D, 2.0, 2.0, 0x01, W, None, pf) == 0
    torch.cuda.synchronize()


def test_semiGlobalAggregate_equals_the_raw_call(dfe, cuda):
    vol = _volume(33, 130, 15, False, 5)
    tv = torch.from_numpy(vol).to(cuda)
    for paths, ring in ((0x0f, 0), (0xff, 15), (0x40, 130)):
        agg, flow = aggregate(dfe, cuda, vol, 0.5, 4.0, paths, ring, True, True)
        f, a = dfe.semiGlobalAggregate(tv, 0.5, 4.0, paths=paths, ring=ring)
        assert tuple(f.shape) == (33, 130) and tuple(a.shape) == (33, 130, 15)
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(agg)) and np.array_equal(f.cpu().numpy(), flow)
        f2, none = dfe.semiGlobalAggregate(tv, 0.5, 4.0, paths=paths, ring=ring, want_volume=False)
        assert none is None and torch.equal(f2, f)
    f, a = dfe.semiGlobalAggregate(tv, 0.5, 4.0)              # the defaults: 4 paths on the plane
    agg, flow = aggregate(dfe, cuda, vol, 0.5, 4.0, 0x0f, 0, True, True)
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(agg)) and np.array_equal(f.cpu().numpy(), flow)
    f, a = dfe.semiGlobalAggregate(tv.permute(1, 0, 2), 0.5, 4.0)      # a view: made contiguous
    agg, flow = aggregate(dfe, cuda, np.ascontiguousarray(vol.transpose(1, 0, 2)), 0.5, 4.0, 0x0f, 0, True, True)
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(agg)) and np.array_equal(f.cpu().numpy(), flow)
    for bad in (dict(paths=0), dict(paths=256), dict(paths=1.0), dict(paths=True), dict(ring=-1), dict(ring=131), dict(ring=1.0), dict(P1=-1.0),
                dict(P1=5.0), dict(P2=float("nan")), dict(P2=float("inf")), dict(P1="a")):
        with pytest.raises(ValueError):
            dfe.semiGlobalAggregate(tv, **{**dict(P1=0.5, P2=4.0), **bad})
    with pytest.raises(TypeError):
        dfe.semiGlobalAggregate(tv.double(), 0.5, 4.0)
    for badvol in (tv[0], torch.zeros((3, 4, 33), device=cuda), torch.zeros((0, 4, 5), device=cuda)):
        with pytest.raises(ValueError):
            dfe.semiGlobalAggregate(badvol, 0.5, 4.0)
