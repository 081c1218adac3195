"""The byte entries at scale 1 (dfe_flow_depth_pair_u8, dfe_flow_depth_pair_u8_slot) without the float copy of the frames: the pack kernel
reads the bytes as they are and writes the frame's border, the int8 sweep does the rest -- two launches.  All four outputs, pre-filled
with -7, equal dfe_flow_depth_pair_f32 on float(bytes) byte for byte: one output row, a shifted last tile column, several strips, frame
widths that are no multiple of 4, device buffers at an odd address; the verdict ring across a gated float step, a byte-entry step and a
clean float step on one context; and the routes that stay what they were (another scale, cv_i8 = 0, a 17 x 17 window)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import refpath as rp

K, WIN = 7, 33
PAD = K + WIN - 2
SHAPES = [(1, 9), (5, 23), (9, 48)]   # W = Wo + 38 = 47, 61, 86: none a multiple of 4


def _bytes_pair(Ho, Wo, seed=5, win=WIN):
    H, W = Ho + K + win - 2, Wo + K + win - 2
    f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=seed, max_flow=min(12, max(1, min(H, W) // 8)), integer=True)
    b0, b1 = np.ascontiguousarray(f0.astype(np.uint8)), np.ascontiguousarray(f1.astype(np.uint8))
    assert np.array_equal(b0.astype(np.float32), f0) and np.array_equal(b1.astype(np.float32), f1)
    return b0, b1, foe


def _outs(cuda, H, W):
    return [torch.full((2, H, W), -7.0, device=cuda)] + [torch.full((H, W), -7.0, device=cuda) for _ in range(3)]


def _host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(("flow", "scores", "depth", "conf"), o)}


def _f32(ctx, lib, cuda, f0, f1, foe, thr, win=WIN):
    _, H, W = f0.shape
    t0, t1 = torch.from_numpy(np.ascontiguousarray(f0)).to(cuda), torch.from_numpy(np.ascontiguousarray(f1)).to(cuda)
    o = _outs(cuda, H, W)
    ctx.check(lib.dfe_flow_depth_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, K, win, win, foe[0], foe[1], thr, *(t.data_ptr() for t in o)))
    took = ctx.flow_last_path_i8()
    return _host(o), took


def _u8(ctx, lib, cuda, b0, b1, foe, thr, scale=1.0, odd=False, win=WIN):
    _, H, W = b0.shape
    n = 3 * H * W
    if odd:   # both frames one byte into their buffers
        t0, t1 = (torch.zeros(n + 1, dtype=torch.uint8, device=cuda) for _ in range(2))
        t0[1:] = torch.from_numpy(b0.reshape(-1)).to(cuda)
        t1[1:] = torch.from_numpy(b1.reshape(-1)).to(cuda)
        p0, p1 = t0.data_ptr() + 1, t1.data_ptr() + 1
        assert p0 % 2 == 1 and p1 % 2 == 1
    else:
        t0, t1 = torch.from_numpy(b0).to(cuda), torch.from_numpy(b1).to(cuda)
        p0, p1 = t0.data_ptr(), t1.data_ptr()
    o = _outs(cuda, H, W)
    ctx.check(lib.dfe_flow_depth_pair_u8(ctx.handle, p0, p1, 3, H, W, K, win, win, foe[0], foe[1], thr, scale, *(t.data_ptr() for t in o)))
    took = ctx.flow_last_path_i8()
    return _host(o), took


def _u8_slot(ctx, lib, cuda, b0, b1, foe, thr):
    _, H, W = b0.shape
    h0, h1 = torch.from_numpy(b0).pin_memory(), torch.from_numpy(b1).pin_memory()
    slot = C.c_int(-1)
    ctx.check(lib.dfe_ingest_submit_u8(ctx.handle, h0.data_ptr(), h1.data_ptr(), 3 * H * W, C.byref(slot)))
    o = _outs(cuda, H, W)
    ctx.check(lib.dfe_flow_depth_pair_u8_slot(ctx.handle, slot.value, 3, H, W, K, WIN, WIN, foe[0], foe[1], thr, 1.0, *(t.data_ptr() for t in o)))
    took = ctx.flow_last_path_i8()
    return _host(o), took   # (synchronised: the pinned frames stay alive until the copy has run)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("Ho,Wo", SHAPES)
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_byte_entries_equal_the_float_entry(dfe, cuda, Ho, Wo, thr):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    b0, b1, foe = _bytes_pair(Ho, Wo)
    assert b0.shape[2] % 4 != 0
    ref, took = _f32(ctx, lib, cuda, b0.astype(np.float32), b1.astype(np.float32), foe, thr)
    assert took
    for odd in (False, True):
        got, took = _u8(ctx, lib, cuda, b0, b1, foe, thr, odd=odd)
        assert took
        _same(got, ref)
    got, took = _u8_slot(ctx, lib, cuda, b0, b1, foe, thr)
    assert took
    _same(got, ref)


@pytest.mark.gpu
def test_verdict_ring_across_float_and_byte_entry_steps(dfe, cuda):
    lib = dfe.lib()
    b0, b1, foe = _bytes_pair(9, 48)
    f0, f1 = b0.astype(np.float32), b1.astype(np.float32)
    g0 = f0.copy()
    g0[1, 20, 30] = 0.5
    s0, s1, sfoe = _bytes_pair(5, 23, seed=8)
    ctx = dfe.Context(0, torch.cuda.current_stream(0).cuda_stream)
    try:
        with ctx.options(cv_i8=0):
            want_gated, _ = _f32(ctx, lib, cuda, g0, f1, foe, 0.21)
            want_small, _ = _f32(ctx, lib, cuda, s0.astype(np.float32), s1.astype(np.float32), sfoe, 0.21)
            want_clean, _ = _f32(ctx, lib, cuda, f0, f1, foe, 0.21)
        for _ in range(2):   # twice: every word of the ring has been raised once and cleared again
            got, took = _f32(ctx, lib, cuda, g0, f1, foe, 0.21)
            assert not took
            _same(got, want_gated)
            got, took = _u8(ctx, lib, cuda, s0, s1, sfoe, 0.21)
            assert took
            _same(got, want_small)
            got, took = _f32(ctx, lib, cuda, f0, f1, foe, 0.21)
            assert took
            _same(got, want_clean)
            got, took = _f32(ctx, lib, cuda, g0, f1, foe, 0.21)
            assert not took
            _same(got, want_gated)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_other_routes_stay_what_they_were(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    b0, b1, foe = _bytes_pair(9, 48)
    # another scale: float(byte) * scale, the float entry's result whatever cv_i8 says
    scale, thr = 1.0 / 255.0, 0.21 / 255.0 ** 2
    f0, f1 = b0.astype(np.float32) * np.float32(scale), b1.astype(np.float32) * np.float32(scale)
    ref, _ = _f32(ctx, lib, cuda, f0, f1, foe, thr)
    got, took = _u8(ctx, lib, cuda, b0, b1, foe, thr, scale=scale)
    assert not took
    _same(got, ref)
    # cv_i8 = 0 at scale 1
    with ctx.options(cv_i8=0):
        ref, _ = _f32(ctx, lib, cuda, b0.astype(np.float32), b1.astype(np.float32), foe, 0.21)
        got, took = _u8(ctx, lib, cuda, b0, b1, foe, 0.21)
        assert not took
        _same(got, ref)
    # a 17 x 17 window
    c0, c1, cfoe = _bytes_pair(9, 48, win=17)
    ref, _ = _f32(ctx, lib, cuda, c0.astype(np.float32), c1.astype(np.float32), cfoe, 0.21, win=17)
    got, took = _u8(ctx, lib, cuda, c0, c1, cfoe, 0.21, win=17)
    assert not took
    _same(got, ref)
