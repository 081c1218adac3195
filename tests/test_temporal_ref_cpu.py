"""The numpy restatement of the temporal depth filter (tests/temporal_ref.py; include/dfe.h: dfe_forward_warp_f32, dfe_temporal_fuse_f32,
DESIGN section 4.35) on its own: the properties the definition promises, and what the filter buys on the two-surface scene."""
import numpy as np
import pytest

from tests.temporal_ref import (SCENE_TOL, SCENE_WMAX, TemporalFilterRef, forward_warp_ref, scene, scene_stats, temporal_fuse_ref,
                                temporal_step_ref)

F = np.float32


def field(C=2, H=6, W=9, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(C, H, W)).astype(F), rng.uniform(0.5, 3.0, (H, W)).astype(F)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_zero_flow_without_a_measurement_returns_the_state():
    v, w = field()
    v[0, 1, 2] = -0.0
    r = temporal_step_ref(v, w, np.zeros((2, 6, 9), F), np.zeros_like(v), np.zeros_like(w), tol=1.0, wmax=8.0, key=v[0])
    assert same_bits(r["out"], v) and same_bits(r["wout"], w) and (r["flag"] == 1).all()
    assert np.array_equal(r["src"], np.arange(54, dtype=np.int32).reshape(6, 9))


def test_integer_translation_shifts_exactly_and_leaves_the_strip_empty():
    v, w = field()
    flow = np.zeros((2, 6, 9), F)
    flow[0], flow[1] = 1, -2
    out, wout, src = forward_warp_ref(v, w, flow)
    assert same_bits(out[:, 1:, :7], v[:, :5, 2:]) and same_bits(wout[1:, :7], w[:5, 2:])
    assert (out[:, 0] == 0).all() and (out[:, :, 7:] == 0).all() and (wout[0] == 0).all() and (wout[:, 7:] == 0).all()
    assert (src[0] == -1).all() and (src[:, 7:] == -1).all() and src[1, 0] == 2


def test_smaller_key_wins_and_equal_keys_fall_to_the_smaller_index():
    v = np.arange(4, dtype=F).reshape(1, 1, 4) + 10
    w = np.ones((1, 4), F)
    flow = np.zeros((2, 1, 4), F)
    flow[1, 0] = [2, 1, 0, -1]                                    # every source lands on column 2
    out, wout, src = forward_warp_ref(v, w, flow, key=np.array([[5, 3, 4, 3]], F))
    assert src[0].tolist() == [-1, -1, 1, -1] and out[0, 0, 2] == 11   # keys 3 and 3: the smaller index
    out, wout, src = forward_warp_ref(v, w, flow, key=np.array([[5, 3, 4, -1]], F))
    assert src[0, 2] == 3
    out, wout, src = forward_warp_ref(v, w, flow, key=np.array([[0.0, 1, 1, -0.0]], F))
    assert src[0, 2] == 0                                          # -0 counts as +0: the smaller index
    out, wout, src = forward_warp_ref(v, w, flow)
    assert src[0, 2] == 0


def test_half_fractions_round_up():
    v, w = np.ones((1, 1, 8), F), np.ones((1, 8), F)
    flow = np.zeros((2, 1, 8), F)
    flow[1, 0, 2], flow[1, 0, 5] = 0.5, -0.5                      # 2.5 -> 3, 4.5 -> 5
    flow[1, 0, 0] = -0.75                                          # -0.75 -> -1: dropped
    flow[1, 0, 3], flow[1, 0, 4] = np.nan, np.nan
    _, _, src = forward_warp_ref(v, w, flow)
    assert src[0].tolist() == [-1, 1, -1, 2, -1, 5, 6, 7]
    flow[1, 0, 0] = -0.5                                           # -0.5 -> 0
    assert forward_warp_ref(v, w, flow)[2][0, 0] == 0


def test_gain_bias_decay_and_holes():
    v, w = field(C=2)
    w[0, 0], w[0, 1], w[0, 2], v[1, 0, 3] = 0, 5e-7, np.inf, np.nan
    flow = np.zeros((2, 6, 9), F)
    out, wout, src = forward_warp_ref(v, w, flow, gain=(2.0, 0.5), bias=(1.0, -1.0), decay=0.75)
    assert (src[0, :4] == -1).all() and (out[:, 0, :4] == 0).all() and src[0, 4] == 4
    assert out[0, 2, 2] == F(F(2) * v[0, 2, 2]) + F(1) and wout[2, 2] == w[2, 2] * F(0.75)


def fuse1(z, wp, m, wm, tol=2.0, wmax=8.0):
    o, w, f = temporal_fuse_ref(np.full((1, 1, 1), z, F), np.full((1, 1), wp, F), np.full((1, 1, 1), m, F), np.full((1, 1), wm, F), tol, wmax)
    return float(o[0, 0, 0]), float(w[0, 0]), int(f[0, 0])


def test_every_row_of_the_fusion_table():
    assert fuse1(np.nan, 0, np.nan, 0) == (0.0, 0.0, 0)
    assert fuse1(3, 2, np.nan, 0) == (3.0, 2.0, 1) and fuse1(3, 20, 7, 5e-7) == (3.0, 8.0, 1)       # the weight is capped at wmax
    assert fuse1(np.inf, 2, 7, 1) == (7.0, 1.0, 2) and fuse1(3, np.nan, 7, 9) == (7.0, 8.0, 2)
    assert fuse1(3, 3, 5, 1) == (3.5, 4.0, 3)                      # d2 == tol^2 agrees; out = 5 + 3/4 (3 - 5)
    assert fuse1(3, 7, 4, 6) == (float(F(4) + F(F(7) / F(13)) * F(-1)), 8.0, 3)                      # min(a + b, wmax)
    assert fuse1(3, 3, 5.5, 1) == (3.0, 2.0, 4)                    # the prior survives, weakened
    assert fuse1(3, 1, 5.5, 1) == (5.5, 1.0, 5)                    # a == b: the measurement with its weight
    assert fuse1(3, 1, 5.5, 3) == (5.5, 2.0, 5)
    assert fuse1(3, 1, 9, 1, tol=0.0) == (9.0, 1.0, 5) and fuse1(3, 1, 3, 1, tol=0.0) == (3.0, 2.0, 3)


def test_fusion_sums_squares_over_channels_and_keeps_the_region():
    z, m = np.zeros((2, 4, 5), F), np.zeros((2, 4, 5), F)
    m[0], m[1] = 3, 4                                              # |d|^2 = 25
    one = np.ones((4, 5), F)
    assert (temporal_fuse_ref(z, one, m, one, 5.0)[2] == 3).all() and (temporal_fuse_ref(z, one, m, one, 4.99)[2] == 5).all()
    out, wout, flag = temporal_fuse_ref(z, one, m, one, 5.0, region=(1, 1, 2, 3))
    inside = np.zeros((4, 5), bool)
    inside[1:3, 1:4] = True
    assert (flag[inside] == 3).all() and (flag[~inside] == 0).all() and (wout[~inside] == 0).all() and (out[:, ~inside] == 0).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_filter_on_the_two_surface_scene(seed):
    """after frame 8 the fused median absolute error is at most half the frame's, the fused share of pixels off by more than 1 at most
    a quarter of the frame's, and the fused field covers at least 0.95 of the frame (seeds 0, 1, 2 when this was written: median 0.369 /
    0.361 / 0.378 -> 0.162 / 0.161 / 0.164, off by more than one 13.2 / 10.9 / 12.2 % -> 1.7 / 1.0 / 1.2 %, coverage 0.78 - 0.80 -> 0.99)"""
    f = TemporalFilterRef(SCENE_TOL, SCENE_WMAX, key_channel=0)
    for truth, meas, weight, flow in scene(seed):
        out, wout, flag = f.push(meas, weight, flow)
    med0, bad0, cov0 = scene_stats(truth, meas[0], weight)
    med1, bad1, cov1 = scene_stats(truth, out[0], wout)
    print("seed %d: median %.3f -> %.3f, off by more than one %.4f -> %.4f, coverage %.3f -> %.3f" % (seed, med0, med1, bad0, bad1, cov0, cov1))
    assert med1 <= 0.5 * med0 and bad1 <= 0.25 * bad0 and cov1 >= 0.95
