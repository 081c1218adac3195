"""The four-tap splat's definition (include/dfe.h: dfe_forward_splat_f32) in its numpy restatement
(tests/temporal_splat_ref.py), on the two things the nearest-pixel warp cannot do -- carry a flow below half a pixel per frame, and keep
an expanding field free of holes -- on the case where the two warps must agree bit for bit, and on a noisy scene that moves by fractions
of a pixel.  The numbers printed here are the ones DESIGN.md quotes.  No device."""
import numpy as np

from tests.temporal_ref import SCENE_H, SCENE_TOL, SCENE_W, SCENE_WMAX, TemporalFilterRef, forward_warp_ref, scene_stats
from tests.temporal_splat_ref import UNIT, TemporalFilterSplatRef, forward_splat_ref

F = np.float32


def test_slow_ramp_is_carried():
    """depth 4 + 0.25 x under +0.4 px per frame in x, 8 chained steps.  Per step the position is quantised to 1 / 128 px (0.25 / 128 of
    depth at most) and the value twice to 1 / 1024 (fixed point, then the quotient): 8 (0.25 / 128 + 2 / 1024) = 0.031, bound 0.05.  The
    nearest warp never moves the field: 0.1 per frame.  Columns whose taps left or entered through a side are excluded: a linear ramp is
    carried exactly by a partition of unity only where all of a target's sources exist (3.2 px of travel and one tap of spread per step:
    12 columns on the left, 2 on the right)."""
    H, W = 6, 64
    x = np.arange(W, dtype=F)
    v0 = np.broadcast_to(4 + F(0.25) * x, (1, H, W)).astype(F)
    flow = np.zeros((2, H, W), F)
    flow[1] = 0.4
    for key, ztol in ((False, 0.0), (True, 0.5)):                  # without a front, and with one that lets the slope's neighbours through
        vb, wb, vn, wn = v0.copy(), np.ones((H, W), F), v0.copy(), np.ones((H, W), F)
        for t in range(1, 9):
            vb, wb, cover = forward_splat_ref(vb, wb, flow, vb[0] if key else None, ztol=ztol, quant=1024.0, min_cover=0.25)
            vn, wn, _ = forward_warp_ref(vn, wn, flow, vn[0] if key else None)
            truth = 4 + 0.25 * (x.astype(np.float64) - 0.4 * t)
            eb, en = np.abs(vb[0] - truth)[:, 12:-2].max(), np.abs(vn[0] - truth)[:, 12:-2].max()
            print("frame %d key=%s: bilinear error %.4f, nearest error %.4f, cover %.3f .. %.3f" % (t, key, eb, en, cover[:, 12:-2].min(), cover[:, 12:-2].max()))
            assert abs(en - 0.1 * t) < 1e-5                        # the nearest prior stays where it is
        assert eb <= 0.05
        assert np.array_equal(wb[:, 12:-2], np.ones((H, W - 14), F)) and np.array_equal(cover[:, 12:-2], np.ones((H, W - 14), F))


def test_zoom_leaves_no_hole():
    """a zoom by 1.05 about the centre of 48 x 64: every interior target has a source within 0.525 px per axis, so tent weights of at least
    0.475^2 = 0.23 per source and, from the sources on its other sides, more than min_cover = 0.25 in all; the nearest scatter leaves
    about 1 - 1 / s^2 of the interior targets empty"""
    H, W, s = 48, 64, 1.05
    yy, xx = np.mgrid[0:H, 0:W].astype(F)
    flow = np.stack(((s - 1) * (yy - (H - 1) / 2), (s - 1) * (xx - (W - 1) / 2))).astype(F)
    v, w = (5 + 0.1 * xx)[None].astype(F), np.ones((H, W), F)
    out, wout, cover = forward_splat_ref(v, w, flow, v[0], ztol=0.5, min_cover=0.25)
    _, wn, src = forward_warp_ref(v, w, flow, v[0])
    inner = (slice(2, H - 2), slice(2, W - 2))
    holes_b, holes_n = float((wout[inner] == 0).mean()), float((src[inner] < 0).mean())
    print("zoom %.2f: holes bilinear %.4f, nearest %.4f (1 - 1 / s^2 = %.4f); cover %.3f .. %.3f" % (s, holes_b, holes_n, 1 - 1 / s ** 2, cover[inner].min(),
                                                                                                  cover[inner].max()))
    assert holes_b == 0 and cover[inner].min() >= 0.25
    assert 0.04 < holes_n < 0.12
    truth = 5 + 0.1 * ((xx - (W - 1) / 2) / s + (W - 1) / 2)       # the ramp, zoomed
    assert np.abs(out[0] - truth)[inner].max() < 0.1 * (1 / 128 + 0.05) + 2 / 1024   # position grid, the stretch's own bow, fixed point


def test_integer_flow_without_collisions_gives_the_nearest_warp_s_bits():
    rng = np.random.default_rng(0)
    H, W, region = 17, 23, (2, 2, 13, 19)
    for Cc, shift, gain, bias, decay in ((1, (1, -2), None, None, 1.0), (3, (-2, 3), (2.0, 0.5, -1.0), (0.25, 0.0, 1.0), 0.5)):
        v = (rng.integers(-2048, 2048, (Cc, H, W)) / 512).astype(F)           # gain v + bias on the 1 / 1024 grid, |V| Wf < 2^24 with the weights below
        w = (rng.integers(0, 512, (H, W)) / 128).astype(F)                    # w decay on the 1 / 256 grid, zeros among them
        flow = np.broadcast_to(np.array(shift, F)[:, None, None], (2, H, W)).copy()
        key = rng.uniform(1, 9, (H, W)).astype(F)
        want = forward_warp_ref(v, w, flow, key, region, gain, bias, decay)
        got = forward_splat_ref(v, w, flow, key, region, gain, bias, decay, ztol=0.0, quant=1024.0, min_cover=1.0, sums=True)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert np.array_equal(got[2] == 1, want[2] >= 0) and set(np.unique(got[2])) == {0.0, 1.0}
        assert set(np.unique(got[3]["U"])) == {0, UNIT} and got[3]["taps"].max() == 1


def subpixel_scene(seed, frames=8):
    """temporal_ref.scene with motion in fractions of a pixel and a slanted background: the background 8 + x / 16 moving -0.4 px per
    frame, the foreground at depth 4 moving -1.4 px; the same noise, outliers and holes, drawn in the same order"""
    rng = np.random.default_rng(seed)
    x = np.arange(SCENE_W, dtype=np.float64)
    out = []
    for t in range(frames):
        truth = np.broadcast_to(8 + 0.25 * (x + 0.4 * t) / 4, (SCENE_H, SCENE_W)).copy()
        flow = np.zeros((2, SCENE_H, SCENE_W), F)
        flow[1] = -0.4
        fg = (x >= 40 - 1.4 * t) & (x < 56 - 1.4 * t)
        truth[12:36, fg] = 4
        flow[1, 12:36, fg] = -1.4
        meas = (truth + rng.normal(0, 0.5, truth.shape)).astype(F)
        outlier = rng.random(truth.shape) < 0.10
        meas = np.where(outlier, rng.uniform(1, 12, truth.shape), meas).astype(F)
        weight = np.where(rng.random(truth.shape) < 0.20, 0, 1).astype(F)
        out.append((truth.astype(F), meas[None], weight, flow))
    return out


def test_scene_with_subpixel_flow_bilinear_is_no_worse_than_nearest():
    for seed in (0, 1):
        near, bil = TemporalFilterRef(SCENE_TOL, SCENE_WMAX, key_channel=0), TemporalFilterSplatRef(SCENE_TOL, SCENE_WMAX, key_channel=0)
        for truth, meas, weight, flow in subpixel_scene(seed):
            sn, sb = near.push(meas, weight, flow), bil.push(meas, weight, flow)
        raw = scene_stats(truth, meas[0], weight)
        n, b = scene_stats(truth, sn[0][0], sn[1]), scene_stats(truth, sb[0][0], sb[1])
        print("seed %d, last frame (median error, share off by > 1, coverage): raw %.3f %.3f %.3f; nearest %.3f %.3f %.3f; bilinear %.3f %.3f %.3f" % ((seed,) + raw + n + b))
        assert b[0] <= n[0]                                        # no worse than nearest; the other figures are reported
