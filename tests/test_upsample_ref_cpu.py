"""The numpy restatement of guided upsampling (tests/upsample_ref.py; include/dfe.h: dfe_guided_upsample_f32)
against the consequences its definition states, float32 against the same code in float64, and the two-surface scene: what the guide
buys.  No device."""
import numpy as np
import pytest

from tests.upsample_ref import SCENE, band_error, guided_upsample_ref, image_scale_ref, two_surface_scene

F = np.float32
EPS = 2.0**-24


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def test_equal_sizes_r1_no_guide_is_a_bit_copy_times_gain():
    rng = np.random.default_rng(0)
    v = rng.uniform(-9, 9, size=(3, 7, 9)).astype(F)
    v[0, 0, 0], v[1, 3, 4], v[2, 6, 8] = -0.0, -0.0, 0.0
    out, valid = guided_upsample_ref(v, (7, 9), r=1)
    assert np.array_equal(_bits(out), _bits(v)) and np.signbit(out[0, 0, 0]) and (valid == 1).all(), "-0 included"
    gain = np.array([2.5, -3.0, 0.5], F)
    out, _ = guided_upsample_ref(v, (7, 9), r=1, gain=gain)
    assert np.array_equal(_bits(out), _bits(gain[:, None, None] * v))
    # with a plane of weights the valid pixels are still copied (wt v / wt is v only for wt = 1: a trusted pixel) and the others are holes
    w = np.where(rng.random((7, 9)) < 0.5, 1, 0).astype(F)
    out, valid = guided_upsample_ref(v, (7, 9), w, r=1)
    assert np.array_equal(valid, w) and np.array_equal(_bits(out[:, w > 0]), _bits(v[:, w > 0])) and not out[:, w == 0].any()


@pytest.mark.parametrize("shape,size", [((7, 9), (20, 31)), ((24, 40), (48, 80)), ((1, 1), (5, 6)), ((24, 40), (24, 140)), ((3, 5), (70, 140)), ((7, 9), (7, 9))])
def test_r1_without_guide_or_holes_is_image_scale(shape, size):
    """the tent of r = 1 is the bilinear weight pair and the normalisation S = 1 up to rounding; a dropped edge tap leaves the other
    with all the weight, which is what the clamp gives.  8 eps max|v|: two products and a sum per axis, the sum S and the division."""
    rng = np.random.default_rng(1)
    v = rng.uniform(-16, 16, size=(2,) + shape).astype(F)
    out, valid = guided_upsample_ref(v, size, r=1)
    want = image_scale_ref(v, *size)
    err = np.abs(out.astype(np.float64) - want).max()
    print("%s -> %s: |guided r=1 - imageScale| = %.3g = %.2f of the bound" % (shape, size, err, err / (8 * EPS * np.abs(v).max())))
    assert (valid == 1).all() and err <= 8 * EPS * np.abs(v).max()


@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("shape,size", [((7, 9), (20, 31)), ((24, 40), (48, 80)), ((3, 5), (70, 140)), ((24, 40), (24, 140))])
def test_float32_stays_within_its_bound_of_float64_without_a_guide(shape, size, r):
    """2 x 4 r^2 terms of non-negative weights, each a few roundings: (8 r^2 + 10) eps |gain_c| max|v_c|"""
    rng = np.random.default_rng(r)
    v = rng.uniform(-16, 16, size=(3,) + shape).astype(F)
    w = np.where(rng.random(shape) < 0.6, rng.choice(np.array([1, 0.5, 1e-3, 1e-6], F), size=shape), 0).astype(F)
    gain = np.array([2.5, -3.0, 1.0], F)
    worst = 0.0
    for wgt in (None, w):
        o32, v32 = guided_upsample_ref(v, size, wgt, r=r, gain=gain)
        o64, v64 = guided_upsample_ref(v, size, wgt, r=r, gain=gain, dtype=np.float64)
        assert o32.dtype == F and o64.dtype == np.float64 and np.array_equal(v32, v64)
        for c in range(3):
            bound = (8 * r * r + 10) * EPS * abs(float(gain[c])) * float(np.abs(v[c]).max())
            err = float(np.abs(o32[c].astype(np.float64) - o64[c]).max())
            worst = max(worst, err / bound)
            assert err <= bound, (c, err, bound)
    print("%s -> %s r=%d: float32 within %.3f of the bound" % (shape, size, r, worst))


def test_a_nan_under_zero_weight_never_leaks_and_a_nan_guide_pixel_is_invalid():
    rng = np.random.default_rng(3)
    v = rng.uniform(-4, 4, size=(2, 12, 16)).astype(F)
    w = np.ones((12, 16), F)
    bad = rng.random((12, 16)) < 0.3
    v[0, bad] = np.nan
    v[1, bad] = np.inf
    w[bad] = 0
    gh = rng.uniform(0, 4, size=(3, 30, 37)).astype(F)
    gl = image_scale_ref(gh, 12, 16)
    for guide in (None, gh):
        out, valid = guided_upsample_ref(v, (30, 37), w, guide, None if guide is None else gl, sigma=100.0, r=2)
        assert np.isfinite(out).all() and (valid == 1).all()
    gh[1, 11, 13] = np.nan
    out, valid = guided_upsample_ref(v, (30, 37), w, gh, gl, sigma=100.0, r=2)
    assert valid[11, 13] == 0 and not out[:, 11, 13].any() and valid.sum() == 30 * 37 - 1 and np.isfinite(out).all()
    # sigma <= 0 or NaN: no range term, whatever the guide holds
    for sigma in (0.0, -1.0, np.nan):
        o2, v2 = guided_upsample_ref(v, (30, 37), w, gh, gl, sigma=sigma, r=2)
        o0, v0 = guided_upsample_ref(v, (30, 37), w, r=2)
        assert np.array_equal(_bits(o2), _bits(o0)) and np.array_equal(v2, v0)


def test_edge_taps_are_dropped_and_pixels_without_a_sample_are_zero():
    v = np.array([[[1.0, 2.0], [3.0, 4.0]]], F)
    out, valid = guided_upsample_ref(v, (4, 4), r=1)
    assert (valid == 1).all() and np.array_equal(out[0, 0], np.array([1, 1.25, 1.75, 2], F))   # the corner: one tap left, all the weight
    w = np.array([[0, 0], [0, 1]], F)
    out, valid = guided_upsample_ref(v, (4, 4), w, r=1)
    # the taps of r = 1 reach the sample (1, 1) from the output rows and columns 1 .. 3 only (u = -0.25 at 0: taps -1 and 0)
    assert np.array_equal(valid, np.pad(np.ones((3, 3), F), ((1, 0), (1, 0)))) and np.array_equal(out[0], 4 * valid)
    out, valid = guided_upsample_ref(v, (4, 4), w, r=2)
    assert (valid == 1).all() and (out == 4).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_guide_keeps_the_edge_of_the_two_surface_scene(seed):
    s = two_surface_scene(seed)
    size = (SCENE["Hh"], SCENE["Wh"])
    guided, gvalid = guided_upsample_ref(s["v"], size, s["w"], s["guide_hi"], s["guide_lo"], SCENE["sigma"], SCENE["r"])
    plain, _ = guided_upsample_ref(s["v"], size, s["w"], r=SCENE["r"])
    scaled = image_scale_ref(np.nan_to_num(s["v"], nan=0.0), *size)                   # a hole reads as 0: bilinear does not know it is one
    eg, ep, es = band_error(guided[0], s), band_error(plain[0], s), band_error(scaled[0], s)
    print("seed %d: %d band pixels off by more than 0.5: guided %.3f, unguided %.3f, imageScale %.3f; guided valid on %.4f of the frame"
          % (seed, int(s["band"].sum()), eg, ep, es, gvalid.mean()))
    assert eg <= 0.02 and ep >= 0.5 and es >= 0.3
