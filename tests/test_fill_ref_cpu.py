"""The float64 restatement of the hole-filling operator (tests/fill_ref64.py; include/dfe.h: dfe_fill_holes_f32)
checked on cases whose answer is known without it, and on the scene the feature is for."""
import numpy as np

from tests.fill_ref64 import fill_bound, fill_holes_ref, fill_level_sizes, zoom_band_scene


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _field(C=2, H=20, W=30, density=0.2, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-16, 16, size=(C, H, W)).astype(np.float32)
    w = np.where(rng.random((H, W)) < density, rng.choice(np.array([1, 0.5, 1e-3, 1e-6], np.float32), size=(H, W)), 0).astype(np.float32)
    return v, w


def test_level_sizes():
    assert fill_level_sizes(1, 1) == [(1, 1)]
    assert fill_level_sizes(1, 37) == [(1, 37), (1, 19), (1, 10), (1, 5), (1, 3), (1, 2), (1, 1)]
    assert fill_level_sizes(67, 131)[1:] == [(34, 66), (17, 33), (9, 17), (5, 9), (3, 5), (2, 3), (1, 2), (1, 1)]
    assert fill_level_sizes(442, 602)[3] == (56, 76) and len(fill_level_sizes(442, 602)) - 1 == 10
    assert fill_level_sizes(67, 131, 2) == [(67, 131), (34, 66), (17, 33)] and len(fill_level_sizes(5, 5, 9)) - 1 == 3


def test_trusted_pixels_keep_their_bits_and_the_rest_is_convex():
    for seed, region in ((0, None), (1, (2, 3, 15, 22)), (2, (7, 11, 1, 1))):
        v, w = _field(seed=seed)
        if region and region[2:] == (1, 1):
            w[7, 11] = 1
        ys, xs = np.nonzero(w == 1)
        w[ys[:2], xs[:2]] = (1.5, 1e30)
        out, filled, L = fill_holes_ref(v, w, region, dtype=np.float32)
        y0, x0, Ho, Wo = region or (0, 0, 20, 30)
        inR = np.zeros(w.shape, bool)
        inR[y0 : y0 + Ho, x0 : x0 + Wo] = True
        keep = inR & (w >= 1)
        assert keep.any() and np.array_equal(_bits(out[:, keep]), _bits(v[:, keep]))
        assert not out[:, ~inR].any() and not filled[~inR].any() and filled[inR].all()
        valid = inR & (w >= np.float32(1e-6))
        o64, _, _ = fill_holes_ref(v, w, region)
        for c in range(v.shape[0]):
            lo, hi = v[c][valid].min(), v[c][valid].max()
            eps = fill_bound(L, 16)
            assert o64[c][inR].min() >= lo - 1e-12 and o64[c][inR].max() <= hi + 1e-12, "convexity in float64"
            assert out[c][inR].min() >= lo - eps and out[c][inR].max() <= hi + eps


def test_constant_field_is_reproduced():
    v, w = _field(C=3, density=0.05, seed=3)
    for c, val in enumerate((2.5, -7.0, 0.1)):
        v[c] = val
    v[:, w == 0] = np.nan
    out, filled, _ = fill_holes_ref(v, w)
    assert filled.all()
    for c, val in enumerate((2.5, -7.0, 0.1)):
        assert np.abs(out[c] - np.float32(val)).max() <= 1e-12 * 16


def test_nothing_valid_gives_zeros():
    v, w = _field(seed=4)
    for region in (None, (1, 1, 9, 9)):
        out, filled, _ = fill_holes_ref(v, np.zeros_like(w), region)
        assert not out.any() and not filled.any()
        out, filled, _ = fill_holes_ref(v, np.full_like(w, 5e-7), region)
        assert not out.any() and not filled.any()


def test_one_valid_pixel_fills_the_region():
    v, w = _field(seed=5)
    w[:] = 0
    w[13, 4] = 0.25
    for region in (None, (3, 2, 14, 27)):
        out, filled, _ = fill_holes_ref(v, w, region)
        y0, x0, Ho, Wo = region or (0, 0, 20, 30)
        assert filled[y0 : y0 + Ho, x0 : x0 + Wo].all() and filled.sum() == Ho * Wo
        for c in range(2):
            assert np.abs(out[c, y0 : y0 + Ho, x0 : x0 + Wo] - v[c, 13, 4]).max() <= 1e-13


def test_limited_levels_leave_far_holes():
    v, w = _field(H=40, W=56, seed=6)
    w[:] = 0
    w[8, 8] = 1
    out, filled, L = fill_holes_ref(v, w, levels=2)
    assert L == 2
    # the pixel's level-2 cell is (2, 2); a pull reaches one cell beyond it per level
    assert filled[8, 8] == 1 and filled[:, 24:].sum() == 0 and filled[24:, :].sum() == 0 and 16 <= filled.sum() < 24 * 24
    assert not out[:, filled == 0].any()
    assert fill_holes_ref(v, w, levels=0)[1].all()
    assert np.array_equal(fill_holes_ref(v, w, levels=6)[0], fill_holes_ref(v, w, levels=0)[0]) and fill_holes_ref(v, w, levels=99)[2] == 6


def test_non_finite_values_do_not_leak():
    v, w = _field(C=3, seed=7)
    clean_v, clean_w = v.copy(), w.copy()
    holes = np.argwhere(w == 0)
    valid = np.argwhere(w > 0)
    for n, bad in enumerate((np.nan, np.inf, -np.inf)):            # in holes
        v[n, holes[n][0], holes[n][1]] = bad
    for n, bad in enumerate((np.nan, np.inf, -np.inf, -1.0)):      # weights that make a hole: the value under them is gone
        y, x = valid[n]
        w[y, x] = bad
        clean_w[y, x] = 0
    y, x = valid[5]                                                # a value that is not finite under a weight: a hole
    v[1, y, x] = np.nan
    clean_w[y, x] = 0
    out, filled, _ = fill_holes_ref(v, w)
    want, wfilled, _ = fill_holes_ref(clean_v, clean_w)
    assert np.isfinite(out).all() and np.array_equal(out, want) and np.array_equal(filled, wfilled)


def test_fp32_evaluation_stays_inside_the_first_order_bound():
    worst = 0.0
    for seed, (H, W, region) in enumerate(((24, 40, None), (70, 140, (1, 2, 67, 131)), (1, 37, None))):
        for density in (0.3, 0.05, 0.02):
            v, w = _field(C=2, H=H, W=W, density=density, seed=20 + seed)
            o64, f64, L = fill_holes_ref(v, w, region)
            o32, f32, _ = fill_holes_ref(v, w, region, dtype=np.float32)
            assert np.array_equal(f64, f32)
            worst = max(worst, float(np.abs(o32 - o64).max()) / fill_bound(L, 16))
    print("fp32 against float64: at most %.3f of 24 L 2^-24 max|v|" % worst)
    assert worst <= 1.0


def test_zoom_scene_quality():
    """A 5 % zoom over 64 x 96, R = (4, 6, 55, 83), 30 % random holes and a removed 8-column band.  The field is linear with a slope of
    0.05 px per pixel, and the pull interpolates between cell means: a hole with valid pixels in its own level-1 neighbourhood is
    off by the slope times a distance of at most 2 px, and the band (8 columns: bridged from level 3 / 4, cells of 8 / 16 px) by the
    slope times at most a 16-px cell.  Left at zero, a hole is off by the flow itself."""
    v, w, true, hole = zoom_band_scene()
    out, filled, _ = fill_holes_ref(v, w, (4, 6, 55, 83))
    inR = np.zeros(w.shape, bool)
    inR[4:59, 6:89] = True
    assert filled[inR].all()
    epe = np.hypot(*(out - true))
    kept = inR & ~hole
    assert np.array_equal(_bits(out[:, kept]), _bits(true[:, kept])), "kept pixels are exact"
    band = hole & (np.arange(96)[None, :] >= 40) & (np.arange(96)[None, :] < 48)
    zero = np.hypot(*true)
    print("holes: %d (band %d); end-point error over the holes: median %.4f px, maximum %.4f px (in the band: %s); left at zero: median %.3f px"
          % (hole.sum(), band.sum(), np.median(epe[hole]), epe[hole].max(), bool(epe[band].max() == epe[hole].max()), np.median(zero[hole])))
    assert np.median(epe[hole]) <= 0.05 * 2 and epe[hole].max() <= 0.05 * 16
    assert np.median(epe[hole]) < 0.1 * np.median(zero[hole])
