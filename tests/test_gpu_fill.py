"""Hole filling on the device (include/dfe.h): dfe_fill_holes_f32 against the float64 restatement of its definition
(tests/fill_ref64.py) on random sparse fields that hold every edge case, the per-level kernels against the apex kernel bit for bit, and
flowDepthPair(..., fill=True) against the composition of the public calls it stands for.  Every output is pre-filled with a sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.consistency_ref64 import occlusion_scene
from tests.fill_ref64 import fill_bound, fill_holes_ref, fill_level_sizes
from tests.test_consistency_ref_cpu import SCENE

DFE_E_ARG, DFE_E_SHAPE = -1, -2
FILL = -7.0
# frame -> R; the last: L = 8 with an odd size at every level (67 x 131, 34 x 66, 17 x 33, 9 x 17, 5 x 9, 3 x 5, 2 x 3, 1 x 2, 1 x 1)
SHAPES = {
    "whole": ((24, 40), (0, 0, 24, 40)),
    "inner": ((24, 40), (3, 5, 17, 29)),
    "pixel": ((24, 40), (11, 19, 1, 1)),
    "row": ((1, 37), (0, 0, 1, 37)),
    "odd": ((70, 140), (1, 2, 67, 131)),
}
DENSITIES = (0.3, 0.05, 0.02)
WEIGHTS = np.array([1, 0.5, 1e-3, 1e-6], np.float32)


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def sparse_field(C_, shape, region, density, seed):
    """v [C][H][W] in +-16, w [H][W]: a share `density` of valid pixels with weights from WEIGHTS, the rest 0; planted inside R (where it
    has room): NaN / Inf values in holes, NaN / Inf / negative / 5e-7 weights, a non-finite value under w = 1, and weights above 1."""
    H, W = shape
    y0, x0, Ho, Wo = region
    rng = np.random.default_rng(seed)
    v = rng.uniform(-16, 16, size=(C_, H, W)).astype(np.float32)
    valid = rng.random((H, W)) < density
    w = np.where(valid, WEIGHTS[rng.integers(0, 4, size=(H, W))], 0).astype(np.float32)
    cells = rng.permutation(Ho * Wo)[:12]
    if cells.size == 12:
        py, px = y0 + cells // Wo, x0 + cells % Wo
        c = rng.integers(0, C_, size=12)
        w[py[:3], px[:3]] = 0                                   # holes with NaN, +Inf, -Inf in one channel
        v[c[0], py[0], px[0]], v[c[1], py[1], px[1]], v[c[2], py[2], px[2]] = np.nan, np.inf, -np.inf
        w[py[3:7], px[3:7]] = (np.nan, np.inf, -0.5, 5e-7)      # weights that make a hole
        w[py[7:9], px[7:9]] = 1                                 # a trusted weight over a value that is not finite: a hole
        v[c[7], py[7], px[7]], v[c[8], py[8], px[8]] = np.nan, np.inf
        w[py[9:12], px[9:12]] = (1.5, 2.0, 1e30)                # above 1: fully trusted
    return v, w


def fill(dfe, cuda, v, w, region, levels=0, want_filled=True, inplace=False):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C_, H, W = v.shape
    tv, tw = _dev(cuda, v), _dev(cuda, w)
    out = tv if inplace else torch.full((C_, H, W), FILL, device=cuda)
    filled = torch.full((H, W), FILL, device=cuda)
    ctx.check(lib.dfe_fill_holes_f32(ctx.handle, tv.data_ptr(), C_, H, W, tw.data_ptr(), *region, levels, out.data_ptr(), filled.data_ptr() if want_filled else None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), filled.cpu().numpy()


def _inside(shape, region):
    m = np.zeros(shape, bool)
    m[region[0] : region[0] + region[2], region[1] : region[1] + region[3]] = True
    return m


def check_against_ref(out, filled, v, w, region, levels):
    """the assertions of the operator against the float64 restatement; returns |out - ref| / bound at its largest"""
    ref, rfilled, L = fill_holes_ref(v, w, region, levels)
    inR = _inside(w.shape, region)
    assert not (out == FILL).any() and not (filled == FILL).any(), "an element was not written"
    assert not out[:, ~inR].any() and not filled[~inR].any(), "border not zero"
    assert np.array_equal(_bits(filled), _bits(rfilled)), "filled: %d pixels differ" % np.count_nonzero(filled != rfilled)
    assert np.isfinite(out).all(), "a non-finite value leaked"
    with np.errstate(invalid="ignore"):
        a0 = inR & np.isfinite(w) & (w >= np.float32(1e-6)) & np.isfinite(v).all(axis=0)
    vmax = float(np.abs(v[:, a0]).max()) if a0.any() else 0.0
    bound = fill_bound(L, vmax)
    d = float(np.abs(out.astype(np.float64) - ref).max())
    assert d <= bound, "max |out - ref| = %.3g above %.3g" % (d, bound)
    keep = a0 & (w >= 1)
    assert np.array_equal(_bits(out[:, keep]), _bits(v[:, keep])), "a fully trusted pixel lost its bits"
    return d / bound if bound else 0.0


# ---- 1. the operator against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_against_float64(dfe, cuda, name, C_):
    shape, region = SHAPES[name]
    worst = 0.0
    for i, density in enumerate(DENSITIES):
        v, w = sparse_field(C_, shape, region, density, seed=10 * C_ + i)
        if region[2:] == (1, 1):
            w[region[0], region[1]] = (1, 0.5, 0)[i]      # the one pixel: trusted, half trusted, a hole
        out, filled = fill(dfe, cuda, v, w, region)
        worst = max(worst, check_against_ref(out, filled, v, w, region, 0))
        if i == 0:   # filled == NULL
            out2, filled2 = fill(dfe, cuda, v, w, region, want_filled=False)
            assert np.array_equal(_bits(out2), _bits(out)) and (filled2 == FILL).all()
            if region[2] * region[3] > 100:
                assert 0 < np.count_nonzero(w[_inside(shape, region)] >= np.float32(1e-6)) and filled[_inside(shape, region)].all()
    print("%s C=%d: max |out - ref| / bound = %.4f" % (name, C_, worst))


# ---- 2. bit preservation and dead ends -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inner", "odd"])
def test_zero_weights_and_limited_levels(dfe, cuda, name):
    shape, region = SHAPES[name]
    v, w = sparse_field(2, shape, region, 0.02, seed=5)
    out, filled = fill(dfe, cuda, v, np.zeros_like(w), region)
    assert not out.any() and not filled.any(), "nothing valid: zeros"
    inR = _inside(shape, region)
    for levels in (1, 2):
        out, filled = fill(dfe, cuda, v, w, region, levels=levels)
        check_against_ref(out, filled, v, w, region, levels)
        assert filled[inR].any() and not filled[inR].all(), "levels = %d: islands expected" % levels
        assert not out[:, filled == 0].any()
    # more levels than the region has: the full pyramid
    full, ffull = fill(dfe, cuda, v, w, region)
    many, fmany = fill(dfe, cuda, v, w, region, levels=40)
    assert np.array_equal(_bits(many), _bits(full)) and np.array_equal(_bits(fmany), _bits(ffull))


# ---- 3. the per-level kernels and the apex kernel -------------------------------------------------------------------------------------
def launches(dfe, cuda, v, w, region, apex, levels=0):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    ctx.set_option("fill_apex", apex)
    ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
    try:
        out, filled = fill(dfe, cuda, v, w, region, levels=levels)
        ms, n = C.c_double(), C.c_int()
        ctx.check(lib.dfe_profile_read(ctx.handle, C.byref(ms), C.byref(n)))
    finally:
        ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
        ctx.set_option("fill_apex", None)
    return out, filled, n.value


@pytest.mark.gpu
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_hand_over_between_the_two_forms(dfe, cuda, C_):
    """70 x 140, R = 67 x 131, L = 8.  fill_apex = 0: 8 pushes + 8 pulls; 64: the apex from level 4 (5 x 9 = 45 cells; level 3 has 153),
    4 + 1 + 4; 1024: from level 2 (17 x 33 = 561; level 1 has 2244), 2 + 1 + 2; automatic: the whole pyramid, 11804 cells x (C + 1) x 4 B,
    fits the 160 KB of LDS for C <= 2 (one launch), and from level 1 (3027 cells up to the top) for C = 3, 4 (1 + 1 + 1)."""
    shape, region = SHAPES["odd"]
    sizes = fill_level_sizes(region[2], region[3])
    assert len(sizes) - 1 == 8 and sizes[4] == (5, 9) and sizes[2] == (17, 33)
    assert sum(h * w for h, w in sizes) == 11804 and (11804 * (C_ + 1) * 4 <= 160 * 1024) == (C_ <= 2)
    v, w = sparse_field(C_, shape, region, 0.05, seed=40 + C_)
    want = {0: 16, 64: 9, 1024: 5, -1: 1 if C_ <= 2 else 3}
    base = None
    for apex, n_want in want.items():
        out, filled, n = launches(dfe, cuda, v, w, region, apex)
        assert n == n_want, "fill_apex = %d: %d launches, %d planned" % (apex, n, n_want)
        if base is None:
            base = (out, filled)
            check_against_ref(out, filled, v, w, region, 0)
        assert np.array_equal(_bits(out), _bits(base[0])) and np.array_equal(_bits(filled), _bits(base[1])), "fill_apex = %d: other bits" % apex
    # a limited pyramid through the apex: levels = 3 leaves levels 0 .. 3, the apex from level 2 is 1 level high
    o0, f0, n0 = launches(dfe, cuda, v, w, region, 0, levels=3)
    o1, f1, n1 = launches(dfe, cuda, v, w, region, 1024, levels=3)
    assert (n0, n1) == (6, 5) and np.array_equal(_bits(o0), _bits(o1)) and np.array_equal(_bits(f0), _bits(f1))
    check_against_ref(o1, f1, v, w, region, 3)
    # small frames: one launch whatever the region, except where the frame is more than twice the region (the border is the grid's work)
    for name, n_want in (("whole", 1), ("inner", 1), ("row", 1), ("pixel", 1)):
        shape2, region2 = SHAPES[name]
        v2, w2 = sparse_field(C_, shape2, region2, 0.3, seed=50)
        w2[region2[0], region2[1]] = 1
        oa, fa, na = launches(dfe, cuda, v2, w2, region2, -1)
        ob, fb, nb = launches(dfe, cuda, v2, w2, region2, 0)
        L = len(fill_level_sizes(region2[2], region2[3])) - 1
        assert na == n_want and nb == max(2 * L, 1), (name, na, nb)
        assert np.array_equal(_bits(oa), _bits(ob)) and np.array_equal(_bits(fa), _bits(fb)), name


# ---- 4. in place ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("apex", [0, 64, -1])
@pytest.mark.parametrize("name", ["inner", "odd"])
def test_in_place(dfe, cuda, name, apex):
    shape, region = SHAPES[name]
    v, w = sparse_field(2, shape, region, 0.05, seed=7)
    dfe.get_ctx(0).set_option("fill_apex", apex)
    out, filled = fill(dfe, cuda, v, w, region)
    out2, filled2 = fill(dfe, cuda, v, w, region, inplace=True)
    assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(filled2), _bits(filled))


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_launch_nothing(dfe, cuda):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W = 24, 40
    v = torch.zeros((4, H, W), device=cuda)
    w = torch.ones((H, W), device=cuda)
    out = torch.full((5, H, W), FILL, device=cuda)
    filled = torch.full((H, W), FILL, device=cuda)
    vp, wp, op, fp = v.data_ptr(), w.data_ptr(), out.data_ptr(), filled.data_ptr()
    fn = lib.dfe_fill_holes_f32
    for C_ in (0, 5, -1):
        assert fn(ctx.handle, vp, C_, H, W, wp, 0, 0, H, W, 0, op, fp) == DFE_E_ARG, C_
    for reg in ((0, 0, H + 1, W), (0, 0, H, W + 1), (-1, 0, H, W), (0, -1, H, W), (1, 0, H, W), (0, 1, H, W), (0, 0, 0, W), (0, 0, H, 0), (0, 0, H, -3),
                (2**31 - 1, 0, 1, 1), (0, 0, 1, 2**31 - 1)):
        assert fn(ctx.handle, vp, 2, H, W, wp, *reg, 0, op, fp) == DFE_E_SHAPE, reg
        assert lib.dfe_last_error(ctx.handle).startswith(b"dfe_fill_holes_f32: region")
    assert fn(ctx.handle, vp, 2, 0, W, wp, 0, 0, 1, 1, 0, op, fp) == DFE_E_SHAPE
    assert fn(ctx.handle, vp, 2, H, W, wp, 0, 0, H, W, -1, op, fp) == DFE_E_ARG and b"levels" in lib.dfe_last_error(ctx.handle)
    assert fn(ctx.handle, None, 2, H, W, wp, 0, 0, H, W, 0, op, fp) == DFE_E_ARG
    assert fn(ctx.handle, vp, 2, H, W, None, 0, 0, H, W, 0, op, fp) == DFE_E_ARG
    assert fn(ctx.handle, vp, 2, H, W, wp, 0, 0, H, W, 0, None, fp) == DFE_E_ARG
    assert fn(None, vp, 2, H, W, wp, 0, 0, H, W, 0, op, fp) == DFE_E_ARG
    torch.cuda.synchronize()
    assert (out == FILL).all() and (filled == FILL).all(), "a refused call wrote an output"
    with pytest.raises(dfe.DfeError):
        dfe.fillHoles(v[:2], w, levels=-1)
    with pytest.raises(dfe.DfeError):
        dfe.fillHoles(v[:2], w, region=(0, 0, H, W + 1))
    with pytest.raises(ValueError):
        dfe.fillHoles(v[:2], w[:, :5])
    with pytest.raises(ValueError):
        dfe.fillHoles(out, w)
    with pytest.raises(TypeError):
        dfe.fillHoles(v[:2].double(), w)
    # the Python call is the C call
    vv, ww = sparse_field(2, (H, W), SHAPES["inner"][1], 0.3, seed=3)
    o, f = dfe.fillHoles(_dev(cuda, vv), _dev(cuda, ww), region=SHAPES["inner"][1], levels=2)
    eo, ef = fill(dfe, cuda, vv, ww, SHAPES["inner"][1], levels=2)
    assert np.array_equal(_bits(o.cpu().numpy()), _bits(eo)) and np.array_equal(_bits(f.cpu().numpy()), _bits(ef))


# ---- 6. flowDepthPair(..., fill=True) ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tol", [None, 1.0])
def test_flow_depth_pair_fill(dfe, cuda, tol):
    """The occlusion scene of tests/test_consistency_ref_cpu.py (64 x 96, k = 5, a 9 x 9 window): the new keys are the composition of the
    public calls, the old keys are untouched, everything in R is filled, and -- the point of the feature -- the dense flow is closer to
    the background's motion on the band that the rectangle covers than the step's own flow there.  That needs the band to be REJECTED
    first: "below" is asserted with consistency=tol.  Without it every pixel of this scene passes extractOutput with a score above 0 (the
    CPU oracle's scores and the float64 restatement say so: no hole in R, dense flow = flow), so there the assertion is "not above"."""
    s = SCENE
    H, W, k, win = s["H"], s["W"], s["k"], s["win"]
    Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
    R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo)
    f0, f1, covered, _ = occlusion_scene(H, W, s["bg"], s["fg"], s["rect"], (win - 1) // 2 + (k - 1) // 2, R, seed=0)
    t0, t1 = _dev(cuda, f0), _dev(cuda, f1)
    foe = (W / 2.0, H / 2.0)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    old = dfe.flowDepthPair(t0, t1, k, win, win, foe, consistency=tol)
    new = dfe.flowDepthPair(t0, t1, k, win, win, foe, consistency=tol, fill=True)
    assert sorted(new) == sorted(list(old) + ["flow_dense", "filled", "depth_dense"])
    for key in old:
        assert np.array_equal(_bits(new[key].cpu().numpy()), _bits(old[key].cpu().numpy())), key
    # the composition of the public calls
    wgt = (old["scores"] > 0).float()
    if tol is not None:
        wgt = wgt * old["consistent"]
    dense, filled = dfe.fillHoles(old["flow"], wgt, R, 0)
    depth, conf = (torch.full((H, W), FILL, device=cuda) for _ in range(2))
    ctx.check(lib.dfe_flow_to_depth_cartesian(ctx.handle, dense.data_ptr(), H, W, foe[0], foe[1], 0, depth.data_ptr(), conf.data_ptr()))
    torch.cuda.synchronize()
    for key, want in (("flow_dense", dense), ("filled", filled), ("depth_dense", depth)):
        assert np.array_equal(_bits(new[key].cpu().numpy()), _bits(want.cpu().numpy())), key
    inR = _inside((H, W), R)
    g, wg = new["filled"].cpu().numpy(), wgt.cpu().numpy()
    assert g[inR].all() and not g[~inR].any()
    assert 0.3 < wg[inR].mean() <= 1.0 and (tol is None or wg[inR].mean() < 1.0), "the scene has kept pixels and, with the mask, holes"
    flow, fd = new["flow"].cpu().numpy(), new["flow_dense"].cpu().numpy()
    kept = inR & (wg == 1)
    assert np.array_equal(_bits(fd[:, kept]), _bits(flow[:, kept])), "kept pixels keep their flow"
    bg = np.array(s["bg"], np.float32).reshape(2, 1)
    epe = lambda f: float(np.median(np.hypot(*(f[:, covered] - bg))))
    print("consistency=%s: covered band (%d pixels, %d of them holes): median end-point error %.3f px filled, %.3f px as the step leaves it"
          % (tol, covered.sum(), np.count_nonzero(wg[covered] == 0), epe(fd), epe(flow)))
    assert epe(fd) < epe(flow) if tol is not None else epe(fd) <= epe(flow)
    # a finite levels through the one-call
    two = dfe.flowDepthPair(t0, t1, k, win, win, foe, consistency=tol, fill=2)
    d2, g2 = dfe.fillHoles(old["flow"], wgt, R, 2)
    assert np.array_equal(_bits(two["flow_dense"].cpu().numpy()), _bits(d2.cpu().numpy())) and np.array_equal(_bits(two["filled"].cpu().numpy()), _bits(g2.cpu().numpy()))
    # depth_dense against the step's own depth where the flow was kept
    dd, d = new["depth_dense"].cpu().numpy(), new["depth"].cpu().numpy()
    assert np.array_equal(_bits(dd[kept]), _bits(d[kept])), "depth of a kept pixel: %d differ" % np.count_nonzero(_bits(dd[kept]) != _bits(d[kept]))
