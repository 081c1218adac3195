"""GPU suite (-m gpu), part 10: the seven kernels of csrc/egopose.hip and csrc/egomotion.hip -- hypotheses, scoring, refit sums, flow
sampling, homography warp, undistortion, FOE sums -- at the sizes where their code takes another path: fewer points than a wave, one
partial block, the switch of the refit grid at N = 16384, the first frame above the warp's grid cap (256 * 32 blocks of 256 pixels), the
FOE's 256-block cap, sources behind the camera, sparse weights, zero-length and non-finite flow vectors.

References, independent of the kernels (tests/ref64.py, float64 numpy from the definitions): sampson64, fund_from_pose64,
homography_warp64, undistort64, foe64; the planted pose of the synthetic two-view geometry; and, as a second opinion only, the CPU
oracle (which restates the device code closely: agreement with it is kept at the project's 1e-6 / +-2 / 5e-5).
The cases are those of tests/egomotion_cases.py, which tests/test_egomotion_cpu.py runs through the oracle.  Every figure a test bounds
is printed before it is asserted (-s shows it).  Image outputs are written into buffers pre-filled with -7 that are 64 floats longer than
the result: the tail must keep its -7, the inside must lose every one."""
import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import ref64
from tests import egomotion_cases as cases
from tests.egomotion_cases import rot_angle, t_angle

pytestmark = pytest.mark.gpu

FILL, TAIL = -7.0, 64


def note(test, case, name, value, bound):
    print("%s %s: %s = %.3e (bound %.3e)" % (test, case, name, value, bound))


def T(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)                # (a copy: the shared cases are read-only)


def pose(dfe, cuda, p1, p2, K, iterations, seed, weights=None, max_dist=1.0):
    R, Tt, nf, ni, F = dfe.sfm2.getEgoMotion2(K, pts1=T(p1, cuda), pts2=T(p2, cuda), weights=T(weights, cuda) if weights is not None else None,
                                              ransacMaxDist=max_dist, iterations=iterations, seed=seed)
    return R.numpy(), Tt.numpy(), nf, ni, F.numpy()


def assert_matches_oracle(got, want):
    """the project's rule for the device against the oracle's restatement (same draws): R, T, F to 1e-6, inliers to +-2"""
    (R, Tt, _, ni, F), (rc, Ro, To, nio, Fo) = got, want
    assert rc == 0
    assert np.abs(R - Ro).max() < 1e-6 and np.abs(Tt - To).max() < 1e-6 and np.abs(F - Fo).max() < 1e-6 and abs(ni - nio) <= 2


# ------------------------------------------------------------------------------------------------------------------ 1. pose, size edges
@pytest.mark.parametrize("N", cases.POSE_NS)
def test_pose_at_the_size_edges(dfe, cuda, N):
    """Noise-free prefixes of one pool, 64 iterations, seed 5.  The planted pose comes back with at most 10 x the oracle's own error on
    the same input (floor 1e-4 degrees): both sides share the float32 rounding of the inputs, which dominates; the factor covers the
    FMA contraction of the device's double arithmetic.  R is a rotation and |T| = 1 to 1e-9, F is the F of the returned pose to 1e-9,
    every point is an inlier and within 1e-3 px (float64 Sampson distance) of the returned F; the oracle is met to 1e-6 / +-2; the same
    call twice gives the same bits."""
    p1, p2, K, R, Tt = cases.pose_pool()
    a, b = p1[:N], p2[:N]
    got = pose(dfe, cuda, a, b, K, 64, 5)
    want = orc.ego_motion_from_points(a, b, K, 1.0, 64, 5)
    Rg, Tg, nf, ni, Fg = got
    er, et = rot_angle(R, Rg), t_angle(Tt, Tg)
    br, bt = max(10 * rot_angle(R, want[1]), 1e-4), max(10 * t_angle(Tt, want[2]), 1e-4)
    d = ref64.sampson64(Fg, a, b).max()
    note("pose", N, "rotation error [deg]", er, br)
    note("pose", N, "T error [deg]", et, bt)
    note("pose", N, "max Sampson distance [px]", d, 1e-3)
    assert er <= br and et <= bt
    cases.check_pose_algebra(K, Rg, Tg, Fg)
    assert nf == N and ni == N and d < 1e-3
    assert_matches_oracle(got, want)
    again = pose(dfe, cuda, a, b, K, 64, 5)
    assert np.array_equal(Rg, again[0]) and np.array_equal(Tg, again[1]) and np.array_equal(Fg, again[4]) and ni == again[3]


@pytest.mark.parametrize("N", cases.NOISY_NS)
def test_pose_with_noise_and_outliers(dfe, cuda, N):
    """0.15 px noise, a quarter uniform outliers, 256 iterations: egomotion_cases.check_noisy_pose -- the planted pose within 0.15 / 2
    degrees (N = 65 and 257: twice the error of the float64 eight-point fit over the same inliers), nInliers at most the float64 recount
    of ALL points within ransacMaxDist of the returned F and at least 0.99 of it, and the pose equal to that float64 fit where the
    sets coincide -- then the oracle by the project's rule, and the same bits from a second call."""
    _, _, K, R, Tt = cases.pose_pool()
    q1, q2 = cases.noisy_prefix(N)
    got = pose(dfe, cuda, q1, q2, K, 256, 5)
    Rg, Tg, _, ni, Fg = got
    cases.check_noisy_pose(N, Rg, Tg, ni, Fg, label="device")
    assert_matches_oracle(got, orc.ego_motion_from_points(q1, q2, K, 1.0, 256, 5))
    again = pose(dfe, cuda, q1, q2, K, 256, 5)
    assert np.array_equal(Rg, again[0]) and np.array_equal(Tg, again[1]) and ni == again[3]


# --------------------------------------------------------------------------------------------------- 2. weights and the dense-flow entry
@pytest.mark.parametrize("frac", cases.WEIGHT_FRACTIONS)
def test_pose_with_sparse_weights(dfe, cuda, frac):
    """N = 20000 noise-free correspondences of which 20 %, 5 %, 2 %, 1 % are valid: the draws are taken among the valid ones, so the
    planted pose comes back with the bounds of test_pose_at_the_size_edges and every valid point is an inlier.  (Drawing from all N and
    rejecting w <= 0 after at most 64 tries per slot found no hypothesis at 1 %.)  All-ones weights give the bits of no weights; fewer
    than 8 valid correspondences is still the error."""
    _, _, K, R, Tt = cases.pose_pool()
    a, b, w = cases.weight_case(frac)
    got = pose(dfe, cuda, a, b, K, 512, 5, weights=w)
    want = orc.ego_motion_from_points(a, b, K, 1.0, 512, 5, weights=w)
    Rg, Tg, nf, ni, Fg = got
    br, bt = max(10 * rot_angle(R, want[1]), 1e-4), max(10 * t_angle(Tt, want[2]), 1e-4)
    note("weights", frac, "rotation error [deg]", rot_angle(R, Rg), br)
    note("weights", frac, "T error [deg]", t_angle(Tt, Tg), bt)
    assert rot_angle(R, Rg) <= br and t_angle(Tt, Tg) <= bt
    cases.check_pose_algebra(K, Rg, Tg, Fg)
    assert nf == int(w.sum()) == ni == cases.recount64(Fg, a, b, 1.0, w)
    assert_matches_oracle(got, want)
    ones = pose(dfe, cuda, a[:300], b[:300], K, 64, 5, weights=np.ones(300, np.float32))
    none = pose(dfe, cuda, a[:300], b[:300], K, 64, 5)
    assert np.array_equal(ones[0], none[0]) and np.array_equal(ones[1], none[1]) and np.array_equal(ones[4], none[4]) and ones[3] == none[3]
    w7 = np.zeros(len(w), np.float32)
    w7[np.flatnonzero(w)[:7]] = 1
    with pytest.raises(dfe.DfeError):
        pose(dfe, cuda, a, b, K, 64, 5, weights=w7)


@pytest.mark.parametrize("H,W,max_points,gentle", [(8, 8, 8, 1.0), (8, 8, 64, 0.1), (9, 17, 64, 1.0), (37, 53, 400, 1.0), (240, 320, 1500, 1.0),
                                                   (480, 640, 20000, 1.0)])
def test_pose_from_dense_flow(dfe, cuda, H, W, max_points, gentle):
    """The dense-flow entry on the analytic flow of the planted motion, grids with ragged sample counts (9, 45, 234, 1200 and 19200 samples:
    the last above the refit grid's switch, with confidences zero on all but 2 % of the pixels).  nFound is the numpy count of the
    documented centred grid under conf > 0, finite flow and both endpoints inside the frame; R, T, F and nInliers agree with the oracle
    on the same samples; one NaN and one Inf vector on sampled nodes are not counted and change nothing (the result has the bits of a
    run that switches those two nodes off by their confidence).  At 8 x 8 with 8 points only 4 of the 9 samples stay inside the frame: the
    error for fewer than 8 usable samples, on both sides; with every pixel a sample and a tenth of the translation a pose comes from 8 x 8 too."""
    flow, Ks = cases.flow_case(H, W, gentle)
    conf = np.ones((H, W), np.float32)
    if (H, W) == (480, 640):
        conf = (np.random.default_rng(5).random((H, W)) < 0.02).astype(np.float32)
    s1, s2, w, (sy, sx) = cases.flow_samples(flow, conf, max_points)
    nvalid = int(w.sum())

    def run(f, c):
        R, Tt, nf, ni, F = dfe.sfm2.getEgoMotion2(Ks, flow=T(f, cuda), confidences=T(c, cuda) if c is not None else None, maxPoints=max_points,
                                                  ransacMaxDist=0.5, iterations=256, seed=2)
        return R.numpy(), Tt.numpy(), nf, ni, F.numpy()

    want = orc.ego_motion_from_points(s1, s2, Ks, 0.5, 256, 2, weights=w)
    if nvalid < 8:
        assert (H, W, max_points) == (8, 8, 8) and want[0] != 0
        with pytest.raises(dfe.DfeError, match="only %d usable" % nvalid):
            run(flow, conf)
        return
    got = run(flow, conf)
    note("dense flow", (H, W, max_points), "nFound", got[2], nvalid)
    assert got[2] == nvalid
    assert_matches_oracle(got, want)
    if (H, W) != (480, 640):
        assert np.array_equal(run(flow, None)[0], got[0])                  # all-ones confidences = none
    # non-finite vectors on two valid sampled nodes
    v = np.flatnonzero(w)
    i, j = v[len(v) // 3], v[2 * len(v) // 3]
    bad, off = flow.copy(), conf.copy()
    bad[0, sy[i], sx[i]] = np.nan
    bad[1, sy[j], sx[j]] = np.inf
    off[sy[i], sx[i]] = off[sy[j], sx[j]] = 0
    g_bad, g_off = run(bad, conf), run(flow, off)
    assert g_bad[2] == g_off[2] == nvalid - 2 == int(cases.flow_samples(bad, conf, max_points)[2].sum())
    assert np.array_equal(g_bad[0], g_off[0]) and np.array_equal(g_bad[1], g_off[1]) and g_bad[3] == g_off[3]
    assert np.isfinite(g_bad[0]).all()


# ------------------------------------------------------------------------------------------------------------- 3. warp and undistort
def guarded_warp(dfe, cuda, img, K, R, inverse, with_mask=True):
    """dfe_remove_ego_motion_f32 through the raw ABI into guarded buffers -> (out [C][H][W], mask [H][W]) as numpy"""
    C, H, W = img.shape
    ctx = dfe.get_ctx(0)
    t = T(img, cuda)
    out = torch.full((C * H * W + TAIL,), FILL, device=cuda)
    mask = torch.full((H * W + TAIL,), FILL, device=cuda)
    ctx.check(dfe.lib().dfe_remove_ego_motion_f32(ctx.handle, t.data_ptr(), C, H, W, dfe.sfm2._d(K, 9), dfe.sfm2._d(R, 9), int(inverse), out.data_ptr(),
                                                  mask.data_ptr() if with_mask else None))
    o, m = out.cpu().numpy(), mask.cpu().numpy()
    assert (o[C * H * W:] == np.float32(FILL)).all() and not (o[: C * H * W] == np.float32(FILL)).any(), "warp: wrote behind the output / left pixels unwritten"
    if with_mask:
        assert (m[H * W:] == np.float32(FILL)).all() and not (m[: H * W] == np.float32(FILL)).any(), "warp: wrote behind the mask / left pixels unwritten"
    else:
        assert (m == np.float32(FILL)).all()
    return o[: C * H * W].reshape(C, H, W), m[: H * W].reshape(H, W)


def guarded_undistort(dfe, cuda, img, K, dist):
    C, H, W = img.shape
    ctx = dfe.get_ctx(0)
    t = T(img, cuda)
    out = torch.full((C * H * W + TAIL,), FILL, device=cuda)
    ctx.check(dfe.lib().dfe_undistort_image_f32(ctx.handle, t.data_ptr(), C, H, W, dfe.sfm2._d(K, 9), dfe.sfm2._d(dist, 5), out.data_ptr()))
    o = out.cpu().numpy()
    assert (o[C * H * W:] == np.float32(FILL)).all() and not (o[: C * H * W] == np.float32(FILL)).any(), "undistort: wrote behind the output / left pixels unwritten"
    return o[: C * H * W].reshape(C, H, W)


def skew_of(H, W):
    return 0.8 if (H, W) == (33, 257) else 0.0                             # one K with skew


@pytest.mark.parametrize("C,H,W", cases.FRAMES)
def test_warp_identity_and_small_rotation(dfe, cuda, C, H, W):
    """R = I returns the input bit for bit with a mask of ones (K I K^-1 is cleaned of its noise-level entries on the host).  A 0.02 /
    -0.015 rad rotation and its inverse against homography_warp64: the mask is the reference's except where the float64 source lies
    within 1e-3 px of the frame edge (at most 1 % of the frame: tests/test_egomotion_cpu.py checks that on the reference alone), and
    away from those pixels |out - ref64| <= (error bound of the float32 source coordinates, every rounding counted: homography_warp64
    states it) x (the largest neighbour difference of the image in the 3 x 3 cells around the source: ref64.local_lipschitz64) + 2^-22
    (four roundings of the bilinear arithmetic on values in [0, 1)).  Inside the band a pixel carries the reference's value or 0, and
    nothing anywhere is NaN.  Against the oracle, which differs by the FMA contraction of the coordinates only: the project's 5e-5
    (measured at most 1.2e-5 up to 257 wide).  From x = 1024 a coordinate ulp is 1.2e-4 px, times the unit gradient of white noise:
    5e-5 cannot hold at 1031 x 2039 (measured 2.6e-4).  The oracle is a float32 evaluation too and so within the same bound of the
    float64 reference: there the device is held to twice that bound against the oracle, per pixel."""
    img, K, R = cases.frame_case(C, H, W, skew_of(H, W))
    out, mask = guarded_warp(dfe, cuda, img, K, np.eye(3), False)
    assert np.array_equal(out, img) and (mask == 1).all()
    assert np.array_equal(guarded_warp(dfe, cuda, img, K, np.eye(3), True, with_mask=False)[0], img)
    for inverse in (False, True):
        r = cases.warp_ref(C, H, W, inverse, skew_of(H, W))
        gy, gx = ref64.local_lipschitz64(img, r["sy"], r["sx"])
        out, mask = guarded_warp(dfe, cuda, img, K, R, inverse)
        band = r["edge"] < cases.EDGE_BAND
        ok = r["mask"] & ~band
        tol = r["cerr_x"] * gx + r["cerr_y"] * gy + 2.0 ** -22
        err = np.abs(out - r["out"]).max(0)
        oo, om = orc.remove_ego_motion(img, K, R, inverse=inverse)
        otol = np.full((H, W), 5e-5) if max(H, W) <= 1024 else 2 * tol
        note("warp", (C, H, W, inverse), "edge-band pixels", band.sum(), 0.01 * H * W)
        note("warp", (C, H, W, inverse), "max |out - ref64|", err[ok].max() if ok.any() else 0, tol[ok].max() if ok.any() else 0)
        note("warp", (C, H, W, inverse), "max |out - oracle|", np.abs(out - oo).max(0)[ok].max() if ok.any() else 0, otol[ok].max() if ok.any() else 0)
        assert band.sum() <= 0.01 * H * W
        assert set(np.unique(mask)) <= {0.0, 1.0} and np.array_equal((mask > 0)[~band], r["mask"][~band])
        assert (err[ok] <= tol[ok]).all() and (out[:, ~r["mask"] & ~band] == 0).all()
        berr = np.abs(out - r["val"]).max(0)[band]                         # on the edge: the sample there, or 0
        assert np.isfinite(out).all() and ((berr <= tol[band]) | (out[:, band] == 0).all(0)).all()
        assert np.array_equal((mask > 0)[~band], (om > 0)[~band]) and (np.abs(out - oo).max(0)[ok] <= otol[ok]).all()


def test_warp_behind_the_camera(dfe, cuda):
    """1.4 rad about y under a wide-angle K at 90 x 120: Z <= 0 on 5130 pixels, 4042 of which would find a source inside the frame if the
    sign of Z were ignored.  Mask 0 and output 0 there, nothing NaN, and the rest of the frame meets the float64 reference."""
    img, K, R = cases.behind_camera_case()
    r = ref64.homography_warp64(img, K, R)
    out, mask = guarded_warp(dfe, cuda, img, K, R, False)
    behind = r["Z"] <= 0
    assert behind.sum() > 1000 and not np.isnan(out).any() and not np.isnan(mask).any()
    assert (mask[behind] == 0).all() and (out[:, behind] == 0).all()
    band = r["edge"] < cases.EDGE_BAND
    gy, gx = ref64.local_lipschitz64(img, r["sy"], r["sx"])
    ok = r["mask"] & ~band
    assert ok.sum() > 1000 and np.array_equal((mask > 0)[~band], r["mask"][~band])
    tol = r["cerr_x"] * gx + r["cerr_y"] * gy + 2.0 ** -22
    err = np.abs(out - r["out"]).max(0)
    note("warp behind", (2, 90, 120), "max |out - ref64|", err[ok].max(), tol[ok].max())
    assert (err[ok] <= tol[ok]).all()


@pytest.mark.parametrize("C,H,W", cases.FRAMES)
def test_undistort(dfe, cuda, C, H, W):
    """The ardrone coefficients and zeros against undistort64, by the rule of the warp: inside / outside decided as the reference does
    except within 1e-3 px of the frame edge, and |out - ref64| <= (counted rounding budget of the coordinates: ref64._undistort_budget) x
    (largest neighbour difference around the source) + 2^-22.
    Zero coefficients map every pixel onto itself, so the whole border is ON the edge: a border pixel either reproduces the input or,
    where the float32 round trip ((x - cx) / fx) fx + cx lands an ulp outside, is 0.  The project's 1e-5 for zeros holds where a
    coordinate ulp times the unit gradient of white noise is below it (up to 120 wide: ulp 7.6e-6 px); above, the derived bound."""
    img, K, _ = cases.frame_case(C, H, W)
    for dist in (cases.ARDRONE_DIST, (0.0,) * 5):
        r = cases.undistort_ref(C, H, W, dist)
        gy, gx = ref64.local_lipschitz64(img, r["sy"], r["sx"])
        out = guarded_undistort(dfe, cuda, img, K, dist)
        band = r["edge"] < cases.EDGE_BAND
        ok = r["mask"] & ~band
        tol = r["cerr_x"] * gx + r["cerr_y"] * gy + 2.0 ** -22
        if not any(dist) and max(H, W) <= 128:
            tol = np.minimum(tol, 1e-5)
        err = np.abs(out - r["out"]).max(0)
        note("undistort", (C, H, W, dist[0]), "edge-band pixels", band.sum(), H * W)
        note("undistort", (C, H, W, dist[0]), "max |out - ref64|", err[ok].max() if ok.any() else 0, tol[ok].max() if ok.any() else 0)
        assert (err[ok] <= tol[ok]).all() and (out[:, ~r["mask"] & ~band] == 0).all()
        berr = np.abs(out - r["val"]).max(0)[band]                         # on the edge: the sample there, or 0
        assert np.isfinite(out).all() and ((berr <= tol[band]) | (out[:, band] == 0).all(0)).all()


# ------------------------------------------------------------------------------------------------------------------------------ 4. FOE
def foe(dfe, cuda, flow, conf, min_flow, iterations):
    return dfe.sfm2.getFOEFromFlow(T(flow, cuda), T(conf, cuda) if conf is not None else None, min_flow=min_flow, iterations=iterations)


@pytest.mark.parametrize("H,W", cases.FOE_SIZES)
def test_foe_against_float64(dfe, cuda, H, W):
    """Planted radial fields flow = 0.05 (p - c), c off-centre at a sub-pixel position: one partial block, exactly one block, ragged
    blocks, the 256-block cap with many trips.  Against foe64 within 1e-6 px and the weight sum within 1e-6 relative (both sides sum in
    double; the kernel's unit normals carry a float32 rounding each, 6e-8 rad x at most 2400 px from c, averaged over the frame), at 0, 2
    and 16 re-weightings."""
    flow, (cx, cy) = cases.radial_field(H, W)
    mf = cases.foe_min_flow(flow, 0.02)
    for it in (0, 2, 16):
        (rx, ry), rn = ref64.foe64(flow, None, mf, it)
        (gx, gy), gn = foe(dfe, cuda, flow, None, mf, it)
        note("foe", (H, W, it), "|foe - foe64| [px]", np.hypot(gx - rx, gy - ry), 1e-6)
        note("foe", (H, W, it), "weight sum, relative", abs(gn - rn) / rn, 1e-6)
        assert np.hypot(gx - rx, gy - ry) < 1e-6 and abs(gn - rn) <= 1e-6 * rn
        rc, (ox, oy), on = orc.foe_from_flow(flow, None, mf, it)
        assert rc == 0 and abs(ox - gx) < 1e-6 and abs(oy - gy) < 1e-6 and abs(on - gn) < 1e-6 * gn


def test_foe_outliers_unusable_vectors_and_errors(dfe, cuda):
    """A 40 x 60 block of uniform outliers, 4 re-weightings: within 1 px of the planted centre.  Zero vectors at min_flow = 0, NaN / Inf
    vectors at min_flow = 0.5, conf <= 0 and NaN confidences are skipped: the planted centre comes back (1e-5 px: the field is rounded to
    float32), foe64 is met to 1e-6 and the weight sum counts the usable vectors.  Parallel flow and an all-masked field raise DfeError."""
    flow, (cx, cy) = cases.radial_field(240, 320)
    bad = flow.copy()
    bad[:, 20:60, 30:90] = np.random.default_rng(2).uniform(-8, 8, (2, 40, 60)).astype(np.float32)
    (hx, hy), _ = foe(dfe, cuda, bad, None, 1.0, 4)
    (rx, ry), _ = ref64.foe64(bad, None, 1.0, 4)
    note("foe outliers", (240, 320), "|foe - c| [px]", np.hypot(hx - cx, hy - cy), 1.0)
    note("foe outliers", (240, 320), "|foe64 - c| [px]", np.hypot(rx - cx, ry - cy), 1.0)
    assert abs(hx - cx) < 1.0 and abs(hy - cy) < 1.0

    flow, (cx, cy) = cases.radial_field(37, 53)
    zero = flow.copy()
    zero[:, 5, 7] = 0
    zero[:, 20, 20:30] = 0
    nanf = flow.copy()
    nanf[0, 5, 7] = np.nan
    nanf[1, 9, 9] = np.inf
    nanf[:, 3, 3] = np.nan
    nanf[1, 30, 40] = -np.inf
    conf = np.ones((37, 53), np.float32)
    conf[10:20] = 0
    conf[30, :] = -1
    conf[3, 4] = np.nan
    for name, f, c, mf in (("zero vectors", zero, None, 0.0), ("non-finite vectors", nanf, None, 0.5), ("confidences", flow, conf, 0.5)):
        (rx, ry), rn = ref64.foe64(f, c, mf, 2)
        (gx, gy), gn = foe(dfe, cuda, f, c, mf, 2)
        note("foe skips", name, "|foe - c| [px]", np.hypot(gx - cx, gy - cy), 1e-5)
        note("foe skips", name, "|foe - foe64| [px]", np.hypot(gx - rx, gy - ry), 1e-6)
        assert np.hypot(gx - cx, gy - cy) < 1e-5 and np.hypot(gx - rx, gy - ry) < 1e-6 and abs(gn - rn) <= 1e-6 * rn
    assert ref64.foe64(zero, None, 0.0, 2)[1] == 37 * 53 - 11
    with pytest.raises(dfe.DfeError):
        foe(dfe, cuda, flow, np.zeros((37, 53), np.float32), 0.5, 2)
    par = np.zeros((2, 40, 50), np.float32)
    par[1] = 3.0
    with pytest.raises(dfe.DfeError):
        foe(dfe, cuda, par, None, 0.5, 2)
