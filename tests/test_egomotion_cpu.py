"""CPU suite, next-row N4: the oracle's relative-pose restatement (sfm2.getEgoMotion2's role: radial/radial_opticalflow_data.lua:211-231)
on synthetic two-view geometry with a known answer.  sfm2 is un-vendored: parity with the reference is unpinned; what is pinned
here is the geometry (the planted pose comes back, the epipole is K T, the rotation-only warp is undone by removeEgoMotion)."""
import numpy as np
import pytest

from tests import oracle as orc
from tests import ref64
from tests.egomotion_cases import (  # noqa: F401  (two_views, rot_angle: imported from here by tests/test_gpu_multiscale_radial.py)
    two_views, rot_angle, POSE_NS, NOISY_NS, WEIGHT_FRACTIONS, FRAMES, FOE_SIZES, ARDRONE_DIST,
    EDGE_BAND, pose_pool, noisy_prefix, weight_case, t_angle, check_pose_algebra, recount64, frame_case,
    warp_ref, undistort_ref, behind_camera_case, radial_field, foe_min_flow, flow_case, flow_samples, check_noisy_pose,
)


def test_oracle_pose_recovers_the_planted_motion():
    p1, p2, K, R, T, nout = two_views()
    rc, Re, Te, ni, F = orc.ego_motion_from_points(p1, p2, K, 1.0, 512, 7)
    assert rc == 0
    assert abs(np.linalg.det(Re) - 1) < 1e-9 and np.abs(Re @ Re.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.norm(Te) - 1) < 1e-9
    assert rot_angle(R, Re) < 0.15                              # degrees
    assert np.degrees(np.arccos(np.clip(Te @ T, -1, 1))) < 2.0  # the direction of translation (its length is unobservable)
    n = len(p1)
    assert n - nout - 25 <= ni <= n - nout + 12                 # the consensus set = the non-outliers, give or take the noise tail
    # the fundamental matrix has rank 2, unit norm, and the true correspondences satisfy it
    assert abs(np.linalg.norm(F) - 1) < 1e-9 and abs(np.linalg.det(F)) < 1e-12
    h1 = np.concatenate([p1[nout:], np.ones((n - nout, 1), np.float32)], 1).astype(np.float64)
    h2 = np.concatenate([p2[nout:], np.ones((n - nout, 1), np.float32)], 1).astype(np.float64)
    l = h1 @ F.T
    d = np.abs((h2 * l).sum(1)) / np.hypot(l[:, 0], l[:, 1])
    assert np.median(d) < 0.3
    # the epipole in the current frame is K T (radial_opticalflow_data.lua:218-219)
    rc, e_est = orc.epipole(K, Te)
    rc2, e_true = orc.epipole(K, T)
    assert rc == 0 == rc2 and np.hypot(e_est[0] - e_true[0], e_est[1] - e_true[1]) < 20.0   # (2 degrees of T at f = 520 px)
    # deterministic for a seed; weights <= 0 exclude correspondences (here: every planted outlier -> all inliers)
    rc, Re2, Te2, ni2, _ = orc.ego_motion_from_points(p1, p2, K, 1.0, 512, 7)
    assert np.array_equal(Re, Re2) and np.array_equal(Te, Te2) and ni == ni2
    w = np.ones(n, np.float32)
    w[:nout] = 0
    rc, Re3, Te3, ni3, _ = orc.ego_motion_from_points(p1, p2, K, 1.0, 256, 3, weights=w)
    assert rc == 0 and rot_angle(R, Re3) < 0.15 and ni3 >= n - nout - 25
    # too few points / nothing consistent
    assert orc.ego_motion_from_points(p1[:5], p2[:5], K, 1.0, 16, 1)[0] != 0
    rng = np.random.default_rng(1)
    junk = rng.uniform(0, 400, (60, 2)).astype(np.float32)
    assert orc.ego_motion_from_points(junk, rng.uniform(0, 400, (60, 2)).astype(np.float32), K, 0.05, 64, 1)[0] != 0


def test_oracle_rotation_warp_and_undistortion_properties():
    """removeEgoMotion undoes a pure rotation (the reason the callers apply it before the polar warp); undistortImage with zero
    coefficients is the identity; the epipole of a sideways translation is at infinity."""
    rng = np.random.default_rng(0)
    H, W = 60, 80
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    smooth = np.stack([np.sin(xs / 9) + np.cos(ys / 7)] * 2).astype(np.float32)
    K = np.array([[90.0, 0, 40.0], [0, 88.0, 30.0], [0, 0, 1]])
    a = 0.04
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    w1, m1 = orc.remove_ego_motion(smooth, K, R)
    back, m2 = orc.remove_ego_motion(w1, K, R, inverse=True)
    ok = (m2 > 0) & (np.roll(m1, 0) > 0)
    ok[:, :8] = ok[:, -8:] = False
    ok[:6] = ok[-6:] = False
    assert ok.sum() > 1000 and np.abs(back - smooth)[:, ok].max() < 3e-2
    assert np.array_equal(orc.remove_ego_motion(smooth, K, np.eye(3))[0], smooth)
    assert np.abs(orc.undistort_image(smooth, K, np.zeros(5)) - smooth).max() < 1e-5
    und = orc.undistort_image(smooth, K, [-0.38, 0.21, 0.003, 0.0009, -0.07])
    assert np.abs(und - smooth)[:, 25:35, 35:45].max() < 0.02 and np.abs(und - smooth).max() > 0.05   # the centre barely moves, the corners do
    assert orc.epipole(K, [1.0, 0.0, 0.0])[0] != 0
    del rng


# ------------------------------------------------------------------------------------------------------------------------------------
# The size edges of the pose, warp and FOE code, against float64 references written from the definitions (tests/ref64.py); the cases are
# those of tests/egomotion_cases.py, which the device suite (tests/test_gpu_egomotion.py) runs through the kernels.
@pytest.mark.parametrize("N", POSE_NS)
def test_oracle_pose_at_the_size_edges(N):
    """Noise-free prefixes of one pool, 64 iterations, seed 5: the planted pose comes back, R is a rotation, |T| = 1, the returned F is
    the F of the returned pose, every point is an inlier and lies within 1e-3 px (Sampson, recounted in float64) of the returned F.
    Pose bounds: the inputs are rounded to float32 (2^-24 * 640 px = 4e-5 px, 4e-6 degrees at f = 520 px); 8 to 9 points amplify that by
    the conditioning of the minimal problem, hundreds of points average it: 1e-3 degrees for R and 1e-2 for T (measured: at most 2.9e-5
    and 8.7e-4 at N = 8, 3e-6 and 3.1e-5 from N = 63)."""
    p1, p2, K, R, T = pose_pool()
    a, b = p1[:N], p2[:N]
    rc, Re, Te, ni, F = orc.ego_motion_from_points(a, b, K, 1.0, 64, 5)
    assert rc == 0
    check_pose_algebra(K, Re, Te, F)
    assert rot_angle(R, Re) < 1e-3 and t_angle(T, Te) < 1e-2
    assert ni == N and ref64.sampson64(F, a, b).max() < 1e-3
    again = orc.ego_motion_from_points(a, b, K, 1.0, 64, 5)
    assert np.array_equal(Re, again[1]) and np.array_equal(Te, again[2]) and np.array_equal(F, again[4]) and ni == again[3]


@pytest.mark.parametrize("N", NOISY_NS)
def test_oracle_pose_with_noise_and_outliers(N):
    """0.15 px noise, a quarter uniform outliers, 256 iterations: egomotion_cases.check_noisy_pose (measured: 52/52, 196/196,
    12319/12331, 30084/30092 inliers; the pose 0.000 / 0.000 degrees from the float64 fit over the same set at N = 65 and 257)."""
    _, _, K, R, T = pose_pool()
    q1, q2 = noisy_prefix(N)
    rc, Re, Te, ni, F = orc.ego_motion_from_points(q1, q2, K, 1.0, 256, 5)
    assert rc == 0
    check_noisy_pose(N, Re, Te, ni, F, label="oracle")


@pytest.mark.parametrize("frac", WEIGHT_FRACTIONS)
def test_oracle_pose_with_sparse_weights(frac):
    """However few of the N = 20000 correspondences are valid, the draws are taken among the valid ones: the planted pose comes back and
    every valid point is an inlier.  (Drawing from all N and rejecting w <= 0 with 64 tries per slot returned rc = -2 at 1 % valid.)"""
    _, _, K, R, T = pose_pool()
    a, b, w = weight_case(frac)
    rc, Re, Te, ni, F = orc.ego_motion_from_points(a, b, K, 1.0, 512, 5, weights=w)
    assert rc == 0
    check_pose_algebra(K, Re, Te, F)
    assert rot_angle(R, Re) < 1e-3 and t_angle(T, Te) < 1e-2
    assert ni == int(w.sum()) == recount64(F, a, b, 1.0, w)
    # an all-ones weight vector draws what no weights draw; fewer than 8 valid is still the error
    assert np.array_equal(orc.ego_motion_from_points(a[:300], b[:300], K, 1.0, 64, 5, weights=np.ones(300, np.float32))[1],
                          orc.ego_motion_from_points(a[:300], b[:300], K, 1.0, 64, 5)[1])
    w7 = np.zeros(len(w), np.float32)
    w7[np.flatnonzero(w)[:7]] = 1
    assert orc.ego_motion_from_points(a, b, K, 1.0, 64, 5, weights=w7)[0] == -2


@pytest.mark.parametrize("C,H,W", FRAMES)
def test_warp_reference_edge_band_is_thin(C, H, W):
    """The pixels whose float64 source lies within EDGE_BAND of the frame edge -- where a float32 evaluation may decide the mask the other
    way, so the device suite leaves them out -- are at most 1 % of the frame; and the oracle meets the float64 reference elsewhere:
    equal masks, |out - ref64| <= coordinate error bound x largest neighbour difference around the source + 2^-22 (four roundings of the bilinear
    arithmetic on values in [0, 1))."""
    img, K, R = frame_case(C, H, W, skew=0.8 if (H, W) == (33, 257) else 0.0)
    for inverse in (False, True):
        r = warp_ref(C, H, W, inverse, skew=0.8 if (H, W) == (33, 257) else 0.0)
        gy, gx = ref64.local_lipschitz64(img, r["sy"], r["sx"])
        band = r["edge"] < EDGE_BAND
        assert band.sum() <= 0.01 * H * W
        out, mask = orc.remove_ego_motion(img, K, R, inverse=inverse)
        assert np.array_equal((mask > 0)[~band], r["mask"][~band])
        tol = r["cerr_x"] * gx + r["cerr_y"] * gy + 2.0 ** -22
        ok = r["mask"] & ~band
        assert (np.abs(out - r["out"])[:, ok] <= tol[ok]).all()
    assert np.array_equal(orc.remove_ego_motion(img, K, np.eye(3))[0], img)


def test_warp_reference_behind_the_camera():
    """1.4 rad about y under a wide-angle K: Z <= 0 on part of the frame, and most of those pixels have a source inside the frame if the
    sign of Z is ignored -- the case the Z > 0 test exists for.  Mask 0, output 0, nothing NaN there."""
    img, K, R = behind_camera_case()
    r = ref64.homography_warp64(img, K, R)
    behind = r["Z"] <= 0
    with np.errstate(invalid="ignore"):
        inside = (r["sx"] >= 0) & (r["sx"] <= 119) & (r["sy"] >= 0) & (r["sy"] <= 89)
    assert behind.sum() > 1000 and (behind & inside).sum() > 1000 and r["mask"].sum() > 1000
    out, mask = orc.remove_ego_motion(img, K, R)
    assert not np.isnan(out).any() and (mask[behind] == 0).all() and (out[:, behind] == 0).all()
    assert np.array_equal(mask > 0, r["mask"]) or ((mask > 0) != r["mask"])[r["edge"] >= EDGE_BAND].sum() == 0


@pytest.mark.parametrize("H,W", FOE_SIZES)
def test_oracle_foe_against_float64(H, W):
    flow, (cx, cy) = radial_field(H, W)
    mf = foe_min_flow(flow, 0.02)
    for it in (0, 2, 16):
        (rx, ry), rn = ref64.foe64(flow, None, mf, it)
        rc, (ox, oy), on = orc.foe_from_flow(flow, None, mf, it)
        assert rc == 0 and np.hypot(ox - rx, oy - ry) < 1e-6 and abs(on - rn) <= 1e-6 * rn
        assert np.hypot(rx - cx, ry - cy) < 1e-5


def test_oracle_foe_skips_zero_and_non_finite_vectors():
    """min_flow = 0 with zero vectors present, NaN / Inf vectors at min_flow = 0.5, conf <= 0 and NaN confidences: all skipped, the
    planted centre comes back (to 1e-5 px: the field is rounded to float32) and the weight sum counts the usable vectors only.  (A
    zero vector used to pass `mag < min_flow` at min_flow = 0 and a NaN passes it at any min_flow: 0 / 0 in the sums, rc = -1.)"""
    flow, (cx, cy) = radial_field(37, 53)
    f = flow.copy()
    f[:, 5, 7] = 0
    f[:, 20, 20:30] = 0
    rc, (ox, oy), on = orc.foe_from_flow(f, None, 0.0, 2)
    assert rc == 0 and np.hypot(ox - cx, oy - cy) < 1e-5 and abs(on - (37 * 53 - 11)) < 1e-3
    f = flow.copy()
    f[0, 5, 7] = np.nan
    f[1, 9, 9] = np.inf
    f[:, 3, 3] = np.nan
    f[1, 30, 40] = -np.inf
    (rx, ry), rn = ref64.foe64(f, None, 0.5, 2)
    rc, (ox, oy), on = orc.foe_from_flow(f, None, 0.5, 2)
    assert rc == 0 and np.hypot(ox - cx, oy - cy) < 1e-5 and np.hypot(ox - rx, oy - ry) < 1e-6 and abs(on - rn) <= 1e-6 * rn
    c = np.ones((37, 53), np.float32)
    c[10:20] = 0
    c[30, :] = -1
    c[3, 4] = np.nan
    (rx, ry), rn = ref64.foe64(flow, c, 0.5, 2)
    rc, (ox, oy), on = orc.foe_from_flow(flow, c, 0.5, 2)
    assert rc == 0 and np.hypot(ox - cx, oy - cy) < 1e-5 and np.hypot(ox - rx, oy - ry) < 1e-6 and abs(on - rn) <= 1e-6 * rn
    assert rn == float(((np.hypot(flow[0], flow[1]) >= 0.5) & (c > 0)).sum())
    # nothing usable / parallel flow: still an error
    assert orc.foe_from_flow(flow, np.zeros((37, 53), np.float32), 0.5, 2)[0] != 0
    par = np.zeros((2, 40, 50), np.float32)
    par[1] = 3.0
    assert orc.foe_from_flow(par, None, 0.5, 2)[0] != 0
