"""GPU suite (-m gpu), part 11: the kernels of csrc/tracker.hip -- corner response, corner selection, pyramid step, pyramidal
Lucas-Kanade -- each against the float64 reference written from its definition (tests/tracker_ref64.py, itself pinned against planted
truths by tests/test_tracker_ref_cpu.py), and the one-call route two images -> pose against the hybrid route (the device's corners ->
lk64 -> the oracle's pose).  Every figure a test bounds is printed before it is asserted (-s shows it).  Outputs are written into
buffers pre-filled with -7 that are 64 elements longer than the result: the tail must keep its -7."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import oracle as orc
from tests import tracker_ref64 as tr
from tests.egomotion_cases import check_pose_algebra, rot_angle, t_angle
from tests.tracker_cases import MIN_EIG, TRACKER_CASES, tracker_points

pytestmark = pytest.mark.gpu

FILL, TAIL = -7.0, 64
E_ARG = -1                                                        # DFE_E_ARG (include/dfe.h)
# largest |device - lk64| position difference at eps = 0 over the tracker cases below, measured on an MI355X: 1.378e-5 px (the win 3 case;
# the others 1.9e-6 .. 1.34e-5 -- DESIGN 4.23, profiles/tracker_pytest_gpu.log).  The bound is 4 x it (FMA contraction and reduction order
# differ between compilers) and never more than 0.002 px.
LK_MEASURED = 1.378e-5
LK_BOUND = min(4 * LK_MEASURED, 0.002)


def note(test, case, name, value, bound):
    print("%s %s: %s = %.3e (bound %.3e)" % (test, case, name, value, bound))


def T(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def guarded(n, cuda, dtype=torch.float32):
    return torch.full((n + TAIL,), FILL, device=cuda, dtype=dtype)


def unguard(buf, n, what, written=True):
    b = buf.cpu().numpy()
    assert (b[n:] == FILL).all(), "%s: wrote behind the output" % what
    if written and b.dtype == np.float32:
        assert not (b[:n] == np.float32(FILL)).any(), "%s: left elements unwritten" % what
    return b[:n]


def response(dfe, cuda, Y):
    H, W = Y.shape
    ctx, out, src = dfe.get_ctx(0), guarded(H * W, cuda), T(Y, cuda)      # (src stays alive until the result has been copied back)
    ctx.check(dfe.lib().dfe_corner_response_f32(ctx.handle, src.data_ptr(), H, W, out.data_ptr()))
    return unguard(out, H * W, "response").reshape(H, W)


def select(dfe, cuda, resp_t, H, W, quality, min_dist, max_points):
    ctx = dfe.get_ctx(0)
    pts, val, n = guarded(2 * max_points, cuda), guarded(max_points, cuda), C.c_int(-1)
    ctx.check(dfe.lib().dfe_select_corners_f32(ctx.handle, resp_t.data_ptr(), H, W, quality, min_dist, max_points, pts.data_ptr(), val.data_ptr(), C.byref(n)))
    assert 0 <= n.value <= max_points
    p, v = unguard(pts, 2 * max_points, "select pts", False), unguard(val, max_points, "select responses", False)
    assert (p[2 * n.value:] == FILL).all() and (v[n.value:] == FILL).all(), "select: wrote behind the n-th corner"
    return p[: 2 * n.value].reshape(-1, 2), v[: n.value], n.value


def track(dfe, cuda, Y0, Y1, pts, **kw):
    H, W = Y0.shape
    N = len(pts)
    ctx = dfe.get_ctx(0)
    p = dfe.sfm2._tracker_params(1, 0, 1, kw["win"], kw["levels"], kw["max_iters"], kw["eps"], kw["min_eig"], kw.get("max_err", 0.0))
    out, st, err = guarded(2 * N, cuda), guarded(N, cuda, torch.int32), guarded(N, cuda)
    a, b, pt = T(Y0, cuda), T(Y1, cuda), T(pts, cuda)                     # (alive until the results have been copied back)
    ctx.check(dfe.lib().dfe_track_points_lk_f32(ctx.handle, a.data_ptr(), b.data_ptr(), H, W, pt.data_ptr(), N, C.byref(p), out.data_ptr(), st.data_ptr(),
                                                err.data_ptr()))
    s = st.cpu().numpy()
    assert (s[N:] == int(FILL)).all() and np.isin(s[:N], (0, 1)).all(), "track: status"
    return unguard(out, 2 * N, "track pts", False).reshape(N, 2), s[:N], unguard(err, N, "track err", False)


# ------------------------------------------------------------------------------------------------------------------ 1. response
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (3, 3), (17, 65), (64, 64), (67, 129), (480, 640)])
def test_corner_response_against_float64(dfe, cuda, H, W):
    """A texture frame: |resp - resp64| <= 64 x 2^-24 x (a + c) per pixel, a and c from the reference (a dozen rounded operations per tensor
    entry, the square root's error bounded by the trace; a wrong tap gives an error of order a + c).  The same frame rounded to integers:
    a, b, c are exact in float32, so 4 ulp of the response + 2^-24 (a + c)."""
    tex = tr.texture(seed=5)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    frame = tex(x, y).astype(np.float32)
    for name, Y in (("texture", frame), ("integers", np.rint(frame).astype(np.float32))):
        ref, a, c = tr.corner_response64(Y)
        got = response(dfe, cuda, Y)
        tol = 64 * 2.0 ** -24 * (a + c) if name == "texture" else 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 2.0 ** -24 * (a + c)
        excess = np.abs(got - ref) - tol
        i = np.unravel_index(excess.argmax(), excess.shape)
        note("response", (H, W, name), "|resp - resp64| at the worst pixel", np.abs(got - ref)[i], tol[i])
        assert np.isfinite(got).all() and (excess <= 0).all()


# ----------------------------------------------------------------------------------------------------------------- 2. selection
def selection_maps(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    nan = rng.random((H, W), np.float32) - np.float32(0.3)
    nan[rng.random((H, W)) < 0.1] = np.nan
    return (("random", rng.random((H, W), np.float32) - np.float32(0.2)), ("quantised", rng.integers(0, 8, (H, W)).astype(np.float32)),
            ("all equal", np.full((H, W), 2.5, np.float32)), ("none positive", -rng.random((H, W), np.float32)), ("NaNs", nan))


@pytest.mark.parametrize("H,W", [(1, 1), (5, 300), (64, 64), (97, 131)])
def test_corner_selection_equals_the_definition(dfe, cuda, H, W):
    """Response maps made by the test, so the comparison with select64 is exact: the same points in the same order, the same responses, the
    same n -- for min_dist 1, 1.5, 5 and 30 (a disc larger than some of the frames), quality 0 and 1, and max_points 4096, n_kept,
    n_kept - 1 and 1."""
    calls = 0
    for name, resp in selection_maps(H, W):
        rt = T(resp, cuda)
        for md in (1.0, 1.5, 5.0, 30.0):
            for quality in (0.0, 1.0):
                pts, val, kept = tr.select64(resp, quality, md, 4096)
                assert kept <= 4096 or H * W > 4096
                for mp in sorted({4096, min(max(kept, 1), 4096), min(max(kept - 1, 1), 4096), 1}):
                    gp, gv, gn = select(dfe, cuda, rt, H, W, quality, md, mp)
                    calls += 1
                    want = min(kept, mp)
                    assert gn == want, "%s min_dist %g quality %g max_points %d: n = %d, reference %d" % (name, md, quality, mp, gn, want)
                    assert np.array_equal(gp, pts[:want]) and np.array_equal(gv, val[:want]), (name, md, quality, mp)
                if name == "all equal":
                    assert kept == 1 and pts.tolist() == [[0, 0]]
                if name == "none positive":
                    assert kept == 0
    print("selection %s: %d calls equal to the reference" % ((H, W), calls))


def test_corner_selection_on_the_device_response_and_argument_errors(dfe, cuda):
    tex = tr.texture(seed=6)
    x, y = np.meshgrid(np.arange(160, dtype=np.float64), np.arange(120, dtype=np.float64))
    resp = response(dfe, cuda, tex(x, y).astype(np.float32))
    rt = T(resp, cuda)
    for quality, md, mp in ((0.01, 10.0, 300), (1e-4, 30.0, 1000), (0.0, 1.0, 4096), (0.0, 2.0, 50)):
        pts, val, kept = tr.select64(resp, quality, md, mp)
        gp, gv, gn = select(dfe, cuda, rt, 120, 160, quality, md, mp)
        print("selection on the device's response: quality %g min_dist %g max_points %d -> %d kept, %d returned" % (quality, md, mp, kept, gn))
        assert gn == len(pts) and np.array_equal(gp, pts) and np.array_equal(gv, val)
    ctx, n = dfe.get_ctx(0), C.c_int()
    out = guarded(2 * 4096, cuda)
    for quality, md, mp in ((-0.1, 5.0, 10), (1.5, 5.0, 10), (0.5, 0.5, 10), (0.5, 5.0, 0), (0.5, 5.0, 4097), (float("nan"), 5.0, 10)):
        assert dfe.lib().dfe_select_corners_f32(ctx.handle, rt.data_ptr(), 120, 160, quality, md, mp, out.data_ptr(), None, C.byref(n)) == E_ARG


# ------------------------------------------------------------------------------------------------------------------- 3. pyramid
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (3, 5), (64, 64), (65, 127), (480, 640)])
def test_pyr_down_against_float64(dfe, cuda, H, W):
    """|out - out64| <= 8 x 2^-24 x max |in|: ten products and sums of non-negative terms of at most max |in|"""
    img = (np.random.default_rng(H + W).random((H, W), np.float32) * 255).astype(np.float32)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ctx, out, src = dfe.get_ctx(0), guarded(Ho * Wo, cuda), T(img, cuda)
    ctx.check(dfe.lib().dfe_pyr_down_f32(ctx.handle, src.data_ptr(), H, W, out.data_ptr()))
    got = unguard(out, Ho * Wo, "pyr_down").reshape(Ho, Wo)
    err, bound = np.abs(got - tr.pyr_down64(img)).max(), 8 * 2.0 ** -24 * np.abs(img).max()
    note("pyr_down", (H, W), "max |out - out64|", err, bound)
    assert err <= bound
    assert np.array_equal(dfe.sfm2.pyrDown(src).cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------------------------- 4. tracker
@pytest.mark.parametrize("case", TRACKER_CASES, ids=[c[0] for c in TRACKER_CASES])
def test_tracker_against_lk64(dfe, cuda, case):
    """Point by point against lk64 on the same input (a shared wrong minimum is no failure).  Positions of the points both sides track:
    within LK_BOUND at eps = 0, + eps otherwise (one side may take a last step shorter than eps that the other does not).  The status is
    equal except where the reference itself is within 1 % of min_eig or within 0.5 px of the frame edge -- at most 5 % of a case.  err:
    (largest |grad T| of the point's window) x (the position bound) + 255 x 2^-20.  Lost points keep their position and err = 0.  The same
    call twice gives the same bits."""
    name, (H, W), d, N, win, levels, iters, eps = case
    Y0, Y1 = tr.shifted_pair(H, W, *d)
    pts = tracker_points(H, W, N, N + win, [(W / 2 + 0.25, H / 2 - 0.5), (0, 0), (W - 1, H - 1), (np.nan, 5), (7.5, np.inf)] if N > 1 else [(80.25, 60.5)])
    kw = dict(win=win, levels=levels, max_iters=iters, eps=eps, min_eig=MIN_EIG)
    ref = tr.lk64(Y0, Y1, pts, **kw)
    gp, gs, ge = track(dfe, cuda, Y0, Y1, pts, **kw)
    bound = LK_BOUND + eps
    doubt = (np.abs(ref["lam"] - MIN_EIG) <= 0.01 * MIN_EIG) | (np.abs(ref["edge"]) < 0.5)
    note("tracker", name, "points in doubt (min_eig / frame edge)", doubt.sum(), 0.05 * N)
    note("tracker", name, "tracked by the reference", ref["status"].sum(), N)
    assert doubt.sum() <= 0.05 * N
    assert np.array_equal(gs[~doubt], ref["status"][~doubt]), "status differs at %s" % np.flatnonzero((gs != ref["status"]) & ~doubt)
    both = (gs == 1) & (ref["status"] == 1)
    assert both.sum() >= 0.75 * N                                 # the comparison below is about tracked points: most of a case must be
    dpos = np.hypot(*(gp[both] - ref["pts1"][both]).T)
    note("tracker", name, "max |pts1 - lk64| [px]", dpos.max(), bound)
    ebound = ref["grad"][both] * bound + 255 * 2.0 ** -20
    derr = np.abs(ge[both] - ref["err"][both])
    note("tracker", name, "max |err - lk64| / its bound", (derr / ebound).max(), 1.0)
    assert dpos.max() <= bound and (derr <= ebound).all()
    lost = gs == 0
    assert np.array_equal(gp[lost], pts[lost], equal_nan=True) and (ge[lost] == 0).all()
    if N > 1:
        assert gs[3] == 0 and gs[4] == 0                          # the NaN and the Inf point
    gp2, gs2, ge2 = track(dfe, cuda, Y0, Y1, pts, **kw)
    assert np.array_equal(gp, gp2, equal_nan=True) and np.array_equal(gs, gs2) and np.array_equal(ge, ge2)


def test_tracker_arguments_and_python_layer(dfe, cuda):
    Y0, Y1 = tr.shifted_pair(120, 160, 3.3, -2.6)
    pts = tracker_points(120, 160, 40, 3, [])
    ctx = dfe.get_ctx(0)
    a, b, p = T(Y0, cuda), T(Y1, cuda), T(pts, cuda)
    out, st = guarded(80, cuda), guarded(40, cuda, torch.int32)
    P = dfe._lib.TrackerParams
    for bad in (P(1, 0, 1, 4, 3, 10, 0, 0, 0), P(1, 0, 1, 33, 3, 10, 0, 0, 0), P(1, 0, 1, 1, 3, 10, 0, 0, 0), P(1, 0, 1, 21, 0, 10, 0, 0, 0), P(1, 0, 1, 21, 9, 10, 0, 0, 0),
                P(1, 0, 1, 21, 3, 0, 0, 0, 0), P(1, 0, 1, 21, 3, 65, 0, 0, 0), P(1, 0, 1, 21, 3, 10, -1.0, 0, 0)):
        assert dfe.lib().dfe_track_points_lk_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 120, 160, p.data_ptr(), 40, C.byref(bad), out.data_ptr(), st.data_ptr(),
                                                 None) == E_ARG
    good = P(1, 0, 1, 21, 3, 10, 0.01, MIN_EIG, 0)
    ctx.check(dfe.lib().dfe_track_points_lk_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 120, 160, p.data_ptr(), 0, C.byref(good), out.data_ptr(), st.data_ptr(), None))
    assert (out.cpu().numpy() == FILL).all()                      # N = 0 does nothing
    ctx.check(dfe.lib().dfe_track_points_lk_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 120, 160, p.data_ptr(), 40, C.byref(good), out.data_ptr(), st.data_ptr(), None))
    q, s, e = dfe.sfm2.trackPoints(a, b, p, winSize=21, levels=3, maxIters=10, eps=0.01, minEig=MIN_EIG)
    assert np.array_equal(q.cpu().numpy().reshape(-1), unguard(out, 80, "track", False)) and np.array_equal(s.cpu().numpy(), st.cpu().numpy()[:40])
    # max_err: the points whose residual exceeds it are lost, the others keep their bits
    thr = float(np.median(e.cpu().numpy()[s.cpu().numpy() == 1]))
    q2, s2, e2 = dfe.sfm2.trackPoints(a, b, p, winSize=21, levels=3, maxIters=10, eps=0.01, minEig=MIN_EIG, maxErr=thr)
    keep = (s.cpu().numpy() == 1) & (e.cpu().numpy() <= thr)
    assert np.array_equal(s2.cpu().numpy() == 1, keep) and 0 < keep.sum() < (s.cpu().numpy() == 1).sum()
    assert np.array_equal(q2.cpu().numpy()[keep], q.cpu().numpy()[keep]) and np.array_equal(q2.cpu().numpy()[~keep], pts[~keep])
    c = dfe.sfm2.findCorners(a, maxPoints=50, pointsQuality=0.01, pointsMinDistance=10).cpu().numpy()
    assert np.array_equal(c, tr.select64(response(dfe, cuda, Y0), 0.01, 10, 50)[0])


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def test_two_images_to_pose(dfe, cuda):
    """getEgoMotion2(K, im1=, im2=) on the two-view pair (flow up to 20 px: one level cannot follow it) against the hybrid route -- the
    DEVICE's corner list -> lk64 -> the oracle's pose with the same RANSAC distance, iterations and seed: the device's rotation and T errors
    against the planted pose are at most twice the hybrid's (floor 0.02 degrees)."""
    tv, q = tr.two_view_pair(), tr.ROUTE
    K = tv["K"]
    im0, im1 = T(tv["im0"], cuda), T(tv["im1"], cuda)
    kw = dict(maxPoints=q["max_points"], pointsQuality=q["quality"], pointsMinDistance=q["min_dist"], trackerWinSize=q["win"], trackerLevels=q["levels"],
              trackerMaxIters=q["max_iters"], trackerEps=q["eps"], trackerMinEig=q["min_eig"], ransacMaxDist=q["ransac"], iterations=q["iterations"], seed=q["seed"])
    R, Tt, nf, ni, F, p0, p1, st = dfe.sfm2.getEgoMotion2(K, im1=im0, im2=im1, returnTracks=True, **kw)
    R, Tt, F, p0, p1, st = R.numpy(), Tt.numpy(), F.numpy(), p0.cpu().numpy(), p1.cpu().numpy(), st.cpu().numpy()
    # the stages the call is made of
    assert np.array_equal(p0, tr.select64(response(dfe, cuda, tv["im0"]), q["quality"], q["min_dist"], q["max_points"])[0])
    gp, gs, _ = track(dfe, cuda, tv["im0"], tv["im1"], p0, win=q["win"], levels=q["levels"], max_iters=q["max_iters"], eps=q["eps"], min_eig=q["min_eig"])
    assert np.array_equal(gp, p1) and np.array_equal(gs, st) and nf == int(st.sum())
    ref = tr.lk64(tv["im0"], tv["im1"], p0, q["win"], q["levels"], q["max_iters"], q["eps"], q["min_eig"])
    rc, Rh, Th, nih, _ = orc.ego_motion_from_points(p0, ref["pts1"].astype(np.float32), K, q["ransac"], q["iterations"], q["seed"], weights=ref["status"].astype(np.float32))
    assert rc == 0
    print("two images: %d corners, %d tracked (lk64: %d), %d inliers (hybrid: %d)" % (len(p0), nf, ref["status"].sum(), ni, nih))
    er, et, hr, ht = rot_angle(tv["R"], R), t_angle(tv["T"], Tt), rot_angle(tv["R"], Rh), t_angle(tv["T"], Th)
    note("two images", "hybrid", "rotation error [deg]", hr, 0.5)
    note("two images", "hybrid", "T error [deg]", ht, 3.0)
    note("two images", "device", "rotation error [deg]", er, max(2 * hr, 0.02))
    note("two images", "device", "T error [deg]", et, max(2 * ht, 0.02))
    assert er <= max(2 * hr, 0.02) and et <= max(2 * ht, 0.02)
    check_pose_algebra(K, R, Tt, F)
    # the reference's four-result form, positional and table style
    for got in (dfe.sfm2.getEgoMotion(im0, im1, K, 300, **{k: v for k, v in kw.items() if k != "maxPoints"}), dfe.sfm2.getEgoMotion(dict(im1=im0, im2=im1, K=K, **kw))):
        assert len(got) == 4 and np.array_equal(got[0].numpy(), R) and np.array_equal(got[1].numpy(), Tt) and got[2:] == (nf, ni)
    # what the pose is for: the rotation taken out of the previous frame, and the epipole
    warped, mask = dfe.sfm2.removeEgoMotion(im0.unsqueeze(0), K, R, inverse=True)
    ex, ey = dfe.sfm2.getEpipole(K, Tt)
    e = K @ tv["T"]
    print("two images: epipole (%.1f, %.1f), planted (%.1f, %.1f); %d of %d pixels warped" % (ex, ey, e[0] / e[2], e[1] / e[2], int(mask.sum()), mask.numel()))
    assert torch.isfinite(warped).all() and mask.sum() > 0.9 * mask.numel() and np.isfinite([ex, ey]).all()
    # RGB frames: the luminance route on rgb2y of them, bit for bit
    w = torch.tensor([0.9, 1.0, 1.1], device=cuda).reshape(3, 1, 1)
    rgb0, rgb1 = (im0.unsqueeze(0) * w).contiguous(), (im1.unsqueeze(0) * w).contiguous()
    y0, y1 = dfe.sfm2._gray(rgb0, "rgb0")[0], dfe.sfm2._gray(rgb1, "rgb1")[0]
    a, b = dfe.sfm2.getEgoMotion2(K, im1=rgb0, im2=rgb1, returnTracks=True, **kw), dfe.sfm2.getEgoMotion2(K, im1=y0, im2=y1, returnTracks=True, **kw)
    assert all(np.array_equal(u.cpu().numpy() if hasattr(u, "cpu") else u, v.cpu().numpy() if hasattr(v, "cpu") else v) for u, v in zip(a, b))
    # too few corners is an error, not a pose
    with pytest.raises(dfe.DfeError, match="corners"):
        dfe.sfm2.getEgoMotion2(K, im1=torch.zeros(64, 64, device=cuda), im2=torch.zeros(64, 64, device=cuda))
