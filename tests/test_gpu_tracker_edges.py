"""GPU suite (-m gpu), part 11b: csrc/tracker.hip where tests/test_gpu_tracker.py does not reach.
  1. the tracker at every window size the first list leaves out (the lane <-> cell map's carry), on frames whose pyramid levels do not halve
     evenly, a portrait frame, all eight levels, N mod 4 = 2, finite points far outside the frame, err = NULL -- the cases of
     tests/tracker_cases.py, whose conditions tests/test_tracker_cases_cpu.py checks on the references alone; the bound is the first list's;
  2. the selection on maps of more than 262 144 pixels (sel_max_kernel's stride loop), with more than 4096 kept corners (the full LDS list
     and the bitwise search), on one row and one column, and on + Inf and sub-normal responses -- exact against select64;
  3. the response on exact rank-1 frames: + 0.0 at every pixel;
  4. the one call against the staged public calls and the pose from points, bit for bit, on odd-sized landscape and portrait frames, and
     what it writes into *n_corners / *n_found before each refusal.
Every figure a test bounds is printed before it is asserted (-s shows it)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.test_gpu_tracker as gt
from tests import tracker_ref64 as tr
from tests.tracker_cases import EDGE_CASES, MIN_EIG, N_SPECIAL, case_points, edge_specials

pytestmark = pytest.mark.gpu

FILL, E_ARG = gt.FILL, gt.E_ARG
note, T, guarded, unguard = gt.note, gt.T, gt.guarded, gt.unguard


# ------------------------------------------------------------------------------------------------------------------- 1. tracker
def track(dfe, cuda, Y0, Y1, pts, with_err=True, **kw):
    """gt.track with the err output optional -> (pts1, status, err or None)"""
    if with_err:
        return gt.track(dfe, cuda, Y0, Y1, pts, **kw)
    H, W = Y0.shape
    N = len(pts)
    ctx = dfe.get_ctx(0)
    p = dfe.sfm2._tracker_params(1, 0, 1, kw["win"], kw["levels"], kw["max_iters"], kw["eps"], kw["min_eig"], 0.0)
    out, st = guarded(2 * N, cuda), guarded(N, cuda, torch.int32)
    a, b, pt = T(Y0, cuda), T(Y1, cuda), T(pts, cuda)
    ctx.check(dfe.lib().dfe_track_points_lk_f32(ctx.handle, a.data_ptr(), b.data_ptr(), H, W, pt.data_ptr(), N, C.byref(p), out.data_ptr(), st.data_ptr(), None))
    s = st.cpu().numpy()
    assert (s[N:] == int(FILL)).all() and np.isin(s[:N], (0, 1)).all(), "track: status"
    return unguard(out, 2 * N, "track pts", False).reshape(N, 2), s[:N], None


def check_against_lk64(dfe, cuda, case, specials):
    """the body of test_gpu_tracker.test_tracker_against_lk64 (same assertions, same bound) for a case of tests/tracker_cases.py, then the
    same call with err = NULL: the same pts1 and status bits"""
    name, (H, W), d, N, win, levels, iters, eps = case
    Y0, Y1 = tr.shifted_pair(H, W, *d)
    pts = case_points(case, specials)
    kw = dict(win=win, levels=levels, max_iters=iters, eps=eps, min_eig=MIN_EIG)
    ref = tr.lk64(Y0, Y1, pts, **kw)
    gp, gs, ge = track(dfe, cuda, Y0, Y1, pts, **kw)
    bound = gt.LK_BOUND + eps
    doubt = (np.abs(ref["lam"] - MIN_EIG) <= 0.01 * MIN_EIG) | (np.abs(ref["edge"]) < 0.5)
    note("tracker", name, "points in doubt (min_eig / frame edge)", doubt.sum(), 0.05 * N)
    note("tracker", name, "tracked by the reference", ref["status"].sum(), N)
    assert doubt.sum() <= 0.05 * N
    assert np.array_equal(gs[~doubt], ref["status"][~doubt]), "status differs at %s" % np.flatnonzero((gs != ref["status"]) & ~doubt)
    both = (gs == 1) & (ref["status"] == 1)
    assert both.sum() >= 0.75 * N
    dpos = np.hypot(*(gp[both] - ref["pts1"][both]).T)
    note("tracker", name, "max |pts1 - lk64| [px]", dpos.max(), bound)
    ebound = ref["grad"][both] * bound + 255 * 2.0 ** -20
    derr = np.abs(ge[both] - ref["err"][both])
    note("tracker", name, "max |err - lk64| / its bound", (derr / ebound).max(), 1.0)
    assert dpos.max() <= bound and (derr <= ebound).all()
    lost = gs == 0
    assert np.array_equal(gp[lost].view(np.uint32), pts[lost].view(np.uint32)) and (ge[lost] == 0).all()      # bit for bit, NaN payloads included
    if N >= N_SPECIAL:
        assert not gs[3:N_SPECIAL].any(), "NaN, Inf and the four points far outside the frame are lost: %s" % gs[3:N_SPECIAL]
    gp2, gs2, ge2 = track(dfe, cuda, Y0, Y1, pts, **kw)
    assert np.array_equal(gp.view(np.uint32), gp2.view(np.uint32)) and np.array_equal(gs, gs2) and np.array_equal(ge.view(np.uint32), ge2.view(np.uint32))
    gp3, gs3, _ = track(dfe, cuda, Y0, Y1, pts, with_err=False, **kw)
    assert np.array_equal(gp.view(np.uint32), gp3.view(np.uint32)) and np.array_equal(gs, gs3), "err = NULL changes pts1 or the status"


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_tracker_edge_cases_against_lk64(dfe, cuda, case):
    check_against_lk64(dfe, cuda, case, edge_specials)


# ----------------------------------------------------------------------------------------------------------------- 2. selection
def check_selection(dfe, cuda, name, resp, quality, min_dist, max_points_list):
    """exact against select64: n, the points, their order, the responses -> n_kept of the reference"""
    H, W = resp.shape
    rt = T(resp, cuda)
    pts, val, kept = tr.select64(resp, quality, min_dist, 4096)
    for mp in max_points_list:
        gp, gv, gn = gt.select(dfe, cuda, rt, H, W, quality, min_dist, mp)
        want = min(kept, mp)
        assert gn == want, "%s min_dist %g quality %g max_points %d: n = %d, reference %d" % (name, min_dist, quality, mp, gn, want)
        assert np.array_equal(gp, pts[:want]) and np.array_equal(gv.view(np.uint32), val[:want].view(np.uint32)), (name, min_dist, quality, mp)
    print("selection %s %s: quality %g min_dist %g -> %d kept, max_points %s equal to the reference" % (name, (H, W), quality, min_dist, kept, list(max_points_list)))
    return kept


@pytest.mark.parametrize("H,W", [(480, 640), (9, 30000)])
def test_selection_beyond_one_pass_of_the_maximum(dfe, cuda, H, W):
    """P > 262 144 = 1024 blocks x 256 threads: sel_max_kernel's loop turns, and the maximum (7.0 at flat index P - 3) lies where only the
    later turns read.  At quality 0.5 the threshold 3.5 leaves that one pixel; a maximum taken over the first pass alone (< 0.8) keeps
    thousands.  At quality 0 far more than 4096 are kept, so the bitwise search runs over a long list."""
    P = H * W
    assert P > 262144 + 3
    resp = np.random.default_rng(H * 1000 + W).random((H, W), np.float32) - np.float32(0.2)
    resp.reshape(-1)[P - 3] = 7.0
    assert resp.reshape(-1)[:262144].max() < 0.8
    for md in (1.0, 1.5, 5.0):
        kept = check_selection(dfe, cuda, "random + planted maximum", resp, 0.0, md, (4096, 4095, 1))
        assert kept > 2048
        assert check_selection(dfe, cuda, "random + planted maximum", resp, 0.5, md, (4096, 4095, 1)) == 1
    assert check_selection(dfe, cuda, "random + planted maximum", resp, 0.0, 1.0, (4096,)) > 4096


def test_selection_with_more_than_4096_kept(dfe, cuda):
    """160 x 200, min_dist 1: more corners are kept than the LDS list holds, the device returns the best 4096 in order.  In the quantised
    map equal responses cross the cut, so the index half of the key decides who is in."""
    H, W = 160, 200
    rng = np.random.default_rng(H * 1000 + W)
    for name, resp in (("random", rng.random((H, W), np.float32) - np.float32(0.2)), ("quantised", rng.integers(0, 8, (H, W)).astype(np.float32))):
        kept = check_selection(dfe, cuda, name, resp, 0.0, 1.0, (4096, 4095, 2049))
        assert kept > 4096
        if name == "quantised":
            v = tr.select64(resp, 0.0, 1.0, 4097)[1]
            assert v[4095] == v[4096], "the cut does not fall inside a run of equal responses"


@pytest.mark.parametrize("H,W", [(1, 32768), (32768, 1)])
def test_selection_on_one_row_and_one_column(dfe, cuda, H, W):
    resp = np.random.default_rng(H + 2 * W).random((H, W), np.float32) - np.float32(0.2)
    for md in (1.0, 5.0):
        kept = check_selection(dfe, cuda, "random", resp, 0.0, md, (4096, 1))
        assert kept > (4096 if md == 1.0 else 2048)


def test_selection_with_infinite_and_subnormal_responses(dfe, cuda):
    """+ Inf: the bit-pattern maximum is Inf; quality 0 makes the threshold 0 x Inf = NaN, which no response reaches (the definition's one
    float32 product), quality 0.5 and 1 keep the two Inf pixels in index order.  Sub-normal responses: positive, ordered as their bit
    patterns, and the product quality x M is sub-normal too; a kernel that flushes them returns nothing."""
    rng = np.random.default_rng(64064)
    resp = rng.random((64, 64), np.float32) - np.float32(0.2)
    resp[40, 7] = resp[3, 50] = np.inf
    for quality, want in ((0.0, 0), (0.5, 2), (1.0, 2)):
        for md in (1.0, 5.0):
            assert check_selection(dfe, cuda, "+ Inf", resp, quality, md, (4096, 1)) == want
    assert tr.select64(resp, 1.0, 5.0, 10)[0].tolist() == [[50, 3], [7, 40]]
    sub = rng.integers(1, 1 << 20, (64, 64)).astype(np.uint32).view(np.float32)
    assert (sub > 0).all() and sub.max() < np.finfo(np.float32).tiny
    counts = [check_selection(dfe, cuda, "sub-normal", sub, quality, 5.0, (4096, 1)) for quality in (0.0, 0.5, 1.0)]
    assert counts[0] >= counts[1] >= counts[2] >= 1 and counts[0] > 8


# ------------------------------------------------------------------------------------------------------------------ 3. response
def rank1_frame(H, W, axis, seed=0):
    """integer values 0 .. 255 that vary along one axis only ("x": every row the same)"""
    rng = np.random.default_rng(seed + H * 1000 + W)
    if axis == "x":
        return np.tile(rng.integers(0, 256, W).astype(np.float32), (H, 1))
    return np.tile(rng.integers(0, 256, H).astype(np.float32)[:, None], (1, W))


@pytest.mark.parametrize("H,W", [(5, 67), (67, 5)])
def test_response_of_exact_rank1_frames_is_plus_zero(dfe, cuda, H, W):
    """One gradient is 0 everywhere, so b = 0 and one of a, c is 0; the other is a sum of nine squares of half-integers up to 127.5: exact
    in float32.  The definition gives (s - sqrt(s^2)) / 2 = + 0.0, and the selection finds no corner and writes nothing."""
    for axis in ("x", "y"):
        Y = rank1_frame(H, W, axis)
        assert np.ptp(Y) > 100 and np.array_equal(tr.corner_response64(Y)[0], np.zeros((H, W)))
        got = gt.response(dfe, cuda, Y)
        bits = got.view(np.uint32)
        print("response %s, varying in %s: %d of %d pixels are + 0.0" % ((H, W), axis, (bits == 0).sum(), H * W))
        assert (bits == 0).all()
        for quality in (0.0, 1.0):
            gp, gv, gn = gt.select(dfe, cuda, T(got, cuda), H, W, quality, 1.0, 4096)
            assert gn == 0 and len(gp) == 0


# ------------------------------------------------------------------------------------------------------------------ 4. one call
COUNT0 = -5                                                       # what the counts hold before a call


def params(dfe, q, **over):
    q = dict(q, **over)
    return dfe._lib.TrackerParams(q["max_points"], q["quality"], q["min_dist"], q["win"], q["levels"], q["max_iters"], q["eps"], q["min_eig"], 0.0)


def one_call(dfe, cuda, im0, im1, K, prm, q):
    """the raw entry on device tensors [H][W] or [3][H][W], every output pre-filled -> (rc, message, dict)"""
    Cc = 1 if im0.dim() == 2 else im0.shape[0]
    H, W = im0.shape[-2:]
    mp = max(prm.max_points, 1)
    ctx = dfe.get_ctx(0)
    R, T3, F = (C.c_double * 9)(*([FILL] * 9)), (C.c_double * 3)(*([FILL] * 3)), (C.c_double * 9)(*([FILL] * 9))
    nf, ni, nc = C.c_int(COUNT0), C.c_int(COUNT0), C.c_int(COUNT0)
    p0, p1, st = guarded(2 * mp, cuda), guarded(2 * mp, cuda), guarded(mp, cuda, torch.int32)
    rc = dfe.lib().dfe_ego_motion_from_images_f32(ctx.handle, im0.data_ptr(), im1.data_ptr(), Cc, H, W, (C.c_double * 9)(*np.asarray(K, np.float64).reshape(-1)),
                                                  C.byref(prm), q["ransac"], q["iterations"], q["seed"], R, T3, C.byref(nf), C.byref(ni), F, p0.data_ptr(), p1.data_ptr(),
                                                  st.data_ptr(), C.byref(nc))
    torch.cuda.synchronize()
    msg = dfe.lib().dfe_last_error(ctx.handle).decode() if rc else ""
    n = nc.value if rc == 0 or (nc.value >= 8 and nf.value == 0) else 0     # (the lists are copied out before the tracked corners are counted)
    a, b, s = unguard(p0, 2 * mp, "pts0_out", False), unguard(p1, 2 * mp, "pts1_out", False), st.cpu().numpy()
    assert (a[2 * n:] == FILL).all() and (b[2 * n:] == FILL).all() and (s[n:] == int(FILL)).all(), "the one call wrote behind the n-th corner"
    return rc, msg, dict(R=np.array(R[:]), T=np.array(T3[:]), F=np.array(F[:]), n_found=nf.value, n_inliers=ni.value, n_corners=nc.value,
                         pts0=a[: 2 * n].reshape(-1, 2).copy(), pts1=b[: 2 * n].reshape(-1, 2).copy(), status=s[:n].copy())


def same_bits(a, b):
    """two results of one_call: the counts equal, the arrays of the same shape and bytes"""
    return all((a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def staged(dfe, cuda, Y0, Y1, q):
    """response -> select -> track by the public calls -> (pts0, pts1, status)"""
    H, W = Y0.shape
    p0, _, n = gt.select(dfe, cuda, T(gt.response(dfe, cuda, Y0), cuda), H, W, q["quality"], q["min_dist"], q["max_points"])
    p1, st, _ = gt.track(dfe, cuda, Y0, Y1, p0, win=q["win"], levels=q["levels"], max_iters=q["max_iters"], eps=q["eps"], min_eig=q["min_eig"])
    return p0, p1, st


@pytest.mark.parametrize("H,W", [(149, 203), (203, 149)])
def test_one_call_is_its_stages_and_the_pose_from_points(dfe, cuda, H, W):
    """An odd-sized landscape and a portrait frame.  pts0 / pts1 / status / n_corners / n_found equal the staged public calls, and R, T, F,
    n_inliers equal getEgoMotion2(K, pts1=, pts2=, weights=status) on those lists with the same distance, iterations and seed, bit for
    bit: the pose step got the status as its weights (all-ones weights would let the lost points, which keep pts1 = pts0, vote).  RGB
    frames give the bits of their luminance frames."""
    tv, q = tr.two_view_pair(H, W), tr.ROUTE
    K = tv["K"]
    im0, im1 = T(tv["im0"], cuda), T(tv["im1"], cuda)
    rc, msg, got = one_call(dfe, cuda, im0, im1, K, params(dfe, q), q)
    assert rc == 0, msg
    p0, p1, st = staged(dfe, cuda, tv["im0"], tv["im1"], q)
    print("one call %s: %d corners, %d tracked, %d inliers" % ((H, W), got["n_corners"], got["n_found"], got["n_inliers"]))
    assert got["n_corners"] == len(p0) >= 8 and got["n_found"] == int(st.sum()) >= 8 and got["n_found"] < got["n_corners"]
    assert np.array_equal(got["pts0"], p0) and np.array_equal(got["pts1"].view(np.uint32), p1.view(np.uint32)) and np.array_equal(got["status"], st)
    R, Tt, nf, ni, F = dfe.sfm2.getEgoMotion2(K, pts1=T(p0, cuda), pts2=T(p1, cuda), weights=T(st.astype(np.float32), cuda), ransacMaxDist=q["ransac"],
                                              iterations=q["iterations"], seed=q["seed"])
    assert nf == got["n_found"] and ni == got["n_inliers"]
    for name, a, b in (("R", R, got["R"]), ("T", Tt, got["T"]), ("F", F, got["F"])):
        assert np.array_equal(a.numpy().reshape(-1).view(np.uint64), b.view(np.uint64)), "%s differs from the pose of the staged lists: %s / %s" % (name, a, b)
    ones = dfe.sfm2.getEgoMotion2(K, pts1=T(p0, cuda), pts2=T(p1, cuda), weights=None, ransacMaxDist=q["ransac"], iterations=q["iterations"], seed=q["seed"])
    assert not np.array_equal(ones[4].numpy().reshape(-1), got["F"]), "the case does not tell the status from all-ones weights"
    # C = 3 against the luminance frames
    w = torch.tensor([0.9, 1.0, 1.1], device=cuda).reshape(3, 1, 1)
    rgb0, rgb1 = (im0.unsqueeze(0) * w).contiguous(), (im1.unsqueeze(0) * w).contiguous()
    y0, y1 = dfe.sfm2._gray(rgb0, "rgb0")[0][0].contiguous(), dfe.sfm2._gray(rgb1, "rgb1")[0][0].contiguous()
    rc3, msg3, got3 = one_call(dfe, cuda, rgb0, rgb1, K, params(dfe, q), q)
    rc1, msg1, got1 = one_call(dfe, cuda, y0, y1, K, params(dfe, q), q)
    assert rc3 == 0 and rc1 == 0, (msg3, msg1)
    assert got3["n_corners"] >= 8 and same_bits(got3, got1)


def test_one_call_refusals_write_the_counts_they_explain(dfe, cuda):
    """*n_corners and *n_found are written before the "fewer than 8" refusal they explain and by no argument error (the video session tells
    the two apart by them), and a refusal leaves nothing behind: the good call gives the bits it gave before."""
    H, W = 149, 203
    tv, q = tr.two_view_pair(H, W), tr.ROUTE
    K = tv["K"]
    im0, im1 = T(tv["im0"], cuda), T(tv["im1"], cuda)
    rc, msg, good = one_call(dfe, cuda, im0, im1, K, params(dfe, q), q)
    assert rc == 0, msg

    def good_again(after):
        rc, msg, again = one_call(dfe, cuda, im0, im1, K, params(dfe, q), q)
        assert rc == 0 and same_bits(good, again), "after %s: %s" % (after, msg)

    # no corner: two frames that vary in x only
    f0, f1 = T(rank1_frame(64, 64, "x"), cuda), T(rank1_frame(64, 64, "x", seed=1), cuda)
    rc, msg, got = one_call(dfe, cuda, f0, f1, K, params(dfe, q), q)
    print("refusal, no corner: rc %d, n_corners %d, n_found %d, '%s'" % (rc, got["n_corners"], got["n_found"], msg))
    assert rc == E_ARG and (got["n_corners"], got["n_found"], got["n_inliers"]) == (0, 0, COUNT0) and "only 0 corners" in msg
    assert (got["R"] == FILL).all() and (got["T"] == FILL).all()
    good_again("the no-corner refusal")
    # corners, none tracked: every level-0 window is weaker than min_eig = 1e9
    assert tr.lk64(tv["im0"], tv["im1"], good["pts0"], q["win"], q["levels"], q["max_iters"], q["eps"], 1e9)["status"].sum() == 0
    n_staged = len(staged(dfe, cuda, tv["im0"], tv["im1"], q)[0])
    rc, msg, got = one_call(dfe, cuda, im0, im1, K, params(dfe, q, min_eig=1e9), q)
    print("refusal, none tracked: rc %d, n_corners %d, n_found %d, '%s'" % (rc, got["n_corners"], got["n_found"], msg))
    assert rc == E_ARG and got["n_corners"] == n_staged >= 8 and (got["n_found"], got["n_inliers"]) == (0, COUNT0)
    assert "only 0 of %d corners tracked" % n_staged in msg and (got["R"] == FILL).all()
    assert np.array_equal(got["pts0"], good["pts0"]) and np.array_equal(got["pts1"], got["pts0"]) and not got["status"].any()
    good_again("the none-tracked refusal")
    # argument errors: the counts are not touched
    for what, over in (("win = 4", dict(win=4)), ("max_points = 0", dict(max_points=0))):
        rc, msg, got = one_call(dfe, cuda, im0, im1, K, params(dfe, q, **over), q)
        print("refusal, %s: rc %d, n_corners %d, n_found %d, '%s'" % (what, rc, got["n_corners"], got["n_found"], msg))
        assert rc == E_ARG and (got["n_corners"], got["n_found"], got["n_inliers"]) == (COUNT0, COUNT0, COUNT0), what
        good_again(what)
