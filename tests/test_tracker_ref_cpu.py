"""CPU suite: the float64 reference of the corner tracker (tests/tracker_ref64.py) against planted truths -- the GPU tests of
tests/test_gpu_tracker.py compare the kernels with this reference, so it has to be right on its own --, the host-side argument checks
of the Python layer (sfm2.findCorners / trackPoints / getEgoMotion / getEgoMotion2), and the compiler's resource report of the tracker
kernel.  Every bounded figure is printed before it is asserted."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle as orc
from tests import ref64
from tests import tracker_ref64 as tr
from tests.egomotion_cases import rot_angle, t_angle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what lk64 with three levels leaves against the planted translation on the 120 x 160 texture (60 interior points, win 21): 0.0226 px at
# every one of the three shifts, at eps = 0 and at eps = 0.01 -- the bilinear interpolation's own bias on wavelengths from 8 px
LK64_MEASURED = 0.0226
ROUTE = tr.ROUTE


def note(test, case, name, value, bound):
    print("%s %s: %s = %.3e (bound %.3e)" % (test, case, name, value, bound))


def interior_points(H, W, n, seed=1, margin=30):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, W - margin, n), rng.uniform(margin, H - margin, n)], 1).astype(np.float32)


@pytest.mark.parametrize("d", [(0.37, -0.21), (3.3, -2.6), (9.3, -6.6)])
def test_lk64_recovers_planted_translations(d):
    H, W = 120, 160
    a, b = tr.shifted_pair(H, W, *d)
    pts = interior_points(H, W, 60)
    for eps in (0.0, 0.01):
        r = tr.lk64(a, b, pts, win=21, levels=3, max_iters=30, eps=eps)
        e = np.hypot(*(r["pts1"] - pts - np.array(d)).T).max()
        note("lk64", (d, eps), "max |d - truth| [px], 3 levels", e, 2 * LK64_MEASURED)
        assert r["status"].all() and e <= 2 * LK64_MEASURED
    if d == (9.3, -6.6):                                          # the pyramid is needed: one level cannot follow this shift
        r = tr.lk64(a, b, pts, win=21, levels=1, max_iters=30, eps=0.01)
        med = np.median(np.hypot(*(r["pts1"] - pts - np.array(d)).T))
        note("lk64", d, "median |d - truth| [px], 1 level (a LOWER bound)", med, 5.0)
        assert med > 5.0


def test_lk64_lost_points():
    a, b = tr.shifted_pair(120, 160, 3.3, -2.6)
    pts = np.array([[80, 60], [np.nan, 5], [158.5, 60], [80, np.inf]], np.float32)
    r = tr.lk64(a, b, pts, win=21, levels=3, max_iters=30, eps=0.01)
    assert r["status"].tolist() == [1, 0, 0, 0]                   # NaN, leaves the frame (158.5 + 3.3 > 159), Inf
    assert np.array_equal(r["pts1"][1:], pts[1:], equal_nan=True) and (r["err"][1:] == 0).all() and r["err"][0] > 0
    flat = np.full((40, 50), 7.0, np.float32)
    r = tr.lk64(flat, flat, np.array([[20, 20]], np.float32), win=5, levels=2, max_iters=5, eps=0.0, min_eig=1e-4)
    assert r["status"].tolist() == [0]                            # no texture: below min_eig at level 0
    r = tr.lk64(flat, flat, np.array([[20, 20]], np.float32), win=5, levels=2, max_iters=5, eps=0.0, min_eig=0.0)
    assert r["status"].tolist() == [0]                            # ... and with min_eig = 0 the singular solve is not finite


def test_select64_properties():
    rng = np.random.default_rng(2)
    for name, resp in (("random", rng.random((64, 64), np.float32)), ("ties", rng.integers(0, 8, (64, 64)).astype(np.float32))):
        for md in (1, 1.5, 5, 30):
            pts, v, n = tr.select64(resp, 0.0, md, 4096)
            assert n == len(pts) >= 1
            d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1) + np.eye(len(pts)) * 1e9
            note("select64", (name, md), "smallest pairwise distance (a LOWER bound)", np.sqrt(d2.min()), md)
            assert d2.min() > np.floor(md * md)                  # pairwise more than min_dist apart
            idx = pts[:, 1] * 64 + pts[:, 0]
            assert all(v[i] > v[i + 1] or (v[i] == v[i + 1] and idx[i] < idx[i + 1]) for i in range(len(v) - 1))
            assert np.array_equal(v, resp[pts[:, 1].astype(int), pts[:, 0].astype(int)])
            cut = tr.select64(resp, 0.0, md, max(n - 1, 1))
            assert cut[2] == n and np.array_equal(cut[0], pts[: max(n - 1, 1)])
    # the global maximum is always kept and comes first; quality = 1 keeps only pixels that attain it
    resp = rng.random((20, 30), np.float32)
    pts, v, n = tr.select64(resp, 1.0, 1, 10)
    y, x = np.unravel_index(resp.argmax(), resp.shape)
    assert n == 1 and pts.tolist() == [[x, y]] and v[0] == resp.max()
    # all equal: every pixel but the first is dominated by a neighbour with a smaller index
    pts, v, n = tr.select64(np.full((9, 11), 3.0, np.float32), 0.5, 1, 4096)
    assert n == 1 and pts.tolist() == [[0, 0]]
    assert tr.select64(np.zeros((9, 11), np.float32), 0.0, 1, 10)[2] == 0 and tr.select64(-np.ones((3, 3), np.float32), 0.0, 1, 10)[2] == 0
    # NaN is never a candidate and never dominates
    resp = np.array([[1, np.nan, 1], [np.nan, np.nan, np.nan]], np.float32)
    pts, v, n = tr.select64(resp, 0.0, 1, 10)
    assert pts.tolist() == [[0, 0], [2, 0]]
    assert tr.select64(np.full((2, 2), np.nan, np.float32), 0.0, 1, 10)[2] == 0


def test_response64_and_pyr_down64_on_known_inputs():
    x = np.arange(12, dtype=np.float64)
    ramp = np.tile(3 * x, (9, 1))                                  # one gradient direction: the smaller eigenvalue is 0
    resp, a, c = tr.corner_response64(ramp)
    assert np.abs(resp).max() < 1e-9 and a[4, 5] == 9 * 9.0 and c.max() == 0 and a[4, 0] == 3 * 9.0 + 6 * 2.25
    sad = np.add.outer(np.arange(9.0) ** 2, -x ** 2)              # a saddle: both eigenvalues positive away from the centre lines
    assert tr.corner_response64(sad)[0][6, 8] > 0
    assert np.array_equal(tr.pyr_down64(np.full((7, 10), 5.0)), np.full((4, 5), 5.0))
    assert tr.pyr_down64(np.array([[2.0]])).tolist() == [[2.0]] and tr.pyr_down64(np.array([[1.0, 3.0]])).tolist() == [[(6 + 2 * 1) / 16 * 1 + 8 / 16 * 3]]
    assert np.allclose(tr.pyr_down64(ramp)[:, 1:-1], ramp[::2, ::2][:, 1:-1])    # linear functions pass a symmetric kernel unchanged
    assert tr._reflect(np.array([-2, -1, 0, 4, 5, 6]), 5).tolist() == [2, 1, 0, 4, 3, 2] and tr._reflect(np.array([-2, 3]), 2).tolist() == [0, 1]


def test_reference_route_recovers_the_planted_pose():
    """corners64 -> lk64 -> the oracle's pose on the two-view pair: the condition for the end-to-end GPU test to mean something"""
    tv, q = tr.two_view_pair(), ROUTE
    c = tr.corners64(tv["im0"], q["quality"], q["min_dist"], q["max_points"])
    r = tr.lk64(tv["im0"], tv["im1"], c, q["win"], q["levels"], q["max_iters"], q["eps"], q["min_eig"])
    ok = r["status"] > 0
    s = ref64.sampson64(ref64.fund_from_pose64(tv["K"], tv["R"], tv["T"]), c[ok], r["pts1"][ok].astype(np.float32))
    rc, R, T, ni, _ = orc.ego_motion_from_points(c, r["pts1"].astype(np.float32), tv["K"], q["ransac"], q["iterations"], q["seed"], weights=ok.astype(np.float32))
    print("route: %d corners, %d tracked, %.0f %% within 1 px of the planted F, %d inliers, largest flow %.1f px" % (len(c), ok.sum(), 100 * (s <= 1).mean(), ni,
                                                                                                                 tv["flow_max"]))
    note("route", "reference", "rotation error [deg]", rot_angle(tv["R"], R), 0.5)
    note("route", "reference", "T error [deg]", t_angle(tv["T"], T), 3.0)
    assert rc == 0 and len(c) >= 150 and ok.sum() >= 0.8 * len(c) and tv["flow_max"] > 15
    assert rot_angle(tv["R"], R) <= 0.5 and t_angle(tv["T"], T) <= 3.0


def test_python_layer_checks_its_arguments_without_a_device(dfe):
    import torch

    s = dfe.sfm2
    img, pts, K = torch.zeros(8, 8), torch.zeros(4, 2), np.eye(3)
    for kw in (dict(winSize=4), dict(winSize=1), dict(winSize=33), dict(levels=0), dict(levels=9), dict(maxIters=0), dict(maxIters=65), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            s.trackPoints(img, img, pts, **kw)
    for kw in (dict(maxPoints=0), dict(maxPoints=4097), dict(pointsQuality=-0.1), dict(pointsQuality=1.5), dict(pointsMinDistance=0.5)):
        with pytest.raises(ValueError):
            s.selectCorners(img, **kw)
        with pytest.raises(ValueError):
            s.getEgoMotion2(K, im1=img, im2=img, **kw)
    with pytest.raises(ValueError):
        s.trackPoints(img, img, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        s.getEgoMotion2(K, im1=img)                               # one image only
    with pytest.raises(ValueError):
        s.getEgoMotion2(K, im1=img, im2=img, pts1=pts, pts2=pts)  # two sources of correspondences
    with pytest.raises(ValueError):
        s.getEgoMotion2(K, im1=torch.zeros(2, 8, 8), im2=torch.zeros(2, 8, 8))
    with pytest.raises(ValueError):
        s.getEgoMotion2(K)
    with pytest.raises(ValueError):
        s.getEgoMotion(img, img)                                  # no K
    # the existing positional order is unchanged and the new keywords trail it
    names = list(inspect.signature(s.getEgoMotion2).parameters)
    assert names[:10] == ["K", "flow", "confidences", "pts1", "pts2", "weights", "maxPoints", "ransacMaxDist", "iterations", "seed"]
    assert names[10:15] == ["im1", "im2", "pointsQuality", "pointsMinDistance", "trackerWinSize"]
    # defaults: a given keyword, then the calibration's sfm table, then the .cal files' values
    cal = dict(K=K, sfm=dict(max_points=500, points_min_dist=20, tracker_win_size=15))
    assert s._sfm(cal, "max_points", None) == 500 and s._sfm(cal, "max_points", 7) == 7 and s._sfm(cal, "points_quality", None) == 1e-4
    assert s._sfm(None, "tracker_win_size", None) == 21 and s._sfm(None, "points_min_dist", None) == 30 and s._sfm(None, "max_points", None) == 1000
    p = s._tracker_params(1000, 1e-4, 30, 21, 3, 30, 0.01, 1e-4, 0)
    assert (p.max_points, p.win, p.levels, p.max_iters) == (1000, 21, 3, 30) and abs(p.min_dist - 30) == 0


def test_tracker_kernel_does_not_spill():
    """tools/kres.py on csrc/tracker.hip: the tracker keeps T, Tx, Ty (48 registers) and its bilinear taps in registers -- no scratch in
    any kernel of the file, and the tracker inside the 128 registers that let two blocks share a compute unit's SIMDs."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "tracker.hip"), "_kernel"],
                         capture_output=True, text=True).stdout
    rows = {m[0]: tuple(int(x) for x in m[1:]) for m in re.findall(r"(\w+_kernel)\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)}
    assert set(rows) == {"corner_response_kernel", "sel_max_kernel", "sel_keep_kernel", "sel_top_kernel", "pyr_down_kernel", "lk_track_kernel"}, out
    assert all(v[1] == 0 for v in rows.values()), rows
    assert rows["lk_track_kernel"][0] <= 128, rows
