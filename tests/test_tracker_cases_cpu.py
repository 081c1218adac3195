"""CPU suite: the conditions the GPU tracker tests rest on, checked on the references alone for every case of both lists of
tests/tracker_cases.py.  The device is compared with lk64 point by point, outside a doubt set, to LK_BOUND (+ eps); that means something
only if the doubt set is small, most points are tracked, and the float32 rounding the DEFINITION carries on the case's input -- lk32, the
definition restated in float32 (tests/tracker_ref32.py), against lk64 -- stays under half the bound, so that the other half is left to the
summation order, the one thing the device may differ from lk32 in.  A case that does not meet these is replaced, not excused.  Every figure
is printed before it is asserted."""
import numpy as np
import pytest

from tests import tracker_ref64 as tr
from tests.test_gpu_tracker import LK_BOUND
from tests.tracker_cases import EDGE_CASES, MIN_EIG, N_SPECIAL, TRACKER_CASES, case_points, edge_specials, first_specials
from tests.tracker_ref32 import lk32, pyr_down32, sample32

ALL = [(c, first_specials) for c in TRACKER_CASES] + [(c, edge_specials) for c in EDGE_CASES]


def note(test, case, name, value, bound):
    print("%s %s: %s = %.3e (bound %.3e)" % (test, case, name, value, bound))


def test_case_lists_cover_what_they_claim():
    wins = sorted({c[4] for c in TRACKER_CASES + EDGE_CASES})
    assert wins == list(range(3, 32, 2))                           # every window size the entry accepts
    assert {c[4] for c in EDGE_CASES if 64 - (64 // c[4]) * c[4] >= 12} >= {13, 17, 23, 25}
    assert any(c[5] == 8 for c in EDGE_CASES) and any(c[1][0] > c[1][1] for c in EDGE_CASES)
    assert any(c[3] % 4 == 2 for c in EDGE_CASES) and len({c[0] for c in EDGE_CASES}) == len(EDGE_CASES) == 18
    for (H, W), levels in {(c[1], c[5]) for c in EDGE_CASES if c[1] not in ((120, 160), (24, 32))}:
        dims = [(H, W)]
        for _ in range(levels - 1):
            dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
        assert any(h % 2 or w % 2 for h, w in dims[:-1]) or levels == 1, "(h + 1) / 2 is not told apart from h / 2 on %s" % ((H, W),)


def test_float32_pieces_against_float64():
    rng = np.random.default_rng(0)
    img = (rng.random((37, 53)) * 255).astype(np.float32)
    d = np.abs(pyr_down32(img) - tr.pyr_down64(img)).max()
    note("lk32", "pyr_down32", "max |out32 - out64|", d, 8 * 2.0 ** -24 * 255)
    assert pyr_down32(img).dtype == np.float32 and d <= 8 * 2.0 ** -24 * 255
    x, y = (rng.uniform(-5, 60, 500)).astype(np.float32), (rng.uniform(-5, 45, 500)).astype(np.float32)
    s = sample32(img, x, y)
    d = np.abs(s - tr.sample64(img, x.astype(np.float64), y.astype(np.float64))).max()
    note("lk32", "sample32", "max |s32 - s64|", d, 8 * 2.0 ** -24 * 255)
    assert s.dtype == np.float32 and d <= 8 * 2.0 ** -24 * 255


@pytest.mark.parametrize("case,specials", ALL, ids=[c[0] for c, _ in ALL])
def test_case_conditions_on_the_references(case, specials):
    name, (H, W), d, N, win, levels, iters, eps = case
    Y0, Y1 = tr.shifted_pair(H, W, *d)
    pts = case_points(case, specials)
    kw = dict(win=win, levels=levels, max_iters=iters, eps=eps, min_eig=MIN_EIG)
    ref, r32 = tr.lk64(Y0, Y1, pts, **kw), lk32(Y0, Y1, pts, **kw)
    doubt = (np.abs(ref["lam"] - MIN_EIG) <= 0.01 * MIN_EIG) | (np.abs(ref["edge"]) < 0.5)
    note("cases", name, "points in doubt (min_eig / frame edge)", doubt.sum(), 0.05 * N)
    note("cases", name, "tracked by lk64", ref["status"].sum(), 0.75 * N)
    assert doubt.sum() <= 0.05 * N and ref["status"].sum() >= 0.75 * N
    assert np.array_equal(r32["status"][~doubt], ref["status"][~doubt]), "lk32 status differs at %s" % np.flatnonzero((r32["status"] != ref["status"]) & ~doubt)
    both = (r32["status"] == 1) & (ref["status"] == 1)
    dpos = np.hypot(*(r32["pts1"][both] - ref["pts1"][both]).T).max()
    note("cases", name, "max |lk32 - lk64| [px]", dpos, LK_BOUND / 2 + eps)
    assert dpos <= LK_BOUND / 2 + eps
    lost = r32["status"] == 0
    assert np.array_equal(r32["pts1"][lost], pts[lost], equal_nan=True) and (r32["err"][lost] == 0).all()
    if len(pts) >= N_SPECIAL and specials is edge_specials:        # NaN, Inf and the four finite points far outside: lost on both references
        assert not ref["status"][3:N_SPECIAL].any() and not r32["status"][3:N_SPECIAL].any() and not doubt[3:N_SPECIAL].any()
        assert np.array_equal(ref["pts1"][3:N_SPECIAL].astype(np.float32), pts[3:N_SPECIAL], equal_nan=True) and (ref["err"][3:N_SPECIAL] == 0).all()


def test_two_step_cases_depend_on_the_pyramid_geometry(monkeypatch):
    """lk64 over a pyramid whose levels are read as (h / 2) x (w / 2) images from the (h + 1) / 2 x (w + 1) / 2 buffers -- what a host that
    halves the level sizes the wrong way hands the kernel.  Both frames shear alike, so a level-0 loop that converges hides it: the ten-step
    case on the same frame moves by less than the bound.  The two-step cases move by far more than the bound at half their points: they are
    the ones that tell (h + 1) / 2 from h / 2."""
    full = tr.pyr_down64

    def floor_halved(I):
        H, W = np.asarray(I).shape
        return full(I).reshape(-1)[: (H // 2) * (W // 2)].reshape(H // 2, W // 2).copy()

    by_name = {c[0]: c for c in EDGE_CASES}
    for name, sees_it in (("win 11", False), ("three levels, two steps", True), ("portrait, three levels, two steps", True)):
        _, (H, W), d, N, win, levels, iters, eps = by_name[name]
        Y0, Y1 = tr.shifted_pair(H, W, *d)
        pts = case_points(by_name[name], edge_specials)
        kw = dict(win=win, levels=levels, max_iters=iters, eps=eps, min_eig=MIN_EIG)
        ref = tr.lk64(Y0, Y1, pts, **kw)
        monkeypatch.setattr(tr, "pyr_down64", floor_halved)
        bad = tr.lk64(Y0, Y1, pts, **kw)
        monkeypatch.setattr(tr, "pyr_down64", full)
        both = (bad["status"] == 1) & (ref["status"] == 1)
        moved = np.hypot(*(bad["pts1"][both] - ref["pts1"][both]).T)
        note("cases", name, "lk64 on the wrongly halved pyramid: max |pts1 - lk64| [px]", moved.max(), LK_BOUND)
        note("cases", name, "... median", np.median(moved), 100 * LK_BOUND)
        assert both.sum() >= 0.75 * N and (np.median(moved) > 100 * LK_BOUND if sees_it else moved.max() < LK_BOUND)
