"""The tracker cases the CPU and the GPU suite share (tests/test_tracker_cases_cpu.py checks on the reference alone what
tests/test_gpu_tracker.py and tests/test_gpu_tracker_edges.py rest on): the point generator, the first case list, and the edge cases --
every odd window size the first list leaves out (the kernel's lane <-> cell map carries by r64 = 64 mod win per step: 12, 13, 18 and 14 at
win 13, 17, 23 and 25 against 1, 1 and 2 at the win 3, 21 and 31 of the first list; win 5 and 7 are the one-step regime with idle lanes),
frames whose pyramid levels do not halve evenly, a portrait frame, all eight levels, and point counts with N mod 4 = 2."""
import numpy as np


def tracker_points(H, W, N, seed, specials):
    """N points: random over the frame less a 2 px rim (most windows hang over the frame edge on purpose; the rim keeps the share of results
    within 0.5 px of the edge, where the status may differ, small), the first ones replaced by the special points"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(2, W - 3, N), rng.uniform(2, H - 3, N)], 1).astype(np.float32)
    sp = np.array(specials, np.float32).reshape(-1, 2)[:N]
    pts[: len(sp)] = sp
    return pts


TRACKER_CASES = [
    # name,                 frame,     shift,         N,   win, levels, max_iters, eps
    ("one point",           (120, 160), (3.3, -2.6),   1,   21, 3, 10, 0.0),
    ("win 3, one level",    (120, 160), (0.37, -0.21), 63,  3,  1, 10, 0.0),
    ("win 31, four levels", (120, 160), (9.3, -6.6),   64,  31, 4, 10, 0.0),
    ("win 21, one level",   (120, 160), (0.37, -0.21), 65,  21, 1, 10, 0.0),
    ("257 points",          (120, 160), (3.3, -2.6),   257, 21, 3, 10, 0.0),
    ("257 points, eps",     (120, 160), (3.3, -2.6),   257, 21, 3, 30, 0.01),
    ("24 x 32, four levels", (24, 32),  (1.3, -0.8),   65,  21, 4, 10, 0.0),
    ("24 x 32, eps",        (24, 32),   (1.3, -0.8),   64,  3,  3, 30, 0.01),
]
MIN_EIG = 1.0

EDGE_CASES = [
    ("win 5",                      (37, 53),   (0.37, -0.21), 66, 5,  1, 10, 0.0),
    ("win 7, two levels",          (37, 53),   (0.9, -0.6),   66, 7,  2, 10, 0.0),
    ("win 9, portrait",            (101, 75),  (1.3, -0.8),   62, 9,  2, 10, 0.0),
    ("win 11",                     (75, 101),  (1.3, -0.8),   66, 11, 3, 10, 0.0),
] + [
    ("win %d" % w,                 (75, 101),  (3.3, -2.6),   66, w,  3, 10, 0.0) for w in (13, 15, 17, 19, 23, 25, 27, 29)
] + [
    ("eight levels",               (120, 160), (3.3, -2.6),   66, 21, 8, 10, 0.0),
    ("eight levels, 24 x 32",      (24, 32),   (1.3, -0.8),   66, 21, 8, 10, 0.0),
    ("eight levels, 37 x 53, eps", (37, 53),   (1.3, -0.8),   66, 15, 8, 30, 0.01),
    ("two points",                 (75, 101),  (3.3, -2.6),   2,  21, 3, 10, 0.0),
    # Two steps per level.  Ten steps converge at level 0 from any start within the window's basin, so the result above does not depend on
    # what the coarser levels handed down: a pyramid read with (h / 2) x (w / 2) geometry -- sheared alike in both frames -- moves lk64 by
    # at most 6e-6 px on the win 9, 11 and 13 cases, inside the bound.  After two steps the hand-down still shows: the same error moves lk64
    # by up to 0.56 px (median 0.019 px) here and 3.5 px (median 0.040 px) on the portrait frame (tests/test_tracker_cases_cpu.py).
    ("three levels, two steps",           (75, 101), (3.3, -2.6), 66, 21, 3, 2, 0.0),
    ("portrait, three levels, two steps", (101, 75), (3.3, -2.6), 66, 15, 3, 2, 0.0),
]

N_SPECIAL = 9                     # points 3 .. 8 of them are lost by definition: not finite, or finite and far outside the frame


def first_specials(H, W, N):
    """the special points of TRACKER_CASES: a half-pixel centre, two frame corners, a NaN and an Inf point"""
    return [(W / 2 + 0.25, H / 2 - 0.5), (0, 0), (W - 1, H - 1), (np.nan, 5), (7.5, np.inf)] if N > 1 else [(80.25, 60.5)]


def edge_specials(H, W, N):
    """the special points of EDGE_CASES: those five and four finite points far outside the frame (every window sample clamps to the frame's
    border, so the level-0 tensor has rank <= 1 and the point is lost: pts1 = p bit for bit, err = 0); a case with fewer than nine points
    has the centre only"""
    if N < N_SPECIAL:
        return [(W / 2 + 0.25, H / 2 - 0.5)]
    return first_specials(H, W, N) + [(-40.5, 10), (W + 30, H / 2), (1e6, 1e6), (3e38, -3e38)]


def case_points(case, specials):
    """the point list of a case: seed N + win, as the first tracker test had it"""
    _, (H, W), _, N, win = case[:5]
    return tracker_points(H, W, N, N + win, specials(H, W, N))
