"""Cases shared by tests/test_postfilter_ref_cpu.py (the numpy definitions against the oracle) and tests/test_gpu_postfilters.py (the
device against the oracle): the inputs of the depth, warp, polar-grid, post-filter, mask and extractor kernels at their size edges,
with centres and flows off the float grid.  tests/test_postfilter_ref_cpu.py::test_the_cases_reach_every_edge asserts that the
inputs below still hold the edges they are named for."""
import numpy as np

F = np.float32
INF = float("inf")
BELOW_01 = float(np.nextafter(F(0.1), F(0)))
_cache = {}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- radial flow -> depth ----------------------------------------------------------------------------------------------------------
# (name, H, W, (xc, yc)).  `d10`: pixel (0, 0) lies at d = 10 exactly (confidence 0), pixel (9, 16) at d^2 = 101 (confidence 1)
RADIAL_FRAMES = (("9x13", 9, 13, (4.3, 2.6)), ("60x80", 60, 80, (33.3, 27.7)), ("outside", 23, 31, (-20.5, 100.25)), ("H1", 1, 40, (12.7, 0.4)),
                 ("W1", 40, 1, (0.3, 17.6)), ("d10", 20, 20, (6.0, 8.0)))
RADIAL_INFTY = 37.7
RADIAL_SPECIALS = (float(F(0.1)), BELOW_01, 0.0, -1.75, INF)   # exactly 0.1f, the float below it, 0, negative, +inf
BIG = (1025, 2049)                                            # 2 100 225 pixels: the first frame above the 1-D grid cap of 2 097 152
BIG_CENTRE = (1000.3, 500.7)


def radial_flow(H, W, seed=0):
    """uniform in [0, 3) with each of RADIAL_SPECIALS at every 11th pixel"""
    def make():
        f = (np.random.default_rng(seed).random((H, W)) * 3).astype(F)
        for s, v in enumerate(RADIAL_SPECIALS):
            f.reshape(-1)[s::11] = v
        return _ro(f)
    return _cached(("radial", H, W, seed), make)


# ---- cartesian flow -> depth -------------------------------------------------------------------------------------------------------
CART_FRAME = (37, 53)
CART_FOE = (31.7, 23.4)
CART_PLANTED = ((0.0, float(np.nextafter(F(0.2), F(0)))), (0.0, float(F(0.2))), (0.0, float(np.nextafter(F(0.2), F(1)))), (0.12, 0.16), (-0.16, 0.12),
                (0.0, 0.0), (0.141, -0.141), (0.1415, 0.1415))   # (dy, dx): |flow| just below, at and above 0.2
PAIR_STEP = (96, 130, 3, 9, 12)                                 # H, W, k, window of the one pair step (tests/test_gpu_subpixel.py's shape)


def cart_flow():
    """standard_normal * 3 as float32 with CART_PLANTED at every 13th pixel"""
    def make():
        H, W = CART_FRAME
        f = (np.random.default_rng(20).standard_normal((2, H, W)) * 3).astype(F)
        for s, (dy, dx) in enumerate(CART_PLANTED):
            f[0].reshape(-1)[s::13] = dy
            f[1].reshape(-1)[s::13] = dx
        return _ro(f)
    return _cached("cart", make)


# ---- ardrone flow -> depth ---------------------------------------------------------------------------------------------------------
ARDRONE_FRAMES = (("W1", 9, 1), ("H1", 1, 12), ("2x2", 2, 2), ("11x17", 11, 17), ("8x9", 8, 9))
ARDRONE_M = 0.37
# halves round away from zero; -8.4 / 11.4 land in the first / last bin, -8.5 / 11.5 round to -9 / 12 and are dropped
ARDRONE_VALUES = (0.5, -0.5, 1.5, -1.5, -8.4, 11.4, -8.5, 11.5, 2.2, -2.4, 1.0, -1.0, 0.2, 3.0)


def ardrone_case(H, W, seed=0):
    """(xflow, mask): flows drawn from ARDRONE_VALUES, mask from {0, 0.3, 1} (0.3: counted in the histograms, no depth of its own)"""
    def make():
        rng = np.random.default_rng(100 + seed + 31 * H + W)
        xflow = rng.choice(np.array(ARDRONE_VALUES, F), size=(H, W))
        mask = rng.choice(np.array([0.0, 0.3, 1.0], F), size=(H, W), p=[0.15, 0.15, 0.7])
        return _ro(xflow, mask)
    return _cached(("ardrone", H, W, seed), make)


def ardrone_big():
    def make():
        rng = np.random.default_rng(7)
        xflow = (rng.standard_normal(BIG) * 3).astype(F)
        mask = rng.choice(np.array([0.0, 0.3, 1.0], F), size=BIG, p=[0.2, 0.1, 0.7])
        return _ro(xflow, mask)
    return _cached("ardrone_big", make)


# ---- bilinear warp -----------------------------------------------------------------------------------------------------------------
WARP_CASES = (("C1-1x7", 1, 1, 7), ("C3-7x1", 3, 7, 1), ("C5-5x6", 5, 5, 6), ("C3-5x6", 3, 5, 6))


def _axis_coords(n, with_nan):
    """coordinates along an axis of n pixels: every integer, n - 1, outside on both sides, +-inf, fractions [, NaN]"""
    v = list(range(n)) + [n - 1, -3.5, n + 10, INF, -INF, 0.3, n - 1 - 0.3, (n - 1) * 0.37, (n - 1) / 3, n - 1 + 0.001, -1e-3]
    return np.array(v + ([float("nan")] if with_nan else []), F)


def warp_case(C, H, W, with_nan=True):
    """(img [C][H][W] in +-3.7, mask [2][Hd][Wd]: the cross product of the axis coordinates)"""
    def make():
        img = ((np.random.default_rng(C * 100 + H * 10 + W).random((C, H, W)) - 0.5) * 7.4).astype(F)
        ys, xs = _axis_coords(H, with_nan), _axis_coords(W, with_nan)
        mask = np.stack(np.meshgrid(ys, xs, indexing="ij")).astype(F)
        return _ro(img, mask)
    return _cached(("warp", C, H, W, with_nan), make)


def warp_one_pixel():
    img, _ = warp_case(3, 5, 6)
    return img, _ro(np.array([[[2.3]], [[4.6]]], F))


def warp_big():
    """one plane of BIG pixels sampled at BIG positions, a twentieth of them outside the image"""
    def make():
        H, W = BIG
        rng = np.random.default_rng(8)
        img = ((rng.random((1, H, W)) - 0.5) * 7.4).astype(F)
        mask = np.stack([rng.uniform(-0.03 * H, 1.03 * H, BIG), rng.uniform(-0.03 * W, 1.03 * W, BIG)]).astype(F)
        return _ro(img, mask)
    return _cached("warp_big", make)


# ---- polar grids -------------------------------------------------------------------------------------------------------------------
C2P_PADS = ((0, 0), (3, 0), (0, 5), (1, 7), (12, 12))   # on wdst = 12, hdst = 5; the last: lpad = rpad = wdst
C2P_PAD_GRID = (12, 5)
GRID_ALPHAS = (0.8, 1.0, 1.25)
C2P_GRID = dict(wsrc=128, hsrc=96, wdst=37, hdst=21, xc=70.3, yc=40.7, rmax=81.0)
P2C_GRID = dict(wsrc=37, hsrc=21, wdst=41, hdst=29, xc=17.0, yc=11.0, rmax=27.3)   # pixel (11, 17) is the centre: x = y = 0
P2C_GRID_OFF = dict(P2C_GRID, xc=17.3, yc=10.6)                                    # and a centre off the grid
BIG_GRID = dict(wdst=2049, hdst=1025, xc=1000.3, yc=500.7, rmax=1100.0)


# ---- postProcessImage --------------------------------------------------------------------------------------------------------------
MODE_KS = (1, 2, 3, 4, 5, 7)
MEDIAN_KS = (1, 2, 3, 4, 5)


def _mode_field(H, W, rng):
    """rounded values -7 .. 8 (a span of exactly 15, negative minimum), fractions within +-0.4 and a few exact halves"""
    flow = (rng.integers(-3, 4, size=(2, H, W)) + rng.random((2, H, W)) * 0.8 - 0.4).astype(F)
    flat = flow.reshape(-1)
    flat[2::17] = 2.5                                 # floor(x + 0.5): 3
    flat[3::19] = -2.5                                # -> -2
    flat[1], flat[flat.size - 2] = -7.3, 8.4          # -> -7 and 8
    return flow


def mode_cases(k):
    """[(name, flow [2][H][W], mask [H][W])] for window size k: a frame with windows, H == k (no window: only the lifted border),
    H == k + 1, an all-zero mask"""
    def make():
        out = []
        for name, H, W in (("frame", k + 6, k + 9), ("H==k", k, k + 4), ("H==k+1", k + 1, k + 3)):
            rng = np.random.default_rng(1000 * k + H)
            mask = rng.choice(np.array([0.0, 0.3, 1.0], F), size=(H, W), p=[0.25, 0.15, 0.6])
            mask[:k, :k] = 0                          # an empty window at (0, 0)
            out.append((name, _mode_field(H, W, rng), mask))
        rng = np.random.default_rng(k)
        out.append(("mask0", _mode_field(k + 3, k + 4, rng), np.zeros((k + 3, k + 4), F)))
        for _, f, m in out:
            _ro(f, m)
        return out
    return _cached(("mode", k), make)


def mode_tie_case():
    """k = 3 on a 4 x 4 frame: the one window holds (vy, vx) = (1, 2) four times, (0, 5) four times and (3, 3) once; the minimum 0
    sits outside the window.  Codes vx + 16 vy: 18 and 5 -- the lower one, (0, 5), wins."""
    flow = np.zeros((2, 4, 4), F)
    vy = np.array([[1, 0, 1], [0, 3, 0], [1, 1, 0]], F)
    vx = np.array([[2, 5, 2], [5, 3, 5], [2, 2, 5]], F)
    flow[0, :3, :3], flow[1, :3, :3] = vy + F(0.25), vx - F(0.25)
    return _ro(flow, np.ones((4, 4), F))


def span16(flow):
    """the same frame with its largest value raised by one: a rounded span of 16"""
    f = np.array(flow)
    f.reshape(-1)[np.argmax(f)] += 1
    return f


def median_case(k):
    """(flow, mask): multiples of 1/4 (duplicates), +-inf, no zero of either sign; the first window's mask holds two pixels (k >= 2)"""
    def make():
        H, W = k + 5, k + 8
        rng = np.random.default_rng(50 + k)
        flow = (np.round(rng.standard_normal((2, H, W)) * 8) / 4).astype(F)
        flow[flow == 0] = 0.25
        flow[0, 1, 2], flow[1, 2, 1], flow[0, H - 2, W - 3], flow[1, 1, 1] = INF, -INF, -INF, INF
        flow[0, 0, 0], flow[1, 0, 0], flow[1, k - 1, k - 1] = INF, -INF, -INF   # the first window's medians: +inf and -inf
        mask = rng.choice(np.array([0.0, 0.3, 1.0], F), size=(H, W), p=[0.3, 0.1, 0.6])
        mask[:k, :k] = 0
        mask[0, 0] = mask[k - 1, k - 1] = 1
        mask[H - k - 1 :, W - k - 1 :] = 0            # the last window is empty
        return _ro(flow, mask)
    return _cached(("median", k), make)


def filter_big():
    def make():
        rng = np.random.default_rng(9)
        flow = (rng.standard_normal((2,) + BIG) * 2).clip(-7.4, 7.4).astype(F)
        mask = (rng.random(BIG) > 0.3).astype(F)
        mask[100:110, 200:210] = 0
        return _ro(flow, mask)
    return _cached("filter_big", make)


# ---- enlargeMask -------------------------------------------------------------------------------------------------------------------
ENLARGE_SIZES = ((1, 9), (9, 1), (6, 7))
ENLARGE_WIDTHS = ((0, 0), (0, 2), (2, 0), (1, 1), (3, 2), (9, 1), (20, 20))   # ix = 0 / iy = 0 change nothing; ix >= W


def enlarge_masks(H, W):
    """[(name, mask)]: all ones, all zeros, rows whose only set pixel is the last column, values of exactly 0.5 (not set) and 0.75"""
    def make():
        rng = np.random.default_rng(H * 10 + W)
        last = np.zeros((H, W), F)
        last[:, W - 1] = 1
        half = rng.permutation(np.resize(np.array([0.5, 0.75, 0.0, 0.5, 0.75, 1.0, 0.5], F), H * W)).reshape(H, W)
        rand = (rng.random((H, W)) > 0.4).astype(F)
        out = [("ones", np.ones((H, W), F)), ("zeros", np.zeros((H, W), F)), ("last-column", last), ("halves", half), ("random", rand)]
        for _, m in out:
            _ro(m)
        return out
    return _cached(("enlarge", H, W), make)


# ---- OutputExtractor / marginal sum ------------------------------------------------------------------------------------------------
EXTRACTOR_WINDOWS = ((1, 1), (4, 4), (7, 9), (8, 8), (5, 13), (17, 17), (33, 33))
EXTRACTOR_PS = (1, 3, 99)
EXTRACTOR_OVER_CAP = (32771, 4, 4)          # P above the 8192 blocks x 4 pixels of one launch
MARGINAL_BS = (1, 7, 64, 289)
MARGINAL_OVER_CAP = (2097155, 1, 1)         # P * A above the 8192 blocks x 256 elements of one launch


def probabilities(P, N, seed=0):
    def make():
        p = np.random.default_rng(seed + 7 * P + N).random((P, N), dtype=F)
        p /= p.sum(-1, keepdims=True)
        return _ro(p)
    return _cached(("prob", P, N, seed), make)


def marginal_input(P, A, B):
    return _cached(("marg", P, A, B), lambda: _ro(np.random.default_rng(P + A + B).random((P, A, B), dtype=F)))
