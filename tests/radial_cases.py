"""Cases shared by tests/test_radial_cases_cpu.py (the oracle) and tests/test_gpu_radial_edges.py (the device): the radial one-call path
(csrc/radial_pipeline.hip) at the shapes, filter stacks, windows, polar exponents and epipoles its kernels branch on.  90 x 160 frames of
rp.synth_pair; weights drawn with numpy, so that the oracle and the device's modules (which copy them) see the same numbers.

What each case reaches (hm = hInput - 16 - hWin + 1 matcher rows, Wo = wInput columns after the row filter):
  A  odd hInput (conv_rows_pk_kernel's last block holds one row), feature height 59 (no multiple of 4), interleaved warp with C = 1
  B  Wo = 257 (one column in a second tile), n1 = 8 with tanh, n2 = 8, hWin 16, the epipole on the frame's corner
  C  the planar warp (C = 5), n1 = 4, hWin 12, alpha 0.8, the epipole outside the frame
  D  conv_rows_kernel with a run-time kW (5 taps), feature height 45, hWin 8, the epipole on the frame's right edge
  E  generic row convolution (n1 = 6) + conv_cols_kernel, alpha 1.25
  F  hm = 1, wInput == lpad (every wrap column the argument check allows)
  G  hm = 64 (two whole 32-row blocks of radial_match_kernel), padded polar width 288, tanh
  H  Wo = 256, conv_rows_pk_kernel + generic column convolution (n2 = 7), odd hInput, a fractional epipole above the frame"""
import math

import numpy as np

from tests import oracle as orc
from tests import refpath as rp

HIMG, WIMG = 90, 160
DEFAULT = [[3, 1, 17, 5], [5, 17, 1, 10]]
# name: C, hInput, wInput, hWin, layers, alpha, epipole
CASES = {
    "A": (1, 75, 250, 15, [[1, 1, 17, 5], [5, 17, 1, 10]], 1.0, (70.5, 40.25)),
    "B": (4, 82, 257, 16, [[4, 1, 17, 8], "tanh", [8, 17, 1, 8]], 1.0, (0.0, 0.0)),
    "C": (5, 77, 96, 12, [[5, 1, 17, 4], [4, 17, 1, 10]], 0.8, (-20.5, 105.25)),
    "D": (2, 61, 130, 8, [[2, 1, 5, 5], [5, 17, 1, 10]], 1.0, (159.0, 45.0)),
    "E": (3, 70, 100, 15, [[3, 1, 17, 6], [6, 17, 1, 10]], 1.25, (80.0, 44.0)),
    "F": (3, 31, 8, 15, DEFAULT, 1.0, (80.0, 44.0)),
    "G": (3, 94, 272, 15, [DEFAULT[0], "tanh", DEFAULT[1]], 1.0, (33.0, 71.0)),
    "H": (3, 63, 256, 15, [[3, 1, 17, 5], [5, 17, 1, 7]], 1.0, (80.25, -12.5)),
}
FULL_WINDOW = "ABCDEGH"          # the polar flow takes every value of the window (F has 8 pixels)
TIE_CAP = 0.05                   # share of pixels whose two best costs are close but not equal
TIE_REL = 4e-5                   # "close", of max|volume|: a +-2e-5 perturbation of the oracle's sampling grid moved its volume by 0.7e-5 to 1.2e-5
SEAM_CAP = 0.005
_cache = {}


def networkp(name):
    C, hIn, wIn, hWin, layers, alpha, e2 = CASES[name]
    return dict(hImg=HIMG, wImg=WIMG, hInput=hIn, wInput=wIn, hWin=hWin, layers=layers)


def frames(C):
    """(previous frame, frame) in [0, 1]"""
    if ("frames", C) not in _cache:
        f0, f1, _, _ = rp.synth_pair(HIMG, WIMG, C=C, seed=1, max_flow=6, noise_sigma=0)
        f0, f1 = f0 / np.float32(255), f1 / np.float32(255)
        for a in (f0, f1):
            a.setflags(write=False)
        _cache[("frames", C)] = (f0, f1)
    return _cache[("frames", C)]


def weights(name):
    """(w1 [n1][C][1][kW], b1, w2 [n2][n1][kH][1], b2, tanh between): uniform in +-1 / sqrt(fan-in)"""
    if ("weights", name) not in _cache:
        layers = CASES[name][4]
        rng = np.random.default_rng(0)
        out = []
        for nin, kh, kw, nout in (l for l in layers if l != "tanh"):
            s = 1.0 / math.sqrt(nin * kh * kw)
            out += [rng.uniform(-s, s, (nout, nin, kh, kw)).astype(np.float32), rng.uniform(-s, s, nout).astype(np.float32)]
        for a in out:
            a.setflags(write=False)
        _cache[("weights", name)] = tuple(out) + ("tanh" in layers,)
    return _cache[("weights", name)]


def geometry(name):
    """the P2C and depth constants of test_radial:217-225 as radial_path_oracle derives them"""
    C, hIn, wIn, hWin, layers, alpha, (ex, ey) = CASES[name]
    kH = layers[-1][1]
    rmax = math.floor(math.sqrt(max(ex * ex + ey * ey, (WIMG - ex) ** 2 + ey * ey, ex * ex + (HIMG - ey) ** 2, (WIMG - ex) ** 2 + (HIMG - ey) ** 2)))
    hm = hIn - kH - hWin + 2
    kOut = hm / hIn
    kOut2 = (hIn - (kH - 1) // 2 - hWin + 1) / hIn
    cx, cy = ex * kOut2, ey * kOut2
    infty = math.floor(math.sqrt(max(cx * cx + cy * cy, (WIMG - cx) ** 2 + cy * cy, cx * cx + (HIMG - cy) ** 2, (WIMG - cx) ** 2 + (HIMG - cy) ** 2))) * 0.65
    return dict(rmax=rmax, hm=hm, kOut=kOut, hOut=int(HIMG * kOut), wOut=int(WIMG * kOut), xc=ex * kOut, yc=ey * kOut, nrmax=rmax * kOut, cx=cx, cy=cy,
                infty=infty)


def p2c_grid(name):
    """the oracle's polar -> cartesian grid [2][hOut][wOut] (row coordinate, column coordinate)"""
    if ("p2c", name) not in _cache:
        g, wIn, alpha = geometry(name), CASES[name][2], CASES[name][5]
        m = orc.polar_grid_p2c(wIn, g["hm"], g["wOut"], g["hOut"], g["xc"], g["yc"], g["nrmax"], alpha)
        m.setflags(write=False)
        _cache[("p2c", name)] = m
    return _cache[("p2c", name)]


def reference(name):
    """radial_path_oracle of the case (the last flow row not zeroed), computed once and read-only"""
    if ("ref", name) not in _cache:
        C, hIn, wIn, hWin, layers, alpha, e2 = CASES[name]
        f0, f1 = frames(C)
        w1, b1, w2, b2, th = weights(name)
        ref = rp.radial_path_oracle(f0, f1, e2, networkp(name), w1, b1, w2, b2, tanh_between=th, alpha=alpha)
        for a in ref.values():
            a.setflags(write=False)
        _cache[("ref", name)] = ref
    return _cache[("ref", name)]


def cost_gap(volume):
    """second-smallest - smallest cost of every pixel"""
    s = np.sort(np.asarray(volume, np.float32), -1)
    return s[..., 1] - s[..., 0]


def coord_tol(v):
    """the tolerance the suite holds getP2CMaskOF's coordinates to (tests/test_gpu_multiscale_radial.py: rtol 1e-6, atol 1e-4)"""
    return 1e-4 + 1e-6 * np.abs(v)


def seam_set(name):
    """P2C pixels whose column coordinate lies within its tolerance of the angle seam without sitting on it: the device's atan2 / fmod may
    put them on the other end of the polar row.  (mx == 0 exactly -- atan2(+0, x > 0), a whole row in B -- is exact on both sides.)"""
    mx, wIn = p2c_grid(name)[1], CASES[name][2]
    d = coord_tol(mx)
    return ((mx > 0) & (mx < d)) | ((mx > wIn - d) & (mx < wIn))


def ky_pair(name):
    """getP2CMask's row constant ky = hsrc / rmax^(1 / alpha) as float32, with the scaled radius rounded to float32 before the pow --
    what a `float rmax` argument of the grid entry does -- and with it kept a double, as the reference keeps it (a Lua number up to ky,
    cartesian2polar.lua:59; dfe_polar_grid_p2c_f32, orc_polar_grid_p2c and the one call all take the double)"""
    g, alpha = geometry(name), np.float64(np.float32(CASES[name][5]))
    as_float = np.float32(g["hm"] / np.power(np.float64(np.float32(g["nrmax"])), 1.0 / alpha))
    as_double = np.float32(g["hm"] / np.power(np.float64(g["nrmax"]), 1.0 / alpha))
    return as_float, as_double


def tap_range(pf, grid):
    """max - min of the polar flow over the 3 x 3 cells around the cell the grid's clamped coordinate falls into (clamped at the borders):
    a bilinear sample moves by at most |dy| R + |dx| R when its coordinate moves by (dy, dx) with |dy|, |dx| < 1"""
    H, W = pf.shape
    y0 = np.floor(np.clip(grid[0], 0, H - 1)).astype(int)
    x0 = np.floor(np.clip(grid[1], 0, W - 1)).astype(int)
    lo, hi = np.full(y0.shape, np.inf), np.full(y0.shape, -np.inf)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v = pf[np.clip(y0 + dy, 0, H - 1), np.clip(x0 + dx, 0, W - 1)]
            lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return hi - lo


def subpixel_rule(vol):
    """(bi, bi + off) of include/dfe.h for a volume [...][hWin], float32 throughout: bi the first minimum, off = (cm - cp) /
    (2 ((cm - c0) + (cp - c0))) clamped to [-0.5, 0.5] where bi is inside the window and the denominator positive, else 0 (every numpy
    operation on float32 arrays is one separately rounded IEEE operation, as in the kernel)"""
    vol = np.asarray(vol, np.float32)
    hW = vol.shape[-1]
    bi = vol.argmin(-1)                                   # numpy: the first minimum

    def cell(k):
        return np.take_along_axis(vol, np.clip(k, 0, hW - 1)[..., None], -1)[..., 0]

    c0, cm, cp = cell(bi), cell(bi - 1), cell(bi + 1)
    den = (cm - c0) + (cp - c0)
    ok = (bi >= 1) & (bi + 1 < hW) & (den > 0)
    with np.errstate(all="ignore"):
        off = (cm - cp) / (np.float32(2) * den)
    off = np.minimum(np.maximum(off, np.float32(-0.5)), np.float32(0.5))
    off = np.where(ok, off, np.float32(0)).astype(np.float32)
    assert off.dtype == np.float32 and den.dtype == np.float32
    return bi, bi.astype(np.float32) + off
