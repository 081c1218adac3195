"""The census cost in the pyramid matcher in numpy, written from the definition in include/dfe.h, not from the
device's walk: per scale the box down-sample, the zero padding for the receptive field k + a - 1, the signatures, the aggregated Hamming
cost over the maxh x maxw window, (float)cost * beta; then the soft-min, the cascade with its rings, the arg-max with the centre rule and
the decode of the SSD pyramid's oracle chain.  Whole arrays at a time; nothing here knows about tiles, lanes or classes dealt to waves.
Also the case table that tests/test_gpu_census_pyramid.py runs on the device and tests/test_census_pyramid_ref_cpu.py checks for fitness
on this reference alone, and the exposure scene of the quality table (no tests here)."""
import functools

import numpy as np

from tests import oracle as orc
from tests import pyramid_cases as pc
from tests import refpath as rp
from tests.census_ref import cost_volume, signature

GAIN, OFFSET = 0.5, 40.0     # frame 1's exposure in every row of the table


def default_beta(C, a):
    return 0.25 / (C * a * a)


def scale_volume(f0, f1, r, k, maxh, maxw, a, beta):
    """what dfe_census_pyramid_scale_volume_f32 returns: float32 [H/r][W/r][maxh][maxw]"""
    hp, wp = maxh - 1 + k - 1 + a - 1, maxw - 1 + k - 1 + a - 1
    pt, pl = hp // 2, wp // 2
    sig = []
    for f in (f0, f1):
        d = orc.downsample_box(f, r) if r > 1 else np.ascontiguousarray(f, np.float32)
        sig.append(signature(orc.zero_pad(d, pl, wp - pl, pt, hp - pt), k, k))
    cost = cost_volume(sig[0], sig[1], maxh, maxw, a)
    assert cost.shape == (f0.shape[1] // r, f0.shape[2] // r, maxh, maxw)
    return cost.astype(np.float32) * np.float32(beta)


def chain(f0, f1, k, maxh, maxw, ratios, a, beta):
    """what dfe_multiscale_census_flow_pair_f32 returns, with the joined class tensor: dict(vols, joined, idx, y, x, middle)"""
    H, W = f0.shape[1:]
    vols = [scale_volume(f0, f1, r, k, maxh, maxw, a, beta) for r in ratios]
    probs = [orc.softmin(v.reshape(-1, maxh * maxw)).reshape(v.shape) for v in vols]
    rc, joined = orc.cascade_ring(probs, ratios, H, W, maxh, maxw)
    assert rc == 0
    middle = orc.yx2x_multi(maxh, maxw, ratios, 0, 0)
    idx, _ = orc.argbest_center(joined, middle, True)
    rc, y, x = orc.x2yx_multi(maxh, maxw, ratios, idx)
    assert rc == 0
    return dict(vols=vols, joined=joined, idx=idx, y=y, x=x, middle=middle)


# ---- the case table.  ties / wins: the share of pixels whose two best joined values lie within pyramid_cases.TIE_GAP and the reference's
# winner count per scale, as measured on this reference; fit: the row goes against the reference chain under the tie rule (the others are
# compared bit for bit with the staged device composition only)
def _case(no, ratios, mh, mw, k, C, H, W, mf, a, why, ties, wins, fit=True):
    c = pc.Case(no, ratios, mh, mw, k, C, H, W, mf, why, ties, wins)
    c.a, c.fit = a, fit
    return c


CASES = [
    _case(1, [1, 2, 4], 8, 8, 7, 3, 96, 136, 14, 3, "the corner: fast kernels, px cascade", 0.0041, [6545, 4711, 1800]),
    _case(2, [1, 2, 4], 8, 8, 7, 1, 96, 136, 14, 5, "C = 1, widest box", 0.0054, [7029, 4679, 1348]),
    _case(3, [1, 2], 8, 8, 7, 3, 34, 42, 7, 3, "W % 8 = 2, H / 2 odd: ragged tiles", 0.0098, [1038, 390]),
    _case(4, [1, 3], 6, 6, 7, 3, 36, 45, 7, 3, "ratio 3, odd W, generic cascade", 0.0037, [999, 621]),
    _case(5, [1, 2, 4], 16, 4, 7, 3, 64, 88, 14, 3, "N = 64, not 8 x 8", 0.0051, [4085, 879, 668]),
    _case(6, [1, 2], 4, 8, 5, 3, 40, 56, 6, 5, "k = 5, maxh = 2 d", 0.0031, [2080, 160]),
    _case(7, [1, 2, 4], 8, 8, 7, 3, 96, 136, 14, 1, "no box (tie share 0.0285: bit-for-bit checks only)", None, [6347, 5394, 1315], fit=False),
    _case(8, [1], 5, 7, 3, 2, 19, 23, 2, 3, "one scale, k = 3, nothing aligned (tie share 0.016: bit-for-bit checks only)", None, [437], fit=False),
    _case(9, [1, 2], 8, 8, 7, 2, 34, 42, 7, 3, "C = 2 in the fast kernels (bit-for-bit checks only)", None, None, fit=False),
    _case(10, [1, 2], 8, 8, 7, 4, 34, 42, 7, 3, "C = 4 in the fast kernels (bit-for-bit checks only)", None, None, fit=False),
]
BY_NO = {c.no: c for c in CASES}
FIT = [c for c in CASES if c.fit]
FIT_TIE_CAP = 0.015          # three quarters of pyramid_cases.TIE_CAP: the cap cannot hide a failure


def beta_of(c):
    return default_beta(c.C, c.a)


def frames(c):
    """the row's frame pair, byte-valued float32: pyramid_cases' planted flow, frame 1 darker and offset"""
    f0, f1, _, _ = rp.synth_pair(c.H, c.W, C=c.C, seed=1, max_flow=c.mf, noise_sigma=2.0)
    return f0, np.floor(f1 * np.float32(GAIN) + np.float32(OFFSET)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(no):
    """the reference chain of row `no`, computed once per process and shared read-only: vols, idx, top2, middle"""
    c = BY_NO[no]
    f0, f1 = frames(c)
    ref = chain(f0, f1, c.k, c.mh, c.mw, c.ratios, c.a, beta_of(c))
    out = dict(vols=ref["vols"], idx=ref["idx"], top2=pc._top2(ref["joined"]), middle=ref["middle"])
    for a in [out["idx"], out["top2"]] + out["vols"]:
        a.setflags(write=False)
    return out


# ---- the exposure scene: census_ref.scene's recipe at 96 x 128, three channels, a margin of 40 and a move of one's choice ----
SCENE = dict(H=96, W=128, C=3, k=7, win=8, ratios=(1, 2, 4), a=3, margin=40, border=16, sigma=1.0)
MOVES = (((2, -3), 0), ((5, -6), 1), ((9, -11), 2))      # (move (y, x), tolerance in pixels)


def scene(seed, move, gain=GAIN, offset=OFFSET):
    """two byte-valued float32 frames [3][96][128]: frame 1 is frame 0's texture moved by `move` (y, x), times gain, plus offset, plus
    N(0, 1); both floored and clipped to 0 .. 255"""
    rng = np.random.RandomState(seed)
    H, W, C, m = SCENE["H"], SCENE["W"], SCENE["C"], SCENE["margin"]
    my, mx = move
    f0s, f1s = [], []
    for _ in range(C):
        t = rng.uniform(size=(H + 2 * m, W + 2 * m))
        for _ in range(4):                 # the 5-point mean, with wrap-around
            t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
        t = (t - t.min()) / (t.max() - t.min()) * 255.0
        f0s.append(t[m:m + H, m:m + W])
        f1s.append(t[m - my:m - my + H, m - mx:m - mx + W] * gain + offset + rng.normal(0.0, SCENE["sigma"], size=(H, W)))   # f1[p + move] = f0[p]
    to_bytes = lambda f: np.clip(np.floor(np.stack(f)), 0, 255).astype(np.float32)
    return to_bytes(f0s), to_bytes(f1s)


def share_wrong(fy, fx, move, tol):
    """share of the pixels inside the border whose flow is further than tol from the move on either axis"""
    b = SCENE["border"]
    fy, fx = np.asarray(fy, np.float64)[b:-b, b:-b], np.asarray(fx, np.float64)[b:-b, b:-b]
    return float(np.mean((np.abs(fy - move[0]) > tol) | (np.abs(fx - move[1]) > tol)))


def scene_census(seed, move):
    f0, f1 = scene(seed, move)
    s = SCENE
    return chain(f0, f1, s["k"], s["win"], s["win"], list(s["ratios"]), s["a"], default_beta(s["C"], s["a"]))


def scene_ssd(seed, move):
    """the SSD oracle chain on the same frames, as they are"""
    f0, f1 = scene(seed, move)
    s = SCENE
    return rp.multiscale_flow_oracle(f0, f1, s["k"], s["win"], s["win"], list(s["ratios"]))
