"""The raw-patch pyramid matcher off its 8 x 8, k = 7, C = 3 corner: the case table that tests/test_gpu_pyramid_shapes.py runs on the
device and tests/test_pyramid_cases_cpu.py checks for fitness on the oracle alone (no tests here).

Each row names the code path it is there for.  `ties`: the share of pixels whose two best oracle classes lie within 1e-5 of each other, as
measured when the table was made -- the device may differ from the oracle only there, and only on 2 % of the pixels, so a row whose own
tie share came near 2 % would test nothing.  `wins`: the oracle's winner count per scale at that time (None: not pinned); a scale that won
at least 100 pixels then has to keep doing so, or the row no longer reaches that scale's classes."""
import functools
import math

import numpy as np

from tests import oracle as orc
from tests import refpath as rp

TIE_GAP = 1e-5          # _assert_matches_oracle's rule (tests/test_gpu_multiscale_radial.py)
TIE_CAP = 0.02
MIN_WINS = 100


class Case:
    def __init__(self, no, ratios, mh, mw, k, C, H, W, mf, why, ties, wins=None, seed=1):
        self.no, self.ratios, self.mh, self.mw, self.k, self.C, self.H, self.W, self.mf = no, list(ratios), mh, mw, k, C, H, W, mf
        self.why, self.ties, self.wins, self.seed = why, ties, wins, seed

    @property
    def id(self):
        return "row%d-%s-%dx%d-k%d-C%d" % (self.no, "_".join(str(r) for r in self.ratios), self.mh, self.mw, self.k, self.C)


CASES = [
    Case(1, [1, 2], 4, 8, 5, 3, 40, 56, 6, "maxh == 2 d: empty side blocks; one cell per lane, N = 32", 0.0000, [2064, 176]),
    Case(2, [1, 2], 8, 4, 4, 1, 40, 56, 6, "even k, tall window", 0.0018),
    Case(3, [1, 3], 9, 6, 5, 2, 36, 45, 7, "ratio 3, odd W: the generic branch, rinv = 1/3", 0.0000, [1225, 395]),
    Case(4, [1, 3], 6, 6, 7, 3, 36, 45, 7, "the same with a square window", 0.0019),
    Case(5, [1, 4], 8, 8, 5, 3, 32, 44, 6, "8 x 8 that must leave the lane <-> pixel path (d = 3)", 0.0000),
    Case(6, [1, 2, 4], 16, 4, 7, 3, 64, 88, 14, "N = 64 and not 8 x 8: one cell per lane at full lane use", 0.0149, [3738, 998, 896]),
    Case(7, [1, 2, 4], 12, 8, 7, 3, 72, 104, 14, "N = 96: the slow form, non-square", 0.0080, [5079, 1805, 604]),
    Case(8, [1, 2, 6], 12, 12, 5, 3, 72, 96, 30, "N = 144, steps 2 and 3 mixed", 0.0012, [5209, 1250, 453]),
    Case(9, [1, 2, 4, 8, 16, 32], 8, 8, 7, 3, 192, 256, 90, "six scales: the slow form with 8 x 8", 0.0126, [26771, 14155, 7684, 542, 0, 0]),
    Case(10, [1, 2], 4, 4, 9, 4, 22, 30, 3, "pow2 branch with a 6-pixel tail, k = 9, C = 4", 0.0000),
    Case(11, [1, 2], 8, 8, 7, 3, 34, 42, 7, "lane <-> pixel path, W % 8 = 2, H / 2 odd", 0.0098),
    Case(12, [1], 5, 7, 6, 2, 19, 23, 2, "one scale, odd window, nothing aligned", 0.0000),
    Case(13, [1, 2], 8, 8, 5, 2, 40, 56, 7, "lane <-> pixel path with fine_shape false", 0.0004),
]
BY_NO = {c.no: c for c in CASES}

# The corner itself -- 8 x 8, k = 7, C = 3, ratios 1, 2, 4 -- for the launcher switches of tests/test_gpu_pyramid_switches.py: W / 8 = 17
# tiles, a coarsest scale of 24 x 34 (exactly one tile of 5 row groups high, one 32-pixel block and a tail wide), and a planted flow large
# enough that every scale wins pixels, so that a wrong value in any scale's volume moves class ids.  Not a row of CASES: the shapes
# suite does not run it.  `ties16`: the tie share under the fp16 rule of test_row_f16_equals_oracle_chain, as measured.
SWITCH_ORACLE = Case(21, [1, 2, 4], 8, 8, 7, 3, 96, 136, 14, "launcher switches at the 8 x 8 corner", 0.0051, [7374, 4357, 1325])
SWITCH_ORACLE.ties16 = 0.0345
BY_NO[SWITCH_ORACLE.no] = SWITCH_ORACLE

# prep_tiles_kernel off its 64-pixel tile grid (k = 7, 8 x 8 windows): (H, W, C, ratios, byte frames)
PREP_CASES = [
    (1032, 1480, 1, [1, 2, 4, 8], False),        # both sides 8 mod 64: the last tiles are 8 wide and 8 high
    (1040, 1456, 2, [1, 4], False),              # a subset of the ratios with a gap
    (1024, 1472, 3, [1, 2, 4, 8, 16], True),     # uint8 frames, scale 1 / 255
]
PREP_K, PREP_WIN, PREP_MF = 7, 8, 12
# the first of them also goes against the oracle chain
PREP_ORACLE = Case(0, PREP_CASES[0][3], PREP_WIN, PREP_WIN, PREP_K, PREP_CASES[0][2], PREP_CASES[0][0], PREP_CASES[0][1], PREP_MF,
                   "prep_tiles_kernel with ragged last tiles, against the oracle", None)

# the geometries without a ring layout (maxh < 2 d): (ratios, maxh, maxw, scale the message names)
BAD_RINGS = [([1, 2], 4, 12, 1), ([1, 3], 3, 6, 1), ([1, 2, 4], 4, 16, 1)]
# ... and the border that stays legal: maxh == 2 d
EDGE_RINGS = [([1, 2], 4, 8), ([1, 3], 6, 9)]


def ring_widths(ratios, maxw):
    return [0] + [int(math.floor(maxw * (ratios[i] - ratios[i - 1]) / (2.0 * ratios[i]) + 0.5)) for i in range(1, len(ratios))]


def class_bases(ratios, maxh, maxw):
    """0-based first class of every scale in the joined vector, and the total"""
    bases, n = [], 0
    for s, d in enumerate(ring_widths(ratios, maxw)):
        bases.append(n)
        n += maxh * maxw if s == 0 else 2 * d * maxw + 2 * (maxh - 2 * d) * d
    return bases, n


def scale_of(idx, ratios, maxh, maxw):
    """the scale every 1-based class id belongs to"""
    bases, _ = class_bases(ratios, maxh, maxw)
    return np.searchsorted(np.asarray(bases), np.asarray(idx) - 1, side="right") - 1


def frames(c, integer=False):
    """the row's frame pair: float frames are multiples of 1/64 up to 4 (an informative soft-min); integer=True: the byte values"""
    f0, f1, _, _ = rp.synth_pair(c.H, c.W, C=c.C, seed=c.seed, max_flow=c.mf, noise_sigma=2.0)
    if integer:
        return f0, f1
    return f0 / np.float32(64), f1 / np.float32(64)


def _top2(joined, rows=64):
    """the two largest class values per pixel [H][W][2] (ascending), in row bands: np.sort of a 1.5 MP joined tensor would copy 1.3 GB"""
    H, W, n = joined.shape
    out = np.empty((H, W, 2), np.float32)
    for y in range(0, H, rows):
        band = joined[y : y + rows]
        out[y : y + rows] = np.sort(band, -1)[..., -2:] if n >= 2 else np.repeat(band, 2, -1)
    return out


def _reference(c, f16_scale):
    f0, f1 = frames(c)
    ref = rp.multiscale_flow_oracle(f0, f1, c.k, c.mh, c.mw, c.ratios, f16_scale=f16_scale)
    out = dict(idx=ref["idx"], top2=_top2(ref["joined"]), middle=ref["middle"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(no, f16_scale=None):
    """the oracle chain of row `no` (0: PREP_ORACLE), computed once per process and shared read-only: idx, top2, middle"""
    return _reference(PREP_ORACLE if no == 0 else BY_NO[no], f16_scale)


def tie_mask(ref):
    return ref["top2"][..., 1] - ref["top2"][..., 0] <= TIE_GAP


def assert_matches_oracle(gi, gflow, ref, c, tie=None):
    """_assert_matches_oracle's rule (tests/test_gpu_multiscale_radial.py) on the shared reference: indices equal the oracle's except where its
    two best classes lie within 1e-5 (`tie`: another mask, for the fp16 rule); at most 2 % of the pixels differ; the decode of whatever
    index was taken is the codec's, exactly."""
    tie = tie_mask(ref) if tie is None else tie
    same = gi == ref["idx"]
    bad = int((~(same | tie)).sum())
    print("row %d: %d of %d pixels differ from the oracle, %d outside ties; tie share %.4f" % (c.no, int((~same).sum()), same.size, bad, float(tie.mean())))
    assert bad == 0, "%d pixels differ from the oracle outside ties" % bad
    assert (~same).mean() <= TIE_CAP
    rc, ey, ex = orc.x2yx_multi(c.mh, c.mw, c.ratios, gi)
    assert rc == 0 and np.array_equal(gflow[0], ey.astype(np.float32)) and np.array_equal(gflow[1], ex.astype(np.float32))
