"""The arg-min key of the int8 flow sweep (csrc/ssd_flow_i8.hip) in numpy, as the kernel computes it: key = (a'.b' << 9) + plane, with the
plane cell of frame-1 row y1, column q holding -(S1 << 8) + (1 - (q & 1)) - 6 y1 - 2 (q >> 4); a lane (n, g) keeps the plain running maximum of
its candidates 16 T + 4 g + 2 sl, + 1 over the tiles in (dy, T) order, masked outside 0 <= q - n <= 32; the decode adds
6 y + x0 / 8 + 254 back and combines the lanes on (E, 4095 - d).  It must return the FIRST minimum of the cost in index order d = 33 dy + dx
and its exact E = 2 a'.b' - S1, with every intermediate inside 32 bits -- on random bytes, on ties, on 255 against 0 (both ways), and with the
strip placed at the largest row and the largest column that dfe_flow_i8_plan admits ((H + 1) Wp < 2^29, Wp >= 80, H >= 39)."""
import numpy as np
import pytest

K, WIN = 7, 33
I32 = (-(1 << 31), (1 << 31) - 1)


def _patch_sums(x):
    """sum over the 7 x 7 x 3 patch at every position (valid)"""
    c = x.sum(0)
    H, W = c.shape
    out = np.zeros((H - K + 1, W - K + 1), np.int64)
    for i in range(K):
        for j in range(K):
            out += c[i : i + H - K + 1, j : j + W - K + 1]
    return out


def _i32(v):
    v = np.asarray(v, np.int64)
    assert v.min() >= I32[0] and v.max() <= I32[1], (v.min(), v.max())
    return v


def _sweep(f0, f1, Y0, X0):
    """one strip of 16 pixels, every output row of the small frames; the frames' row 0 / column 0 are row Y0 / column X0 of a large frame"""
    a, b = f0.astype(np.int64) - 128, f1.astype(np.int64) - 128
    H, W = a.shape[1:]
    Ho = H - (K + WIN - 2)
    S1 = _patch_sums(b * b)                                        # [H - 6][W - 6]
    rows, cols = np.arange(S1.shape[0])[:, None], np.arange(S1.shape[1])[None, :]
    plane = _i32(-(S1 << 8) + (1 - ((X0 + cols) & 1)) - 6 * (Y0 + rows) - 2 * ((X0 + cols) >> 4))
    got_d, got_E, ref_d, ref_E = [], [], [], []
    for y in range(Ho):
        for n in range(16):
            pa = a[:, y + 16 : y + 16 + K, n + 16 : n + 16 + K].ravel()
            E = np.empty((WIN, 48), np.int64)                     # [dy][q], q = n + dx
            Dot = np.empty((WIN, 48), np.int64)
            for dy in range(WIN):
                for q in range(48):
                    Dot[dy, q] = pa @ b[:, y + dy : y + dy + K, q : q + K].ravel()
                    E[dy, q] = 2 * Dot[dy, q] - S1[y + dy, q]
            valid = (np.arange(48) >= n) & (np.arange(48) <= n + 32)
            cost = np.where(valid[None, :], -E, np.iinfo(np.int64).max)[:, n : n + 33]
            d_ref = int(np.argmin(cost.ravel()))                   # the first minimum in index order
            ref_d.append(d_ref)
            ref_E.append(int(-cost.ravel()[d_ref]))
            # the kernel: 4 lane groups x 2 running keys
            base = 6 * (Y0 + y) + (X0 >> 3)
            best_pair = None
            for g in range(4):
                for sl in range(2):
                    best = I32[0]
                    for dy in range(WIN):
                        for T in range(3):
                            for ib in range(2):
                                q = 16 * T + 4 * g + 2 * sl + ib
                                if not valid[q]:
                                    continue
                                wrapped = ((int(Dot[dy, q]) << 9) + int(plane[y + dy, q])) & 0xFFFFFFFF   # (unsigned)D << 9, + P: mod 2^32
                                k = wrapped - (1 << 32) if wrapped >= (1 << 31) else wrapped
                                assert k == 512 * int(Dot[dy, q]) + int(plane[y + dy, q])                  # nothing was lost
                                best = max(best, k)
                    if best == I32[0]:
                        continue                                   # (a lane slot without a valid candidate loses to every other)
                    bt = int(_i32(best + base + 254))
                    u = 255 - (bt & 255)
                    j, ib = u >> 1, u & 1
                    dy, T = divmod(j, 3)
                    d = dy * 33 + 16 * T + 4 * g + 2 * sl + ib - n
                    pair = (bt >> 8, 4095 - d)
                    best_pair = pair if best_pair is None or pair > best_pair else best_pair
            got_E.append(best_pair[0])
            got_d.append(4095 - best_pair[1])
    return got_d, got_E, ref_d, ref_E


def _frames(kind, Ho):
    H, W = Ho + K + WIN - 2, 16 + K + WIN - 2
    rng = np.random.default_rng(17)
    if kind == "random":
        return rng.integers(0, 256, (3, H, W)), rng.integers(0, 256, (3, H, W))
    if kind == "ties":   # period 8 (x) by 6 (y): many candidates with the same cost
        cell = rng.integers(0, 256, (3, 6, 8))
        t = np.tile(cell, (1, H // 6 + 1, W // 8 + 1))[:, :H, :W]
        return np.roll(t, (3, -5), axis=(1, 2)), t
    if kind == "255-0":
        return np.full((3, H, W), 255), np.zeros((3, H, W), np.int64)
    if kind == "0-255":
        return np.zeros((3, H, W), np.int64), np.full((3, H, W), 255)
    if kind == "flat":   # every candidate ties: index 0 wins
        return np.full((3, H, W), 77), np.full((3, H, W), 77)
    raise KeyError(kind)


# the largest frames the plan admits: Wp = 80 with H + 1 = 2^29 / 80 - 1 rows; H = 39 with Wp the largest multiple of 16 below 2^29 / 40
PLACES = {"origin": (0, 0), "last-rows": ((1 << 29) // 80 - 2 - 40, 0), "last-columns": (0, ((1 << 29) // 40 - 80) // 16 * 16)}


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("kind", ["random", "ties", "255-0", "0-255", "flat"])
def test_key_returns_the_first_minimum_and_its_cost(kind, place):
    Ho = 2
    f0, f1 = _frames(kind, Ho)
    Y0, X0 = PLACES[place]
    got_d, got_E, ref_d, ref_E = _sweep(np.asarray(f0), np.asarray(f1), Y0, X0)
    assert got_d == ref_d
    assert got_E == ref_E
    if kind == "flat":
        assert set(got_d) == {0}


def test_order_terms_of_one_pixel_stay_below_a_cost_step():
    # candidate j = 3 dy + T and the column's parity: the plane's term of a pixel's candidates spans 2 * 98 + 1, less than the 256 that one unit of E weighs
    terms = [(1 - ib) - 2 * (3 * dy + T) for dy in range(WIN) for T in range(3) for ib in range(2)]
    assert max(terms) - min(terms) == 197 < 256
    # the extremes of E = 2 a'.b' - S1 over int8 operands, times 256, plus the largest order term, inside 32 bits
    lo = 147 * min(2 * a * b - b * b for a in (-128, 127) for b in (-128, 127))
    hi = 147 * max(2 * a * b - b * b for a in (-128, 127) for b in (-128, 127))
    assert (lo, hi) == (-7187712, 2408448)
    order = 6 * ((1 << 29) // 80) + 2 * (((1 << 29) // 40) >> 4) + 255
    assert lo * 256 - order > I32[0] and hi * 256 + order < I32[1]
