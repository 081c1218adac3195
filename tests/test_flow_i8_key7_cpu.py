"""The arg-min key of the int8 flow sweep (csrc/ssd_flow_i8.hip) with its 7-bit order field, in numpy, as the kernel computes it:
key = (D << 8) + plane modulo 2^32, where D = a'.b' + (kKeyPen for a candidate outside 0 <= q - n <= 32, the MFMA accumulator's start
value) and the plane cell of frame-1 row y1, column q holds Z - (S1 << 7) - 3 y1 - (q >> 4); a lane (n, g) keeps FOUR running keys, one
per i, the plain maximum over all its candidates 16 T + 4 g + i in every displacement row, masked ones included; the decode adds
3 y + x0 / 16 + 127 - Z back and combines the keys and the lane groups on (E, 4095 - d).  It must return the FIRST minimum of the cost in
index order d = 33 dy + dx and its exact E = 2 a'.b' - S1, with every key, valid or masked, inside 32 bits -- on the frames and at the
places of tests/test_flow_i8_key_cpu.py, which stays as the record of the former key."""
import numpy as np
import pytest

from tests.test_flow_i8_key_cpu import I32, K, PLACES, WIN, _frames, _i32, _patch_sums

Z = 1 << 30              # kKeyZ
Q = -10485760            # the penalty in units of E = 2 a'.b' - S1
PEN = Q // 2             # kKeyPen: what the accumulator starts from
E_LO, E_HI = -7187712, 2408448


def _sweep(f0, f1, Y0, X0):
    """one strip of 16 pixels, every output row of the small frames; the frames' row 0 / column 0 are row Y0 / column X0 of a large frame"""
    a, b = f0.astype(np.int64) - 128, f1.astype(np.int64) - 128
    H, W = a.shape[1:]
    Ho = H - (K + WIN - 2)
    S1 = _patch_sums(b * b)                                        # [H - 6][W - 6]
    rows, cols = np.arange(S1.shape[0])[:, None], np.arange(S1.shape[1])[None, :]
    plane = _i32(Z - (S1 << 7) - 3 * (Y0 + rows) - ((X0 + cols) >> 4))
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
            assert E.min() >= E_LO and E.max() <= E_HI
            valid = (np.arange(48) >= n) & (np.arange(48) <= n + 32)
            cost = np.where(valid[None, :], -E, np.iinfo(np.int64).max)[:, n : n + 33]
            d_ref = int(np.argmin(cost.ravel()))                   # the first minimum in index order
            ref_d.append(d_ref)
            ref_E.append(int(-cost.ravel()[d_ref]))
            # the kernel: 4 lane groups x 4 running keys, over all 48 columns
            base = 3 * (Y0 + y) + (X0 >> 4)
            lo_valid, hi_masked = I32[1], I32[0]
            best_pair = None
            for g in range(4):
                for i in range(4):
                    best = I32[0]
                    for dy in range(WIN):
                        for T in range(3):
                            q = 16 * T + 4 * g + i
                            masked = (T == 0 and 4 * g + i < n) or (T == 2 and 4 * g + i > n)
                            assert masked == (not valid[q])
                            D = int(Dot[dy, q]) + (PEN if masked else 0)                           # the accumulator's start value
                            wrapped = ((D << 8) + int(plane[y + dy, q])) & 0xFFFFFFFF              # (unsigned)D << 8, + P: mod 2^32
                            k = wrapped - (1 << 32) if wrapped >= (1 << 31) else wrapped
                            assert k == 256 * D + int(plane[y + dy, q])                            # nothing was lost, masked or not
                            assert k == ((int(E[dy, q]) + (Q if masked else 0)) << 7) + Z - (3 * dy + T) - base
                            if masked:
                                hi_masked = max(hi_masked, k)
                            else:
                                lo_valid = min(lo_valid, k)
                            best = max(best, k)
                    bt = int(_i32(best + (base + 127 - Z)))
                    j = 127 - (bt & 127)
                    dy, T = divmod(j, 3)
                    assert 0 <= dy < WIN and valid[16 * T + 4 * g + i]                             # every running key ends on a valid candidate
                    d = dy * 33 + 16 * T + 4 * g + i - n
                    pair = (bt >> 7, 4095 - d)
                    best_pair = pair if best_pair is None or pair > best_pair else best_pair
            assert hi_masked < lo_valid                                                            # (n = 0 masks tile 2 only, n = 15 tile 0 only)
            got_E.append(best_pair[0])
            got_d.append(4095 - best_pair[1])
    return got_d, got_E, ref_d, ref_E


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("kind", ["random", "ties", "255-0", "0-255", "flat"])
def test_key7_returns_the_first_minimum_and_its_cost(kind, place):
    Ho = 2
    f0, f1 = _frames(kind, Ho)
    Y0, X0 = PLACES[place]
    got_d, got_E, ref_d, ref_E = _sweep(np.asarray(f0), np.asarray(f1), Y0, X0)
    assert got_d == ref_d
    assert got_E == ref_E
    if kind == "flat":
        assert set(got_d) == {0}


def test_masked_keys_lie_below_valid_keys_inside_32_bits():
    lo = 147 * min(2 * a * b - b * b for a in (-128, 127) for b in (-128, 127))
    hi = 147 * max(2 * a * b - b * b for a in (-128, 127) for b in (-128, 127))
    assert (lo, hi) == (E_LO, E_HI)
    assert Q % 2 == 0 and Q <= -(hi - lo) - 2
    # one pixel: all its candidates share base; the order term -j - base has j = 0 .. 98
    for base in (0, 3 * ((1 << 29) // 80) + (((1 << 29) // 40) >> 4)):   # (more than the largest row and the largest column together)
        masked_max = ((hi + Q) << 7) + Z - 0 - base
        valid_min = (lo << 7) + Z - 98 - base
        assert masked_max < valid_min
        masked_min = ((lo + Q) << 7) + Z - 98 - base
        valid_max = (hi << 7) + Z - 0 - base
        assert I32[0] <= masked_min and valid_max <= I32[1]
        # the decode's addend and its result (a running key ends on a valid candidate: only those are decoded)
        assert I32[0] <= base + 127 - Z and I32[0] <= valid_min + base + 127 - Z and valid_max + base + 127 - Z <= I32[1]
    # the accumulator itself: a masked dot product starts at PEN
    assert I32[0] <= PEN - 147 * 128 * 128 and PEN + 147 * 128 * 128 <= I32[1]


def test_order_terms_of_one_pixel_span_less_than_the_order_field():
    terms = [-(3 * dy + T) for dy in range(WIN) for T in range(3)]
    assert max(terms) - min(terms) == 98 < 128
