"""The two-row step of the int8 flow sweep (csrc/ssd_flow_i8.hip, I8Sweep<2, false>::step), restated in numpy: the operands as the lanes of
v_mfma_i32_16x16x64_i8 hold them (row pairs, zeroed halves, the zero eighth pixel), the products C of the six image rows that output rows
y0 and y0 + 1 share, carried one step, and the two edge steps.  One strip of 16 pixels, rows y0 and y0 + 1: S0 + S1 - 2 D must be the
oracle's SSD volume at all 33 x 33 candidates of both rows."""
import numpy as np
import pytest

from tests import oracle as orc

K, WIN = 7, 33
H, W = 2 + K + WIN - 2, 16 + K + WIN - 2   # Ho = 2, Wo = 16
WP = 16 + 64                                # dfe_flow_i8_plan: one strip
Y0, X0 = 0, 0


def _pack(f):
    """(c0 - 128, c1 - 128, c2 - 128, 0) per pixel, zero beyond the frame's width"""
    pk = np.zeros((H, WP, 4), np.int64)
    pk[:, :W, :3] = np.moveaxis(f.astype(np.int64) - 128, 0, 2)
    return pk


def _patch_sums(pk):
    sq = (pk ** 2).sum(axis=2)
    out = np.zeros((H, WP), np.int64)
    for y in range(H - K + 1):
        for x in range(WP - K + 1):
            out[y, x] = sq[y:y + K, x:x + K].sum()
    return out


def _operand(pk, row_lo, row_hi, col, zero_eighth):
    """[16 lanes of a group][4 lane groups][16 bytes]: groups 0, 1 hold the left / right four pixels of row_lo from column col + lane on,
    groups 2, 3 those of row_hi; a row of None is a zeroed half"""
    op = np.zeros((16, 4, 16), np.int64)
    for g in range(4):
        h, up = g & 1, g >> 1
        row = row_hi if up else row_lo
        if row is None:
            continue
        for m in range(16):
            v = pk[row, col + m + 4 * h: col + m + 4 * h + 4].copy()
            if zero_eighth and h:
                v[3] = 0
            op[m, g] = v.reshape(16)
    return op


def _mfma(A, B, acc):
    """D[m][n] = acc[m][n] + sum over the 64 bytes of K"""
    return acc + np.einsum("mgk,ngk->mn", A, B)


def _sweep(f0, f1):
    """cost[r][n][dy][dx] of rows Y0 + r, r = 0, 1, by the two-row step"""
    pk0, pk1 = _pack(f0), _pack(f1)
    s0, s1 = _patch_sums(pk0), _patch_sums(pk1)
    # frame 0: B[t] = rows (Y0 + 16 + t | Y0 + 16 + t + 3), the duplicate row 3 of B[0] zero; Bbot = (zero | row Y0 + 23)
    B = [_operand(pk0, Y0 + 16 + t, None if t == 0 else Y0 + 16 + t + 3, X0 + 16, True) for t in range(4)]
    Bbot = _operand(pk0, None, Y0 + 23, X0 + 16, True)
    cost = np.full((2, 16, WIN, WIN), -1, np.int64)
    C = [None] * 3
    for s in range(WIN + 1):
        first, last = s == 0, s == WIN
        for T in range(3):
            # frame 1: F_t = rows (Y0 + s + t | Y0 + s + t + 3), candidate columns 16 T + m
            F = [_operand(pk1, Y0 + s + t, Y0 + s + t + 3, X0 + 16 * T, False) for t in range(4)]
            D = [None, None]
            if not first:
                D[1] = _mfma(F[3], Bbot, C[T])                     # row Y0 + 1, dy = s - 1: C(s - 1) and its patch row 6
            if not last:
                c = np.zeros((16, 16), np.int64)
                for t in (1, 2, 3):
                    c = _mfma(F[t], B[t], c)
                C[T] = c                                            # frame-0 rows Y0 + 17 .. 22 with frame-1 rows Y0 + s + 1 .. s + 6
                D[0] = _mfma(F[0], B[0], c)                         # row Y0, dy = s: C(s) and its patch row 0
            for r in range(2):
                if D[r] is None:
                    continue
                dy = s - r
                for m in range(16):
                    for n in range(16):
                        dx = 16 * T + m - n
                        if 0 <= dx < WIN:
                            assert cost[r, n, dy, dx] == -1
                            # both rows read the one plane row Y0 + s = (Y0 + r) + dy
                            cost[r, n, dy, dx] = s0[Y0 + r + 16, X0 + n + 16] + s1[Y0 + s, X0 + 16 * T + m] - 2 * D[r][m, n]
    return cost


def _frames():
    rng = np.random.default_rng(41)
    rnd0, rnd1 = (rng.integers(0, 256, (3, H, W)).astype(np.float32) for _ in range(2))
    yield "random", rnd0, rnd1
    yield "0-255", np.zeros((3, H, W), np.float32), np.full((3, H, W), 255.0, np.float32)
    yield "255-0", np.full((3, H, W), 255.0, np.float32), np.zeros((3, H, W), np.float32)
    one = rnd0.copy()
    one[:, 23, :] = rng.integers(0, 256, (3, W)).astype(np.float32)   # (frame-0 row Y0 + 23 is row Y0 + 1's alone; in frame 1 it meets every patch row)
    yield "one-row-frame1", rnd0, one
    yield "one-row-frame0", one, rnd0


@pytest.mark.parametrize("name,f0,f1", list(_frames()), ids=[f[0] for f in _frames()])
def test_two_row_step_is_the_ssd_volume(name, f0, f1):
    vol = orc.ssd_cost_volume(f0, f1, K, K, WIN, WIN)   # [Ho][Wo][dy][dx]
    assert vol.shape == (2, 16, WIN, WIN)
    cost = _sweep(f0, f1)
    assert (cost >= 0).all()                            # every candidate of both rows was formed, once
    assert np.array_equal(vol, np.rint(vol)) and np.array_equal(cost, vol.astype(np.int64))
