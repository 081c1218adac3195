"""The census matching cost in numpy, written from the definition in include/dfe.h, not from the device's walk:
signature, Hamming distance, box aggregation, the first minimum with the centre rule, the match score, the paste.  Whole arrays at a
time; nothing here knows about tiles, bands or lanes.  Also the exposure scene of the quality table."""
import numpy as np

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def popcount(x):
    """bits set in every element of a uint64 array"""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    return _POP8[x.view(np.uint8).reshape(x.shape + (8,))].sum(-1)


def signature(I, kh, kw):
    """I [C][H][W] (any dtype; compared as stored) -> uint64 [C][Hp][Wp]: bit b = the b-th cell of the patch, row-major without the centre,
    is strictly below the centre"""
    C, H, W = I.shape
    Hp, Wp = H - kh + 1, W - kw + 1
    ci, cj = kh // 2, kw // 2
    centre = I[:, ci:ci + Hp, cj:cj + Wp]
    S = np.zeros((C, Hp, Wp), dtype=np.uint64)
    b = 0
    with np.errstate(invalid="ignore"):
        for i in range(kh):
            for j in range(kw):
                if (i, j) == (ci, cj):
                    continue
                S |= (I[:, i:i + Hp, j:j + Wp] < centre).astype(np.uint64) << np.uint64(b)
                b += 1
    assert b == kh * kw - 1
    return S


def hamming(S0, S1, hWin, wWin):
    """h[y][x][dy][dx] = sum_c popcount(S0[c][y+oy][x+ox] ^ S1[c][y+dy][x+dx]): int64 [Ho][Wo][hWin][wWin]"""
    C, Hp, Wp = S0.shape
    Ho, Wo = Hp - hWin + 1, Wp - wWin + 1
    oy, ox = (hWin - 1) // 2, (wWin - 1) // 2
    a = S0[:, oy:oy + Ho, ox:ox + Wo]
    h = np.empty((Ho, Wo, hWin, wWin), dtype=np.int64)
    for dy in range(hWin):
        for dx in range(wWin):
            h[:, :, dy, dx] = popcount(a ^ S1[:, dy:dy + Ho, dx:dx + Wo]).sum(0)
    return h


def aggregate(h, a):
    """cost[y][x] = sum_{u < a, v < a} h[y+u][x+v], per class"""
    Ho, Wo = h.shape[:2]
    Ha, Wa = Ho - a + 1, Wo - a + 1
    cost = np.zeros((Ha, Wa) + h.shape[2:], dtype=np.int64)
    for u in range(a):
        for v in range(a):
            cost += h[u:u + Ha, v:v + Wa]
    return cost


def cost_volume(S0, S1, hWin, wWin, a):
    return aggregate(hamming(S0, S1, hWin, wWin), a)


def middle_index(hWin, wWin):
    """getMiddleIndex, 1-based"""
    return (wWin + 1) // 2 + wWin * ((hWin + 1) // 2 - 1)


def arg_best(cost):
    """(idx 1-based int64, best int64): the first minimum in class order; the centre class wins an exact tie with the best"""
    Ha, Wa, hWin, wWin = cost.shape
    flat = cost.reshape(Ha, Wa, hWin * wWin)
    idx = flat.argmin(-1) + 1          # numpy's argmin is the first one
    best = flat.min(-1)
    mid = middle_index(hWin, wWin)
    idx[flat[:, :, mid - 1] == best] = mid
    return idx.astype(np.int64), best


def decode(idx, hWin, wWin):
    """dfe_x2yx: (flow_y, flow_x) as float32"""
    fl = (idx - 1) // wWin
    return (fl - (hWin - 1) // 2).astype(np.float32), (idx - 1 - fl * wWin - (wWin - 1) // 2).astype(np.float32)


def match_score(best, nbits, C, a):
    """1.0f - (float)best / (float)(nbits C a^2): one rounded fp32 division, one rounded subtraction"""
    return (np.float32(1.0) - best.astype(np.float32) / np.float32(nbits * C * a * a)).astype(np.float32)


def flow(S0, S1, nbits, hWin, wWin, a):
    """what dfe_census_flow_f32 returns"""
    idx, best = arg_best(cost_volume(S0, S1, hWin, wWin, a))
    fy, fx = decode(idx, hWin, wWin)
    return dict(idx=idx, best=best.astype(np.float32), match=match_score(best, nbits, S0.shape[0], a), flow_y=fy, flow_x=fx)


def region(H, W, kh, kw, hWin, wWin, a):
    """(pad_t, pad_l, Ha, Wa) of the pasted output"""
    Ha, Wa = H - kh + 1 - hWin + 1 - a + 1, W - kw + 1 - wWin + 1 - a + 1
    return (H - Ha) // 2, (W - Wa) // 2, Ha, Wa


def paste(plane, H, W, pad_t, pad_l):
    out = np.zeros((H, W), dtype=plane.dtype)
    out[pad_t:pad_t + plane.shape[0], pad_l:pad_l + plane.shape[1]] = plane
    return out


def pair(I0, I1, k, hWin, wWin, a):
    """what dfe_census_flow_depth_pair_* returns before depth: (flow [2][H][W], match [H][W])"""
    C, H, W = I0.shape
    r = flow(signature(I0, k, k), signature(I1, k, k), k * k - 1, hWin, wWin, a)
    pt, pl, _, _ = region(H, W, k, k, hWin, wWin, a)
    return np.stack([paste(r["flow_y"], H, W, pt, pl), paste(r["flow_x"], H, W, pt, pl)]), paste(r["match"], H, W, pt, pl)


# ---- the exposure scene: a smooth random texture moved by a whole number of pixels, the second frame darker, offset and noisy ----
SCENE = dict(H=72, W=104, k=7, win=9, move=(2, -3), gain=0.5, offset=40.0, sigma=1.0, margin=8)


def scene(seed, gain=SCENE["gain"], offset=SCENE["offset"]):
    """two uint8 frames [1][72][104]: frame 1 is frame 0's texture moved by (+2, -3) pixels (y, x), times gain, plus offset, plus N(0, 1);
    both floored and clipped to 0 .. 255"""
    rng = np.random.RandomState(seed)
    H, W, m = SCENE["H"], SCENE["W"], SCENE["margin"]
    t = rng.uniform(size=(H + 2 * m, W + 2 * m))
    for _ in range(4):                     # the 5-point mean, with wrap-around
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    my, mx = SCENE["move"]
    f0 = t[m:m + H, m:m + W]
    f1 = t[m - my:m - my + H, m - mx:m - mx + W] * gain + offset + rng.normal(0.0, SCENE["sigma"], size=(H, W))   # f1[p + move] = f0[p]
    to_u8 = lambda f: np.clip(np.floor(f), 0, 255).astype(np.uint8)[None]
    return to_u8(f0), to_u8(f1)


def share_wrong(fy, fx):
    my, mx = SCENE["move"]
    return float(np.mean((fy != my) | (fx != mx)))
