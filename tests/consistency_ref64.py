"""Forward-backward flow consistency (dfe_flow_consistency_f32; include/dfe.h) restated in numpy: q, the reach test
and the bilinear weights in fp32 as the definition says, the sample, the residual and its norm in float64.  Plus the scene the feature is
for: a textured background translating by one vector with a textured rectangle translating by another over it, so that a known band of
the background is covered in frame 1.  Test infrastructure (no test in this file)."""
import numpy as np

from tests.test_gpu_subpixel import translation, warped_pair


def consistency_ref(fw, bw, region, tol):
    """fw, bw [2][H][W] (y, x); region = (y0, x0, Ho, Wo) inside the frame.  Returns (mask float32 [H][W], err float64 [H][W])."""
    fw = np.ascontiguousarray(fw, np.float32)
    bw64 = np.ascontiguousarray(bw, np.float32).astype(np.float64)
    _, H, W = fw.shape
    y0, x0, Ho, Wo = region
    assert Ho > 0 and Wo > 0 and y0 >= 0 and x0 >= 0 and y0 + Ho <= H and x0 + Wo <= W
    yi, xi = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inR = (yi >= y0) & (yi < y0 + Ho) & (xi >= x0) & (xi < x0 + Wo)
    fin = np.isfinite(fw[0]) & np.isfinite(fw[1])
    with np.errstate(invalid="ignore", over="ignore"):
        qy, qx = yi.astype(np.float32) + fw[0], xi.astype(np.float32) + fw[1]   # fp32
        assert qy.dtype == np.float32
        fly, cly, flx, clx = np.floor(qy), np.ceil(qy), np.floor(qx), np.ceil(qx)
        reach = fin & (fly >= y0) & (cly <= y0 + Ho - 1) & (flx >= x0) & (clx <= x0 + Wo - 1)
        wy, wx = qy - fly, qx - flx                                              # fp32
        uy, ux = np.float32(1) - wy, np.float32(1) - wx
        assert wy.dtype == np.float32 and uy.dtype == np.float32
        r0, r1 = (np.where(reach, v, y0).astype(np.int64) for v in (fly, cly))
        c0, c1 = (np.where(reach, v, x0).astype(np.int64) for v in (flx, clx))
        b = np.zeros((2, H, W))
        for fa, fb, rr, cc in ((uy, ux, r0, c0), (uy, wx, r0, c1), (wy, ux, r1, c0), (wy, wx, r1, c1)):
            read = reach & (fa != 0) & (fb != 0)           # a tap with a zero factor is not read
            w = fa.astype(np.float64) * fb.astype(np.float64)
            b += np.where(read, w * bw64[:, rr, cc], 0.0)
        ok = inR & reach & np.isfinite(b[0]) & np.isfinite(b[1])
        e = fw.astype(np.float64) + b
        d2 = e[0] * e[0] + e[1] * e[1]
    err = np.where(inR, np.inf, 0.0)
    err[ok] = np.sqrt(d2[ok])
    tol2 = float(np.float32(tol) * np.float32(tol))
    mask = np.zeros((H, W), np.float32)
    mask[ok & (d2 <= tol2)] = 1.0
    return mask, err


def _box(H, W, y, x, h, w):
    m = np.zeros((H, W), bool)
    m[max(y, 0) : max(y + h, 0), max(x, 0) : max(x + w, 0)] = True
    return m


def occlusion_scene(H, W, bg, fg, rect, reach, region, seed=0, sigma=2.0):
    """Byte-valued float32 frames [3][H][W]: the background moves by bg = (dy, dx), the rectangle rect = (y, x, h, w) of frame 0 by
    fg = (dy, dx) (integers).  Returns f0, f1 and two boolean maps of frame 0 inside region = (y0, x0, Ho, Wo):
      covered   background pixels whose place in frame 1 lies under the rectangle (no true match exists there),
      interior  visible pixels more than `reach` from every motion boundary (the rectangle's outline in either frame, carried back along
                either motion) and from the region's edge."""
    b0, b1 = warped_pair(H, W, translation(*bg), seed=seed, sigma=sigma)
    o0, o1 = warped_pair(H, W, translation(*fg), seed=seed + 1000, sigma=sigma)
    y, x, h, w = rect
    in0, in1 = _box(H, W, y, x, h, w), _box(H, W, y + fg[0], x + fg[1], h, w)
    f0, f1 = np.where(in0, o0, b0), np.where(in1, o1, b1)
    y0, x0, Ho, Wo = region
    R = _box(H, W, y0, x0, Ho, Wo)
    covered = R & ~in0 & _box(H, W, y + fg[0] - bg[0], x + fg[1] - bg[1], h, w)
    # every place a motion boundary can show up for a frame-0 pixel: the outline in frame 0, in frame 1, and frame 1's carried back by bg
    ys = (y, y + fg[0], y + fg[0] - bg[0])
    xs = (x, x + fg[1], x + fg[1] - bg[1])
    near = _box(H, W, min(ys) - reach, min(xs) - reach, max(ys) - min(ys) + h + 2 * reach, max(xs) - min(xs) + w + 2 * reach)
    deep = _box(H, W, max(ys) + reach, max(xs) + reach, min(ys) + h - max(ys) - 2 * reach, min(xs) + w - max(xs) - 2 * reach)
    interior = _box(H, W, y0 + reach, x0 + reach, Ho - 2 * reach, Wo - 2 * reach) & (~near | deep)
    return np.ascontiguousarray(f0, np.float32), np.ascontiguousarray(f1, np.float32), covered, interior
