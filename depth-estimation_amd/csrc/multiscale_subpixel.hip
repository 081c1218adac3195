// multiscale_subpixel.hip -- sub-pixel refinement of the raw-patch pyramid matcher's flow (not in the reference).
//   dfe_multiscale_subpixel_launch    behind the one-call matcher (multiscale.hip: ms_run, then this) and the stand-alone entry
// Per fine pixel: its class id decodes to a scale s (ratio r) and a cell (a, b) of that scale's window; the SSD costs of the cell and
// of its two neighbours on either axis are formed from scale s's padded frames at the scale's pixel (y / r, x / r) -- the values
// dfe_pyramid_scale_volume_f32 holds there -- and the parabola through them (subpixel_offset.h) moves the integer flow d r by r off
// (include/dfe.h).
//
// Layout: that of the single-scale refinement (subpixel.hip).  A wave is 64 consecutive fine pixels of one row, one pixel per lane, no
// LDS, both frames through L1 / L2, the five costs with shared reads (subpixel_costs.h: 390 loads at k = 7, C = 3).  Where the finest
// scale wins -- nearly every pixel of a textured frame -- frame 0's rows are the same for every lane and frame 1's coalesce wherever
// neighbours share their class.  The r fine pixels in a row under one coarse pixel that share a coarse class read the same addresses:
// one fetch serves them (and the r rows of fine pixels above each other meet in L2).  The scale is a per-lane value, not a branch: a
// wave whose lanes won on different scales runs the same instructions on different base pointers and pitches.
#include "dfe_internal.h"
#include "subpixel_offset.h"   // the parabola's vertex on one axis
#include "subpixel_costs.h"    // the five costs, from the frames

namespace {

template <int K>
__global__ __launch_bounds__(256) void multiscale_refine_subpixel_kernel(MsSubpixelArgs a) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const long long p = (long long)y * a.W + x;
    const long long id = a.idx[p];
    if (id < 1 || id > a.ncls) return;   // (not a class: the pixel's flow stays as it is)
    int n = (int)id - 1;
    // the class's scale: the last whose first class is not above it; its frames and sizes picked up on the way (the scale differs from
    // lane to lane: selects over the few scales, no indexed read of the arguments)
    const float *p0 = a.p0[0], *p1 = a.p1[0];
    int r = a.r[0], Wp = a.Wp[0], Hp = a.Hp[0], base = 0, d = 0;
    for (int i = 1; i < a.nratios; ++i)
        if (n >= a.base[i]) { p0 = a.p0[i]; p1 = a.p1[i]; r = a.r[i]; Wp = a.Wp[i]; Hp = a.Hp[i]; base = a.base[i]; d = a.d[i]; }
    n -= base;
    // class -> cell (ca, cb).  Scale 1: the whole window, row-major.  A coarser scale: the ring of width d around the hole, in the
    // blocks top (d rows of maxw), left, right (maxh - 2 d rows of d each), bottom (x2yxMultiNumber, multi_decode_t)
    const int mh = a.maxh, mw = a.maxw;
    int rowlen = mw, row0 = 0, col0 = 0;
    if (base > 0) {
        const int top = d * mw, side = (mh - 2 * d) * d;
        if (n >= top + 2 * side) { n -= top + 2 * side; row0 = mh - d; }
        else if (n >= top + side) { n -= top + side; rowlen = d; row0 = d; col0 = mw - d; }
        else if (n >= top) { n -= top; rowlen = d; row0 = d; }
    }
    const int q = n / rowlen;
    const int ca = q + row0, cb = n - q * rowlen + col0;
    // neighbours outside the window are not read: their cells are replaced by the centre cell (in bounds) and the axis gives off = 0
    const bool inx = cb >= 1 && cb + 1 < mw, iny = ca >= 1 && ca + 1 < mh;
    const int bm = inx ? cb - 1 : cb, bp = inx ? cb + 1 : cb, am = iny ? ca - 1 : ca, ap = iny ? ca + 1 : ca;
    const int oy = (mh - 1) / 2, ox = (mw - 1) / 2;
    const int ys = y / r, xs = x / r;
    const float *A = p0 + (long long)(ys + oy) * Wp + xs + ox;   // frame-0 patch of the scale's pixel
    const float *B = p1 + (long long)ys * Wp + xs + cb;          // frame-1 column of the cell, row 0 of the pixel's window
    float c0, cxm, cxp, cym, cyp;
    subpixel_five_costs<K>(A, B, (long long)Hp * Wp, Wp, a.C, a.k, a.k, ca, am, ap, bm - cb, bp - cb, c0, cxm, cxp, cym, cyp);
    const float rf = (float)r;
    const float sy = rf * subpixel_offset(iny, cym, c0, cyp), sx = rf * subpixel_offset(inx, cxm, c0, cxp);
    a.fy[p] = (float)((ca - oy) * r) + sy;
    a.fx[p] = (float)((cb - ox) * r) + sx;
}

}  // namespace

int dfe_multiscale_subpixel_launch(dfe_ctx *ctx, const MsSubpixelArgs &a) {
    const dim3 grid((unsigned)dfe_cdiv(a.W, 64), (unsigned)dfe_cdiv(a.H, 4));
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    if (a.k == 7) hipLaunchKernelGGL(multiscale_refine_subpixel_kernel<7>, grid, dim3(256), 0, ctx->stream, a);
    else if (a.k == 5) hipLaunchKernelGGL(multiscale_refine_subpixel_kernel<5>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(multiscale_refine_subpixel_kernel<0>, grid, dim3(256), 0, ctx->stream, a);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}
