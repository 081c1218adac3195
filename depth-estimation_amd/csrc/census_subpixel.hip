// census_subpixel.hip -- sub-pixel flow on the raw census cost: the single-scale matcher and the pyramid (NOT in the reference; DESIGN.md
// section 4.37).  The rule -- the equiangular ("vee") fit per axis through the integer census costs of the chosen cell and its two
// neighbours -- is in include/dfe.h and restated in numpy in tests/census_subpixel_ref.py; the costs are integers and the fit is one
// IEEE division, so the device is tested against that bit for bit.
//   cenfit_refine_kernel<A>           behind the unchanged sweep (census.hip) and the stand-alone entry: a thread per pixel of the Ha x Wa
//       region, a wave on 64 consecutive pixels of a row.  It is no epilogue of the sweep: there a tile's classes are dealt to four waves,
//       so the winner's neighbours sit in other waves.
//   cenfit_pyramid_refine_kernel<A>   behind the unchanged census pyramid (multiscale.hip) and its stand-alone entry: a thread per fine pixel,
//       the class id's decode (scale, cell) in front of the same device function, one launch for all scales.
// The five costs (cenfit_five_costs) are re-formed from the two signature planes the one call already holds: per channel frame 0's A x A
// box of signatures, shared by all five cells and kept in registers, and frame 1's plus-shaped footprint of (A + 2)^2 - 4 signatures, walked
// row by row: a row of frame 1 meets frame 0's row above it, its own and the one below it (the y neighbours and the cell itself) and, shifted
// by one, its own again (the x neighbours).  Every index is an unrolled constant; the channel loop is not unrolled, so a lane holds one
// channel's box at a time (50 registers at A = 5).  No LDS: a wave's frame-0 loads are consecutive, frame 1's wherever neighbours share
// their class.
#include "dfe_internal.h"

namespace {

typedef unsigned long long u64;

// a0: frame 0's signature at the box's top-left, b0: frame 1's at the chosen cell's, channel 0 both; plane / pitch: signatures of a channel /
// of a row.  inx / iny: the axis has both neighbours inside the window; where it has not, their reads fall on the cell's own footprint (in
// bounds) and the sums are not used.
template <int A>
__device__ __forceinline__ void cenfit_five_costs(const u64 *__restrict__ a0, const u64 *__restrict__ b0, long long plane, int pitch, int C, bool inx,
                                                  bool iny, int &c0, int &cxm, int &cxp, int &cym, int &cyp) {
    const int lo = inx ? -1 : 0, hi = inx ? A : A - 1;
    const long long up = iny ? -(long long)pitch : 0, dn = (long long)(iny ? A : A - 1) * pitch;
    c0 = cxm = cxp = cym = cyp = 0;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const u64 *__restrict__ a = a0 + c * plane;
        const u64 *__restrict__ b = b0 + c * plane;
        u64 f[A][A];
#pragma unroll
        for (int u = 0; u < A; ++u)
#pragma unroll
            for (int v = 0; v < A; ++v) f[u][v] = a[(long long)u * pitch + v];
#pragma unroll
        for (int v = 0; v < A; ++v) cym += __popcll(f[0][v] ^ b[up + v]);              // the row above the cell's box
#pragma unroll
        for (int j = 0; j < A; ++j) {
            const u64 *__restrict__ bj = b + (long long)j * pitch;
            u64 t[A];
#pragma unroll
            for (int v = 0; v < A; ++v) t[v] = bj[v];
            const u64 tl = bj[lo], tr = bj[hi];
#pragma unroll
            for (int v = 0; v < A; ++v) {            // (in this order: with the two edge terms taken out of the loop the a = 5 pyramid form needs 133 VGPRs)
                c0 += __popcll(f[j][v] ^ t[v]);
                cxm += __popcll(f[j][v] ^ (v > 0 ? t[v > 0 ? v - 1 : 0] : tl));
                cxp += __popcll(f[j][v] ^ (v + 1 < A ? t[v + 1 < A ? v + 1 : 0] : tr));
                if (j + 1 < A) cym += __popcll(f[j + 1 < A ? j + 1 : 0][v] ^ t[v]);
                if (j > 0) cyp += __popcll(f[j > 0 ? j - 1 : 0][v] ^ t[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < A; ++v) cyp += __popcll(f[A - 1][v] ^ b[dn + v]);          // the row below it
    }
}

// the vee's apex on one axis (include/dfe.h): integers up to the one IEEE division
__device__ __forceinline__ float cenfit_offset(bool inside, int cm, int c0, int cp) {
    const int dm = cm - c0, dp = cp - c0;
    const int m = dm > dp ? dm : dp;
    float off = 0.f;
    if (inside && m > 0) {
        off = (float)(cm - cp) / (float)(2 * m);
        off = fminf(fmaxf(off, -0.5f), 0.5f);
    }
    return off;
}

struct CenfitArgs {
    const u64 *s0, *s1;          // [C][Hp][Wp]
    int C, Hp, Wp, hWin, wWin, Ha, Wa;
    const long long *idx;        // [Ha][Wa], 1-based
    const float *match_in;       // [Ha][Wa] or NULL: the one call's match score, pasted on the way
    float *match, *fy, *fx;      // at [(y + pad_t) pitch + x + pad_l]
    int pitch, pad_t, pad_l;
};

template <int A>
__global__ __launch_bounds__(256) void cenfit_refine_kernel(const CenfitArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.Wa || y >= a.Ha) return;
    const long long o = (long long)y * a.Wa + x, op = (long long)(y + a.pad_t) * a.pitch + x + a.pad_l;
    if (a.match_in) a.match[op] = a.match_in[o];
    const long long id = a.idx[o];
    if (id < 1 || id > (long long)a.hWin * a.wWin) return;   // (not a class: the pixel's flow stays as it is)
    const int r = ((int)id - 1) / a.wWin, s = (int)id - 1 - r * a.wWin;
    const bool inx = s >= 1 && s + 1 < a.wWin, iny = r >= 1 && r + 1 < a.hWin;
    const int oy = (a.hWin - 1) / 2, ox = (a.wWin - 1) / 2;
    int c0, cxm, cxp, cym, cyp;
    cenfit_five_costs<A>(a.s0 + (long long)(y + oy) * a.Wp + x + ox, a.s1 + (long long)(y + r) * a.Wp + x + s, (long long)a.Hp * a.Wp, a.Wp, a.C, inx, iny, c0,
                         cxm, cxp, cym, cyp);
    a.fy[op] = (float)(r - oy) + cenfit_offset(iny, cym, c0, cyp);
    a.fx[op] = (float)(s - ox) + cenfit_offset(inx, cxm, c0, cxp);
}

template <int A>
__global__ __launch_bounds__(256) void cenfit_pyramid_refine_kernel(const DfeCenfitPyramid a) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const long long p = (long long)y * a.W + x;
    const long long id = a.idx[p];
    if (id < 1 || id > a.ncls) return;   // (not a class: the pixel's flow stays as it is)
    int n = (int)id - 1;
    // the class's scale: the last whose first class is not above it (a per-lane value: selects over the few scales, as in
    // multiscale_refine_subpixel_kernel)
    const u64 *s0 = (const u64 *)a.s0[0], *s1 = (const u64 *)a.s1[0];
    int r = a.r[0], Wg = a.Wg[0], Hg = a.Hg[0], base = 0, d = 0;
    for (int i = 1; i < a.nratios; ++i)
        if (n >= a.base[i]) { s0 = (const u64 *)a.s0[i]; s1 = (const u64 *)a.s1[i]; r = a.r[i]; Wg = a.Wg[i]; Hg = a.Hg[i]; base = a.base[i]; d = a.d[i]; }
    n -= base;
    // class -> cell (ca, cb).  Scale 1: the whole window, row-major.  A coarser scale: the ring of width d around the hole, in the blocks
    // top (d rows of maxw), left, right (maxh - 2 d rows of d each), bottom (x2yxMultiNumber)
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
    const bool inx = cb >= 1 && cb + 1 < mw, iny = ca >= 1 && ca + 1 < mh;
    const int oy = (mh - 1) / 2, ox = (mw - 1) / 2;
    const int ys = y / r, xs = x / r;
    int c0, cxm, cxp, cym, cyp;
    cenfit_five_costs<A>(s0 + (long long)(ys + oy) * Wg + xs + ox, s1 + (long long)(ys + ca) * Wg + xs + cb, (long long)Hg * Wg, Wg, a.C, inx, iny, c0, cxm, cxp,
                         cym, cyp);
    const float rf = (float)r;
    const float sy = rf * cenfit_offset(iny, cym, c0, cyp), sx = rf * cenfit_offset(inx, cxm, c0, cxp);
    a.fy[p] = (float)((ca - oy) * r) + sy;
    a.fx[p] = (float)((cb - ox) * r) + sx;
}

// the checks and the geometry of dfe_census_flow_f32 (census.hip keeps its own to itself), in its order and with its codes
int cenfit_geom(dfe_ctx *ctx, const char *fn, int C, int Hp, int Wp, int hWin, int wWin, int agg, CenfitArgs *g) {
    DFE_REQUIRE(ctx, C >= 1 && C <= 4, DFE_E_ARG, "%s: C=%d channels (1 .. 4)", fn, C);
    DFE_REQUIRE(ctx, agg == 1 || agg == 3 || agg == 5, DFE_E_ARG, "%s: agg=%d must be 1, 3 or 5", fn, agg);
    DFE_REQUIRE(ctx, hWin >= 1 && wWin >= 1, DFE_E_ARG, "%s: window %dx%d", fn, hWin, wWin);
    DFE_REQUIRE(ctx, (long long)hWin * wWin <= kDfeMaxWindowCells, DFE_E_UNSUPPORTED, "%s: window %dx%d has more than %d cells", fn, hWin, wWin,
                kDfeMaxWindowCells);
    DFE_REQUIRE(ctx, Hp >= 1 && Wp >= 1 && Hp <= 32768 && Wp <= 32768, DFE_E_SHAPE, "%s: %dx%d patch positions (1 .. 32768 each)", fn, Hp, Wp);
    g->C = C; g->Hp = Hp; g->Wp = Wp; g->hWin = hWin; g->wWin = wWin;
    g->Ha = Hp - hWin + 1 - agg + 1;
    g->Wa = Wp - wWin + 1 - agg + 1;
    DFE_REQUIRE(ctx, g->Ha >= 1 && g->Wa >= 1, DFE_E_SHAPE, "%s: %dx%d patch positions leave no pixel for a %dx%d window summed over %dx%d", fn, Hp, Wp, hWin,
                wWin, agg, agg);
    return DFE_OK;
}

int cenfit_run(dfe_ctx *ctx, const CenfitArgs &a, int agg) {
    const dim3 grid((unsigned)dfe_cdiv(a.Wa, 64), (unsigned)dfe_cdiv(a.Ha, 4));
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    DfeProfScope prof(ctx);
    if (agg == 1) hipLaunchKernelGGL(cenfit_refine_kernel<1>, grid, dim3(256), 0, ctx->stream, a);
    else if (agg == 3) hipLaunchKernelGGL(cenfit_refine_kernel<3>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(cenfit_refine_kernel<5>, grid, dim3(256), 0, ctx->stream, a);
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "cenfit_refine_kernel";
    return DFE_OK;
}

// the one call behind its device guard.  The sweep is census.hip's, reached through its public entry: it leaves the class map and the
// match score of the region in the arena, and the refinement writes the flow -- integer part and offset -- and the score at the pasted
// positions.  The border and depth pass is the plain one call's.
int cenfit_pair(dfe_ctx *ctx, const char *fn, const void *I0, const void *I1, bool bytes, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                float foe_y, float *flow, float *match, float *depth, float *depth_conf) {
    DfeCensusPair p;
    int rc = dfe_census_pair_check(ctx, fn, I0 && I1 && flow && match, (depth == nullptr) == (depth_conf == nullptr), C, H, W, k, hWin, wWin, agg, &p);
    if (rc) return rc;
    CenfitArgs a{};
    rc = cenfit_geom(ctx, fn, C, p.Hp, p.Wp, hWin, wWin, agg, &a);   // (checked above: the kernel's form of it)
    if (rc) return rc;
    uint64_t *sig0 = nullptr, *sig1 = nullptr;
    int64_t *idx = nullptr;
    float *m = nullptr;
    const size_t n = (size_t)C * p.Hp * p.Wp, na = (size_t)p.Ha * p.Wa;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        sig0 = c.take<uint64_t>(n);
        sig1 = c.take<uint64_t>(n);
        idx = c.take<int64_t>(na);
        m = c.take<float>(na);
    });
    if (rc) return rc;
    rc = dfe_census_pair_transforms(ctx, I0, I1, bytes, C, H, W, k, sig0, sig1);
    if (rc) return rc;
    rc = dfe_census_flow_f32(ctx, sig0, sig1, C, p.Hp, p.Wp, k * k - 1, hWin, wWin, agg, idx, nullptr, m, nullptr, nullptr);
    if (rc) return rc;
    a.s0 = (const u64 *)sig0; a.s1 = (const u64 *)sig1;
    a.idx = (const long long *)idx; a.match_in = m; a.match = match; a.fy = flow; a.fx = flow + (long long)H * W;
    a.pitch = W; a.pad_t = p.pad_t; a.pad_l = p.pad_l;
    rc = cenfit_run(ctx, a, agg);
    if (rc) return rc;
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    return dfe_pair_border_depth(ctx, flow, match, H, W, p.pad_t, p.pad_l, p.Ha, p.Wa, foe_x, foe_y, depth, depth_conf);
}

}  // namespace

int dfe_census_pyramid_subpixel_launch(dfe_ctx *ctx, const DfeCenfitPyramid &a) {
    const dim3 grid((unsigned)dfe_cdiv(a.W, 64), (unsigned)dfe_cdiv(a.H, 4));
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    DfeProfScope prof(ctx);
    if (a.agg == 1) hipLaunchKernelGGL(cenfit_pyramid_refine_kernel<1>, grid, dim3(256), 0, ctx->stream, a);
    else if (a.agg == 3) hipLaunchKernelGGL(cenfit_pyramid_refine_kernel<3>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(cenfit_pyramid_refine_kernel<5>, grid, dim3(256), 0, ctx->stream, a);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

extern "C" {

int dfe_census_refine_subpixel_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int Wp, int hWin, int wWin, int agg,
                                   const int64_t *idx, float *fy, float *fx, int pitch, int pad_t, int pad_l) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_census_refine_subpixel_f32";
    DFE_REQUIRE(ctx, sig0 && sig1 && idx && fy && fx, DFE_E_ARG, "%s: NULL tensor", fn);
    CenfitArgs a{};
    const int rc = cenfit_geom(ctx, fn, C, Hp, Wp, hWin, wWin, agg, &a);
    if (rc) return rc;
    DFE_REQUIRE(ctx, pad_t >= 0 && pad_l >= 0 && pitch >= pad_l + a.Wa, DFE_E_SHAPE, "%s: pitch %d, pad %d/%d for %d columns", fn, pitch, pad_t, pad_l, a.Wa);
    a.s0 = (const u64 *)sig0; a.s1 = (const u64 *)sig1;
    a.idx = (const long long *)idx; a.fy = fy; a.fx = fx;
    a.pitch = pitch; a.pad_t = pad_t; a.pad_l = pad_l;
    return cenfit_run(ctx, a, agg);
}

int dfe_census_flow_depth_pair_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, int agg,
                                            float foe_x, float foe_y, float *flow, float *match, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    return cenfit_pair(ctx, "dfe_census_flow_depth_pair_subpixel_f32", I0, I1, false, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, flow, match, depth, depth_conf);
}

int dfe_census_flow_depth_pair_subpixel_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, int agg,
                                           float foe_x, float foe_y, float scale, float *flow, float *match, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, scale > 0, DFE_E_ARG, "dfe_census_flow_depth_pair_subpixel_u8: scale=%g must be positive", (double)scale);
    return cenfit_pair(ctx, "dfe_census_flow_depth_pair_subpixel_u8", I0, I1, true, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, flow, match, depth, depth_conf);
}

int dfe_multiscale_census_flow_pair_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int maxh, int maxw,
                                                 const int *ratios, int nratios, int agg, float beta, float *flow, int64_t *idx) {
    DFE_ENTER(ctx);
    return dfe_multiscale_census_pair(ctx, I0, I1, false, C, H, W, k, maxh, maxw, ratios, nratios, agg, beta, flow, idx,
                                      "dfe_multiscale_census_flow_pair_subpixel_f32", true);
}

int dfe_multiscale_census_flow_pair_subpixel_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int maxh, int maxw,
                                                const int *ratios, int nratios, int agg, float beta, float *flow, int64_t *idx) {
    DFE_ENTER(ctx);
    return dfe_multiscale_census_pair(ctx, I0, I1, true, C, H, W, k, maxh, maxw, ratios, nratios, agg, beta, flow, idx,
                                      "dfe_multiscale_census_flow_pair_subpixel_u8", true);
}

}  // extern "C"
