// subpixel.hip -- sub-pixel refinement of the single-scale SSD flow (not in the reference).
//   dfe_flow_depth_pair_subpixel_f32    dfe_flow_depth_pair_f32, then the refinement of its flow (and depth / confidence from it)
//   dfe_flow_depth_pair_subpixel_u8     the same on uint8 frames (ingest.hip: the step's converted frames)
//   dfe_flow_refine_subpixel_f32        the refinement alone, from dfe_ssd_flow_f32's 1-based idx
// Per pixel and axis: the SSD costs of the arg-min cell and of its two neighbours on that axis are recomputed from the frames, and a
// parabola through the three moves the integer flow by off = (cm - cp) / (2 ((cm - c0) + (cp - c0))), clamped to [-0.5, 0.5]; 0 where a
// neighbour lies outside the searched window or the curvature is not positive (include/dfe.h).
//
// Layout: no LDS tile.  A wave is 64 consecutive output pixels of one row, one pixel per lane, reading both frames through L1/L2:
// frame 0's rows are the same for every lane and coalesce to two 128-B lines per load; frame 1's rows coalesce wherever neighbouring
// pixels share their flow, which is most of a frame.  The five costs share their reads and are the bit patterns of
// dfe_ssd_cost_volume_f32's reference kernel (subpixel_costs.h).
#include "dfe_internal.h"
#include "cv_records.h"        // pair_depth_px
#include "subpixel_offset.h"   // the parabola's vertex on one axis (include/dfe.h: this order, IEEE division)
#include "subpixel_costs.h"    // the five costs, from the frames

namespace {

struct RefineArgs {
    const float *I0, *I1;          // [C][H][W]
    int C, H, W, kh, kw, hWin, wWin, Ho, Wo;
    const long long *idx;          // [Ho][Wo], 1-based (stand-alone form) or null: the integer flow is read from fy / fx
    float *fy, *fx;                // at (y + pad_t) * pitch + x + pad_l; read (pair form) and written
    int pitch, pad_t, pad_l;
    float *depth, *conf;           // pair form only, same addressing as fy / fx; or null
    float mw, mh, infty;           // focus of expansion, depth clamp (pair_depth_px)
};

// K > 0: a K x K patch, known at compile time; K == 0: any patch (subpixel_costs.h).
template <int K>
__global__ __launch_bounds__(256) void flow_refine_subpixel_kernel(RefineArgs a) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.Wo || y >= a.Ho) return;
    const long long fo = (long long)(y + a.pad_t) * a.pitch + x + a.pad_l;
    const int oy = (a.hWin - 1) / 2, ox = (a.wWin - 1) / 2;
    int r, s;
    if (a.idx) {
        const long long id = a.idx[(long long)y * a.Wo + x];
        if (id < 1 || id > (long long)a.hWin * a.wWin) return;   // (not a cell of the window: the pixel's outputs stay as they are)
        r = (int)((id - 1) / a.wWin);
        s = (int)(id - 1) - r * a.wWin;
    } else {
        r = (int)a.fy[fo] + oy;
        s = (int)a.fx[fo] + ox;
        if (r < 0 || r >= a.hWin || s < 0 || s >= a.wWin) return;
    }
    // neighbours outside the window are not read: their cells are replaced by the centre cell (in bounds) and the axis gives off = 0
    const bool inx = s >= 1 && s + 1 < a.wWin, iny = r >= 1 && r + 1 < a.hWin;
    const int sm = inx ? s - 1 : s, sp = inx ? s + 1 : s, rm = iny ? r - 1 : r, rp = iny ? r + 1 : r;
    const long long plane = (long long)a.H * a.W;
    const float *A = a.I0 + (long long)(y + oy) * a.W + x + ox;   // frame-0 patch, row i at A + i W
    const float *B = a.I1 + (long long)y * a.W + x + s;           // frame-1 column of the arg-min cell, row 0 of the pixel's window
    float c0, cxm, cxp, cym, cyp;
    subpixel_five_costs<K>(A, B, plane, a.W, a.C, a.kh, a.kw, r, rm, rp, sm - s, sp - s, c0, cxm, cxp, cym, cyp);
    const float fy = (float)(r - oy) + subpixel_offset(iny, cym, c0, cyp);
    const float fx = (float)(s - ox) + subpixel_offset(inx, cxm, c0, cxp);
    a.fy[fo] = fy;
    a.fx[fo] = fx;
    if (a.depth) pair_depth_px(y + a.pad_t, x + a.pad_l, fy, fx, a.mw, a.mh, a.infty, &a.depth[fo], &a.conf[fo]);
}

int launch_refine(dfe_ctx *ctx, const RefineArgs &a) {
    const dim3 grid((unsigned)dfe_cdiv(a.Wo, 64), (unsigned)dfe_cdiv(a.Ho, 4));
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    if (a.kh == 7 && a.kw == 7) hipLaunchKernelGGL(flow_refine_subpixel_kernel<7>, grid, dim3(256), 0, ctx->stream, a);
    else if (a.kh == 5 && a.kw == 5) hipLaunchKernelGGL(flow_refine_subpixel_kernel<5>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(flow_refine_subpixel_kernel<0>, grid, dim3(256), 0, ctx->stream, a);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_flow_depth_pair_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                                     float foe_x, float foe_y, double extract_threshold, float *flow, float *scores, float *depth,
                                     float *depth_conf) {
    DFE_ENTER(ctx);
    // (the step checks every argument; after it, the frame holds at least one output pixel)
    int rc = dfe_flow_depth_pair_f32(ctx, I0, I1, C, H, W, k, hWin, wWin, foe_x, foe_y, extract_threshold, flow, scores, depth, depth_conf);
    if (rc) return rc;
    const int Ho = H - k + 1 - hWin + 1, Wo = W - k + 1 - wWin + 1;
    const long long HW = (long long)H * W;
    RefineArgs a{};
    a.I0 = I0; a.I1 = I1; a.C = C; a.H = H; a.W = W; a.kh = k; a.kw = k; a.hWin = hWin; a.wWin = wWin; a.Ho = Ho; a.Wo = Wo;
    a.idx = nullptr; a.fy = flow; a.fx = flow + HW;
    a.pitch = W; a.pad_t = (H - Ho) / 2; a.pad_l = (W - Wo) / 2;   // (the step's centre paste)
    a.depth = depth; a.conf = depth_conf;
    a.mw = foe_x; a.mh = foe_y; a.infty = (float)((double)W / 2);   // (as dfe_pair_border_depth)
    return launch_refine(ctx, a);
}

int dfe_flow_refine_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int kh, int kw, int hWin, int wWin,
                                 const int64_t *idx, float *fy, float *fx, int pitch, int pad_t, int pad_l) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, I0 && I1 && idx && fy && fx, DFE_E_ARG, "dfe_flow_refine_subpixel_f32: NULL tensor");
    DFE_REQUIRE(ctx, C > 0 && kh > 0 && kw > 0 && hWin > 0 && wWin > 0, DFE_E_ARG,
                "dfe_flow_refine_subpixel_f32: C=%d k=%dx%d win=%dx%d must be positive", C, kh, kw, hWin, wWin);
    const int Ho = H - kh + 1 - hWin + 1, Wo = W - kw + 1 - wWin + 1;
    DFE_REQUIRE(ctx, Ho > 0 && Wo > 0, DFE_E_SHAPE, "dfe_flow_refine_subpixel_f32: frame %dx%d too small for kernel %dx%d + window %dx%d", H, W,
                kh, kw, hWin, wWin);
    DFE_REQUIRE(ctx, pad_t >= 0 && pad_l >= 0 && pitch >= pad_l + Wo, DFE_E_SHAPE, "dfe_flow_refine_subpixel_f32: pitch %d, pad %d/%d for %d columns",
                pitch, pad_t, pad_l, Wo);
    RefineArgs a{};
    a.I0 = I0; a.I1 = I1; a.C = C; a.H = H; a.W = W; a.kh = kh; a.kw = kw; a.hWin = hWin; a.wWin = wWin; a.Ho = Ho; a.Wo = Wo;
    a.idx = (const long long *)idx; a.fy = fy; a.fx = fx;
    a.pitch = pitch; a.pad_t = pad_t; a.pad_l = pad_l;
    return launch_refine(ctx, a);
}

}  // extern "C"
