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
// pixels share their flow, which is most of a frame.  The five costs share their reads: per channel, frame 1's k + 2 rows around the
// arg-min cell are read once, k + 2 values each (the x neighbours are the same row shifted by one), and each frame-0 row once, kept in a
// ring of three rows (row t of frame 1 meets frame-0 rows t - 1, t, t + 1 for the y+1 cost, the centre row and the y-1 cost).  That is
// C (kh kw + (kh + 2)(kw + 2)) loads per pixel -- 390 at k = 7, C = 3 -- against 5 C kh kw = 735 for five independent sums.
// The sums run in the reference's (c, i, j) order with separately rounded multiply and add (ssd_cv_ref_kernel), so each cost is the
// bit pattern dfe_ssd_cost_volume_f32's reference kernel gives for that cell.
#include "dfe_internal.h"
#include "subpixel_offset.h"   // the parabola's vertex on one axis (include/dfe.h: this order, IEEE division)

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

// K > 0: a K x K patch, known at compile time: frame-0 rows stay in registers (the ring above) and the row loop unrolls, so that a
// channel's loads are in flight together; K == 0: any patch, each term read where it is used (6 loads per term).
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
    float c0 = 0.f, cxm = 0.f, cxp = 0.f, cym = 0.f, cyp = 0.f;
    for (int c = 0; c < a.C; ++c) {
        const float *A = a.I0 + c * plane + (long long)(y + oy) * a.W + x + ox;   // frame-0 patch, row i at A + i W
        const float *B = a.I1 + c * plane + x + s;                               // frame-1 column of the arg-min cell
        if constexpr (K > 0) {
            constexpr int KW = K;
            float ap[KW], ac[KW], an[KW];   // frame-0 rows t - 1, t, t + 1
#pragma unroll
            for (int j = 0; j < KW; ++j) { ap[j] = 0.f; ac[j] = 0.f; an[j] = 0.f; }
#pragma unroll
            for (int t = -1; t <= K; ++t) {
                // frame-1 row r + t (rows -1 and kh only feed the y-1 / y+1 costs: rm, rp stand in for them at the window's edge),
                // columns s - 1 .. s + KW (the end columns only feed the x costs: sm, sp at the edge)
                const int row = t < 0 ? rm : t >= K ? rp + K - 1 : r + t;
                const float *bp = B + (long long)(y + row) * a.W;
                float b[KW + 2];
                b[0] = bp[sm - s];
#pragma unroll
                for (int j = 0; j < KW; ++j) b[j + 1] = bp[j];
                b[KW + 1] = bp[sp - s + KW - 1];
#pragma unroll
                for (int j = 0; j < KW; ++j) { ap[j] = ac[j]; ac[j] = an[j]; }
                if (t + 1 < K) {
#pragma unroll
                    for (int j = 0; j < KW; ++j) an[j] = A[(long long)(t + 1) * a.W + j];
                }
                // ap / ac / an now hold frame-0 rows t - 1, t, t + 1
                if (t >= 0 && t < K) {
#pragma unroll
                    for (int j = 0; j < KW; ++j) {
                        float d = ac[j] - b[j + 1]; float d2 = d * d; c0 = c0 + d2;
                        d = ac[j] - b[j]; d2 = d * d; cxm = cxm + d2;
                        d = ac[j] - b[j + 2]; d2 = d * d; cxp = cxp + d2;
                    }
                }
                if (t + 1 < K) {   // row t of frame 1 against frame-0 row t + 1: the cell one row up
#pragma unroll
                    for (int j = 0; j < KW; ++j) { const float d = an[j] - b[j + 1]; const float d2 = d * d; cym = cym + d2; }
                }
                if (t >= 1) {         // against frame-0 row t - 1: the cell one row down
#pragma unroll
                    for (int j = 0; j < KW; ++j) { const float d = ap[j] - b[j + 1]; const float d2 = d * d; cyp = cyp + d2; }
                }
            }
        } else {
            for (int i = 0; i < a.kh; ++i) {
                const float *ar = A + (long long)i * a.W;
                const float *b0 = B + (long long)(y + r + i) * a.W, *bm = B + (long long)(y + rm + i) * a.W, *bq = B + (long long)(y + rp + i) * a.W;
                for (int j = 0; j < a.kw; ++j) {
                    const float v = ar[j];
                    float d = v - b0[j]; float d2 = d * d; c0 = c0 + d2;
                    d = v - b0[j + sm - s]; d2 = d * d; cxm = cxm + d2;
                    d = v - b0[j + sp - s]; d2 = d * d; cxp = cxp + d2;
                    d = v - bm[j]; d2 = d * d; cym = cym + d2;
                    d = v - bq[j]; d2 = d * d; cyp = cyp + d2;
                }
            }
        }
    }
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
