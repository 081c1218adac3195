// consistency.hip -- forward-backward consistency of two flow fields, and the pair step in both directions (not in the reference; DESIGN
// section 4.25).
//   dfe_flow_consistency_f32      mask / residual of any two flow fields [2][H][W] over a region R (the definition: include/dfe.h)
//   dfe_flow_depth_pair_fb_f32    dfe_flow_depth_pair_f32 (or its _subpixel_ form), the backward flow, and their consistency in one call
//   (dfe_flow_depth_pair_fb_u8 stands in ingest.hip, next to the conversion it shares between the two directions)
//
// Layout: no LDS.  One thread per pixel of the FRAME, a wave = 64 consecutive pixels of one row, so the reads of fw and the stores of
// mask / err (and the in-place gate of scores / depth_conf) are whole 256-B runs; the zero border is written by the same launch.  The
// (up to) four taps of bw are gathered through L1 / L2: displacements are bounded by the search window, so a wave's taps lie in a few
// rows around its own.
#include "dfe_field.h"

namespace {

struct ConsistencyArgs {
    const float *fw, *bw;          // [2][H][W], plane 0 = y, plane 1 = x
    int H, W, y0, x0, Ho, Wo;      // R = rows y0 .. y0+Ho-1, columns x0 .. x0+Wo-1, inside the frame
    float tol2;                    // tol * tol (fp32)
    float *mask, *err;             // [H][W]; err may be null
    float *scores, *conf;          // [H][W] or null: multiplied in place by the mask inside R (the gate of the one-call)
};

__global__ __launch_bounds__(256) void flow_consistency_kernel(ConsistencyArgs a) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const long long HW = (long long)a.H * a.W, p = (long long)y * a.W + x;
    float m = 0.f, e = 0.f;
    const bool inR = y >= a.y0 && y < a.y0 + a.Ho && x >= a.x0 && x < a.x0 + a.Wo;
    if (inR) {
        const float fy = a.fw[p], fx = a.fw[HW + p];
        e = __builtin_inff();
        if (dfe_finite(fy) && dfe_finite(fx)) {
            const float qy = (float)y + fy, qx = (float)x + fx;
            const float fly = floorf(qy), cly = ceilf(qy), flx = floorf(qx), clx = ceilf(qx);
            // reach, decided on the floats: only coordinates inside R (inside the frame) are converted to int
            if (fly >= (float)a.y0 && cly <= (float)(a.y0 + a.Ho - 1) && flx >= (float)a.x0 && clx <= (float)(a.x0 + a.Wo - 1)) {
                const float wy = qy - fly, wx = qx - flx, uy = 1.f - wy, ux = 1.f - wx;
                const long long r0 = (long long)(int)fly * a.W, r1 = (long long)(int)cly * a.W;
                const int c0 = (int)flx, c1 = (int)clx;
                float by = 0.f, bx = 0.f;
                // a tap with a zero factor is not read (an integral q reads one pixel; a NaN beside it stays out of the sum)
                if (uy != 0.f && ux != 0.f) { const float w = uy * ux; by += w * a.bw[r0 + c0]; bx += w * a.bw[HW + r0 + c0]; }
                if (uy != 0.f && wx != 0.f) { const float w = uy * wx; by += w * a.bw[r0 + c1]; bx += w * a.bw[HW + r0 + c1]; }
                if (wy != 0.f && ux != 0.f) { const float w = wy * ux; by += w * a.bw[r1 + c0]; bx += w * a.bw[HW + r1 + c0]; }
                if (wy != 0.f && wx != 0.f) { const float w = wy * wx; by += w * a.bw[r1 + c1]; bx += w * a.bw[HW + r1 + c1]; }
                if (dfe_finite(by) && dfe_finite(bx)) {
                    const float ey = fy + by, ex = fx + bx;
                    const float d2 = ey * ey + ex * ex;
                    e = sqrtf(d2);
                    m = d2 <= a.tol2 ? 1.f : 0.f;
                }
            }
        }
        if (a.scores) a.scores[p] = a.scores[p] * m;
        if (a.conf) a.conf[p] = a.conf[p] * m;
    }
    a.mask[p] = m;
    if (a.err) a.err[p] = e;
}

int launch_consistency(dfe_ctx *ctx, const float *fw, const float *bw, int H, int W, int y0, int x0, int Ho, int Wo, float tol, float *mask, float *err,
                       float *scores, float *conf) {
    ConsistencyArgs a{};
    a.fw = fw; a.bw = bw; a.H = H; a.W = W; a.y0 = y0; a.x0 = x0; a.Ho = Ho; a.Wo = Wo;
    a.tol2 = tol * tol;
    a.mask = mask; a.err = err; a.scores = scores; a.conf = conf;
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    hipLaunchKernelGGL(flow_consistency_kernel, dim3((unsigned)dfe_cdiv(W, 64), (unsigned)dfe_cdiv(H, 4)), dim3(256), 0, ctx->stream, a);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

}  // namespace

int dfe_flow_pair_fb_run(dfe_ctx *ctx, const char *fn, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                         float foe_y, double extract_threshold, int subpixel, float tol, int gate, float *flow, float *scores, float *depth,
                         float *depth_conf, float *flow_bw, float *mask, float *err) {
    DFE_REQUIRE(ctx, mask, DFE_E_ARG, "%s: mask is NULL", fn);
    DFE_REQUIRE(ctx, tol >= 0.f, DFE_E_ARG, "%s: tol=%g must be >= 0", fn, (double)tol);
    // forward: the step as it is (it checks every other argument in front of its first launch)
    auto step = subpixel ? dfe_flow_depth_pair_subpixel_f32 : dfe_flow_depth_pair_f32;
    int rc = step(ctx, I0, I1, C, H, W, k, hWin, wWin, foe_x, foe_y, extract_threshold, flow, scores, depth, depth_conf);
    if (rc) return rc;
    if (!flow_bw) {   // the ctx's side buffer, not the arena: the backward step carves the arena anew
        void *aux = nullptr;
        rc = dfe_aux_scratch(ctx, DfeCarve::up((size_t)2 * H * W * sizeof(float)), &aux);
        if (rc) return rc;
        DfeCarve c(aux);
        flow_bw = c.take<float>((size_t)2 * H * W);
    }
    // backward: the frames swapped, the two flow planes only -- the finalize skips extractOutput and depth where they are not asked for and
    // still zeroes the border; the refinement likewise makes no depth
    rc = step(ctx, I1, I0, C, H, W, k, hWin, wWin, foe_x, foe_y, extract_threshold, flow_bw, nullptr, nullptr, nullptr);
    if (rc) return rc;
    const int Ho = H - k + 1 - hWin + 1, Wo = W - k + 1 - wWin + 1;
    return launch_consistency(ctx, flow, flow_bw, H, W, (H - Ho) / 2, (W - Wo) / 2, Ho, Wo, tol, mask, err, gate ? scores : nullptr,
                              gate ? depth_conf : nullptr);
}

extern "C" {

int dfe_flow_consistency_f32(dfe_ctx *ctx, const float *fw, const float *bw, int H, int W, int y0, int x0, int Ho, int Wo, float tol, float *mask,
                             float *err) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, fw && bw && mask, DFE_E_ARG, "dfe_flow_consistency_f32: NULL tensor");
    DFE_REQUIRE(ctx, tol >= 0.f, DFE_E_ARG, "dfe_flow_consistency_f32: tol=%g must be >= 0", (double)tol);   // (false for NaN)
    if (int rc = dfe_region_check(ctx, "dfe_flow_consistency_f32", H, W, y0, x0, Ho, Wo)) return rc;
    return launch_consistency(ctx, fw, bw, H, W, y0, x0, Ho, Wo, tol, mask, err, nullptr, nullptr);
}

int dfe_flow_depth_pair_fb_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                               float foe_y, double extract_threshold, int subpixel, float tol, int gate, float *flow, float *scores, float *depth,
                               float *depth_conf, float *flow_bw, float *mask, float *err) {
    DFE_ENTER(ctx);
    return dfe_flow_pair_fb_run(ctx, "dfe_flow_depth_pair_fb_f32", I0, I1, C, H, W, k, hWin, wWin, foe_x, foe_y, extract_threshold, subpixel, tol, gate,
                                flow, scores, depth, depth_conf, flow_bw, mask, err);
}

}  // extern "C"
