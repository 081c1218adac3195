// flow_step.hip -- the host pipeline of the single-scale flow step: from a frame pair to flow (and depth) through the kernels of
// ssd_cost_volume.hip (volume builds, the volume-free sweep), ssd_flow_i8.hip (the int8 sweep) and postops.hip (finalize, tail, border +
// depth).  Host code only: no kernel lives here, so a change to the pipeline leaves every kernel's translation unit as it was.
#include "dfe_internal.h"
#include "cv_records.h"
#include <cmath>
#include <limits>
#include <memory>

// the largest float <= t (NaN stays NaN): for every float v, v > float_at_or_below(t) <=> (double)v > t -- a hit strictly above a float
// f <= t is at least the next float, which lies above t -- so the kernel compares in fp32 exactly as the finalize does in fp64
static float float_at_or_below(double t) {
    if (std::isnan(t)) return std::numeric_limits<float>::quiet_NaN();
    if (t >= (double)std::numeric_limits<float>::max()) return std::isinf(t) ? std::numeric_limits<float>::infinity() : std::numeric_limits<float>::max();
    if (t < -(double)std::numeric_limits<float>::max()) return -std::numeric_limits<float>::infinity();
    float f = (float)t;
    if ((double)f > t) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
    return f;
}

// Which route a step takes, asked by every caller of the same two functions.
// flow_step_novol_ok: the volume-free sweep takes the step (3 channels, k = 7, a window that leaves records, fp32 volume semantics, no
// forced static tiles; the finalize's 32-bit pixel arithmetic).
static bool flow_step_novol_ok(const dfe_ctx *ctx, int C, int H, int W, int kh, int kw, int hWin, int wWin, float f16_scale, const DfePairDepth *pd) {
    const int Ho = H - kh + 1 - hWin + 1, Wo = W - kw + 1 - wWin + 1;
    if (!(kh == kw && kh == 7 && cv_writes_records(C, hWin, wWin) && f16_scale == 0.f)) return false;
    if (!(ctx->opt_bool(DFE_OPT_CV_NOVOL, true) && (ctx->cv_mode == 0 || ctx->cv_mode == 3) && (ctx->cv_tyq == 0 || ctx->cv_tyq == 1))) return false;   // (forced static tiles: the volume path)
    return Wo >= 8 && (long long)Ho * Wo < (1ll << 31) && !(pd && (long long)pd->H * pd->W >= (1ll << 31));
}
// flow_step_i8_ok: ... and it may take int8 (option "cv_i8", the 33 x 33 window, the int8 kernel's and the gated sweep's plans); *ib: the sizes
static bool flow_step_i8_ok(const dfe_ctx *ctx, int C, int H, int W, int kh, int kw, int hWin, int wWin, float f16_scale, const DfePairDepth *pd,
                            DfeFlowI8Bufs *ib) {
    return flow_step_novol_ok(ctx, C, H, W, kh, kw, hWin, wWin, f16_scale, pd) && hWin == 33 && wWin == 33 && ctx->opt_bool(DFE_OPT_CV_I8, true) &&
           dfe_flow_i8_plan(H, W, ib) != 0 && cv_flow_sweep_gated_ok(ctx, H, W);
}

// The flow step without its cost volume (option "cv_novol", default on; the caller has asked flow_step_novol_ok): the volume-free fused
// sweep leaves records and, for the rare
// pixels whose lead cells hold fewer than M hits, the fallback plane; one launch for the whole pair (no bands: 112 B of scratch per
// pixel instead of 4356), then the record finalize.
// Option "cv_i8" (default on): the frames are packed to bytes and checked on the device; the int8 matrix-core kernel (ssd_flow_i8.hip)
// writes the results of its pixels itself if every value is an integer in 0..255; the launch behind it writes the frame's border and, if
// not, runs the float sweep and finalizes its records -- three launches, and no host round trip decides.
static int flow_pipeline_novol(dfe_ctx *ctx, const float *I0, const float *I1, int H, int W, int hWin, int wWin, double thr, const TailOut &out,
                               const DfePairDepth *pd, bool *pd_done, bool *done) {
    constexpr int K = 7;
    *done = false;
    ctx->i8_last = false;
    const int Ho = H - K + 1 - hWin + 1, Wo = W - K + 1 - wWin + 1;
    const long long P = (long long)Ho * Wo;
    const size_t nrec = (size_t)dfe_cdiv(Wo, 8) * Ho;   // tile-row records
    DfeFlowI8Bufs ib{};
    const bool i8 = flow_step_i8_ok(ctx, 3, H, W, K, K, hWin, wWin, 0.f, pd, &ib);
    int rc = i8 ? dfe_flow_i8_turn(ctx, &ib) : DFE_OK;
    if (rc) return rc;
    CvFuseArgs fa{};
    CvNovolArgs nv;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        fa.rec = c.take<float>(nrec * DFE_REC);       // [tile column][output row][DFE_REC]
        nv.fb = c.take<float>(nrec * 8 * DFE_FB);     // [tile column][output row][8][DFE_FB]
        if (i8) ib.take(c);
    });
    if (rc) return rc;
    fa.rec_rows = Ho;
    fa.row_off = 0;
    fa.Ptot = P;
    nv.thr = float_at_or_below(thr);
    nv.M = thr < 0.2 ? 8 : 4;   // extract_output.cpp:83-85
    {
        DfeStageScope match(ctx, DFE_STAGE_MATCH);
        if (i8) {
            rc = dfe_flow_i8_launch(ctx, I0, I1, H, W, ib, nv, out, pd);
            if (rc) return rc;
        } else {
            bool handled = false;
            rc = cv_flow_sweep(ctx, I0, I1, H, W, fa, nv, &handled);
            if (rc || !handled) return rc;
        }
    }
    *done = true;
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    // behind the int8 kernel, whose waves finish their own pixels: ONE launch, the frame's border and -- only if the frames were not
    // byte-valued -- the float sweep with the finalize of its records.  (The stage timers then count that sweep under `extract`:
    // include/dfe.h.)
    rc = i8 ? cv_flow_sweep_gated(ctx, I0, I1, H, W, fa, nv, ib.verdict, thr, out, pd) : dfe_flow_finalize(ctx, fa, true, 1, nullptr, &nv, thr, Ho, hWin, wWin, out, pd);
    if (pd && pd_done) *pd_done = true;
    return rc;
}

// One pair through build + flow extraction.  Preferred: the fused build (per-chunk minimum + first index, the centre
// cell and the pixel's first 16 cells leave the kernel with the volume, ~210 compact bytes per pixel) + a finalize that
// reads only those; it goes back to the volume only for pixels whose first 16 cells hold fewer than M values above
// the extractOutput threshold.
// Fallback (shapes without a fused instantiation): build, then the full pass dfe_flow_tail.
// out: where the results go (dfe_tailout, Wo = this pair's); each band gets its row_off / p_off here.
static int flow_pipeline(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int kh, int kw, int hWin, int wWin,
                         double thr, const TailOut &out, const DfePairDepth *pd = nullptr, bool *pd_done = nullptr, float f16_scale = 0.f) {
    // f16_scale != 0: the volume is materialised as fp16 (cost * f16_scale); arg-min, centre and lead cells still come from
    // the fp32 sums in the kernel, so indices and minima are those of the fp32 path.  No extractOutput scores then (its
    // rare fall-back reads the volume).
    // per-pixel records of the role-split row-image kernels (one whole 128-B line per pixel instead of entries in the three planes)
    const bool want_rec = kh == kw && kh == 7 && cv_writes_records(C, hWin, wWin);
    ctx->i8_last = false;   // (dfe_flow_last_path speaks of THIS step)
    if (flow_step_novol_ok(ctx, C, H, W, kh, kw, hWin, wWin, f16_scale, pd)) {
        bool done = false;
        int rc = flow_pipeline_novol(ctx, I0, I1, H, W, hWin, wWin, thr, out, pd, pd_done, &done);
        if (rc || done) return rc;
    }
    const int Ho = H - kh + 1 - hWin + 1, Wo = W - kw + 1 - wWin + 1;
    const int D = hWin * wWin, nch = (D + 63) / 64;
    const long long P = (long long)Ho * Wo;
    const int elem = f16_scale != 0.f ? 2 : 4;
    const int band = band_rows(ctx, Ho, Wo, D, elem);
    float *vol;
    CvFuseArgs fa{};
    int rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        vol = (float *)c.take<char>((size_t)band * Wo * D * elem);
        fa.part = c.take<float2>((size_t)nch * P);
        fa.centre = c.take<float>((size_t)P);
        fa.lead = c.take<float>((size_t)P * DFE_LEAD);
        fa.rec = c.take<float>(want_rec ? (size_t)dfe_cdiv(Wo, 8) * Ho * DFE_REC : 0);   // [tile column][output row][DFE_REC]
    });
    if (rc) return rc;
    fa.rec_rows = Ho;
    fa.Ptot = P;
    {
        const int middle = dfe_window_middle(hWin, wWin);
        fa.cmid = (middle - 1) >> 6; fa.lmid = (middle - 1) & 63;
    }
    const int nb = band_count(Ho, band);
    TailOut o = out;
    for (int bi = 0; bi < nb; ++bi) {
        const int r0 = (int)((long long)bi * Ho / nb), nr = (int)((long long)(bi + 1) * Ho / nb) - r0;   // (nr <= band)
        const int Hb = nr + kh - 1 + hWin - 1;
        o.row_off = r0;
        o.p_off = (long long)r0 * Wo;
        const float *b0 = I0 + (long long)r0 * W, *b1 = I1 + (long long)r0 * W;
        bool fused = false, recs = false;
        int nparts = nch;
        std::unique_ptr<DfeStageScope> match_scope(new DfeStageScope(ctx, DFE_STAGE_MATCH));   // (closed in front of the finalize / tail pass below)
        if (kh == kw && f16_scale != 0.f) {
            fa.row_off = r0;
            rc = cv_frames_dispatch_f16(ctx, b0, b1, C, Hb, W, (long long)H * W, kh, hWin, wWin, f16_scale, vol, &fa, &fused, &recs);
            if (rc) return rc;
            nparts = 2;
            if (!fused) return dfe_fail(ctx, DFE_E_UNSUPPORTED, "no fused fp16 cost-volume kernel for C=%d k=%d win=%dx%d out=%dx%d (band of %d rows)", C, kh, hWin, wWin, Ho, Wo, nr);
        } else if (kh == kw) {
            fa.row_off = r0;
            rc = cv_frames_dispatch_fused(ctx, b0, b1, C, Hb, W, (long long)H * W, kh, hWin, wWin, vol, fa, &fused, &nparts, &recs);
            if (rc) return rc;
        }
        if (fused) {
            match_scope.reset();
            DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
            // one band: the finalize launch also zeroes the frame border and makes depth (pair step: 2 launches instead of 3)
            const bool frame_mode = pd && nr == Ho;
            rc = dfe_flow_finalize(ctx, fa, recs, nparts, vol, nullptr, thr, nr, hWin, wWin, o, frame_mode ? pd : nullptr);
            if (frame_mode && pd_done) *pd_done = true;
        } else {
            rc = cv_frames_dispatch(ctx, b0, b1, C, Hb, W, (long long)H * W, kh, kw, hWin, wWin, vol);
            if (rc) return rc;
            match_scope.reset();
            DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
            rc = dfe_flow_tail_run(ctx, vol, nr, hWin, wWin, thr, o);
        }
        if (rc) return rc;
    }
    return DFE_OK;
}

// The body of the pair entries dfe_flow_depth_pair_f32 / _f16 (fn: the entry's name in the error texts).  f16: the volume is fp16
// (cost * scale), idx / best are [Ho][Wo] like dfe_ssd_flow_f32's and there are no scores; else scores, and thr is extractOutput's.
// flow is the centre-pasted [2][H][W] in both
static int flow_depth_pair(dfe_ctx *ctx, const char *fn, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                           float foe_y, double thr, bool f16, float scale, int64_t *idx, float *best, float *flow, float *scores, float *depth,
                           float *depth_conf) {
    DFE_REQUIRE(ctx, I0 && I1 && flow, DFE_E_ARG, "%s: NULL tensor", fn);
    if (f16) {
        DFE_REQUIRE(ctx, C > 0 && k > 0 && hWin > 0 && wWin > 0 && scale > 0, DFE_E_ARG, "%s: C=%d k=%d win=%dx%d scale=%g", fn, C, k, hWin, wWin, (double)scale);
    } else {
        DFE_REQUIRE(ctx, C > 0 && k > 0 && hWin > 0 && wWin > 0, DFE_E_ARG, "%s: C=%d k=%d win=%dx%d", fn, C, k, hWin, wWin);
    }
    DFE_REQUIRE(ctx, (depth == nullptr) == (depth_conf == nullptr), DFE_E_ARG, "%s: depth and depth_conf go together", fn);
    const int Ho = H - k + 1 - hWin + 1, Wo = W - k + 1 - wWin + 1;
    DFE_REQUIRE(ctx, Ho > 0 && Wo > 0, DFE_E_SHAPE, "%s: frame %dx%d too small for kernel %d + window %dx%d", fn, H, W, k, hWin, wWin);
    const long long HW = (long long)H * W;
    // centre-paste offsets: opticalflow_model.lua:228-230 floor((hImg-h)/2)
    //   == radial/radial_opticalflow_groundtruth.lua:27-32 floor((hWin-1)/2)+floor((k-1)/2)
    const int pad_t = (H - Ho) / 2, pad_l = (W - Wo) / 2;
    // the pipeline writes every interior pixel of flow / scores; one pass afterwards zeroes the border and makes depth
    const DfePairDepth pd{H, W, foe_x, foe_y, depth, depth_conf};
    bool pd_done = false;
    int rc = flow_pipeline(ctx, I0, I1, C, H, W, k, k, hWin, wWin, thr,
                           dfe_tailout(idx, best, flow, flow + HW, scores, nullptr, Wo, /*pitch*/ W, pad_t, pad_l, /*scores_padded*/ 1), &pd, &pd_done,
                           f16 ? scale : 0.f);
    if (rc || pd_done) return rc;
    // several bands, or no fused build for this shape: one pass afterwards zeroes the border and makes depth
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    return dfe_pair_border_depth(ctx, flow, scores, H, W, pad_t, pad_l, Ho, Wo, foe_x, foe_y, depth, depth_conf);
}

extern "C" {
int dfe_ssd_flow_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int kh, int kw, int hWin,
                     int wWin, double extract_threshold, int64_t *idx, float *best, float *flow_y, float *flow_x,
                     float *scores, int64_t *imaxs) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, I0 && I1, DFE_E_ARG, "dfe_ssd_flow_f32: NULL frame");
    DFE_REQUIRE(ctx, C > 0 && kh > 0 && kw > 0 && hWin > 0 && wWin > 0, DFE_E_ARG,
                "dfe_ssd_flow_f32: C=%d k=%dx%d win=%dx%d must be positive", C, kh, kw, hWin, wWin);
    const int Ho = H - kh + 1 - hWin + 1, Wo = W - kw + 1 - wWin + 1;
    DFE_REQUIRE(ctx, Ho > 0 && Wo > 0, DFE_E_SHAPE, "dfe_ssd_flow_f32: frame %dx%d too small for kernel %dx%d + window %dx%d",
                H, W, kh, kw, hWin, wWin);
    DFE_REQUIRE(ctx, (scores == nullptr) == (imaxs == nullptr), DFE_E_ARG, "dfe_ssd_flow_f32: scores and imaxs go together");
    return flow_pipeline(ctx, I0, I1, C, H, W, kh, kw, hWin, wWin, extract_threshold,
                         dfe_tailout(idx, best, flow_y, flow_x, scores, imaxs, Wo, /*pitch*/ Wo, /*pad_t*/ 0, /*pad_l*/ 0, /*scores_padded*/ 0));
}

int dfe_flow_depth_pair_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                            float foe_x, float foe_y, double extract_threshold, float *flow, float *scores, float *depth,
                            float *depth_conf) {
    DFE_ENTER(ctx);
    return flow_depth_pair(ctx, "dfe_flow_depth_pair_f32", I0, I1, C, H, W, k, hWin, wWin, foe_x, foe_y, extract_threshold, false, 0.f, nullptr, nullptr,
                           flow, scores, depth, depth_conf);
}

}  // extern "C"

// The byte entries at scale 1 (ingest.hip): pack-from-bytes, which also writes the frame's border, and the int8 sweep -- no float copy of
// the frames, no gated launch, nothing to extract.  Whatever flow_depth_pair would refuse, and every step that may not take int8, is
// left to the caller's float route (*done = false, nothing launched).
int dfe_flow_depth_pair_bytes(dfe_ctx *ctx, const unsigned char *I0, const unsigned char *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                              float foe_y, double extract_threshold, float scale, float *flow, float *scores, float *depth, float *depth_conf, bool *done) {
    *done = false;
    if (scale != 1.0f || !I0 || !I1 || !flow || C <= 0 || k <= 0 || hWin <= 0 || wWin <= 0 || (depth == nullptr) != (depth_conf == nullptr)) return DFE_OK;
    const int Ho = H - k + 1 - hWin + 1, Wo = W - k + 1 - wWin + 1;
    if (Ho <= 0 || Wo <= 0) return DFE_OK;
    const DfePairDepth pd{H, W, foe_x, foe_y, depth, depth_conf};
    DfeFlowI8Bufs ib{};
    if (!flow_step_i8_ok(ctx, C, H, W, k, k, hWin, wWin, 0.f, &pd, &ib)) return DFE_OK;
    ctx->i8_last = false;
    int rc = dfe_flow_i8_turn(ctx, &ib);
    if (rc) return rc;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) { ib.take(c); });
    if (rc) return rc;
    CvNovolArgs nv{};
    nv.thr = float_at_or_below(extract_threshold);
    nv.M = extract_threshold < 0.2 ? 8 : 4;   // extract_output.cpp:83-85
    const int pad_t = (H - Ho) / 2, pad_l = (W - Wo) / 2;
    const long long HW = (long long)H * W;
    DfeStageScope match(ctx, DFE_STAGE_MATCH);
    rc = dfe_flow_i8_launch_bytes(ctx, I0, I1, H, W, ib, nv, dfe_tailout(nullptr, nullptr, flow, flow + HW, scores, nullptr, Wo, /*pitch*/ W, pad_t, pad_l, /*scores_padded*/ 1), &pd);
    *done = rc == DFE_OK;
    return rc;
}

extern "C" {
int dfe_flow_depth_pair_f16(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                            float foe_y, float scale, int64_t *idx, float *best, float *flow, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    return flow_depth_pair(ctx, "dfe_flow_depth_pair_f16", I0, I1, C, H, W, k, hWin, wWin, foe_x, foe_y, 0.0, true, scale, idx, best, flow, nullptr, depth,
                           depth_conf);
}
}  // extern "C"
