// single_scale.hip -- the single-scale trained model as ONE call: what depth_estimation_opticalflow.lua:66-116 runs per frame pair for a
// model that is not multiscale --
//   filter:forward(frame) of both frames                      getFilter, opticalflow_model.lua:45-79 (conv [tanh] conv ...)
//   prepareInput(geometry, last_im, im)                       :131-151: patch 1 narrowed by the search window (rows ceil(maxh/2).., H - maxh + 1 of them)
//   model:forward(input), getModel(geometry, true, true)      :81-129: SpatialMatching(maxh, maxw) -> Minus -> SoftMax over the window
//   processOutput(geometry, moutput, true [, threshold])      :201-252: arg-max with the centre tie-break (or extractOutput(p, 0.11) and
//                                                             scores > threshold), x2yx minus centered2onebased(0, 0), centre paste into
//                                                             full [2][hImg][wImg] and full_confidences [hImg][wImg]
// Module by module (network.py getModel + opticalflow_model.py processOutput) the matcher writes the H1 x W1 x maxh x maxw volume (291 MB
// for a VGA pair at 16 x 16), Minus and the soft-max re-stream it and processOutput streams it once more.  Here the window never leaves
// the CU: the flat-tile matcher's soft-max epilogue (feat_matching_flat.hip, FF_SOFT) does the per-pixel tail on the costs it has just
// summed.  Shapes that kernel does not take go through the stand-alone device ops in the same order (the same arithmetic: every soft-max
// on the device is softmin_body's), so the results are the module path's bit for bit either way.
// dfe_flow_pair_filtered_mean_f32 is the same step for a model built with output_extraction_method 'mean': processOutput's 'mean' branch
// (:171-199, 218-226: soft arg-max y, x, confidence from extractOutput on the row marginals) behind the soft-max, in the matcher's FF_MEAN
// epilogue or through the stand-alone ops.
#include "dfe_internal.h"

namespace {

// out [C][Hc][Wc] = in [C][H][W] rows y0.., columns x0..
__global__ __launch_bounds__(256) void ss_crop_kernel(const float *__restrict__ in, long long plane, int W, int y0, int x0, int Hc, int Wc, long long total,
                                                      float *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long row = e / Wc;
        const int x = (int)(e - row * Wc);
        const long long c = row / Hc;
        const int y = (int)(row - c * Hc);
        out[e] = in[c * plane + (long long)(y0 + y) * W + x0 + x];
    }
}

// the index's decode and the centre paste of processOutput (opticalflow_model.lua:207-250) for the path that went through the volume
__global__ __launch_bounds__(256) void ss_paste_kernel(const long long *__restrict__ idx, const float *__restrict__ scores, int H1, int W1, int maxh, int maxw,
                                                       int use_thr, float thr, int ho, int wo, int wFull, long long fullplane, float *__restrict__ full,
                                                       float *__restrict__ full_conf) {
    const long long P = (long long)H1 * W1;
    const int yoff = (maxh + 1) / 2, xoff = (maxw + 1) / 2;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(p / W1), x = (int)(p - (long long)y * W1);
        const int i0 = (int)idx[p] - 1, ty = i0 / maxw;
        const long long fo = (long long)(ho + y) * wFull + wo + x;
        if (full) {
            full[fo] = (float)(ty + 1 - yoff);
            full[fullplane + fo] = (float)(i0 - ty * maxw + 1 - xoff);
        }
        if (full_conf) full_conf[fo] = use_thr ? (scores[p] > thr ? 1.f : 0.f) : 1.f;
    }
}

// processOutput's 'mean' branch (opticalflow_model.lua:218-250) behind the stand-alone OutputExtractor / marginal / extractOutput ops:
// index = yx2x(floor(y + 0.5), floor(x + 0.5)) in fp32, y and x minus centered2onebased(0, 0), confidence = scores > 0, centre paste
__global__ __launch_bounds__(256) void ss_paste_mean_kernel(const float *__restrict__ y, const float *__restrict__ x, const float *__restrict__ scores, int H1,
                                                            int W1, int maxh, int maxw, int ho, int wo, int wFull, long long fullplane, float *__restrict__ full,
                                                            float *__restrict__ full_conf, long long *__restrict__ idx) {
#pragma clang fp contract(off)
    const long long P = (long long)H1 * W1;
    const float yoff = (float)((maxh + 1) / 2), xoff = (float)((maxw + 1) / 2);
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        const int py = (int)(p / W1), px = (int)(p - (long long)py * W1);
        const float yv = y[p], xv = x[p];
        if (idx) idx[p] = (long long)((floorf(yv + 0.5f) - 1.f) * (float)maxw + floorf(xv + 0.5f));
        const long long fo = (long long)(ho + py) * wFull + wo + px;
        if (full) {
            full[fo] = yv - yoff;
            full[fullplane + fo] = xv - xoff;
        }
        if (full_conf) full_conf[fo] = scores[p] > 0.f ? 1.f : 0.f;
    }
}

// torch.Tensor(2, hImg, wImg):zero() / full_confidences:zero() (opticalflow_model.lua:236,243) where the paste does not write: the frame
// around the pasted region (two hipMemsetAsync of the whole planes cost 10 us of a 200-us step)
__global__ __launch_bounds__(256) void ss_border_kernel(float *__restrict__ full, float *__restrict__ full_conf, int hImg, int wImg, int ho, int wo, int H1, int W1) {
    const long long P = (long long)hImg * wImg;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(p / wImg), x = (int)(p - (long long)y * wImg);
        if (y >= ho && y < ho + H1 && x >= wo && x < wo + W1) continue;
        if (full) { full[p] = 0.f; full[P + p] = 0.f; }
        if (full_conf) full_conf[p] = 0.f;
    }
}

// imaxs = middle, scores = 0 where extractOutput will write nothing (the reference passes uninitialised tensors: SURVEY appendix A)
__global__ __launch_bounds__(256) void ss_fill_kernel(long long *__restrict__ idx, float *__restrict__ scores, long long P, long long middle) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        idx[p] = middle;
        scores[p] = 0.f;
    }
}

}  // namespace

// dfe_flow_pair_filtered_f32 (mean = false) and dfe_flow_pair_filtered_mean_f32 (mean = true: processOutput's 'mean' branch, no threshold,
// no scores); fn: the entry's name for the messages
static int ss_flow_pair(dfe_ctx *ctx, const char *fn, bool mean, const float *I0, const float *I1, int C, int H, int W, const dfe_filter_layer *layers,
                        int nlayers, int maxh, int maxw, int use_threshold, double threshold, int hImg, int wImg, float *full, float *full_conf,
                        int64_t *index, float *scores) {
    DFE_REQUIRE(ctx, I0 && I1 && (nlayers == 0 || layers), DFE_E_ARG, "%s: NULL argument", fn);
    DFE_REQUIRE(ctx, full || full_conf || index || scores, DFE_E_ARG, "%s: no output requested", fn);
    DFE_REQUIRE(ctx, C > 0 && H > 0 && W > 0 && nlayers >= 0 && nlayers <= 8 && maxh > 0 && maxw > 0, DFE_E_ARG,
                "%s: C=%d %dx%d, %d layers, window %dx%d", fn, C, H, W, nlayers, maxh, maxw);
    DfeStackGeom sg;
    int rc = dfe_filter_stack_geom(ctx, fn, layers, nlayers, C, &sg);
    if (rc) return rc;
    const int hk = sg.hk, wk = sg.wk, K = sg.K, maxplanes = sg.maxplanes;
    const int Hf = H - hk + 1, Wf = W - wk + 1;                     // the feature maps (in2 of the matcher)
    const int H1 = Hf - maxh + 1, W1 = Wf - maxw + 1;               // the model's output region = the narrowed in1
    DFE_REQUIRE(ctx, H1 > 0 && W1 > 0, DFE_E_SHAPE, "%s: frame %dx%d too small for window %dx%d behind a %dx%d filter", fn, H, W, maxh, maxw, hk, wk);
    DFE_REQUIRE(ctx, !(full || full_conf) || (hImg >= H1 && wImg >= W1), DFE_E_SHAPE, "%s: full frame %dx%d smaller than the output %dx%d", fn, hImg, wImg,
                H1, W1);
    const int ny = dfe_window_lead(maxh), nx = dfe_window_lead(maxw);   // prepareInput's narrow: first row / column of patch 1
    const int N = maxh * maxw;
    const long long P1 = (long long)H1 * W1;
    // The job of the matcher with the per-pixel tail in its epilogue.  It reads the narrowed in1 in place when the caller ran the filter
    // (prefilter: a view of frame 0, rows W, planes H W floats apart, with the frames' own alignment), else contiguous maps of the arena to
    // come; fm_select sees exactly what will run, so the volume is planned wherever that kernel is not the pick
    DfeSoftOut so{};
    so.use_threshold = use_threshold ? 1 : 0; so.threshold = (float)threshold;
    so.hFull = hImg; so.wFull = wImg; so.full = full; so.full_conf = full_conf; so.index = (long long *)index; so.scores = scores;
    FmJob job = fm_job(mean ? FM_MEAN : FM_SOFT, nullptr, nullptr, K, H1, W1, maxh, maxw);
    job.soft = &so;
    if (!nlayers) { job.in1 = I0 + (long long)ny * W + nx; job.pitch1 = W; job.plane1 = (long long)H * W; job.in2 = I1; }
    const bool lean = fm_select(dfe_fm_env(ctx), job).kernel != FM_K_NONE;
    // arena: cropped frame 0 | two ping-pong feature buffers per branch | (fallback) contiguous in1 | volume | probabilities | index | scores
    // ('mean' fallback: imaxs | scores | x | y | row marginals in place of index and scores)
    const int Hc = H1 + hk - 1, Wc = W1 + wk - 1;                   // the part of frame 0 the narrowed features come from
    const size_t f_c0 = nlayers ? (size_t)C * Hc * Wc : 0;
    const size_t f_fa = nlayers ? (size_t)maxplanes * Hc * Wc : 0, f_fb = nlayers ? (size_t)maxplanes * H * W : 0;
    const size_t f_in1 = (!lean && !nlayers) ? (size_t)K * P1 : 0;
    const size_t f_vol = lean ? 0 : (size_t)P1 * N;
    const size_t n_idx = (lean || index || mean) ? 0 : (size_t)P1, f_sc = (lean || scores || !use_threshold || mean) ? 0 : (size_t)P1;
    const size_t f_mean = (lean || !mean) ? 0 : (size_t)P1 * (5 + maxh);
    float *c0, *fa[2], *fb[2], *in1c, *vol, *prob, *sc_s, *mean_s;
    long long *idx_s;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        c0 = c.take<float>(f_c0);
        for (float *&f : fa) f = c.take<float>(f_fa);
        for (float *&f : fb) f = c.take<float>(f_fb);
        in1c = c.take<float>(f_in1); vol = c.take<float>(f_vol); prob = c.take<float>(f_vol);
        idx_s = c.take<long long>(n_idx); sc_s = c.take<float>(f_sc); mean_s = c.take<float>(f_mean);
    }, nlayers > 0);
    if (rc) return rc;
    const float *in1 = job.in1, *in2 = job.in2;   // (prefilter: patch 1's narrow is a view of the caller's map, depth_estimation_opticalflow.lua:66-75)
    if (nlayers) {
        DfeStageScope st(ctx, DFE_STAGE_FILTER);
        // the first branch filters only what the narrow keeps: a convolution is 'valid' and shift-invariant, so the features of the cropped
        // frame ARE the narrowed features of the whole frame, bit for bit
        // -- and the first layer reads that part of frame 0 in place (rows W apart, planes H * W apart) where the batched kernel takes the
        // layer; otherwise it is copied out first
        const float *ia = I0 + (long long)ny * W + nx, *ib = I1;
        int ha = Hc, wa = Wc, hb = H, wb = W;
        for (int i = 0; i < nlayers; ++i) {
            const float *in_[2] = {ia, ib};
            const dfe_filter_layer *L2[2] = {&layers[i], &layers[i]};
            const int H2[2] = {ha, hb}, W2[2] = {wa, wb};
            float *o2[2] = {fa[i & 1], fb[i & 1]};
            bool viewed = false;
            if (i == 0) {
                const int pit[2] = {W, W};
                const long long pla[2] = {(long long)H * W, (long long)H * W};
                rc = dfe_filter_layer_forward_batch_view(ctx, 2, in_, L2, H2, W2, pit, pla, o2, &viewed);
                if (rc) return rc;
                if (!viewed) {
                    hipLaunchKernelGGL(ss_crop_kernel, dim3(dfe_grid1d((long long)C * Hc * Wc, 256, 16384)), dim3(256), 0, ctx->stream, I0, (long long)H * W, W, ny, nx, Hc, Wc,
                                       (long long)C * Hc * Wc, c0);
                    DFE_LAUNCH_CHECK(ctx);
                    in_[0] = c0;
                }
            }
            if (!viewed) rc = dfe_filter_layer_forward_batch(ctx, 2, in_, L2, H2, W2, o2);
            if (rc) return rc;
            ia = o2[0]; ib = o2[1];
            ha -= layers[i].kH - 1; wa -= layers[i].kW - 1; hb -= layers[i].kH - 1; wb -= layers[i].kW - 1;
        }
        DFE_REQUIRE(ctx, ha == H1 && wa == W1 && hb == Hf && wb == Wf, DFE_E_SHAPE, "%s: internal shape mismatch", fn);
        in1 = ia; in2 = ib;
    }
    const int ho = (hImg - H1) / 2, wo = (wImg - W1) / 2;
    if ((full || full_conf) && (hImg > H1 || wImg > W1)) {
        hipLaunchKernelGGL(ss_border_kernel, dim3(dfe_grid1d((long long)hImg * wImg, 256, 16384)), dim3(256), 0, ctx->stream, full, full_conf, hImg, wImg, ho, wo, H1, W1);
        DFE_LAUNCH_CHECK(ctx);
    }
    if (lean) {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        job.in1 = in1; job.in2 = in2;
        return dfe_fm_run(ctx, job);
    }
    if (!nlayers) {
        hipLaunchKernelGGL(ss_crop_kernel, dim3(dfe_grid1d((long long)K * P1, 256, 16384)), dim3(256), 0, ctx->stream, I0, (long long)H * W, W, ny, nx, H1, W1, (long long)K * P1, in1c);
        DFE_LAUNCH_CHECK(ctx);
        in1 = in1c;
    }
    {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        rc = dfe_spatial_matching_dispatch(ctx, in1, in2, K, H1, W1, maxh, maxw, vol);
        if (rc) return rc;
        rc = dfe_softmin_f32(ctx, vol, P1, N, prob);                // nn.Minus + the soft-max over the window
        if (rc) return rc;
    }
    DfeStageScope st(ctx, DFE_STAGE_EXTRACT);
    if (mean) {
        // getOutputConfidences2 (opticalflow_model.lua:171-199): OutputExtractor, the row marginals, extractOutput on them into zeroed scores
        long long *im = (long long *)mean_s;
        float *sc = mean_s + 2 * P1, *xs = sc + P1, *ys = xs + P1, *marg = ys + P1;
        rc = dfe_output_extractor_f32(ctx, prob, P1, maxh, maxw, xs, ys);
        if (rc) return rc;
        rc = dfe_marginal_sum_f32(ctx, prob, P1, maxh, maxw, marg);
        if (rc) return rc;
        DFE_HIP(ctx, hipMemsetAsync(mean_s, 0, (size_t)P1 * 3 * sizeof(float), ctx->stream));   // imaxs and scores
        rc = dfe_extract_output(ctx, marg, H1, W1, maxh, sc, 0.11, (int64_t *)im);
        if (rc) return rc;
        hipLaunchKernelGGL(ss_paste_mean_kernel, dim3(dfe_grid1d(P1, 256, 16384)), dim3(256), 0, ctx->stream, ys, xs, sc, H1, W1, maxh, maxw, ho, wo, wImg, (long long)hImg * wImg,
                           full, full_conf, (long long *)index);
        DFE_LAUNCH_CHECK(ctx);
        return DFE_OK;
    }
    long long *idx_d = index ? (long long *)index : idx_s;
    float *sc_d = scores ? scores : sc_s;
    const int middle = dfe_window_middle(maxh, maxw);
    if (!use_threshold) {
        rc = dfe_argbest_center(ctx, prob, P1, N, middle, 1, (int64_t *)idx_d, nullptr);
        if (rc) return rc;
        if (scores) DFE_HIP(ctx, hipMemsetAsync(scores, 0, (size_t)P1 * sizeof(float), ctx->stream));
    } else {
        hipLaunchKernelGGL(ss_fill_kernel, dim3(dfe_grid1d(P1, 256, 16384)), dim3(256), 0, ctx->stream, idx_d, sc_d, P1, (long long)middle);
        DFE_LAUNCH_CHECK(ctx);
        rc = dfe_extract_output(ctx, prob, H1, W1, N, sc_d, 0.11, (int64_t *)idx_d);
        if (rc) return rc;
    }
    if (full || full_conf) {
        hipLaunchKernelGGL(ss_paste_kernel, dim3(dfe_grid1d(P1, 256, 16384)), dim3(256), 0, ctx->stream, idx_d, sc_d, H1, W1, maxh, maxw, use_threshold ? 1 : 0, (float)threshold, ho, wo,
                           wImg, (long long)hImg * wImg, full, full_conf);
        DFE_LAUNCH_CHECK(ctx);
    }
    return DFE_OK;
}

extern "C" int dfe_flow_pair_filtered_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, const dfe_filter_layer *layers, int nlayers,
                                          int maxh, int maxw, int use_threshold, double threshold, int hImg, int wImg, float *full, float *full_conf,
                                          int64_t *index, float *scores) {
    DFE_ENTER(ctx);
    return ss_flow_pair(ctx, "dfe_flow_pair_filtered_f32", false, I0, I1, C, H, W, layers, nlayers, maxh, maxw, use_threshold, threshold, hImg, wImg, full,
                        full_conf, index, scores);
}

extern "C" int dfe_flow_pair_filtered_mean_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, const dfe_filter_layer *layers,
                                               int nlayers, int maxh, int maxw, int hImg, int wImg, float *full, float *full_conf, int64_t *index) {
    DFE_ENTER(ctx);
    return ss_flow_pair(ctx, "dfe_flow_pair_filtered_mean_f32", true, I0, I1, C, H, W, layers, nlayers, maxh, maxw, 0, 0.0, hImg, wImg, full, full_conf, index,
                        nullptr);
}

// nn.SpatialMatching whose first input is a VIEW (rows pitch1 floats apart, planes plane1 floats apart): prepareInput's narrow handed on
// without the contiguous copy
extern "C" int dfe_spatial_matching_strided_f32(dfe_ctx *ctx, const float *in1, int in1_pitch, int64_t in1_plane, const float *in2, int K, int H1, int W1, int maxh,
                                                int maxw, float *out) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, in1 && in2 && out, DFE_E_ARG, "dfe_spatial_matching_strided_f32: NULL tensor");
    DFE_REQUIRE(ctx, K > 0 && H1 > 0 && W1 > 0 && maxh > 0 && maxw > 0, DFE_E_SHAPE, "dfe_spatial_matching_strided_f32: K=%d H1=%d W1=%d maxh=%d maxw=%d must be positive", K, H1,
                W1, maxh, maxw);
    DFE_REQUIRE(ctx, in1_pitch >= W1 && in1_plane >= (int64_t)(H1 - 1) * in1_pitch + W1, DFE_E_SHAPE, "dfe_spatial_matching_strided_f32: pitch %d / plane %lld too small for %dx%d",
                in1_pitch, (long long)in1_plane, H1, W1);
    FmJob job = fm_job(FM_VOLUME, in1, in2, K, H1, W1, maxh, maxw);
    job.pitch1 = in1_pitch; job.plane1 = in1_plane; job.out = out;
    FmPick pk;
    int rc = dfe_fm_run(ctx, job, &pk);
    if (rc || pk.kernel != FM_K_NONE) return rc;
    float *scr = nullptr;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) { scr = c.take<float>((size_t)K * H1 * W1); });
    if (rc) return rc;
    // (a view with rows pitch apart inside planes plane apart: the crop kernel's (plane, W) pair)
    hipLaunchKernelGGL(ss_crop_kernel, dim3(dfe_grid1d((long long)K * H1 * W1, 256, 16384)), dim3(256), 0, ctx->stream, in1, (long long)in1_plane, in1_pitch, 0, 0, H1, W1,
                       (long long)K * H1 * W1, scr);
    DFE_LAUNCH_CHECK(ctx);
    return dfe_spatial_matching_dispatch(ctx, scr, in2, K, H1, W1, maxh, maxw, out);
}
