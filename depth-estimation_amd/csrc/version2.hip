// version2.hip -- the single-scale learned model of version2/ as ONE call: what version2/test.lua:40-53 does with getNetwork(datap)
// (version2/network.lua:5-39) for a frame pair:
//   filter1 = SpatialContrastiveNormalization(C, gaussian1D(normalization_k)) -> SpatialPadding(-lWin, -tWin, -rWin, -bWin) -> conv stack
//   filter2 = the same normalisation -> the same conv stack (shared weights)
//   SpatialMatching(hWin, wWin) on the two feature maps, then the dense decode of test.lua:45-51: first minimum over the window,
//   yflow = floor(idx / wWin) - tWin, xflow = idx - floor(idx / wWin) * wWin - lWin.
// Every stage is the stand-alone device op (same kernels, same order of operations), so the one-call result equals the staged host
// path bit for bit.
#include "dfe_internal.h"

namespace {

// one wave per pixel: first minimum of the window's N cells (index order), decoded as version2/test.lua:45-51 does
__global__ __launch_bounds__(256) void v2_argmin_decode_kernel(const float *__restrict__ vol, long long P, int N, int wWin, int lWin, int tWin,
                                                               long long *__restrict__ idx, float *__restrict__ xflow, float *__restrict__ yflow) {
    const int lane = threadIdx.x & 63;
    const long long wid = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long px = wid; px < P; px += nw) {
        const float *v = vol + px * N;
        float best = __int_as_float(0x7f800000);
        int bi = 0x7fffffff;
        for (int i = lane; i < N; i += 64) {
            const float c = v[i];
            if (c < best) { best = c; bi = i; }       // (strict: the lane keeps its first minimum; a NaN never wins -- torch.min would return it: the
                                                      //  equality with the staged host path holds for volumes without NaN)
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            if (bi == 0x7fffffff) bi = 0;
            const int fy = bi / wWin;
            if (idx) idx[px] = (long long)bi + 1;
            if (yflow) yflow[px] = (float)(fy - tWin);
            if (xflow) xflow[px] = (float)(bi - fy * wWin - lWin);
        }
    }
}

}  // namespace

// the matcher into a volume, then the first-minimum decode of it (idx / xflow / yflow, each may be NULL; none: the volume only)
static int v2_volume_argmin(dfe_ctx *ctx, const float *in1, const float *in2, int K, int H1, int W1, int hWin, int wWin, float *vol, long long *idx, float *xflow,
                            float *yflow) {
    {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        int rc = dfe_spatial_matching_dispatch(ctx, in1, in2, K, H1, W1, hWin, wWin, vol);
        if (rc) return rc;
    }
    DfeStageScope st(ctx, DFE_STAGE_EXTRACT);
    if (xflow || yflow || idx) {
        const long long P1 = (long long)H1 * W1;
        hipLaunchKernelGGL(v2_argmin_decode_kernel, dim3(dfe_grid1d(P1, 4, 65535 * 16)), dim3(256), 0, ctx->stream, vol, P1, hWin * wWin, wWin, dfe_window_lead(wWin),
                           dfe_window_lead(hWin), idx, xflow, yflow);
        DFE_LAUNCH_CHECK(ctx);
    }
    return DFE_OK;
}

extern "C" int dfe_version2_flow_pair_f32(dfe_ctx *ctx, const float *prev, const float *cur, int C, int H, int W, const float *norm_kernel_host,
                                          int norm_k, float threshold, float thresval, const dfe_filter_layer *layers, int nlayers, int hWin,
                                          int wWin, float *xflow, float *yflow, int64_t *idx, float *volume) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, prev && cur && norm_kernel_host && layers, DFE_E_ARG, "dfe_version2_flow_pair_f32: NULL argument");
    DFE_REQUIRE(ctx, C > 0 && H > 0 && W > 0 && nlayers > 0 && nlayers <= 8 && hWin > 0 && wWin > 0, DFE_E_ARG,
                "dfe_version2_flow_pair_f32: C=%d %dx%d, %d layers, window %dx%d", C, H, W, nlayers, hWin, wWin);
    DfeStackGeom sg;
    int rc = dfe_filter_stack_geom(ctx, "dfe_version2_flow_pair_f32", layers, nlayers, C, &sg);
    if (rc) return rc;
    const int hk = sg.hk, wk = sg.wk, K = sg.K, maxplanes = sg.maxplanes;
    const int lWin = dfe_window_lead(wWin), tWin = dfe_window_lead(hWin);   // datap.lWin, tWin; rWin = floor(wWin / 2), bWin = floor(hWin / 2)
    const int Hc = H - (hWin - 1), Wc = W - (wWin - 1);           // the cropped branch's frame
    const int H1 = Hc - hk + 1, W1 = Wc - wk + 1;                 // matcher output = the dense inference region
    DFE_REQUIRE(ctx, H1 > 0 && W1 > 0, DFE_E_SHAPE, "dfe_version2_flow_pair_f32: frame %dx%d too small for window %dx%d + kernel %dx%d", H, W, hWin, wWin, hk, wk);
    const int N = hWin * wWin;
    const long long P = (long long)H * W, P1 = (long long)H1 * W1;
    // arena: normalisation scratch | normalised cur | cropped normalised prev | two ping-pong feature buffers per branch | volume (unless the caller gave one)
    const size_t f_cn = ((size_t)C + 3) * P, f_n = (size_t)C * P, f_c = (size_t)C * Hc * Wc;
    const size_t f_fa = (size_t)maxplanes * Hc * Wc, f_fb = (size_t)maxplanes * P;
    // nobody asked for the volume: matcher and decode in one kernel where fm_select has one for the shape (bit-identical to the volume
    // path: the same sums, the same first minimum).  The job is the one that runs below, its maps arena buffers to come
    FmJob job = fm_job(FM_ARGMIN, nullptr, nullptr, K, H1, W1, hWin, wWin);
    job.idx = (long long *)idx; job.xflow = xflow; job.yflow = yflow;
    const FmPick plan = (!volume && (xflow || yflow || idx)) ? fm_select(dfe_fm_env(ctx), job) : FmPick{};
    // (the volume needs a place in the arena only when nobody gave one AND no such kernel takes the shape: 316 MB at VGA, 2.4 GB at 1080p
    //  that the lean path never touches)
    const bool lean = plan.kernel != FM_K_NONE;
    const size_t f_vol = (volume || lean) ? 0 : (size_t)P1 * N;
    // both matrix-core options on: the last layer's convolution leaves the features' squared norms for the matcher (no pass of its own)
    const bool mm_both = ctx->opt[DFE_OPT_CONV_MFMA] > 0 && plan.kernel == FM_K_MFMA && layers[nlayers - 1].nOut <= 32 && !layers[nlayers - 1].conn;
    const size_t f_nrm = mm_both ? fm_mfma_scratch(job) : 0;
    float *s_cn, *n1, *c0, *fa[2], *fb[2], *vol, *nrm;            // nrm: |a|^2 [H1][W1] | |b|^2 [H2][W2]
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        s_cn = c.take<float>(f_cn); n1 = c.take<float>(f_n); c0 = c.take<float>(f_c);
        for (float *&f : fa) f = c.take<float>(f_fa);
        for (float *&f : fb) f = c.take<float>(f_fb);
        vol = c.take<float>(f_vol); nrm = c.take<float>(f_nrm);
    });
    if (rc) return rc;
    if (volume) vol = volume;
    bool norms_ready = false;
    const float *ia = c0, *ib = n1;
    {
        DfeStageScope st(ctx, DFE_STAGE_FILTER);
        // both frames in the normalisation's two launches; the first branch's crop (SpatialPadding(-lWin, -tWin, -rWin, -bWin)) is the
        // window its last launch writes
        rc = dfe_contrastive_normalization_run2(ctx, prev, cur, C, H, W, norm_kernel_host, norm_k, threshold, thresval, s_cn, c0, n1, lWin, tWin, Wc, Hc);
        if (rc) return rc;
        int ha = Hc, wa = Wc, hb = H, wb = W;
        for (int i = 0; i < nlayers; ++i) {
            const float *in2[2] = {ia, ib};
            const dfe_filter_layer *L2[2] = {&layers[i], &layers[i]};
            const int H2[2] = {ha, hb}, W2[2] = {wa, wb};
            float *o2[2] = {fa[i & 1], fb[i & 1]};
            bool mm = false;
            if (ctx->opt[DFE_OPT_CONV_MFMA] > 0) {   // opt-in: the layer as an implicit GEMM on the matrix cores (fused multiply-adds)
                float *n2[2] = {nrm, nrm ? nrm + (size_t)H1 * W1 : nullptr};
                const bool last = mm_both && i == nlayers - 1;
                rc = dfe_conv_mfma_res_batch(ctx, 2, in2, H2, W2, nullptr, nullptr, layers[i], o2, &mm, last ? n2 : nullptr);
                if (rc) return rc;
                norms_ready = mm && last;
            }
            if (!mm) rc = dfe_filter_layer_forward_batch(ctx, 2, in2, L2, H2, W2, o2);
            if (rc) return rc;
            ia = o2[0]; ib = o2[1];
            ha -= layers[i].kH - 1; wa -= layers[i].kW - 1; hb -= layers[i].kH - 1; wb -= layers[i].kW - 1;
        }
        DFE_REQUIRE(ctx, ha == H1 && wa == W1 && hb == H1 + hWin - 1 && wb == W1 + wWin - 1, DFE_E_SHAPE, "dfe_version2_flow_pair_f32: internal shape mismatch");
    }
    if (lean) {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        job.in1 = ia; job.in2 = ib; job.norms = norms_ready ? nrm : nullptr; job.norms_ready = norms_ready;
        return dfe_fm_run(ctx, job);
    }
    return v2_volume_argmin(ctx, ia, ib, K, H1, W1, hWin, wWin, vol, (long long *)idx, xflow, yflow);
}

// nn.SpatialMatching(maxh, maxw) followed by `output:min(3)` and the decode of version2/test.lua:45-51 (radial_opticalflow_groundtruth.lua:88-100
// without the centre override), on feature maps that are already there: matcher and first-minimum decode in one kernel where the flat-tile
// matcher takes the shape, the matcher into the scratch arena + the decode kernel otherwise -- the same sums and the same first minimum
// either way.
extern "C" int dfe_spatial_matching_argmin_f32(dfe_ctx *ctx, const float *in1, const float *in2, int K, int H1, int W1, int maxh, int maxw,
                                               int64_t *idx, float *xflow, float *yflow) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, in1 && in2 && (idx || xflow || yflow), DFE_E_ARG, "dfe_spatial_matching_argmin_f32: NULL argument");
    DFE_REQUIRE(ctx, K > 0 && H1 > 0 && W1 > 0 && maxh > 0 && maxw > 0, DFE_E_ARG, "dfe_spatial_matching_argmin_f32: K=%d %dx%d window %dx%d", K, H1, W1, maxh, maxw);
    FmJob job = fm_job(FM_ARGMIN, in1, in2, K, H1, W1, maxh, maxw);
    job.idx = (long long *)idx; job.xflow = xflow; job.yflow = yflow;
    {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        FmPick pk;
        int rc = dfe_fm_run(ctx, job, &pk);
        if (rc || pk.kernel != FM_K_NONE) return rc;
    }
    void *scr = nullptr;
    int rc = dfe_scratch(ctx, (size_t)H1 * W1 * maxh * maxw * sizeof(float), &scr);
    if (rc) return rc;
    return v2_volume_argmin(ctx, in1, in2, K, H1, W1, maxh, maxw, (float *)scr, (long long *)idx, xflow, yflow);
}
