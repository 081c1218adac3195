// temporal.hip -- the temporal depth filter: a field carried along its own flow to the next frame's grid and fused with that frame's
// measurement (not in the reference).
//   dfe_forward_warp_f32     values [C][H][W] and weights [H][W] scattered along flow [2][H][W] over a region R, a z-buffer deciding which
//                            source keeps a target (the definition: include/dfe.h)
//   dfe_temporal_fuse_f32    a propagated prior and a new measurement, pointwise
//   dfe_temporal_step_f32    both in one call: the prior stays in registers
//
// Layout: no LDS.  The z-buffer is one 64-bit word per pixel of R in the ctx's side buffer, (ordered key << 32 | source index), all-ones
// = no source (a source index is below 2^31).  Clear = a memset of the stream; splat = one thread per pixel of R, one no-return 64-bit
// integer minimum on the target's word (an integer minimum does not depend on the order of arrival: the word, and with it every output
// bit, is reproducible); resolve = one thread per pixel of the FRAME, a wave = 64 consecutive pixels of one row, so the word is read and
// every output is stored in whole runs, the winner's planes are gathered through L2 (displacements are a few pixels: a wave's winners
// lie in a few rows around its own), and the zero border is written by the same launch.  The staged resolve, the staged fusion and the
// fused resolve run the SAME device functions (temporal_gather; temporal_fuse_px in temporal_common.h, which the four-tap splat of
// temporal_splat.hip shares), so the one call gives the bits of the two.
#include "temporal_common.h"

namespace {

constexpr unsigned long long kTemporalEmpty = ~0ull;

// ---- splat: one thread per pixel of R ----
template <int C> __global__ __launch_bounds__(256) void temporal_splat_kernel(TemporalFrame f, WarpArgs a, unsigned long long *z) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= f.Wo || y >= f.Ho) return;
    const int Y = f.y0 + y, X = f.x0 + x;
    const long long HW = (long long)f.H * f.W, p = (long long)Y * f.W + X;
    float val[C];
    if (dfe_sample_read<C>(a.v, a.w, HW, p, val) == 0.f) return;
    const float fy = a.flow[p], fx = a.flow[HW + p];
    if (!(dfe_finite(fy) && dfe_finite(fx))) return;
    float k = 0.f;
    if (a.key) {
        k = a.key[p];
        if (!dfe_finite(k)) return;
        k = k + 0.0f;   // -0 counts as +0
    }
    const float ty = floorf(((float)Y + fy) + 0.5f), tx = floorf(((float)X + fx) + 0.5f);
    // decided on the floats: only a target inside R (inside the frame) is converted to int
    if (!(ty >= (float)f.y0 && ty <= (float)(f.y0 + f.Ho - 1) && tx >= (float)f.x0 && tx <= (float)(f.x0 + f.Wo - 1))) return;
    const int yt = (int)ty - f.y0, xt = (int)tx - f.x0;
    if (yt >= f.Ho || xt >= f.Wo) return;   // (a bound above 2^24 that rounded up as a float)
    const long long t = (long long)yt * f.Wo + xt;
    const unsigned long long word = ((unsigned long long)temporal_ordered(k) << 32) | (unsigned)p;   // p < 2^31: the launcher's condition
    (void)__hip_atomic_fetch_min(z + t, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- what the resolve leaves at a pixel of R: the winner's values through gain / bias, its weight through decay, its index ----
template <int C> __device__ __forceinline__ void temporal_gather(const TemporalFrame &f, const WarpArgs &a, const unsigned long long *z, int Y, int X,
                                                                 float (&val)[C], float *wv, int *s) {
#pragma clang fp contract(off)
    const unsigned long long word = z[(long long)(Y - f.y0) * f.Wo + (X - f.x0)];
    *s = -1;
    *wv = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = 0.f;
    if (word == kTemporalEmpty) return;
    const int q = (int)(unsigned)word;
    const long long HW = (long long)f.H * f.W;
    *s = q;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float t = a.v[c * HW + q];
        if (a.has_gain) t = a.gain[c] * t;
        if (a.has_bias) t = t + a.bias[c];
        val[c] = t;
    }
    const float w = a.w[q];
    *wv = a.decay == 1.f ? w : w * a.decay;
}

// ---- resolve: one thread per pixel of the frame ----
template <int C> __global__ __launch_bounds__(256) void temporal_resolve_kernel(TemporalFrame f, WarpArgs a, const unsigned long long *z) {
    int Y, X, s = -1;
    bool inR;
    if (!temporal_pixel(f, &Y, &X, &inR)) return;
    const long long HW = (long long)f.H * f.W, p = (long long)Y * f.W + X;
    float val[C], wv = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = 0.f;
    if (inR) temporal_gather<C>(f, a, z, Y, X, val, &wv, &s);
#pragma unroll
    for (int c = 0; c < C; ++c) a.out[c * HW + p] = val[c];
    a.wout[p] = wv;
    if (a.src) a.src[p] = s;
}

// ---- fusion alone: one thread per pixel of the frame; out may be prior or meas, wout may be wp or wm (a pixel reads before it writes) ----
template <int C> __global__ __launch_bounds__(256) void temporal_fuse_kernel(TemporalFrame f, FuseArgs u) {
    int Y, X;
    bool inR;
    if (!temporal_pixel(f, &Y, &X, &inR)) return;
    const long long HW = (long long)f.H * f.W, p = (long long)Y * f.W + X;
    float z[C], m[C], wp = 0.f, wm = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = m[c] = 0.f;
    if (inR) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            z[c] = u.prior[c * HW + p];
            m[c] = u.meas[c * HW + p];
        }
        wp = u.wp[p];
        wm = u.wm[p];
    }
    temporal_fuse_store<C>(f, u, p, inR, z, wp, m, wm);
}

// ---- the fused resolve: gather, fuse in registers; the prior reaches memory only where it is asked for ----
template <int C> __global__ __launch_bounds__(256) void temporal_step_kernel(TemporalFrame f, WarpArgs a, FuseArgs u, const unsigned long long *zbuf) {
    int Y, X, s = -1;
    bool inR;
    if (!temporal_pixel(f, &Y, &X, &inR)) return;
    const long long HW = (long long)f.H * f.W, p = (long long)Y * f.W + X;
    float z[C], m[C], wp = 0.f, wm = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = m[c] = 0.f;
    if (inR) {
        temporal_gather<C>(f, a, zbuf, Y, X, z, &wp, &s);
#pragma unroll
        for (int c = 0; c < C; ++c) m[c] = u.meas[c * HW + p];
        wm = u.wm[p];
    }
    if (a.out) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.out[c * HW + p] = z[c];
    }
    if (a.wout) a.wout[p] = wp;
    if (a.src) a.src[p] = s;
    temporal_fuse_store<C>(f, u, p, inR, z, wp, m, wm);
}

// ---- host ----
// the z-buffer in the ctx's side buffer (grown once, then no allocation per call), cleared, and the splat
template <int C> int temporal_splat(dfe_ctx *ctx, const TemporalFrame &f, const WarpArgs &a, unsigned long long **zout) {
    const size_t words = (size_t)f.Ho * f.Wo;
    void *aux = nullptr;
    if (int rc = dfe_aux_scratch(ctx, DfeCarve::up(words * sizeof(unsigned long long)), &aux)) return rc;
    DfeCarve carve(aux);
    unsigned long long *z = carve.take<unsigned long long>(words);
    {
        DfeProfScope prof(ctx);
        DFE_HIP(ctx, hipMemsetAsync(z, 0xff, words * sizeof(unsigned long long), ctx->stream));
    }
    {
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((temporal_splat_kernel<C>), temporal_grid(f.Ho, f.Wo), dim3(256), 0, ctx->stream, f, a, z);
        DFE_LAUNCH_CHECK(ctx);
    }
    *zout = z;
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_forward_warp_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key, int y0, int x0, int Ho,
                         int Wo, const float *gain, const float *bias, float decay, float *out, float *wout, int32_t *src) {
    static const char *fn = "dfe_forward_warp_f32";
    DFE_ENTER(ctx);
    WarpArgs a{};
    if (int rc = temporal_warp_check(ctx, fn, v, C, H, W, w, flow, gain, bias, decay, &a)) return rc;
    DFE_REQUIRE(ctx, out && wout, DFE_E_ARG, "%s: NULL tensor", fn);
    if (int rc = dfe_region_check(ctx, fn, H, W, y0, x0, Ho, Wo)) return rc;
    const long long HW = (long long)H * W;
    const TemporalSpan outs[] = {{out, C * HW}, {wout, HW}, {src, HW}}, ins[] = {{v, C * HW}, {w, HW}, {flow, 2 * HW}, {key, HW}};
    if (int rc = temporal_overlap_check(ctx, fn, outs, 3, ins, 4)) return rc;
    a.key = key; a.out = out; a.wout = wout; a.src = src;
    const TemporalFrame f{H, W, y0, x0, Ho, Wo};
    return dfe_dispatch_1to4(C, [&](auto c) {
        constexpr int Cc = decltype(c)::value;
        DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
        unsigned long long *z = nullptr;
        if (int rc = temporal_splat<Cc>(ctx, f, a, &z)) return rc;
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((temporal_resolve_kernel<Cc>), temporal_grid(H, W), dim3(256), 0, ctx->stream, f, a, (const unsigned long long *)z);
        DFE_LAUNCH_CHECK(ctx);
        return (int)DFE_OK;
    });
}

int dfe_temporal_fuse_f32(dfe_ctx *ctx, const float *prior, const float *wp, const float *meas, const float *wm, int C, int H, int W, int y0, int x0,
                          int Ho, int Wo, float tol, float wmax, float *out, float *wout, float *flag) {
    static const char *fn = "dfe_temporal_fuse_f32";
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, prior && wp && meas && wm && out && wout, DFE_E_ARG, "%s: NULL tensor", fn);
    if (int rc = dfe_channels_check(ctx, fn, C)) return rc;
    if (int rc = temporal_fuse_check(ctx, fn, tol, wmax)) return rc;
    if (int rc = dfe_region_check(ctx, fn, H, W, y0, x0, Ho, Wo)) return rc;
    const TemporalFrame f{H, W, y0, x0, Ho, Wo};
    const FuseArgs u{prior, wp, meas, wm, tol * tol, wmax, out, wout, flag};
    return dfe_dispatch_1to4(C, [&](auto c) {
        DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((temporal_fuse_kernel<decltype(c)::value>), temporal_grid(H, W), dim3(256), 0, ctx->stream, f, u);
        DFE_LAUNCH_CHECK(ctx);
        return (int)DFE_OK;
    });
}

int dfe_temporal_step_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key, int y0, int x0, int Ho,
                          int Wo, const float *gain, const float *bias, float decay, const float *meas, const float *wm, float tol, float wmax,
                          float *out, float *wout, float *flag, float *prior, float *wprior, int32_t *src) {
    static const char *fn = "dfe_temporal_step_f32";
    DFE_ENTER(ctx);
    WarpArgs a{};
    if (int rc = temporal_warp_check(ctx, fn, v, C, H, W, w, flow, gain, bias, decay, &a)) return rc;
    DFE_REQUIRE(ctx, meas && wm && out && wout, DFE_E_ARG, "%s: NULL tensor", fn);
    if (int rc = temporal_fuse_check(ctx, fn, tol, wmax)) return rc;
    if (int rc = dfe_region_check(ctx, fn, H, W, y0, x0, Ho, Wo)) return rc;
    const long long HW = (long long)H * W;
    // the state is gathered while every output is written: none may overlap it, nor another output; out / wout may be meas / wm (pointwise)
    const TemporalSpan outs[] = {{out, C * HW}, {wout, HW}, {flag, HW}, {prior, C * HW}, {wprior, HW}, {src, HW}};
    const TemporalSpan ins[] = {{v, C * HW}, {w, HW}, {flow, 2 * HW}, {key, HW}};
    if (int rc = temporal_overlap_check(ctx, fn, outs, 6, ins, 4)) return rc;
    const TemporalSpan late[] = {{flag, HW}, {prior, C * HW}, {wprior, HW}, {src, HW}}, pointwise[] = {{meas, C * HW}, {wm, HW}};
    if (int rc = temporal_overlap_check(ctx, fn, late, 4, pointwise, 2)) return rc;
    a.key = key; a.out = prior; a.wout = wprior; a.src = src;
    const TemporalFrame f{H, W, y0, x0, Ho, Wo};
    const FuseArgs u{nullptr, nullptr, meas, wm, tol * tol, wmax, out, wout, flag};
    return dfe_dispatch_1to4(C, [&](auto c) {
        constexpr int Cc = decltype(c)::value;
        DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
        unsigned long long *z = nullptr;
        if (int rc = temporal_splat<Cc>(ctx, f, a, &z)) return rc;
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((temporal_step_kernel<Cc>), temporal_grid(H, W), dim3(256), 0, ctx->stream, f, a, u, (const unsigned long long *)z);
        DFE_LAUNCH_CHECK(ctx);
        return (int)DFE_OK;
    });
}

}  // extern "C"
