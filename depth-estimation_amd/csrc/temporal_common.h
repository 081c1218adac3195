// temporal_common.h -- what the two forward warps of the temporal depth filter share (temporal.hip: the nearest-pixel z-buffer warp;
// temporal_splat.hip: the four-tap splat on integer accumulators; DESIGN sections 4.35, 4.36): the frame and argument structs, the
// ordered image of a key, the ONE statement of the fusion at a pixel (temporal_fuse_px: the staged fusion and both fused resolves run
// it, so a one-call entry gives the bits of its two stages), and the host checks of the entries.
#pragma once
#include "dfe_field.h"

struct TemporalFrame { int H, W, y0, x0, Ho, Wo; };

struct WarpArgs {
    const float *v, *w, *flow, *key;    // [C][H][W], [H][W], [2][H][W], [H][W] or null
    float gain[4], bias[4], decay;
    bool has_gain, has_bias;
    float *out, *wout;                  // [C][H][W], [H][W]; null in the one call where the prior is not asked for
    int *src;                           // [H][W] or null
};

struct FuseArgs {
    const float *prior, *wp, *meas, *wm;   // prior, wp: null in the one call (the prior is in registers)
    float tol2, wmax;
    float *out, *wout, *flag;              // flag may be null
};

// frame pixel (Y, X) of this thread and whether it lies in R; false: outside the frame
__device__ __forceinline__ bool temporal_pixel(const TemporalFrame &f, int *Y, int *X, bool *inR) {
    *X = blockIdx.x * 64 + (threadIdx.x & 63);
    *Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    *inR = *Y >= f.y0 && *Y < f.y0 + f.Ho && *X >= f.x0 && *X < f.x0 + f.Wo;
    return *X < f.W && *Y < f.H;
}

// the usual monotone map of fp32 bits to unsigned: the sign bit flipped for non-negative values, every bit for negative ones
__device__ __forceinline__ unsigned temporal_ordered(float k) {
    const unsigned u = __float_as_uint(k);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- the fusion of a prior (z, wp) and a measurement (m, wm) at one pixel ----
// min(w, wmax) where the sample exists by the field rule (dfe_field.h; the weight counts observations: not clipped at 1), else 0
template <int C> __device__ __forceinline__ float temporal_weight(const float (&val)[C], float w, float wmax) {
    bool ok = dfe_finite(w) && w >= kDfeFieldMinWeight;
#pragma unroll
    for (int c = 0; c < C; ++c) ok = ok && dfe_finite(val[c]);
    return ok ? fminf(w, wmax) : 0.f;
}

template <int C> __device__ __forceinline__ void temporal_fuse_px(const float (&z)[C], float wp, const float (&m)[C], float wm, float tol2, float wmax,
                                                                  float (&out)[C], float *wout, float *flag) {
#pragma clang fp contract(off)
    const float a = temporal_weight<C>(z, wp, wmax), b = temporal_weight<C>(m, wm, wmax);
    bool use_z;   // the side whose bits are copied
    if (a == 0.f || b == 0.f) {   // what lies under a zero weight is not read into arithmetic
        if (a == 0.f && b == 0.f) {
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = 0.f;
            *wout = 0.f;
            *flag = 0.f;
            return;
        }
        use_z = a != 0.f;
        *wout = use_z ? a : b;
        *flag = use_z ? 1.f : 2.f;
    } else {
        float d[C], d2 = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            d[c] = z[c] - m[c];
            const float sq = d[c] * d[c];
            d2 = c == 0 ? sq : d2 + sq;
        }
        if (d2 <= tol2) {   // agree: the mean weighted by the observations behind each side
            const float s = a + b, r = a / s;
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = m[c] + r * d[c];
            *wout = fminf(s, wmax);
            *flag = 3.f;
            return;
        }
        use_z = a > b;   // the prior survives, weakened by the dissent; else the measurement takes over
        *wout = use_z ? a - b : a == b ? b : b - a;
        *flag = use_z ? 4.f : 5.f;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = use_z ? z[c] : m[c];
}

template <int C> __device__ __forceinline__ void temporal_fuse_store(const TemporalFrame &f, const FuseArgs &u, long long p, bool inR, const float (&z)[C],
                                                                     float wp, const float (&m)[C], float wm) {
    const long long HW = (long long)f.H * f.W;
    float o[C], wo = 0.f, fl = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0.f;
    if (inR) temporal_fuse_px<C>(z, wp, m, wm, u.tol2, u.wmax, o, &wo, &fl);
#pragma unroll
    for (int c = 0; c < C; ++c) u.out[c * HW + p] = o[c];
    u.wout[p] = wo;
    if (u.flag) u.flag[p] = fl;
}

// ---- host ----
static inline dim3 temporal_grid(int h, int w) { return dim3((unsigned)dfe_cdiv(w, 64), (unsigned)dfe_cdiv(h, 4)); }

static inline bool temporal_finite(float v) { return v - v == 0.f; }

// the warp's arguments (every tensor but the outputs, which differ between the entries)
static inline int temporal_warp_check(dfe_ctx *ctx, const char *fn, const float *v, int C, int H, int W, const float *w, const float *flow, const float *gain,
                                      const float *bias, float decay, WarpArgs *a) {
    DFE_REQUIRE(ctx, v && w && flow, DFE_E_ARG, "%s: NULL tensor", fn);
    if (int rc = dfe_channels_check(ctx, fn, C)) return rc;
    DFE_REQUIRE(ctx, decay > 0.f && decay <= 1.f, DFE_E_ARG, "%s: decay=%g must lie in (0, 1]", fn, (double)decay);   // (false for NaN)
    for (int c = 0; c < C; ++c) {
        DFE_REQUIRE(ctx, !gain || temporal_finite(gain[c]), DFE_E_ARG, "%s: gain[%d]=%g is not finite", fn, c, (double)gain[c]);
        DFE_REQUIRE(ctx, !bias || temporal_finite(bias[c]), DFE_E_ARG, "%s: bias[%d]=%g is not finite", fn, c, (double)bias[c]);
        a->gain[c] = gain ? gain[c] : 1.f;
        a->bias[c] = bias ? bias[c] : 0.f;
    }
    DFE_REQUIRE(ctx, H <= 0 || W <= 0 || (long long)H * W <= 2147483647LL, DFE_E_ARG, "%s: H * W = %lld exceeds 2^31 - 1", fn, (long long)H * W);
    a->v = v; a->w = w; a->flow = flow;
    a->has_gain = gain != nullptr; a->has_bias = bias != nullptr; a->decay = decay;
    return DFE_OK;
}

static inline int temporal_fuse_check(dfe_ctx *ctx, const char *fn, float tol, float wmax) {
    DFE_REQUIRE(ctx, tol >= 0.f, DFE_E_ARG, "%s: tol=%g must be >= 0", fn, (double)tol);   // (false for NaN)
    DFE_REQUIRE(ctx, temporal_finite(wmax) && wmax >= kDfeFieldMinWeight, DFE_E_ARG, "%s: wmax=%g must be finite and >= 1e-6", fn, (double)wmax);
    return DFE_OK;
}

// the outputs `outs` (float counts n) overlap none of the inputs `ins` nor each other
struct TemporalSpan { const void *p; long long n; };
static inline int temporal_overlap_check(dfe_ctx *ctx, const char *fn, const TemporalSpan *outs, int nouts, const TemporalSpan *ins, int nins) {
    for (int i = 0; i < nouts; ++i) {
        for (int j = 0; j < nins; ++j)
            DFE_REQUIRE(ctx, !dfe_overlap((const float *)outs[i].p, outs[i].n, (const float *)ins[j].p, ins[j].n), DFE_E_ARG,
                        "%s: an output overlaps an input (the resolve gathers while it writes)", fn);
        for (int j = 0; j < i; ++j)
            DFE_REQUIRE(ctx, !dfe_overlap((const float *)outs[i].p, outs[i].n, (const float *)outs[j].p, outs[j].n), DFE_E_ARG,
                        "%s: two outputs overlap", fn);
    }
    return DFE_OK;
}
