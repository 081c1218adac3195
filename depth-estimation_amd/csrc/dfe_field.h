// dfe_field.h -- what the dense-field operators share (consistency.hip, fill.hip, wmedian.hip, upsample.hip; DESIGN sections 4.25 - 4.28):
// the ONE statement in device code of the sample rule and the guide's range weight that include/dfe.h defines, and the host checks of
// their entries.  The operators are compared with their numpy restatements bit for bit (tests/field_rule.py holds the rule there), so
// the order of operations below is part of the definition; every function that rounds carries its own contraction pragma, because a
// pragma of the including file stands BEHIND this header and does not reach it.
#pragma once
#include <type_traits>

#include "dfe_internal.h"

// ---- device ----
constexpr float kDfeFieldMinWeight = 1e-6f;   // a weight below this (or not finite) is a hole

__device__ __forceinline__ bool dfe_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // (false for NaN)

// The sample at index q of planes v [C][plane] with the weight plane w (NULL reads as ones): it exists where w and every channel are
// finite and w >= 1e-6; val = the C values as they lie in memory, and the result is its validity a = min(w, 1), 0 where it does not exist
// (what lies under a = 0 must not enter arithmetic: the caller's business)
template <int C> __device__ __forceinline__ float dfe_sample_read(const float *v, const float *w, long long plane, long long q, float (&val)[C]) {
#pragma clang fp contract(off)
    const float wv = w ? w[q] : 1.f;
    bool ok = dfe_finite(wv) && wv >= kDfeFieldMinWeight;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        val[c] = v[c * plane + q];
        ok = ok && dfe_finite(val[c]);
    }
    return ok ? fminf(wv, 1.f) : 0.f;
}

// The guide's range weight max(0, 1 - |g(p) - g(q)|^2 inv_s2): gp = the Cg guide values at p, gq[c * plane + q] = channel c at q; the
// squares are summed in channel order from the first one (NaN -> 0; +Inf cannot occur: d2 inv_s2 is >= 0 or NaN)
template <int Cg> __device__ __forceinline__ float dfe_range_weight(const float (&gp)[Cg], const float *gq, int plane, int q, float inv_s2) {
#pragma clang fp contract(off)
    float d2 = 0.f;
#pragma unroll
    for (int c = 0; c < Cg; ++c) {
        const float d = gp[c] - gq[c * plane + q], s = d * d;
        d2 = c == 0 ? s : d2 + s;
    }
    return fmaxf(0.f, 1.f - d2 * inv_s2);
}

// ---- host: the entries' shared checks, each under the entry's own name `fn` ----
// [a, a + na) and [b, b + nb) floats share a byte
static inline bool dfe_overlap(const float *a, long long na, const float *b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}
// the region R = Ho x Wo at (y0, x0) lies inside the H x W frame and neither is empty
static inline int dfe_region_check(dfe_ctx *ctx, const char *fn, int H, int W, int y0, int x0, int Ho, int Wo) {
    DFE_REQUIRE(ctx, H > 0 && W > 0 && Ho > 0 && Wo > 0 && y0 >= 0 && x0 >= 0 && (long long)y0 + Ho <= H && (long long)x0 + Wo <= W, DFE_E_SHAPE,
                "%s: region %dx%d at (%d, %d) does not lie inside the %dx%d frame", fn, Ho, Wo, y0, x0, H, W);
    return DFE_OK;
}
static inline int dfe_channels_check(dfe_ctx *ctx, const char *fn, int C) {
    DFE_REQUIRE(ctx, C >= 1 && C <= 4, DFE_E_ARG, "%s: C=%d must be 1 .. 4", fn, C);
    return DFE_OK;
}
static inline int dfe_guide_channels_check(dfe_ctx *ctx, const char *fn, int Cg) {
    DFE_REQUIRE(ctx, Cg >= 0 && Cg <= 4, DFE_E_ARG, "%s: Cg=%d must be 0 .. 4", fn, Cg);
    return DFE_OK;
}
// f(std::integral_constant<int, n>) for a channel count n that the checks above have left in 1 .. 4
template <class F> int dfe_dispatch_1to4(int n, F &&f) {
    switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
    }
}
