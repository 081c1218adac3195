// image_scale.hip -- image.scale(src, width, height), bilinear: what sits between the full-resolution camera frame and the model's
// geometry (depth_estimation_api.lua:71,144, test_opticalflow.lua:278,283).  `image` is un-vendored, so this is the library's own
// definition (include/dfe.h) and parity is unpinned.
// Per axis, in exact int64 arithmetic: num = (2 x + 1) Ws - Wd, den = 2 Wd; num < 0: i0 = 0, w = 0; otherwise i0 = num / den and
// w = float32(double(num % den) / double(den)); i1 = min(i0 + 1, Ws - 1); i0 >= Ws - 1: i0 = Ws - 1, w = 0 -- pixel centres at
// half-integers, edge clamp, no anti-aliasing.  Value in fp32: top = a + wx (b - a), bot alike, out = top + wy (bot - top); a weight of
// exactly 0 takes the first operand as it is.
// Consequences: equal sizes give a bit copy (num = 2 x Ws: i0 = x, w = 0 on both axes); a 2 x reduction of integer-valued frames is the
// exact 2 x 2 mean (num = Wd (4 x + 1): i0 = 2 x, w = 1/2, and halves of small integers are exact in fp32).
// One thread per output pixel, looping over the planes; a row of threads stores a row of the output.  No LDS: the kernel moves one frame
// and is tiny next to the matcher.
#include "dfe_internal.h"

namespace {

struct ScaleTap { int i0, i1; float w; };

__device__ inline ScaleTap scale_tap(int x, int ns, int nd) {
    const long long num = (2ll * x + 1) * ns - nd, den = 2ll * nd;
    ScaleTap t;
    if (num < 0) { t.i0 = 0; t.w = 0.f; }
    else { t.i0 = (int)(num / den); t.w = (float)((double)(num % den) / (double)den); }
    t.i1 = t.i0 + 1 < ns - 1 ? t.i0 + 1 : ns - 1;
    if (t.i0 >= ns - 1) { t.i0 = ns - 1; t.w = 0.f; }
    return t;
}

__device__ inline float scale_load(const float *p, long long e, float) { return p[e]; }
__device__ inline float scale_load(const unsigned char *p, long long e, float s) { return (float)p[e] * s; }

__device__ inline float scale_lerp(float a, float b, float w) { return w == 0.f ? a : a + w * (b - a); }

template <typename T>
__global__ __launch_bounds__(256) void image_scale_kernel(const T *__restrict__ src, float s, int C, int Hs, int Ws, int Hd, int Wd, float *__restrict__ dst) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= Wd || y >= Hd) return;
    const ScaleTap tx = scale_tap(x, Ws, Wd), ty = scale_tap(y, Hs, Hd);
    const long long r0 = (long long)ty.i0 * Ws, r1 = (long long)ty.i1 * Ws, sp = (long long)Hs * Ws, dp = (long long)Hd * Wd;
    for (int c = 0; c < C; ++c) {
        const long long b = c * sp;
        const float top = scale_lerp(scale_load(src, b + r0 + tx.i0, s), scale_load(src, b + r0 + tx.i1, s), tx.w);
        const float bot = scale_lerp(scale_load(src, b + r1 + tx.i0, s), scale_load(src, b + r1 + tx.i1, s), tx.w);
        dst[c * dp + (long long)y * Wd + x] = scale_lerp(top, bot, ty.w);
    }
}

int scale_check(dfe_ctx *ctx, const char *fn, const void *src, int C, int Hs, int Ws, int Hd, int Wd, const void *dst) {
    DFE_REQUIRE(ctx, src && dst, DFE_E_ARG, "%s: NULL tensor", fn);
    DFE_REQUIRE(ctx, C >= 1 && Hs >= 1 && Hs <= 32768 && Ws >= 1 && Ws <= 32768 && Hd >= 1 && Hd <= 32768 && Wd >= 1 && Wd <= 32768, DFE_E_ARG,
                "%s: C=%d %dx%d -> %dx%d (every size 1..32768)", fn, C, Hs, Ws, Hd, Wd);
    return DFE_OK;
}

}  // namespace

extern "C" int dfe_image_scale_f32(dfe_ctx *ctx, const float *src, int C, int Hs, int Ws, int Hd, int Wd, float *dst) {
    DFE_ENTER(ctx);
    int rc = scale_check(ctx, "dfe_image_scale_f32", src, C, Hs, Ws, Hd, Wd, dst);
    if (rc) return rc;
    hipLaunchKernelGGL(image_scale_kernel<float>, dim3(dfe_cdiv(Wd, 64), dfe_cdiv(Hd, 4)), dim3(64, 4), 0, ctx->stream, src, 1.f, C, Hs, Ws, Hd, Wd, dst);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

extern "C" int dfe_image_scale_u8(dfe_ctx *ctx, const uint8_t *src, float scale, int C, int Hs, int Ws, int Hd, int Wd, float *dst) {
    DFE_ENTER(ctx);
    int rc = scale_check(ctx, "dfe_image_scale_u8", src, C, Hs, Ws, Hd, Wd, dst);
    if (rc) return rc;
    hipLaunchKernelGGL(image_scale_kernel<unsigned char>, dim3(dfe_cdiv(Wd, 64), dfe_cdiv(Hd, 4)), dim3(64, 4), 0, ctx->stream, src, scale, C, Hs, Ws, Hd, Wd, dst);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}
