// upsample.hip -- joint bilateral upsampling of a sparse field with a confidence plane (not in the reference).
//   dfe_guided_upsample_f32   values [C][Hl][Wl], a confidence plane and optionally the frame at both resolutions -> values [C][Hh][Wh]: per
//                             pixel the mean of the (2r)^2 low-resolution samples around it, weighted by a tent in each axis, by the sample's
//                             confidence and by how much the two frames agree there (the definition: include/dfe.h)
//
// The definition fixes the grouping of every product and the order of every sum, so the device is compared with its numpy restatement bit
// for bit; nothing here may contract a multiply into an add.
//   a workgroup   512 threads = a tile of 8 rows x 64 columns of the OUTPUT, a wave on 64 consecutive pixels of a row.  The sizes only
//                 grow (Hl <= Hh, Wl <= Wh), so the taps of T consecutive pixels of an axis span at most T - 1 + 2r low-resolution samples:
//                 the workgroup stages that footprint, (7 + 2r) x (63 + 2r) cells, into LDS once: per cell the C values, the validity a
//                 (decided here, once a sample and not once a tap; values under a = 0 are staged as 0) and the Cg low-resolution guide
//                 values.  A cell outside the low-resolution frame is staged as a = 0, so every thread walks its full 2r x 2r taps and LDS is
//                 indexed inside the footprint by construction.  38340 B at most (r = 4, C = 4, Cg = 4).
//   the tents     tx_j = float(double(n_j) / double(r den)) costs a double division; a pixel needs 2r per axis, but a column of the tile
//                 shares its tx and a row its ty.  The workgroup makes them once, [2r][64] and [2r][8] floats behind the footprint (one or
//                 two divisions a thread instead of 4r), 0 for a tap that does not exist; a zero tent makes a zero weight, and a sample of
//                 weight 0 does not exist.  Lanes read the x table at consecutive words and the y table at one word (a broadcast).
//                 Measured against every thread making its own 4r tents (C = 2, 360 x 640 -> 720 x 1280, table / per thread, ms):
//                 r = 1 0.0112 / 0.0146, r = 2 0.0152 / 0.0213, r = 4 0.0296 / 0.0397 without a guide, 0.0154 / 0.0181, 0.0222 / 0.0274,
//                 0.0469 / 0.0541 with a 3-channel one.
//   a thread      one output pixel: the taps rows ascending, columns ascending, S and N_c started from -0 (x + -0 is x for every x, the
//                 signed zeros included, so the first term starts the sum as the definition asks), then gain_c (N_c / S).
#include <cmath>

#include "dfe_field.h"

#pragma clang fp contract(off)

namespace {

constexpr int kUpMaxR = 4;
constexpr int kUpTileH = 8, kUpTileW = 64;

struct UpFrame {
    const float *v, *w, *guide_hi, *guide_lo;   // [C][Hl][Wl], [Hl][Wl] or null, [Cg][Hh][Wh], [Cg][Hl][Wl]
    float *out, *valid;                         // [C][Hh][Wh], [Hh][Wh] or null
    int Hl, Wl, Hh, Wh, r;
    float inv_s2;
    float gain[4];
};

// j0 = floor(((2 x + 1) nl - nh) / (2 nh)) for 0 <= x and 1 <= nl <= nh <= 32768: (2 x + 1) nl <= 65535 * 32768 < 2^31 while x < nh, and
// the tile's columns beyond the frame (x < nh + 64) are never used, only kept from overflowing
__device__ __forceinline__ int up_j0(int x, int nl, int nh) {
    const long long num = (2ll * x + 1) * nl - nh, den = 2ll * nh;
    return num < 0 ? -1 : (int)((unsigned)num / (unsigned)den);   // (num >= -nh > -den: floor is -1; num < 2^32 by the bound above)
}

// the tent of tap j at pixel x: float(double(n_j) / double(r den)), n_j = r den - |num - j den|; 0 where the tap does not exist
__device__ __forceinline__ float up_tent(int x, int j, int nl, int nh, int r) {
    const long long num = (2ll * x + 1) * nl - nh, den = 2ll * nh, d = num - j * den, n = r * den - (d < 0 ? -d : d);
    return j < 0 || j >= nl || n <= 0 ? 0.f : (float)((double)n / (double)(r * den));
}

// LDS image: planes [C + 1 + Cg][fh][fw] of floats: the values, a, the low-resolution guide; then tx [2r][64] and ty [2r][8]
template <int C, int Cg> __global__ __launch_bounds__(512) void guided_upsample_kernel(UpFrame f) {
    extern __shared__ __attribute__((aligned(16))) float up_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = f.r, taps = 2 * r, fw = kUpTileW - 1 + taps, fh = kUpTileH - 1 + taps, cells = fh * fw;
    const int X0 = blockIdx.x * kUpTileW, Y0 = blockIdx.y * kUpTileH;
    const int X = X0 + lane, Y = Y0 + wave;
    const long long HWl = (long long)f.Hl * f.Wl, HWh = (long long)f.Hh * f.Wh;
    // the footprint's first sample: the first tap of the tile's first pixel (negative at the frame's edge)
    const int jx0 = up_j0(X0, f.Wl, f.Wh), jy0 = up_j0(Y0, f.Hl, f.Hh);
    const int bx = jx0 - r + 1, by = jy0 - r + 1;
    float *const vp = up_lds, *const ap = up_lds + C * cells, *const gp = up_lds + (C + 1) * cells;
    float *const txp = up_lds + (C + 1 + Cg) * cells, *const typ = txp + taps * kUpTileW;
    // ---- stage: wave w takes rows w, w + 8, ... of the footprint ----
    for (int cy = wave; cy < fh; cy += kUpTileH) {
        const int yy = by + cy;
        const bool row_in = yy >= 0 && yy < f.Hl;
        for (int cx = lane; cx < fw; cx += 64) {
            const int xx = bx + cx, cell = cy * fw + cx;
            float a = 0.f, val[C], g[Cg ? Cg : 1];
#pragma unroll
            for (int c = 0; c < C; ++c) val[c] = 0.f;
#pragma unroll
            for (int c = 0; c < Cg; ++c) g[c] = 0.f;
            if (row_in && xx >= 0 && xx < f.Wl) {
                const long long q = (long long)yy * f.Wl + xx;
                a = dfe_sample_read<C>(f.v, f.w, HWl, q, val);
#pragma unroll
                for (int c = 0; c < Cg; ++c) g[c] = f.guide_lo[c * HWl + q];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) vp[c * cells + cell] = a != 0.f ? val[c] : 0.f;
            ap[cell] = a;
#pragma unroll
            for (int c = 0; c < Cg; ++c) gp[c * cells + cell] = g[c];
        }
    }
    // ---- the tents: thread i makes tx of tap i / 64 at column i % 64 (2r <= 8 taps: 512 threads at most), and the first 8 * 2r threads ty
    if (wave < taps) txp[wave * kUpTileW + lane] = X < f.Wh ? up_tent(X, up_j0(X, f.Wl, f.Wh) - r + 1 + wave, f.Wl, f.Wh, r) : 0.f;
    if ((int)threadIdx.x < taps * kUpTileH) {
        const int t = threadIdx.x >> 3, row = threadIdx.x & 7, y = Y0 + row;
        typ[t * kUpTileH + row] = y < f.Hh ? up_tent(y, up_j0(y, f.Hl, f.Hh) - r + 1 + t, f.Hl, f.Hh, r) : 0.f;
    }
    __syncthreads();
    if (X >= f.Wh || Y >= f.Hh) return;
    const long long p = (long long)Y * f.Wh + X;
    // the first tap's cell: j0(X) - jx0 <= lane and j0(Y) - jy0 <= wave because the sizes only grow, so base + (2r - 1)(fw + 1) < cells
    const int base = (up_j0(Y, f.Hl, f.Hh) - jy0) * fw + (up_j0(X, f.Wl, f.Wh) - jx0);
    float gc[Cg ? Cg : 1];
#pragma unroll
    for (int c = 0; c < Cg; ++c) gc[c] = f.guide_hi[c * HWh + p];
    float S = -0.f, N[C];
#pragma unroll
    for (int c = 0; c < C; ++c) N[c] = -0.f;
#pragma clang loop unroll(disable)
    for (int i = 0; i < taps; ++i) {
        const float ty = typ[i * kUpTileH + wave];
#pragma clang loop unroll_count(2) vectorize(disable) interleave(disable)
        for (int j = 0; j < taps; ++j) {
            const int cell = base + i * fw + j;
            const float tent = ty * txp[j * kUpTileW + lane];
            float ar = ap[cell];
            if constexpr (Cg > 0) ar = ar * dfe_range_weight<Cg>(gc, gp, cells, cell, f.inv_s2);
            const float wt = ar * tent;
            // a sample that exists: a > 0, rr > 0, both tents > 0 and no underflow to 0.  One that does not adds -0, which changes no sum
            // (the values are read either way: a load under the test would wait for LDS once more per tap)
            const bool is = wt > 0.f;
            S += is ? wt : -0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float term = wt * vp[c * cells + cell];
                N[c] += is ? term : -0.f;
            }
        }
    }
    const bool any = S > 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) f.out[c * HWh + p] = any ? f.gain[c] * (N[c] / S) : 0.f;
    if (f.valid) f.valid[p] = any ? 1.f : 0.f;
}

// bytes of the staged footprint and the two tent tables (40644 at most: below the 64 KB that need no attribute)
size_t up_lds_bytes(int C, int Cg, int r) {
    return ((size_t)(C + 1 + Cg) * (kUpTileH - 1 + 2 * r) * (kUpTileW - 1 + 2 * r) + (size_t)2 * r * (kUpTileW + kUpTileH)) * sizeof(float);
}

template <int C, int Cg> int upsample_launch(dfe_ctx *ctx, const UpFrame &f) {
    const dim3 grid((unsigned)dfe_cdiv(f.Wh, kUpTileW), (unsigned)dfe_cdiv(f.Hh, kUpTileH));
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    DfeProfScope prof(ctx);
    hipLaunchKernelGGL((guided_upsample_kernel<C, Cg>), grid, dim3(kUpTileH * kUpTileW), up_lds_bytes(C, Cg, f.r), ctx->stream, f);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_guided_upsample_f32(dfe_ctx *ctx, const float *v, int C, int Hl, int Wl, const float *w, const float *guide_hi, const float *guide_lo, int Cg,
                            float sigma, int r, const float *gain, int Hh, int Wh, float *out, float *valid) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, v && out, DFE_E_ARG, "dfe_guided_upsample_f32: NULL tensor");
    if (int rc = dfe_channels_check(ctx, "dfe_guided_upsample_f32", C)) return rc;
    if (int rc = dfe_guide_channels_check(ctx, "dfe_guided_upsample_f32", Cg)) return rc;
    DFE_REQUIRE(ctx, Cg > 0 ? guide_hi && guide_lo : !guide_hi && !guide_lo, DFE_E_ARG,
                "dfe_guided_upsample_f32: Cg=%d takes %s", Cg, Cg > 0 ? "the guide at both resolutions" : "no guide (both NULL)");
    DFE_REQUIRE(ctx, r >= 1 && r <= kUpMaxR, DFE_E_ARG, "dfe_guided_upsample_f32: r=%d must be 1 .. %d", r, kUpMaxR);
    for (int c = 0; gain && c < C; ++c) DFE_REQUIRE(ctx, std::isfinite(gain[c]), DFE_E_ARG, "dfe_guided_upsample_f32: gain[%d] is not finite", c);
    DFE_REQUIRE(ctx, Hl >= 1 && Wl >= 1 && Hh <= 32768 && Wh <= 32768 && Hl <= Hh && Wl <= Wh, DFE_E_SHAPE,
                "dfe_guided_upsample_f32: %dx%d -> %dx%d (every size 1 .. 32768, and none may shrink)", Hl, Wl, Hh, Wh);
    const long long HWl = (long long)Hl * Wl, HWh = (long long)Hh * Wh;
    for (int i = 0; i < 2; ++i) {   // neighbours are read: no output over an input
        const float *o = i ? valid : out;
        const long long no = i ? HWh : C * HWh;
        DFE_REQUIRE(ctx, !dfe_overlap(o, no, v, C * HWl) && !dfe_overlap(o, no, w, HWl) && !dfe_overlap(o, no, guide_hi, Cg * HWh) && !dfe_overlap(o, no, guide_lo, Cg * HWl),
                    DFE_E_ARG, "dfe_guided_upsample_f32: %s overlaps an input", i ? "valid" : "out");
    }
    DFE_REQUIRE(ctx, !dfe_overlap(out, C * HWh, valid, HWh), DFE_E_ARG, "dfe_guided_upsample_f32: out overlaps valid");
    const bool guided = Cg > 0 && sigma > 0.f;
    UpFrame f{v, w, guided ? guide_hi : nullptr, guided ? guide_lo : nullptr, out, valid, Hl, Wl, Hh, Wh, r, guided ? 1.0f / (sigma * sigma) : 0.f, {1.f, 1.f, 1.f, 1.f}};
    for (int c = 0; gain && c < C; ++c) f.gain[c] = gain[c];
    const int cg = guided ? Cg : 0;
    return dfe_dispatch_1to4(C, [&](auto c) {
        constexpr int Cc = decltype(c)::value;
        if (cg == 0) return upsample_launch<Cc, 0>(ctx, f);
        return dfe_dispatch_1to4(cg, [&](auto g) { return upsample_launch<Cc, decltype(g)::value>(ctx, f); });
    });
}

}  // extern "C"
