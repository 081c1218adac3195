// wmedian.hip -- guided weighted median over windows up to 15 x 15 (not in the reference).
//   dfe_weighted_median_f32   values [C][H][W], a confidence plane and an optional guide image over a region R -> per channel the lower
//                             weighted median of the k x k window, and the mask of pixels that had a sample (the definition: include/dfe.h)
//
// The sample weight is an INTEGER (13 bits) made in fp32 by a fixed sequence of operations; everything behind it is integer arithmetic, so
// the sums do not depend on their order and the result is exact.
//   a workgroup   256 threads = a tile of 4 rows x 64 columns of the FRAME, a wave on 64 consecutive pixels of a row; it stages the tile plus
//                 its (k - 1) / 2 halo into LDS once: per cell the C values as order-preserving integer keys, the weight term (Cg == 0: the
//                 integer weight itself, else the validity a as a float) and the Cg guide values.  A cell outside R is staged as a = 0
//                 (such samples do not exist), so every thread walks the full k x k window and LDS is indexed inside the tile by construction.
//   a thread      one pixel: a first pass over the window for T and each channel's smallest and largest weighted key, then a bisection of
//                 that key interval, all channels in the same pass over the window: S_c(mid_c) = sum of the weights of the samples with
//                 key_c <= mid_c; 2 S >= T keeps the lower half.  The smallest m with 2 S(m) >= T is the key of a sample (S steps only there),
//                 so the interval's last key IS the output's bits.  At most 32 passes; a wave leaves when its last lane is done.
//   the weight    with a guide it costs Cg + 1 LDS reads and about 4 Cg + 6 vector instructions a sample.  Up to k = 7 the first pass leaves
//                 it in LDS, a u16 in a table [k k][256] (25 KB at k = 7), and the bisection passes read it back; above that the table
//                 (62 KB at k = 11, 115 KB at k = 15) leaves one workgroup a CU and making the weight again in every pass is faster
//                 (measured: DESIGN section 4.27).  Both forms are the same device code around `Table`.
#include "dfe_field.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWmedMaxK = 15;
constexpr int kWmedTileH = 4, kWmedTileW = 64;
// with a guide, windows up to this size keep their k k weights in LDS (a u16 each) instead of making them again in every pass: measured
// at C = 2, Cg = 3 on the VGA region, table against recomputation: k = 5 0.080 / 0.166 ms, 7 0.209 / 0.313, 11 1.015 / 0.697, 15 1.682 / 1.341
// (the table of k = 11 is 62 KB a workgroup: one workgroup a CU)
constexpr int kWmedTableMaxK = 7;

struct WmedFrame {
    const float *v, *w, *guide;    // [C][H][W], [H][W] or null, [Cg][H][W]
    float *out, *filtered;         // [C][H][W], [H][W] or null
    int H, W, y0, x0, Ho, Wo, k;
    float inv_s2;
};

// the order-preserving integer image of a float's bits (-0 below +0) and back
__device__ __forceinline__ unsigned wmed_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float wmed_unkey(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }
__device__ __forceinline__ unsigned wmed_weight(float ar) { return (unsigned)(ar * 4096.0f + 0.5f); }

// LDS image: planes [C + 1 + Cg][th][tw] of 32-bit words: keys, the weight term, the guide; Table: then the weights [k k][256] u16
template <int C, int Cg, bool Table> __global__ __launch_bounds__(256) void wmedian_kernel(WmedFrame f) {
    static_assert(Cg > 0 || !Table, "a table of weights only where they cost something to make");
    extern __shared__ __attribute__((aligned(16))) unsigned wmed_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = f.k, h = k >> 1, tw = kWmedTileW + k - 1, th = kWmedTileH + k - 1, cells = th * tw;
    const int X0 = blockIdx.x * kWmedTileW, Y0 = blockIdx.y * kWmedTileH;
    const int X = X0 + lane, Y = Y0 + wave;
    const long long HW = (long long)f.H * f.W;
    const bool in_frame = X < f.W && Y < f.H;
    // a tile that R does not touch: the zero border only (uniform for the workgroup, no barrier passed)
    if (X0 >= f.x0 + f.Wo || X0 + kWmedTileW <= f.x0 || Y0 >= f.y0 + f.Ho || Y0 + kWmedTileH <= f.y0) {
        if (in_frame) {
            const long long p = (long long)Y * f.W + X;
#pragma unroll
            for (int c = 0; c < C; ++c) f.out[c * HW + p] = 0.f;
            if (f.filtered) f.filtered[p] = 0.f;
        }
        return;
    }
    unsigned *const kp = wmed_lds, *const ap = wmed_lds + C * cells;
    float *const gp = reinterpret_cast<float *>(wmed_lds + (C + 1) * cells);
    unsigned short *const tab = reinterpret_cast<unsigned short *>(wmed_lds + (C + 1 + Cg) * cells) + threadIdx.x;   // [k k][256] u16, a column a thread
    // ---- stage: wave w takes rows w, w + 4, ... of the tile ----
    for (int cy = wave; cy < th; cy += 4) {
        const int yy = Y0 - h + cy;
        const bool row_in = yy >= f.y0 && yy < f.y0 + f.Ho;
        for (int cx = lane; cx < tw; cx += 64) {
            const int xx = X0 - h + cx, cell = cy * tw + cx;
            float a = 0.f, val[C], g[Cg ? Cg : 1];
#pragma unroll
            for (int c = 0; c < C; ++c) val[c] = 0.f;
#pragma unroll
            for (int c = 0; c < Cg; ++c) g[c] = 0.f;
            if (row_in && xx >= f.x0 && xx < f.x0 + f.Wo) {
                const long long q = (long long)yy * f.W + xx;
                a = dfe_sample_read<C>(f.v, f.w, HW, q, val);
#pragma unroll
                for (int c = 0; c < Cg; ++c) g[c] = f.guide[c * HW + q];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) kp[c * cells + cell] = wmed_key(val[c]);
            ap[cell] = Cg ? __float_as_uint(a) : (a != 0.f ? wmed_weight(a) : 0u);   // (r = 1: a * r is a)
#pragma unroll
            for (int c = 0; c < Cg; ++c) gp[c * cells + cell] = g[c];
        }
    }
    __syncthreads();
    if (!in_frame) return;
    const long long p = (long long)Y * f.W + X;
    const bool in_R = X >= f.x0 && X < f.x0 + f.Wo && Y >= f.y0 && Y < f.y0 + f.Ho;
    unsigned lo[C], hi[C], T = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) { lo[c] = 0xffffffffu; hi[c] = 0u; }
    if (in_R) {
        const int base = wave * tw + lane;           // the window's first cell; the pixel's own is base + h * tw + h
        float gc[Cg ? Cg : 1];
#pragma unroll
        for (int c = 0; c < Cg; ++c) gc[c] = gp[c * cells + base + h * tw + h];
        // the integer weight of the sample in `cell`
        auto weight = [&](int cell) -> unsigned {
            if constexpr (Cg == 0) {
                return ap[cell];
            } else {
                const float a = __uint_as_float(ap[cell]);
                const float r = dfe_range_weight<Cg>(gc, gp, cells, cell, f.inv_s2);
                return a != 0.f ? wmed_weight(a * r) : 0u;
            }
        };
        // the window loops: a row at a time, four samples in flight.  Left to itself the compiler interleaves the C = 1 reduction eight-fold
        // (116 .. 130 VGPRs, SGPR spills)
#pragma clang loop unroll(disable)
        for (int dy = 0; dy < k; ++dy)
#pragma clang loop unroll_count(4) vectorize(disable) interleave(disable)
            for (int dx = 0; dx < k; ++dx) {
                const int cell = base + dy * tw + dx;
                const unsigned wt = weight(cell);
                if constexpr (Table) tab[(dy * k + dx) * 256] = (unsigned short)wt;   // (at most 4096)
                T += wt;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const unsigned key = kp[c * cells + cell];
                    lo[c] = wt && key < lo[c] ? key : lo[c];
                    hi[c] = wt && key > hi[c] ? key : hi[c];
                }
            }
        bool open = false;
#pragma unroll
        for (int c = 0; c < C; ++c) open = open || lo[c] < hi[c];
        while (T && open) {
            unsigned mid[C], S[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { mid[c] = lo[c] + ((hi[c] - lo[c]) >> 1); S[c] = 0u; }
#pragma clang loop unroll(disable)
            for (int dy = 0; dy < k; ++dy)
#pragma clang loop unroll_count(4) vectorize(disable) interleave(disable)
                for (int dx = 0; dx < k; ++dx) {
                    const int cell = base + dy * tw + dx;
                    unsigned wt;
                    if constexpr (Table) wt = tab[(dy * k + dx) * 256];
                    else wt = weight(cell);
#pragma unroll
                    for (int c = 0; c < C; ++c) S[c] += kp[c * cells + cell] <= mid[c] ? wt : 0u;
                }
            open = false;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (lo[c] < hi[c]) {              // (a closed channel: mid = lo = hi, nothing to move)
                    if (2u * S[c] >= T) hi[c] = mid[c];
                    else lo[c] = mid[c] + 1u;
                }
                open = open || lo[c] < hi[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) f.out[c * HW + p] = T ? wmed_unkey(lo[c]) : 0.f;
    if (f.filtered) f.filtered[p] = T ? 1.f : 0.f;
}

// bytes of the staged tile (50544 at most) and of the weight table
size_t wmed_tile_lds(int C, int Cg, int k) { return (size_t)(C + 1 + Cg) * (kWmedTileH + k - 1) * (kWmedTileW + k - 1) * sizeof(unsigned); }
size_t wmed_table_lds(int k) { return (size_t)k * k * 256 * sizeof(unsigned short); }

template <int C, int Cg> int wmedian_launch(dfe_ctx *ctx, const WmedFrame &f) {
    const dim3 grid((unsigned)dfe_cdiv(f.W, kWmedTileW), (unsigned)dfe_cdiv(f.H, kWmedTileH));
    size_t lds = wmed_tile_lds(C, Cg, f.k);
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    if constexpr (Cg > 0) {
        if (f.k <= kWmedTableMaxK) {
            lds += wmed_table_lds(f.k);   // 50288 B at most: below the 64 KB that need no attribute
            DfeProfScope prof(ctx);
            hipLaunchKernelGGL((wmedian_kernel<C, Cg, true>), grid, dim3(256), lds, ctx->stream, f);
            DFE_LAUNCH_CHECK(ctx);
            return DFE_OK;
        }
    }
    DfeProfScope prof(ctx);
    hipLaunchKernelGGL((wmedian_kernel<C, Cg, false>), grid, dim3(256), lds, ctx->stream, f);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_weighted_median_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *guide, int Cg, float sigma, int k, int y0, int x0,
                            int Ho, int Wo, float *out, float *filtered) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, v && out, DFE_E_ARG, "dfe_weighted_median_f32: NULL tensor");
    if (int rc = dfe_channels_check(ctx, "dfe_weighted_median_f32", C)) return rc;
    if (int rc = dfe_guide_channels_check(ctx, "dfe_weighted_median_f32", Cg)) return rc;
    DFE_REQUIRE(ctx, k >= 1 && k <= kWmedMaxK && (k & 1), DFE_E_ARG, "dfe_weighted_median_f32: k=%d must be odd, 1 .. %d", k, kWmedMaxK);
    if (int rc = dfe_region_check(ctx, "dfe_weighted_median_f32", H, W, y0, x0, Ho, Wo)) return rc;
    DFE_REQUIRE(ctx, dfe_cdiv(H, kWmedTileH) <= 65535, DFE_E_SHAPE, "dfe_weighted_median_f32: H=%d above %d rows", H, 65535 * kWmedTileH);
    const long long HW = (long long)H * W;
    const bool guided = guide && Cg > 0 && sigma > 0.f;
    for (int i = 0; i < 2; ++i) {   // neighbours are read: no output over an input
        const float *o = i ? filtered : out;
        const long long no = i ? HW : C * HW;
        DFE_REQUIRE(ctx, !dfe_overlap(o, no, v, C * HW) && !dfe_overlap(o, no, w, HW) && !(Cg > 0 && dfe_overlap(o, no, guide, Cg * HW)), DFE_E_ARG,
                    "dfe_weighted_median_f32: %s overlaps an input", i ? "filtered" : "out");
    }
    DFE_REQUIRE(ctx, !dfe_overlap(out, C * HW, filtered, HW), DFE_E_ARG, "dfe_weighted_median_f32: out overlaps filtered");
    WmedFrame f{v, w, guided ? guide : nullptr, out, filtered, H, W, y0, x0, Ho, Wo, k, guided ? 1.0f / (sigma * sigma) : 0.f};
    const int cg = guided ? Cg : 0;
    return dfe_dispatch_1to4(C, [&](auto c) {
        constexpr int Cc = decltype(c)::value;
        if (cg == 0) return wmedian_launch<Cc, 0>(ctx, f);
        return dfe_dispatch_1to4(cg, [&](auto g) { return wmedian_launch<Cc, decltype(g)::value>(ctx, f); });
    });
}

}  // extern "C"
