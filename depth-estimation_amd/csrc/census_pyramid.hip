// census_pyramid.hip -- the census cost in the pyramid matcher (NOT in the reference, whose pyramid scores raw patches by the sum of
// squared differences).  The definition -- per scale: box down-sample, zero-pad by the receptive field k + a - 1,
// signatures, the aggregated Hamming cost over the maxh x maxw window, (float)cost * beta -- is in include/dfe.h and restated in numpy in
// tests/census_pyramid_ref.py; the cost is an integer and the product one rounded multiply, so the device is tested against that bit for bit.
// The soft-min, the cascade, the ring and the arg-max behind the volumes are multiscale.hip's, unchanged.
//   census_pyramid_sig_kernel<K>       the signatures of every scale and both frames in one launch: blockIdx.y = scale, blockIdx.z = (frame,
//       channel); a workgroup stages a 16 x 64 tile of patch positions with its halo in LDS, as census_transform_kernel stages its 4 x 64,
//       a thread takes four positions of a column from one pass over its K columns, and the bits come in the same order.
//   census_pyramid_volume_kernel<A, C> every scale's 8 x 8-window volume in one launch, the scale from the block index.  A workgroup is
//       four waves on ONE tile of 4 output rows by 4 (16 - (A - 1)) output columns.  A wave's lanes run along x, each 16-lane DPP row on
//       16 - (A - 1) output columns of its own (the last A - 1 lanes only lend their Hamming distance to the row's horizontal box sum, as
//       in census_sweep_kernel).  The waves stage frame 1's signatures of the tile's 4 + A - 1 + 7 rows and its columns' window halo in
//       LDS and keep frame 0's signatures of their column in registers.  The window goes in two halves of 32 classes (4 window rows: 128
//       contiguous bytes of a pixel's 256), each half's classes dealt to the waves, 8 a wave: per class a lane walks down its column
//       once -- one 8-byte LDS read, an xor and two popcounts per channel and row -- sums down in registers and across by row shifts,
//       and leaves (float)cost * beta in an LDS tile [row][class][column].  Then the half leaves as whole 128-byte lines, 16 bytes a lane.
//   census_pyramid_scale_kernel        v *= beta, the last step of the staged route.
#include "dfe_internal.h"
#include <cmath>

namespace {

typedef unsigned long long u64;

constexpr int kCpTy = 16, kCpTx = 64;           // the signature kernel's tile of patch positions
constexpr int kCpPer = kCpTy / 4;               // ... and the positions of a thread: a column of 4
constexpr int kCpWaves = 4;                     // waves of a workgroup of the volume kernel
constexpr int kCpRows = 4;                      // output rows of its tile
constexpr int kCpWin = 8;                       // the window side it is written for

struct CpSig {
    const float *p[2][DFE_MAX_RATIOS];          // padded scale frames [C][Hp][Wp] (frame 0, frame 1)
    u64 *sig[2][DFE_MAX_RATIOS];                // [C][Hp - k + 1][Wp - k + 1]
    int Hp[DFE_MAX_RATIOS], Wp[DFE_MAX_RATIOS];
    int ntx[DFE_MAX_RATIOS], nt[DFE_MAX_RATIOS];   // tiles across, tiles in all
    int C;
};

// K: the patch side (3, 5 or 7).  A thread takes kCpPer positions of one column: the K + kCpPer - 1 rows of its K columns go from LDS to
// registers once and serve all of them, and every index below is an unrolled constant.
template <int K>
__global__ __launch_bounds__(256) void census_pyramid_sig_kernel(const CpSig a) {
    constexpr int TH = kCpTy + K - 1, TW = kCpTx + K - 1, CI = K / 2, NR = kCpPer + K - 1;
    __shared__ float tile[TH * TW];
    const int s = blockIdx.y;
    if ((int)blockIdx.x >= a.nt[s]) return;      // (uniform: a coarser scale has fewer tiles than the finest)
    const int f = blockIdx.z / a.C, c = blockIdx.z - f * a.C;
    const int H = a.Hp[s], W = a.Wp[s], Hg = H - K + 1, Wg = W - K + 1;
    const int by = blockIdx.x / a.ntx[s], bx = blockIdx.x - by * a.ntx[s];
    const int x0 = bx * kCpTx, y0 = by * kCpTy;
    const float *__restrict__ src = a.p[f][s] + (long long)c * H * W;
    const int tx = threadIdx.x & 63, tg = threadIdx.x >> 6;
    for (int ry = tg; ry < TH; ry += 4) {                         // (a cell beyond the frame repeats the last row / column: read by no
        const int gy = y0 + ry < H ? y0 + ry : H - 1;             //  position that is stored)
        for (int rx = tx; rx < TW; rx += 64) {
            const int gx = x0 + rx < W ? x0 + rx : W - 1;
            tile[ry * TW + rx] = src[(long long)gy * W + gx];
        }
    }
    __syncthreads();
    const int x = x0 + tx, yb = y0 + tg * kCpPer;
    if (x >= Wg || yb >= Hg) return;
    float v[NR][K];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int j = 0; j < K; ++j) v[r][j] = tile[(tg * kCpPer + r) * TW + tx + j];
    u64 *__restrict__ dst = a.sig[f][s] + ((long long)c * Hg + yb) * Wg + x;
#pragma unroll
    for (int p = 0; p < kCpPer; ++p) {
        const float centre = v[p + CI][CI];
        u64 bits = 0;
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (i == CI && j == CI) continue;
                const int b = i * K + j - (i * K + j > CI * K + CI ? 1 : 0);   // row-major without the centre: census_transform_kernel's order
                bits |= (u64)(v[p + i][j] < centre) << b;                      // strict, on the stored floats
            }
        if (yb + p < Hg) dst[(long long)p * Wg] = bits;
    }
}

struct CpVol {
    const u64 *s0[DFE_MAX_RATIOS], *s1[DFE_MAX_RATIOS];   // [C][Hg][Wg]
    float *out[DFE_MAX_RATIOS];                           // [Hs][Ws][8][8]
    int Hs[DFE_MAX_RATIOS], Ws[DFE_MAX_RATIOS], Hg[DFE_MAX_RATIOS], Wg[DFE_MAX_RATIOS];
    int tile0[DFE_MAX_RATIOS], ntx[DFE_MAX_RATIOS];       // the scale's first block, its tiles across
    int ns;
    float beta;
};

// lane j: lane j + n's v; past the end of the 16-lane row: 0
__device__ __forceinline__ int cp_row_shl(int v, int n) {
    switch (n) {
    case 1: return __builtin_amdgcn_update_dpp(0, v, 0x101, 0xf, 0xf, true);
    case 2: return __builtin_amdgcn_update_dpp(0, v, 0x102, 0xf, 0xf, true);
    case 3: return __builtin_amdgcn_update_dpp(0, v, 0x103, 0xf, 0xf, true);
    default: return __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0xf, true);
    }
}

template <int A, int C>
__global__ __launch_bounds__(kCpWaves * 64) void census_pyramid_volume_kernel(const CpVol a) {
#pragma clang fp contract(off)
    constexpr int TY = kCpRows;                  // output rows of the workgroup
    constexpr int R = TY + A - 1;                // Hamming rows a lane walks
    constexpr int V = 16 - (A - 1);              // output columns of a 16-lane row
    constexpr int TX = 4 * V;                    // output columns of the workgroup
    constexpr int TC = 3 * V + 16;               // columns its lanes span
    constexpr int PITCH = TC + kCpWin;           // signatures of an LDS row: the lanes' columns and the window's 7 more
    constexpr int ROWS = R + kCpWin - 1;         // rows of frame 1 the tile reads
    constexpr int SP = TX + 2;                   // column pitch of the cost tile: 2 mod 8, so that a 16-byte read of 8 pixels' 8 chunks is 2-way at worst
    constexpr int OY = (kCpWin - 1) / 2;         // frame 0's offset in the window, both axes
    __shared__ u64 sig[C * ROWS * PITCH];
    __shared__ float stage[TY * 32 * SP];
    int s = 0;
    for (int i = 1; i < a.ns; ++i)
        if ((int)blockIdx.x >= a.tile0[i]) s = i;               // (uniform)
    const int Hs = a.Hs[s], Ws = a.Ws[s], Hg = a.Hg[s], Wg = a.Wg[s];
    const int bb = blockIdx.x - a.tile0[s];
    const int by = bb / a.ntx[s], bx = bb - by * a.ntx[s];
    const int x0 = bx * TX, y0 = by * TY;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lx = (lane >> 4) * V + (lane & 15);

    // frame 0's signatures of this lane's column (a position beyond the plane repeats the last one: it reaches no pixel that is stored)
    u64 f0[C][R];
    {
        const u64 *__restrict__ g0 = a.s0[s];
        const int xx = x0 + lx + OY < Wg ? x0 + lx + OY : Wg - 1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int yy = y0 + OY + r < Hg ? y0 + OY + r : Hg - 1;
#pragma unroll
            for (int c = 0; c < C; ++c) f0[c][r] = g0[((long long)c * Hg + yy) * Wg + xx];
        }
    }
    {
        const u64 *__restrict__ g1 = a.s1[s];
        for (int c = 0; c < C; ++c)
            for (int ry = wave; ry < ROWS; ry += kCpWaves) {
                const int gy = y0 + ry < Hg ? y0 + ry : Hg - 1;
                const u64 *__restrict__ src = g1 + ((long long)c * Hg + gy) * Wg;
                for (int rx = lane; rx < TC + kCpWin - 1; rx += 64) {
                    const int gx = x0 + rx < Wg ? x0 + rx : Wg - 1;
                    sig[(c * ROWS + ry) * PITCH + rx] = src[gx];
                }
            }
    }
    __syncthreads();

    float *__restrict__ out = a.out[s];
    const bool lends = (lane & 15) >= V;         // a lane that only lends its Hamming distance to its row's box sum
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        // this half's 32 classes dealt to the waves: class q = 4 i + wave of the half, window row q / 8, column q % 8
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int dy = half * 4 + (i >> 1), dx = wave + 4 * (i & 1);
            const u64 *p = sig + dy * PITCH + lx + dx;
            int h[R];                            // Hamming distance summed over the channels
#pragma unroll
            for (int r = 0; r < R; ++r) {
                h[r] = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) h[r] += __popcll(f0[c][r] ^ p[(c * ROWS + r) * PITCH]);
            }
            const int q = (i >> 1) * kCpWin + dx;
#pragma unroll
            for (int t = 0; t < TY; ++t) {       // the box: down first (TY sums), then across (the row shifts of TY rows, not of R)
                int vs = h[t];
#pragma unroll
                for (int u = 1; u < A; ++u) vs += h[t + u];
                int cost = vs;
#pragma unroll
                for (int v = 1; v < A; ++v) cost += cp_row_shl(vs, v);
                if (!lends) stage[(t * 32 + q) * SP + lx] = (float)cost * a.beta;
            }
        }
        __syncthreads();
        // whole lines: 8 lanes store the half's 128 bytes of a pixel, 16 bytes each
#pragma unroll
        for (int it = 0; it < TY * TX * 8 / (kCpWaves * 64); ++it) {
            const int e = it * (kCpWaves * 64) + threadIdx.x;
            const int t = e / (TX * 8), rem = e - t * (TX * 8);
            const int px = rem >> 3, j = rem & 7;
            const int y = y0 + t, x = x0 + px;
            if (y < Hs && x < Ws) {
                const float *sp = stage + (t * 32 + 4 * j) * SP + px;
                const float4 v = make_float4(sp[0], sp[SP], sp[2 * SP], sp[3 * SP]);
                *reinterpret_cast<float4 *>(out + ((long long)y * Ws + x) * (kCpWin * kCpWin) + half * 32 + 4 * j) = v;
            }
        }
        if (half == 0) __syncthreads();          // the tile is free for the second half
    }
}

__global__ __launch_bounds__(256) void census_pyramid_scale_kernel(float *__restrict__ v, long long n, float beta) {
#pragma clang fp contract(off)
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) v[e] = v[e] * beta;
}

int cp_scale_run(dfe_ctx *ctx, float *v, long long n, float beta) {
    hipLaunchKernelGGL(census_pyramid_scale_kernel, dim3((unsigned)dfe_grid1d(n, 256, 256 * 256)), dim3(256), 0, ctx->stream, v, n, beta);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

int cp_volume_run(dfe_ctx *ctx, const DfeCensusPyramid &a) {
    constexpr int TY = kCpRows;
    const int TX = 4 * (16 - (a.agg - 1));
    CpVol v{};
    v.ns = a.ns; v.beta = a.beta;
    long long tiles = 0;
    for (int s = 0; s < a.ns; ++s) {
        v.s0[s] = (const u64 *)a.sig0[s]; v.s1[s] = (const u64 *)a.sig1[s]; v.out[s] = a.cost[s];
        v.Hg[s] = a.Hp[s] - a.k + 1; v.Wg[s] = a.Wp[s] - a.k + 1;
        v.Hs[s] = v.Hg[s] - (kCpWin - 1) - (a.agg - 1); v.Ws[s] = v.Wg[s] - (kCpWin - 1) - (a.agg - 1);
        v.tile0[s] = (int)tiles; v.ntx[s] = dfe_cdiv(v.Ws[s], TX);
        tiles += (long long)v.ntx[s] * dfe_cdiv(v.Hs[s], TY);
    }
    DFE_REQUIRE(ctx, tiles <= 0x7fffffffll, DFE_E_SHAPE, "census pyramid: %lld tiles", tiles);
    const dim3 grid((unsigned)tiles), block(kCpWaves * 64);
    DfeProfScope prof(ctx);
#define DFE_CP_VOL(AA, CC) hipLaunchKernelGGL((census_pyramid_volume_kernel<AA, CC>), grid, block, 0, ctx->stream, v)
#define DFE_CP_VOL_C(AA)                                           \
    switch (a.C) {                                                 \
    case 1: DFE_CP_VOL(AA, 1); break;                              \
    case 2: DFE_CP_VOL(AA, 2); break;                              \
    case 3: DFE_CP_VOL(AA, 3); break;                              \
    default: DFE_CP_VOL(AA, 4); break;                             \
    }
    if (a.agg == 1) { DFE_CP_VOL_C(1) }
    else if (a.agg == 3) { DFE_CP_VOL_C(3) }
    else { DFE_CP_VOL_C(5) }
#undef DFE_CP_VOL_C
#undef DFE_CP_VOL
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "census_pyramid_volume_kernel";
    return DFE_OK;
}

}  // namespace

// (declared in dfe_internal.h: multiscale.hip's plan makes these checks before its own)
int dfe_census_pyramid_check(dfe_ctx *ctx, const char *fn, int C, int k, int agg, float beta) {
    DFE_REQUIRE(ctx, k >= 3 && (k & 1) && k * k <= 64, DFE_E_ARG, "%s: patch %dx%d: an odd side of at least 3 with at most 64 cells expected", fn, k, k);
    DFE_REQUIRE(ctx, C >= 1 && C <= 4, DFE_E_ARG, "%s: C=%d channels (1 .. 4)", fn, C);
    DFE_REQUIRE(ctx, agg == 1 || agg == 3 || agg == 5, DFE_E_ARG, "%s: agg=%d must be 1, 3 or 5", fn, agg);
    DFE_REQUIRE(ctx, beta > 0.f && beta < INFINITY, DFE_E_ARG, "%s: beta=%g must be finite and positive", fn, (double)beta);
    return DFE_OK;
}

bool dfe_census_pyramid_fast(int maxh, int maxw) { return maxh == kCpWin && maxw == kCpWin; }

int dfe_census_pyramid_signatures(dfe_ctx *ctx, const DfeCensusPyramid &a) {
    CpSig g{};
    g.C = a.C;
    int nt_max = 0;
    for (int s = 0; s < a.ns; ++s) {
        g.p[0][s] = a.p0[s]; g.p[1][s] = a.p1[s];
        g.sig[0][s] = (u64 *)a.sig0[s]; g.sig[1][s] = (u64 *)a.sig1[s];
        g.Hp[s] = a.Hp[s]; g.Wp[s] = a.Wp[s];
        g.ntx[s] = dfe_cdiv(a.Wp[s] - a.k + 1, kCpTx);
        g.nt[s] = g.ntx[s] * dfe_cdiv(a.Hp[s] - a.k + 1, kCpTy);
        if (g.nt[s] > nt_max) nt_max = g.nt[s];
    }
    DfeStageScope st(ctx, DFE_STAGE_FILTER);
    DfeProfScope prof(ctx);
    const dim3 grid((unsigned)nt_max, (unsigned)a.ns, (unsigned)(2 * a.C)), block(256);
    if (a.k == 3) hipLaunchKernelGGL(census_pyramid_sig_kernel<3>, grid, block, 0, ctx->stream, g);
    else if (a.k == 5) hipLaunchKernelGGL(census_pyramid_sig_kernel<5>, grid, block, 0, ctx->stream, g);
    else hipLaunchKernelGGL(census_pyramid_sig_kernel<7>, grid, block, 0, ctx->stream, g);
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "census_pyramid_sig_kernel";
    return DFE_OK;
}

int dfe_census_pyramid_volumes(dfe_ctx *ctx, const DfeCensusPyramid &a) {
    if (dfe_census_pyramid_fast(a.maxh, a.maxw)) {
        ctx->ms_census = "census_pyramid_volume_kernel";
        return cp_volume_run(ctx, a);
    }
    // a window without a fast form: the staged kernels, scale by scale
    ctx->ms_census = "census_volume_kernel";
    for (int s = 0; s < a.ns; ++s) {
        const int Hg = a.Hp[s] - a.k + 1, Wg = a.Wp[s] - a.k + 1;
        int rc = dfe_census_cost_volume_f32(ctx, a.sig0[s], a.sig1[s], a.C, Hg, Wg, a.maxh, a.maxw, a.agg, a.cost[s]);
        if (rc) return rc;
        const long long n = (long long)(Hg - a.maxh + 1 - a.agg + 1) * (Wg - a.maxw + 1 - a.agg + 1) * a.maxh * a.maxw;
        rc = cp_scale_run(ctx, a.cost[s], n, a.beta);
        if (rc) return rc;
    }
    return DFE_OK;
}

extern "C" {

int dfe_census_pyramid_scale_volume_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int r, int k, int maxh, int maxw, int agg,
                                        float beta, float *out) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_census_pyramid_scale_volume_f32";
    DFE_REQUIRE(ctx, I0 && I1 && out, DFE_E_ARG, "%s: NULL tensor", fn);
    int rc = dfe_census_pyramid_check(ctx, fn, C, k, agg, beta);
    if (rc) return rc;
    DFE_REQUIRE(ctx, r > 0 && maxh > 0 && maxw > 0 && H > 0 && W > 0, DFE_E_ARG, "%s: bad size", fn);
    DFE_REQUIRE(ctx, (long long)maxh * maxw <= kDfeMaxWindowCells, DFE_E_UNSUPPORTED, "%s: window %dx%d has more than %d cells", fn, maxh, maxw,
                kDfeMaxWindowCells);
    DFE_REQUIRE(ctx, H % r == 0 && W % r == 0, DFE_E_SHAPE, "%s: frame %dx%d is not a multiple of ratio %d", fn, H, W, r);
    const int Hs = H / r, Ws = W / r;
    const int hp = maxh - 1 + k - 1 + agg - 1, wp = maxw - 1 + k - 1 + agg - 1;   // the pyramid's padding for the receptive field k + agg - 1
    DFE_REQUIRE(ctx, H <= 32768 && W <= 32768 && Hs + hp <= 32768 && Ws + wp <= 32768, DFE_E_SHAPE, "%s: frame %dx%d (padded scale up to 32768 a side)", fn, H,
                W);
    const int pt = hp / 2, pl = wp / 2, Hp = Hs + hp, Wp = Ws + wp, Hg = Hp - k + 1, Wg = Wp - k + 1;
    const size_t nd = (size_t)C * Hs * Ws, np = (size_t)C * Hp * Wp, ng = (size_t)C * Hg * Wg;
    float *d, *p;
    uint64_t *sg;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) { d = c.take<float>(2 * nd); p = c.take<float>(2 * np); sg = c.take<uint64_t>(2 * ng); });
    if (rc) return rc;
    {
        DfeStageScope st(ctx, DFE_STAGE_FILTER);
        rc = dfe_pyramid_prep_scale(ctx, I0, I1, C, H, W, r, pl, pt, Hp, Wp, d, p);
        if (rc) return rc;
        rc = dfe_census_transform_f32(ctx, p, C, Hp, Wp, k, k, sg);
        if (rc) return rc;
        rc = dfe_census_transform_f32(ctx, p + np, C, Hp, Wp, k, k, sg + ng);
        if (rc) return rc;
    }
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    rc = dfe_census_cost_volume_f32(ctx, sg, sg + ng, C, Hg, Wg, maxh, maxw, agg, out);
    if (rc) return rc;
    return cp_scale_run(ctx, out, (long long)Hs * Ws * maxh * maxw, beta);
}

int dfe_multiscale_census_flow_pair_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int maxh, int maxw, const int *ratios,
                                        int nratios, int agg, float beta, float *flow, int64_t *idx) {
    DFE_ENTER(ctx);
    return dfe_multiscale_census_pair(ctx, I0, I1, false, C, H, W, k, maxh, maxw, ratios, nratios, agg, beta, flow, idx, "dfe_multiscale_census_flow_pair_f32");
}

int dfe_multiscale_census_flow_pair_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int maxh, int maxw, const int *ratios,
                                       int nratios, int agg, float beta, float *flow, int64_t *idx) {
    DFE_ENTER(ctx);
    return dfe_multiscale_census_pair(ctx, I0, I1, true, C, H, W, k, maxh, maxw, ratios, nratios, agg, beta, flow, idx, "dfe_multiscale_census_flow_pair_u8");
}

}  // extern "C"
