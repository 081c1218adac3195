// census_radial.hip -- the census cost for the radial (polar) matcher (NOT in the reference, whose radial matcher scores learned features by
// the sum of squared differences).  The definition -- signatures of a polar frame with wrap columns, Hamming distance
// down the polar rows, a box whose columns are a ring, the first minimum, the match score, the sub-pixel rule -- is in include/dfe.h and
// restated in numpy in tests/census_radial_ref.py; everything up to the score is integer arithmetic, and the device is tested against that
// bit for bit.
//   census_radial_volume_kernel      the staged route: a thread per cell of the [Ha][W][hWin] volume, any hWin.
//   census_radial_flow_kernel<A, C>  the fused matcher, one launch.  A workgroup is four waves on ONE tile of TY = 8 output rows by
//       4 (16 - (A - 1)) output columns.  A wave's lanes run along the ring: lane l of a 16-lane DPP row holds the column
//       (x0 - A / 2 + its position) mod W, so the ring needs no special case, and the last A - 1 lanes of a row only lend their Hamming
//       distance to the row's horizontal box sum (A - 1 row shifts), as in census_sweep_kernel.  The waves stage frame 1's signatures of
//       the tile's TY + A - 1 + hWin - 1 rows in LDS, one 8-byte slot per lane and row (a lane only ever reads its own column: the LDS
//       carries rows between the waves, nothing between lanes), keep frame 0's signatures of their column in registers, and take the
//       labels in turn: label d goes to wave d % 4, at most four a wave (hWin <= 16).  Per label a lane walks down its column once -- one
//       LDS read, an xor and two popcounts per channel and row -- sums down in registers and across by row shifts, and keeps the TY costs
//       in registers indexed by unrolled constants.  Then the costs of the tile meet in LDS as floats, [row][column][label] with an odd
//       label pitch: a thread per pixel scans for the first minimum, applies the sub-pixel rule and stores flow, best and match, and the
//       volume leaves as whole lines of the tile's columns times hWin contiguous floats.
//   census_radial_score_kernel       match = the census score of the raw cost at a chosen label (the one call's semi-global route).
#include "dfe_internal.h"
#include "subpixel_offset.h"

namespace {

typedef unsigned long long u64;

constexpr int kCrWaves = 4;                   // waves of a workgroup: one tile, the labels dealt among them
constexpr int kCrLabels = 4;                  // labels a wave takes at the most: hWin <= kCrWaves kCrLabels
constexpr int kCrTy = 8;                      // output rows of a workgroup (measured at three channels against 4: 4 to 19 % less time)

struct CrGeom {
    const u64 *s0, *s1;    // [C][Hp][W]
    int C, Hp, W, hWin, agg, Ha;
};

__global__ __launch_bounds__(256) void census_radial_volume_kernel(const CrGeom g, float *__restrict__ out) {
    const long long n = (long long)g.Ha * g.W * g.hWin;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int d = (int)(e % g.hWin);
        const int p = (int)(e / g.hWin);
        const int y = p / g.W, x = p - y * g.W;
        int cost = 0;
        for (int v = 0; v < g.agg; ++v) {
            int xx = x + v - g.agg / 2;              // (agg <= W: one wrap either way)
            xx = xx < 0 ? xx + g.W : (xx >= g.W ? xx - g.W : xx);
            for (int c = 0; c < g.C; ++c) {
                const u64 *__restrict__ a = g.s0 + ((long long)c * g.Hp + y) * g.W + xx;
                const u64 *__restrict__ b = g.s1 + ((long long)c * g.Hp + y + d) * g.W + xx;
                for (int u = 0; u < g.agg; ++u) cost += __popcll(a[(long long)u * g.W] ^ b[(long long)u * g.W]);
            }
        }
        out[e] = (float)cost;
    }
}

struct CrFlow {
    CrGeom g;
    int rows;              // rows of frame 1 a tile stages: TY + agg - 1 + hWin - 1
    int hp;                // label pitch of the cost tile: hWin | 1
    float den;             // nbits C agg^2
    int subpixel, zero_last;
    float *vol;            // [Ha][W][hWin] or NULL
    float *flow;           // [Ha][W]
    float *best, *match;   // [Ha][W], each may be NULL
};

// lane j: lane j + n's v; past the end of the 16-lane row: 0
__device__ __forceinline__ int cr_row_shl(int v, int n) {
    switch (n) {
    case 1: return __builtin_amdgcn_update_dpp(0, v, 0x101, 0xf, 0xf, true);
    case 2: return __builtin_amdgcn_update_dpp(0, v, 0x102, 0xf, 0xf, true);
    case 3: return __builtin_amdgcn_update_dpp(0, v, 0x103, 0xf, 0xf, true);
    default: return __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0xf, true);
    }
}

template <int A, int C>
__global__ __launch_bounds__(kCrWaves * 64) void census_radial_flow_kernel(const CrFlow a) {
#pragma clang fp contract(off)
    extern __shared__ u64 cr_lds[];              // [C][rows][64]: frame 1's signatures of the tile's rows; then the tile's costs
    constexpr int TY = kCrTy;                    // output rows of the workgroup
    constexpr int R = TY + A - 1;                // Hamming rows a lane walks
    constexpr int V = 16 - (A - 1);              // output columns of a 16-lane row
    constexpr int TX = 4 * V;                    // output columns of the workgroup
    const CrGeom &g = a.g;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform: the label loop and its branches run on the scalar unit)
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int xi = (lane >> 4) * V + (lane & 15);                        // this lane's position along the tile (a lending lane's may pass TX)
    int col = (x0 + xi - A / 2) % g.W;                                   // ... and its column on the ring
    col = col < 0 ? col + g.W : col;

    // frame 0's signatures of this lane's column (a row beyond the plane repeats the last one: it reaches no pixel that is stored)
    u64 s0[C][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int yy = y0 + r < g.Hp ? y0 + r : g.Hp - 1;
#pragma unroll
        for (int c = 0; c < C; ++c) s0[c][r] = g.s0[((long long)c * g.Hp + yy) * g.W + col];
    }
    for (int c = 0; c < C; ++c)
        for (int ry = wave; ry < a.rows; ry += kCrWaves) {
            const int gy = y0 + ry < g.Hp ? y0 + ry : g.Hp - 1;
            cr_lds[(c * a.rows + ry) * 64 + lane] = g.s1[((long long)c * g.Hp + gy) * g.W + col];
        }
    __syncthreads();

    int cost[kCrLabels][TY];
#pragma unroll
    for (int i = 0; i < kCrLabels; ++i) {
        const int d = wave + kCrWaves * i;       // (wave-uniform)
        if (d < g.hWin) {
            const u64 *p = cr_lds + d * 64 + lane;
            int h[R];                            // Hamming distance summed over the channels
#pragma unroll
            for (int r = 0; r < R; ++r) {
                h[r] = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) h[r] += __popcll(s0[c][r] ^ p[(c * a.rows + r) * 64]);
            }
#pragma unroll
            for (int t = 0; t < TY; ++t) {       // the box: down first (TY sums), then across (the row shifts of TY rows, not of R)
                int vs = h[t];
#pragma unroll
                for (int u = 1; u < A; ++u) vs += h[t + u];
                int cs = vs;
#pragma unroll
                for (int v = 1; v < A; ++v) cs += cr_row_shl(vs, v);
                cost[i][t] = cs;
            }
        } else {
#pragma unroll
            for (int t = 0; t < TY; ++t) cost[i][t] = 0;
        }
    }

    // the tile's costs meet in LDS: [TY][TX][hp] floats, hp odd -- a wave's writes of one label and a pixel's scan both go bank by bank
    __syncthreads();                             // every wave has read its labels' rows
    float *tile = (float *)cr_lds;
    if ((lane & 15) < V) {
#pragma unroll
        for (int i = 0; i < kCrLabels; ++i) {
            const int d = wave + kCrWaves * i;
            if (d < g.hWin) {
#pragma unroll
                for (int t = 0; t < TY; ++t) tile[(t * TX + xi) * a.hp + d] = (float)cost[i][t];
            }
        }
    }
    __syncthreads();

    // a thread per pixel: the first minimum by a strict scan from 0, the sub-pixel rule of radial_refine_subpixel_kernel, the score
    for (int item = threadIdx.x; item < TY * TX; item += kCrWaves * 64) {
        const int t = item / TX, px = item - t * TX;
        const int y = y0 + t, x = x0 + px;
        if (y >= g.Ha || x >= g.W) continue;
        const float *c = tile + item * a.hp;
        float b = c[0];
        int bi = 0;
        for (int d = 1; d < g.hWin; ++d) {
            const float v = c[d];
            if (v < b) { b = v; bi = d; }
        }
        float f = (float)bi;
        if (a.subpixel && bi >= 1 && bi + 1 < g.hWin) f = (float)bi + subpixel_offset(true, c[bi - 1], b, c[bi + 1]);
        const long long o = (long long)y * g.W + x;
        a.flow[o] = (a.zero_last && y == g.Ha - 1) ? 0.f : f;
        if (a.best) a.best[o] = b;
        if (a.match) a.match[o] = 1.0f - b / a.den;
    }
    if (a.vol) {                                 // whole lines: the tile's columns of a row are ncol hWin contiguous floats
        const int ncol = g.W - x0 < TX ? g.W - x0 : TX;
        const int n = ncol * g.hWin;
        for (int t = 0; t < TY; ++t) {
            const int y = y0 + t;                // (uniform)
            if (y >= g.Ha) break;
            float *dst = a.vol + ((long long)y * g.W + x0) * g.hWin;
            for (int s = threadIdx.x; s < n; s += kCrWaves * 64) {
                const int px = s / g.hWin, d = s - px * g.hWin;
                dst[s] = tile[(t * TX + px) * a.hp + d];
            }
        }
    }
}

// match[p] = 1 - vol[p][label[p]] / den, label = the integer flow (a whole number in 0 .. hWin - 1 as float)
__global__ __launch_bounds__(256) void census_radial_score_kernel(const float *__restrict__ vol, const float *__restrict__ flow, long long P, int hWin, float den,
                                                                  float *__restrict__ match) {
#pragma clang fp contract(off)
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < P; e += (long long)gridDim.x * blockDim.x) {
        int bi = (int)flow[e];
        bi = bi < 0 ? 0 : (bi > hWin - 1 ? hWin - 1 : bi);
        match[e] = 1.0f - vol[e * hWin + bi] / den;
    }
}

// the checks the three entries share, and the geometry behind them
int cr_geom(dfe_ctx *ctx, const char *fn, int C, int Hp, int W, int hWin, int agg, CrGeom *g) {
    DFE_REQUIRE(ctx, C >= 1 && C <= 4, DFE_E_ARG, "%s: C=%d channels (1 .. 4)", fn, C);
    DFE_REQUIRE(ctx, agg == 1 || agg == 3 || agg == 5, DFE_E_ARG, "%s: agg=%d must be 1, 3 or 5", fn, agg);
    DFE_REQUIRE(ctx, hWin >= 1, DFE_E_ARG, "%s: hWin=%d", fn, hWin);
    DFE_REQUIRE(ctx, Hp >= 1 && W >= 1 && Hp <= 32768 && W <= 32768, DFE_E_SHAPE, "%s: %dx%d patch positions (1 .. 32768 each)", fn, Hp, W);
    DFE_REQUIRE(ctx, agg <= W, DFE_E_ARG, "%s: agg=%d on a ring of %d columns", fn, agg, W);
    DFE_REQUIRE(ctx, hWin <= Hp, DFE_E_SHAPE, "%s: hWin=%d on %d rows of patch positions", fn, hWin, Hp);
    g->C = C; g->Hp = Hp; g->W = W; g->hWin = hWin; g->agg = agg;
    g->Ha = Hp - hWin + 1 - agg + 1;
    DFE_REQUIRE(ctx, g->Ha >= 1, DFE_E_SHAPE, "%s: %d rows of patch positions leave no row for a window of %d summed over %d rows", fn, Hp, hWin, agg);
    return DFE_OK;
}

int cr_flow_check(dfe_ctx *ctx, const char *fn, int nbits, int hWin) {
    DFE_REQUIRE(ctx, nbits >= 1 && nbits <= 63, DFE_E_ARG, "%s: nbits=%d (1 .. 63: the patch's cells less its centre)", fn, nbits);
    DFE_REQUIRE(ctx, hWin == 15 || hWin == 12 || hWin == 8 || hWin == 16, DFE_E_UNSUPPORTED,
                "%s: hWin %d has no instantiation (8, 12, 15, 16); use dfe_census_radial_cost_volume_f32 + dfe_argbest_center + dfe_radial_refine_subpixel_f32",
                fn, hWin);
    return DFE_OK;
}

int cr_volume_run(dfe_ctx *ctx, const CrGeom &g, float *out) {
    DfeProfScope prof(ctx);
    const long long n = (long long)g.Ha * g.W * g.hWin;
    hipLaunchKernelGGL(census_radial_volume_kernel, dim3((unsigned)dfe_grid1d(n, 256, 256 * 256)), dim3(256), 0, ctx->stream, g, out);
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "census_radial_volume_kernel";
    return DFE_OK;
}

// the fused matcher behind its checks (cr_geom, cr_flow_check)
int cr_flow_run(dfe_ctx *ctx, const CrGeom &g, int nbits, int subpixel, int zero_last_row, float *volume, float *flow, float *best, float *match) {
    static_assert(16 <= kCrWaves * kCrLabels, "every label of the widest window has a wave");
    CrFlow a{};
    a.g = g;
    const int TY = kCrTy, V = 16 - (g.agg - 1), TX = 4 * V;
    a.rows = TY + g.agg - 1 + g.hWin - 1;
    a.hp = g.hWin | 1;
    a.den = (float)(nbits * g.C * g.agg * g.agg);
    a.subpixel = subpixel != 0; a.zero_last = zero_last_row != 0;
    a.vol = volume; a.flow = flow; a.best = best; a.match = match;
    size_t lds = (size_t)8 * g.C * a.rows * 64;                              // 55 296 bytes at the most (4 channels, agg 5, hWin 16)
    const size_t tile = (size_t)TY * TX * a.hp * sizeof(float);              // 34 816 at the most (agg 1, hWin 16)
    if (lds < tile) lds = tile;
    const dim3 grid((unsigned)dfe_cdiv(g.W, TX), (unsigned)dfe_cdiv(g.Ha, TY)), block(kCrWaves * 64);
    DfeProfScope prof(ctx);
#define DFE_CR_FLOW(AA, CC) hipLaunchKernelGGL((census_radial_flow_kernel<AA, CC>), grid, block, lds, ctx->stream, a)
#define DFE_CR_FLOW_C(AA)                                          \
    switch (g.C) {                                                 \
    case 1: DFE_CR_FLOW(AA, 1); break;                             \
    case 2: DFE_CR_FLOW(AA, 2); break;                             \
    case 3: DFE_CR_FLOW(AA, 3); break;                             \
    default: DFE_CR_FLOW(AA, 4); break;                            \
    }
    if (g.agg == 1) { DFE_CR_FLOW_C(1) }
    else if (g.agg == 3) { DFE_CR_FLOW_C(3) }
    else { DFE_CR_FLOW_C(5) }
#undef DFE_CR_FLOW_C
#undef DFE_CR_FLOW
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "census_radial_flow_kernel";
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_census_radial_cost_volume_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int W, int hWin, int agg, float *out) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_census_radial_cost_volume_f32";
    DFE_REQUIRE(ctx, sig0 && sig1 && out, DFE_E_ARG, "%s: NULL tensor", fn);
    CrGeom g{};
    const int rc = cr_geom(ctx, fn, C, Hp, W, hWin, agg, &g);
    if (rc) return rc;
    g.s0 = (const u64 *)sig0; g.s1 = (const u64 *)sig1;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    return cr_volume_run(ctx, g, out);
}

int dfe_census_radial_flow_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int W, int nbits, int hWin, int agg, int subpixel,
                               int zero_last_row, float *volume, float *flow, float *best, float *match) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_census_radial_flow_f32";
    DFE_REQUIRE(ctx, sig0 && sig1 && flow, DFE_E_ARG, "%s: NULL tensor", fn);
    CrGeom g{};
    int rc = cr_geom(ctx, fn, C, Hp, W, hWin, agg, &g);
    if (rc) return rc;
    rc = cr_flow_check(ctx, fn, nbits, hWin);
    if (rc) return rc;
    g.s0 = (const u64 *)sig0; g.s1 = (const u64 *)sig1;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    return cr_flow_run(ctx, g, nbits, subpixel, zero_last_row, volume, flow, best, match);
}

int dfe_census_radial_flow_depth_pair_f32(dfe_ctx *ctx, const dfe_census_radial_params *p, const float *prev, const float *cur, double e2x, double e2y,
                                          float P1, float P2, unsigned paths, int ring, int subpixel, float *volume, float *agg_volume, float *polar_flow,
                                          float *match, float *cart_flow, float *depth, float *conf) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_census_radial_flow_depth_pair_f32";
    DFE_REQUIRE(ctx, p && prev && cur, DFE_E_ARG, "%s: NULL argument", fn);
    DFE_REQUIRE(ctx, p->hImg > 0 && p->wImg > 0 && p->hInput > 0 && p->wInput > 0 && p->alpha_polar > 0 && p->kinfty > 0, DFE_E_ARG, "%s: bad parameter block",
                fn);
    DFE_REQUIRE(ctx, p->kh >= 3 && p->kw >= 3 && (p->kh & 1) && (p->kw & 1) && (long long)p->kh * p->kw <= 64, DFE_E_ARG,
                "%s: patch %dx%d: odd sides of at least 3 with at most 64 cells expected", fn, p->kh, p->kw);
    const int H = p->hInput, W = p->wInput, nbits = p->kh * p->kw - 1;
    DFE_REQUIRE(ctx, H <= 32768 && W <= 32768 && p->hImg <= 32768 && p->wImg <= 32768, DFE_E_SHAPE, "%s: frames %dx%d, polar %dx%d (up to 32768 a side)", fn,
                p->hImg, p->wImg, H, W);
    DFE_REQUIRE(ctx, H >= p->kh, DFE_E_SHAPE, "%s: polar height %d below the patch's %d rows", fn, H, p->kh);
    CrGeom g{};
    int rc = cr_geom(ctx, fn, p->C, H - p->kh + 1, W, p->hWin, p->agg, &g);
    if (rc) return rc;
    rc = cr_flow_check(ctx, fn, nbits, p->hWin);
    if (rc) return rc;
    // the radial path's geometry with the census patch and the box in the filter stack's place
    const int kH2 = p->kh + p->agg - 1;
    dfe_radial_params rp{};
    rp.hImg = p->hImg; rp.wImg = p->wImg; rp.hInput = H; rp.wInput = W; rp.hWin = p->hWin; rp.kH2 = kH2;
    int hm, hOut, wOut;
    DFE_REQUIRE(ctx, dfe_radial_out_shape(&rp, &hm, &hOut, &wOut) == DFE_OK && hm == g.Ha && hOut > 0 && wOut > 0, DFE_E_SHAPE,
                "%s: polar height %d too small for patch %d + box %d + window %d", fn, H, p->kh, p->agg, p->hWin);
    const int lpad = (p->kw - 1) / 2, rpad = (p->kw - 1) - lpad;
    DFE_REQUIRE(ctx, rpad <= W && W + lpad + rpad <= 32768, DFE_E_SHAPE, "%s: wInput %d with %d wrap columns (each at most wInput, 32768 in all)", fn, W,
                lpad + rpad);
    const bool sg = paths != 0;
    if (sg) {
        rc = dfe_sgm_check(ctx, fn, hm, W, p->hWin, P1, P2, paths, ring);
        if (rc) return rc;
        DFE_REQUIRE(ctx, !volume || agg_volume != volume, DFE_E_ARG, "%s: agg_volume must not be the volume", fn);
    } else {
        DFE_REQUIRE(ctx, !agg_volume, DFE_E_ARG, "%s: agg_volume without paths: there is no aggregate", fn);
    }
    // the aggregate is stored where it is read again: by the caller, or by the refinement of its minimum
    const bool sg_keep = sg && (agg_volume || subpixel);
    const int Wp = W + lpad + rpad;
    const size_t n_pol = (size_t)p->C * H * Wp, n_sig = (size_t)p->C * g.Hp * W, n_il = (size_t)p->hImg * p->wImg, n_vol = (size_t)hm * W * p->hWin;
    DfeRadialWarpBufs wb{};
    u64 *sig0, *sig1;
    float *pflow, *svol, *sagg, *swork;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        wb.pol0 = c.take<float>(n_pol); wb.pol1 = c.take<float>(n_pol);
        wb.rt = c.take<float>(H); wb.sn = c.take<double>(W); wb.cs = c.take<double>(W);
        wb.i0 = c.take<float4>(n_il); wb.i1 = c.take<float4>(n_il);
        sig0 = c.take<u64>(n_sig); sig1 = c.take<u64>(n_sig);
        pflow = c.take<float>((size_t)hm * W);
        svol = c.take<float>(sg && !volume ? n_vol : 0);                   // the aggregation's volume and aggregate, where the caller keeps
        sagg = c.take<float>(sg_keep && !agg_volume ? n_vol : 0);          // neither,
        swork = c.take<float>(sg ? dfe_sgm_work_planes(paths, sg_keep) * n_vol : 0);   // and its directions' planes
    });
    if (rc) return rc;
    if (polar_flow) pflow = polar_flow;
    g.s0 = sig0; g.s1 = sig1;

    const double rmax = dfe_radial_rmax(p->hImg, p->wImg, e2x, e2y);
    {   // 1. both frames to polar, 2. their signatures
        DfeStageScope st(ctx, DFE_STAGE_FILTER);
        rc = dfe_radial_warp_pair(ctx, prev, cur, p->C, p->hImg, p->wImg, H, W, lpad, Wp, p->alpha_polar, e2x, e2y, rmax, wb);
        if (rc) return rc;
        rc = dfe_census_transform_f32(ctx, wb.pol0, p->C, H, Wp, p->kh, p->kw, (uint64_t *)sig0);
        if (rc) return rc;
        rc = dfe_census_transform_f32(ctx, wb.pol1, p->C, H, Wp, p->kh, p->kw, (uint64_t *)sig1);
        if (rc) return rc;
    }
    {   // 3. the matcher
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        if (!sg) {
            rc = cr_flow_run(ctx, g, nbits, subpixel, p->zero_last_row, volume, pflow, nullptr, match);
            if (rc) return rc;
        } else {   // the matcher for its volume (its own arg-min is overwritten), the aggregate and its first minimum, the score, the refinement, the last row
            float *vol = volume ? volume : svol, *abuf = agg_volume ? agg_volume : sagg;   // (abuf: NULL unless sg_keep)
            rc = cr_flow_run(ctx, g, nbits, 0, 0, vol, pflow, nullptr, nullptr);
            if (rc) return rc;
            rc = dfe_sgm_run(ctx, vol, hm, W, p->hWin, P1, P2, paths, ring, swork, abuf, pflow);
            if (rc) return rc;
            if (match) {
                hipLaunchKernelGGL(census_radial_score_kernel, dim3(dfe_grid1d((long long)hm * W)), dim3(256), 0, ctx->stream, vol, pflow, (long long)hm * W,
                                   p->hWin, (float)(nbits * p->C * p->agg * p->agg), match);
                DFE_LAUNCH_CHECK(ctx);
            }
            if (subpixel) {
                rc = dfe_radial_refine_run(ctx, abuf, pflow, (long long)hm * W, p->hWin, pflow);
                if (rc) return rc;
            }
            if (p->zero_last_row) DFE_HIP(ctx, hipMemsetAsync(pflow + (size_t)(hm - 1) * W, 0, (size_t)W * sizeof(float), ctx->stream));
        }
    }
    {   // 4. polar flow -> cartesian -> depth
        DfeStageScope st(ctx, DFE_STAGE_EXTRACT);
        rc = dfe_radial_p2c_depth(ctx, pflow, p->hImg, p->wImg, H, W, hm, kH2, p->hWin, p->alpha_polar, p->kinfty, e2x, e2y, rmax, hOut, wOut, cart_flow, depth,
                                  conf);
        if (rc) return rc;
    }
    ctx->last_kernel = "census_radial_flow_kernel";
    return DFE_OK;
}

}  // extern "C"
