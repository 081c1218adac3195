// census.hip -- the census matching cost: an exposure-robust single-scale matcher (NOT in the reference, whose raw-frame matchers all
// score by the sum of squared differences).  The definition -- signature, Hamming distance, box aggregation, the
// first minimum with the centre rule, the match score, the paste -- is in include/dfe.h and restated in numpy in tests/census_ref.py;
// everything up to the match score is integer arithmetic, and the device is tested against that bit for bit.
//   census_transform_kernel<T>   a workgroup stages a 4 x 64 tile of patch positions with its halo in LDS (the stored values: floats or
//       bytes), a thread per position compares the kh kw - 1 cells with the centre, row-major.
//   census_volume_kernel         the staged route: a thread per cell of the [Ha][Wa][hWin][wWin] volume, lanes along dx.
//   census_sweep_kernel<A, C>    the fused route, no volume.  A wave's lanes run along x, each 16-lane DPP row on 16 - (A - 1) output
//       columns of its own (the last A - 1 lanes of a row only lend their Hamming distance to the row's horizontal box sum, which is
//       A - 1 row shifts).  A workgroup is four waves on ONE tile of TY = 8 (4 from three channels on) output rows: every lane keeps
//       frame 0's signatures of its TY + A - 1 rows in registers, the workgroup stages frame 1's signatures for a band of window rows
//       (and, for windows wider than some 70 cells, of window columns) in LDS, at most 40 KB in rows of a constant pitch, and the
//       band's classes are dealt to the waves in turn -- a VGA frame has only some 500 tiles, and a wave alone on its SIMD issues an
//       instruction every four or five cycles.  A lane walks down its column once per class: one 8-byte LDS read, an xor and a
//       popcount per channel and row, the box sums, and min() on the key (cost << 11 | class), which IS the first minimum in class
//       order whatever order the classes come in.  The centre class's cost is kept for the tie rule.  At the end the waves' keys
//       meet in LDS.  Plain vector stores, no atomics.
#include "dfe_internal.h"
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int kCtTy = 4, kCtTx = 64;          // the transform's tile of patch positions
constexpr int kCtTile = 24 * 84;              // (kCtTy + kh - 1) (kCtTx + kw - 1) <= this for every odd kh, kw >= 3 with kh kw <= 64
constexpr int kNW = 4;                        // waves of a workgroup of the sweep: one tile, the classes dealt among them
constexpr int kPitch = 128;                   // signatures of an LDS row of the sweep (a constant: a lane's row offsets are immediates)
constexpr int kSweepLds = 40 * 1024;          // bytes of LDS a workgroup of the sweep stages into at most: four workgroups a CU
constexpr int census_ty(int C) { return C <= 2 ? 8 : 4; }   // output rows of a workgroup (fewer where the channels fill the registers)

template <class T>
__global__ __launch_bounds__(256) void census_transform_kernel(const T *__restrict__ I, int H, int W, int kh, int kw, int Hp, int Wp,
                                                               u64 *__restrict__ sig) {
    __shared__ T tile[kCtTile];
    const int c = blockIdx.z, x0 = blockIdx.x * kCtTx, y0 = blockIdx.y * kCtTy;
    const int th = kCtTy + kh - 1, tw = kCtTx + kw - 1;
    const T *__restrict__ src = I + (long long)c * H * W;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int ry = ty; ry < th; ry += 4) {                         // (a cell beyond the frame repeats the last row / column: read by no
        const int gy = y0 + ry < H ? y0 + ry : H - 1;             //  position that is stored)
        for (int rx = tx; rx < tw; rx += 64) {
            const int gx = x0 + rx < W ? x0 + rx : W - 1;
            tile[ry * tw + rx] = src[(long long)gy * W + gx];
        }
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= Wp || y >= Hp) return;
    const int ci = kh / 2, cj = kw / 2;
    const T centre = tile[(ty + ci) * tw + tx + cj];
    u64 bits = 0;
    int b = 0;
    for (int i = 0; i < kh; ++i)
        for (int j = 0; j < kw; ++j) {
            if (i == ci && j == cj) continue;
            bits |= (u64)(tile[(ty + i) * tw + tx + j] < centre) << b;   // strict, on the stored values; false with a NaN on either side
            ++b;
        }
    sig[((long long)c * Hp + y) * Wp + x] = bits;
}

struct CensusGeom {
    const u64 *s0, *s1;    // [C][Hp][Wp]
    int C, Hp, Wp, hWin, wWin, agg, Ha, Wa;
    int oy, ox;            // frame 0's offset: floor((hWin - 1) / 2), floor((wWin - 1) / 2)
};

// the staged route: out[y][x][dy][dx], one thread per cell
__global__ __launch_bounds__(256) void census_volume_kernel(const CensusGeom g, float *__restrict__ out) {
    const int D = g.hWin * g.wWin;
    const long long n = (long long)g.Ha * g.Wa * D;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int cls = (int)(e % D);
        const int p = (int)(e / D);
        const int y = p / g.Wa, x = p - y * g.Wa;
        const int dy = cls / g.wWin, dx = cls - dy * g.wWin;
        int cost = 0;
        for (int c = 0; c < g.C; ++c) {
            const u64 *__restrict__ a = g.s0 + ((long long)c * g.Hp + y + g.oy) * g.Wp + x + g.ox;
            const u64 *__restrict__ b = g.s1 + ((long long)c * g.Hp + y + dy) * g.Wp + x + dx;
            for (int u = 0; u < g.agg; ++u)
                for (int v = 0; v < g.agg; ++v) cost += __popcll(a[(long long)u * g.Wp + v] ^ b[(long long)u * g.Wp + v]);
        }
        out[e] = (float)cost;
    }
}

struct CensusSweep {
    CensusGeom g;
    int dyb, dxb;          // window rows / columns of a band
    int mid0;              // the centre class, 0-based
    float den;             // nbits C agg^2
    long long *idx;        // [Ha][Wa], 1-based; each output may be NULL
    float *best;           // [Ha][Wa]
    float *match, *fy, *fx;   // at [(y + pad_t) pitch + x + pad_l]
    int pitch, pad_t, pad_l;
};

// lane j: lane j + n's v; past the end of the 16-lane row: 0 (bound_ctrl: no move has to zero the destination first)
__device__ __forceinline__ int census_row_shl(int v, int n) {
    switch (n) {
    case 1: return __builtin_amdgcn_update_dpp(0, v, 0x101, 0xf, 0xf, true);
    case 2: return __builtin_amdgcn_update_dpp(0, v, 0x102, 0xf, 0xf, true);
    case 3: return __builtin_amdgcn_update_dpp(0, v, 0x103, 0xf, 0xf, true);
    default: return __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0xf, true);
    }
}

template <int A, int C>
__global__ __launch_bounds__(kNW * 64) void census_sweep_kernel(const CensusSweep a) {
    extern __shared__ u64 census_lds[];          // [C][rows][kPitch]: frame 1's signatures of this band; at the end the waves' keys
    constexpr int TY = census_ty(C);             // output rows of the workgroup
    constexpr int R = TY + A - 1;                // Hamming rows a lane walks
    constexpr int V = 16 - (A - 1);              // output columns of a 16-lane row
    constexpr int TC = 3 * V + 16;               // columns the workgroup spans
    const CensusGeom &g = a.g;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform: the class loop and its branches run on the scalar unit)
    const int xt0 = blockIdx.x * (4 * V), yt0 = blockIdx.y * TY;
    const int lx = (lane >> 4) * V + (lane & 15);
    const int x = xt0 + lx;

    // frame 0's signatures of this lane's column (a position beyond the plane repeats the last one: it reaches no pixel that is stored)
    u64 s0[C][R];
    {
        const int xx = x + g.ox < g.Wp ? x + g.ox : g.Wp - 1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int yy = yt0 + g.oy + r < g.Hp ? yt0 + g.oy + r : g.Hp - 1;
#pragma unroll
            for (int c = 0; c < C; ++c) s0[c][r] = g.s0[((long long)c * g.Hp + yy) * g.Wp + xx];
        }
    }
    unsigned key[TY];
    int cen[TY];
#pragma unroll
    for (int t = 0; t < TY; ++t) { key[t] = 0xffffffffu; cen[t] = -1; }

    for (int dy0 = 0; dy0 < g.hWin; dy0 += a.dyb) {
        const int ndy = g.hWin - dy0 < a.dyb ? g.hWin - dy0 : a.dyb;
        for (int dx0 = 0; dx0 < g.wWin; dx0 += a.dxb) {
            const int ndx = g.wWin - dx0 < a.dxb ? g.wWin - dx0 : a.dxb;
            const int rows = R + ndy - 1, cols = TC + ndx - 1;   // (cols <= kPitch)
            const int plane = rows * kPitch;
            __syncthreads();                     // the band before this one has been read
            for (int c = 0; c < C; ++c)
                for (int ry = wave; ry < rows; ry += kNW) {
                    const int gy = yt0 + dy0 + ry < g.Hp ? yt0 + dy0 + ry : g.Hp - 1;
                    const u64 *__restrict__ src = g.s1 + ((long long)c * g.Hp + gy) * g.Wp;
                    for (int rx = lane; rx < cols; rx += 64) {
                        const int gx = xt0 + dx0 + rx < g.Wp ? xt0 + dx0 + rx : g.Wp - 1;
                        census_lds[c * plane + ry * kPitch + rx] = src[gx];
                    }
                }
            __syncthreads();
            // the band's classes dealt to the waves in turn: class q = dy ndx + dx of the band goes to wave q % kNW
            int dy = 0, dx = wave;
            while (dx >= ndx) { dx -= ndx; ++dy; }
            while (dy < ndy) {
                const u64 *p = census_lds + dy * kPitch + lx + dx;
                int h[R];                        // Hamming distance summed over the channels
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    h[r] = 0;
#pragma unroll
                    for (int c = 0; c < C; ++c) h[r] += __popcll(s0[c][r] ^ p[c * plane + r * kPitch]);
                }
                const int cls = (dy0 + dy) * g.wWin + dx0 + dx;
                const bool centre = cls == a.mid0;   // (wave-uniform)
#pragma unroll
                for (int t = 0; t < TY; ++t) {   // the box: down first (TY sums), then across (the row shifts of TY rows, not of R)
                    int vs = h[t];
#pragma unroll
                    for (int u = 1; u < A; ++u) vs += h[t + u];
                    int cost = vs;
#pragma unroll
                    for (int v = 1; v < A; ++v) cost += census_row_shl(vs, v);
                    const unsigned k = ((unsigned)cost << 11) | (unsigned)cls;
                    key[t] = k < key[t] ? k : key[t];
                    if (centre) cen[t] = cost;
                }
                dx += kNW;
                while (dx >= ndx) { dx -= ndx; ++dy; }
            }
        }
    }

    // the waves' keys and the centre's cost (-1 from the waves that never met the centre) through LDS; wave w finishes rows w, w + kNW, ...
    __syncthreads();
    unsigned *keys = (unsigned *)census_lds;     // [kNW][TY][64], then the centre costs in the same layout
    int *cens = (int *)(keys + kNW * TY * 64);
#pragma unroll
    for (int t = 0; t < TY; ++t) {
        keys[(wave * TY + t) * 64 + lane] = key[t];
        cens[(wave * TY + t) * 64 + lane] = cen[t];
    }
    __syncthreads();
    if ((lane & 15) >= V || x >= g.Wa) return;
    for (int t = wave; t < TY; t += kNW) {
        const int y = yt0 + t;
        if (y >= g.Ha) break;
        unsigned k = keys[t * 64 + lane];
        int ce = cens[t * 64 + lane];
#pragma unroll
        for (int w = 1; w < kNW; ++w) {
            const unsigned ok = keys[(w * TY + t) * 64 + lane];
            const int oc = cens[(w * TY + t) * 64 + lane];
            k = ok < k ? ok : k;
            ce = oc > ce ? oc : ce;
        }
        const int b = (int)(k >> 11);
        int cls = (int)(k & 2047u);
        if (ce == b) cls = a.mid0;               // the centre wins an exact tie with the best
        const long long o = (long long)y * g.Wa + x, op = (long long)(y + a.pad_t) * a.pitch + x + a.pad_l;
        if (a.idx) a.idx[o] = cls + 1;
        if (a.best) a.best[o] = (float)b;
        if (a.match) a.match[op] = 1.0f - (float)b / a.den;
        const int fl = cls / g.wWin;             // dfe_x2yx
        if (a.fy) a.fy[op] = (float)(fl - (g.hWin - 1) / 2);
        if (a.fx) a.fx[op] = (float)(cls - fl * g.wWin - (g.wWin - 1) / 2);
    }
}

// the checks every entry shares, and the geometry behind them
int census_kernel_check(dfe_ctx *ctx, const char *fn, int kh, int kw) {
    DFE_REQUIRE(ctx, kh >= 3 && kw >= 3 && (kh & 1) && (kw & 1) && (long long)kh * kw <= 64, DFE_E_ARG,
                "%s: patch %dx%d: odd sides of at least 3 with at most 64 cells expected", fn, kh, kw);
    return DFE_OK;
}

int census_geom(dfe_ctx *ctx, const char *fn, int C, int Hp, int Wp, int hWin, int wWin, int agg, CensusGeom *g) {
    DFE_REQUIRE(ctx, C >= 1 && C <= 4, DFE_E_ARG, "%s: C=%d channels (1 .. 4)", fn, C);
    DFE_REQUIRE(ctx, agg == 1 || agg == 3 || agg == 5, DFE_E_ARG, "%s: agg=%d must be 1, 3 or 5", fn, agg);
    DFE_REQUIRE(ctx, hWin >= 1 && wWin >= 1, DFE_E_ARG, "%s: window %dx%d", fn, hWin, wWin);
    DFE_REQUIRE(ctx, (long long)hWin * wWin <= kDfeMaxWindowCells, DFE_E_UNSUPPORTED, "%s: window %dx%d has more than %d cells", fn, hWin, wWin,
                kDfeMaxWindowCells);
    DFE_REQUIRE(ctx, Hp >= 1 && Wp >= 1 && Hp <= 32768 && Wp <= 32768, DFE_E_SHAPE, "%s: %dx%d patch positions (1 .. 32768 each)", fn, Hp, Wp);
    g->C = C; g->Hp = Hp; g->Wp = Wp; g->hWin = hWin; g->wWin = wWin; g->agg = agg;
    g->Ha = Hp - hWin + 1 - agg + 1;
    g->Wa = Wp - wWin + 1 - agg + 1;
    g->oy = (hWin - 1) / 2; g->ox = (wWin - 1) / 2;
    DFE_REQUIRE(ctx, g->Ha >= 1 && g->Wa >= 1, DFE_E_SHAPE, "%s: %dx%d patch positions leave no pixel for a %dx%d window summed over %dx%d", fn, Hp, Wp, hWin,
                wWin, agg, agg);
    return DFE_OK;
}

template <class T> int census_transform_run(dfe_ctx *ctx, const T *I, int C, int H, int W, int kh, int kw, u64 *sig) {
    const int Hp = H - kh + 1, Wp = W - kw + 1;
    hipLaunchKernelGGL(census_transform_kernel<T>, dim3((unsigned)dfe_cdiv(Wp, kCtTx), (unsigned)dfe_cdiv(Hp, kCtTy), (unsigned)C), dim3(256), 0, ctx->stream,
                       I, H, W, kh, kw, Hp, Wp, sig);
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "census_transform_kernel";
    return DFE_OK;
}

template <class T> int census_transform_entry(dfe_ctx *ctx, const char *fn, const T *I, int C, int H, int W, int kh, int kw, uint64_t *sig) {
    DFE_REQUIRE(ctx, I && sig, DFE_E_ARG, "%s: NULL tensor", fn);
    int rc = census_kernel_check(ctx, fn, kh, kw);
    if (rc) return rc;
    DFE_REQUIRE(ctx, C >= 1 && C <= 4, DFE_E_ARG, "%s: C=%d channels (1 .. 4)", fn, C);
    DFE_REQUIRE(ctx, H >= kh && W >= kw && H <= 32768 && W <= 32768, DFE_E_SHAPE, "%s: frame %dx%d for a %dx%d patch (up to 32768 a side)", fn, H, W, kh, kw);
    DfeStageScope st(ctx, DFE_STAGE_FILTER);
    return census_transform_run(ctx, I, C, H, W, kh, kw, (u64 *)sig);
}

// the sweep's launch shape: the band of window rows and columns whose signatures fit kSweepLds
struct CensusPlan { int dyb, dxb; size_t lds; };
CensusPlan census_plan(const CensusGeom &g) {
    const int TY = census_ty(g.C), R = TY + g.agg - 1;
    const int V = 16 - (g.agg - 1), TC = 3 * V + 16;
    CensusPlan p;
    p.dxb = g.wWin < kPitch - TC + 1 ? g.wWin : kPitch - TC + 1;
    const int rows = kSweepLds / (8 * g.C * kPitch);        // 10 at the least (4 channels), R is 8 there
    const int fit = rows - R + 1;                           // window rows that fit
    const int nb = dfe_cdiv(g.hWin, fit);                   // ... in bands of equal height
    p.dyb = dfe_cdiv(g.hWin, nb);
    p.lds = (size_t)8 * g.C * (R + p.dyb - 1) * kPitch;
    const size_t merge = (size_t)2 * kNW * TY * 64 * sizeof(int);   // the keys and centre costs at the end
    if (p.lds < merge) p.lds = merge;
    return p;
}

int census_sweep_run(dfe_ctx *ctx, const CensusGeom &g, int nbits, int64_t *idx, float *best, float *match, float *fy, float *fx, int pitch, int pad_t,
                     int pad_l) {
    CensusSweep a{};
    a.g = g;
    const CensusPlan p = census_plan(g);
    a.dyb = p.dyb; a.dxb = p.dxb;
    a.mid0 = dfe_window_middle(g.hWin, g.wWin) - 1;
    a.den = (float)(nbits * g.C * g.agg * g.agg);
    a.idx = (long long *)idx; a.best = best; a.match = match; a.fy = fy; a.fx = fx;
    a.pitch = pitch; a.pad_t = pad_t; a.pad_l = pad_l;
    const int V = 16 - (g.agg - 1);
    const dim3 grid((unsigned)dfe_cdiv(g.Wa, 4 * V), (unsigned)dfe_cdiv(g.Ha, census_ty(g.C))), block(kNW * 64);
    DfeProfScope prof(ctx);
#define DFE_CENSUS_SWEEP(AA, CC) hipLaunchKernelGGL((census_sweep_kernel<AA, CC>), grid, block, p.lds, ctx->stream, a)
#define DFE_CENSUS_SWEEP_C(AA)                                      \
    switch (g.C) {                                                  \
    case 1: DFE_CENSUS_SWEEP(AA, 1); break;                         \
    case 2: DFE_CENSUS_SWEEP(AA, 2); break;                         \
    case 3: DFE_CENSUS_SWEEP(AA, 3); break;                         \
    default: DFE_CENSUS_SWEEP(AA, 4); break;                        \
    }
    if (g.agg == 1) { DFE_CENSUS_SWEEP_C(1) }
    else if (g.agg == 3) { DFE_CENSUS_SWEEP_C(3) }
    else { DFE_CENSUS_SWEEP_C(5) }
#undef DFE_CENSUS_SWEEP_C
#undef DFE_CENSUS_SWEEP
    DFE_LAUNCH_CHECK(ctx);
    // how the window was banded, in the kernel's name (tests pin which shapes take which)
    static const char *const names[4] = {"census_sweep_kernel", "census_sweep_kernel, row bands", "census_sweep_kernel, column bands",
                                         "census_sweep_kernel, row and column bands"};
    ctx->last_kernel = names[(p.dyb < g.hWin ? 1 : 0) + (p.dxb < g.wWin ? 2 : 0)];
    return DFE_OK;
}

}  // namespace

// (declared in dfe_internal.h: the one calls of sgm_pick.hip start with the same two steps)
int dfe_census_pair_check(dfe_ctx *ctx, const char *fn, bool tensors, bool depth_pair, int C, int H, int W, int k, int hWin, int wWin, int agg, DfeCensusPair *p) {
    DFE_REQUIRE(ctx, tensors, DFE_E_ARG, "%s: NULL tensor", fn);
    DFE_REQUIRE(ctx, depth_pair, DFE_E_ARG, "%s: depth and depth_conf go together", fn);
    int rc = census_kernel_check(ctx, fn, k, k);
    if (rc) return rc;
    DFE_REQUIRE(ctx, H >= 1 && W >= 1 && H <= 32768 && W <= 32768, DFE_E_SHAPE, "%s: frame %dx%d (1 .. 32768 each)", fn, H, W);
    DFE_REQUIRE(ctx, H >= k && W >= k, DFE_E_SHAPE, "%s: frame %dx%d too small for a %dx%d patch", fn, H, W, k, k);
    CensusGeom g{};
    rc = census_geom(ctx, fn, C, H - k + 1, W - k + 1, hWin, wWin, agg, &g);
    if (rc) return rc;
    *p = {g.Hp, g.Wp, g.Ha, g.Wa, (H - g.Ha) / 2, (W - g.Wa) / 2};   // (the paste: the rule of flow_step.hip)
    return DFE_OK;
}

// (the bytes compare as they are, whatever the scale)
int dfe_census_pair_transforms(dfe_ctx *ctx, const void *I0, const void *I1, bool bytes, int C, int H, int W, int k, uint64_t *sig0, uint64_t *sig1) {
    DfeStageScope st(ctx, DFE_STAGE_FILTER);
    const void *I[2] = {I0, I1};
    uint64_t *sig[2] = {sig0, sig1};
    for (int f = 0; f < 2; ++f) {
        const int rc = bytes ? census_transform_run(ctx, (const uint8_t *)I[f], C, H, W, k, k, (u64 *)sig[f])
                             : census_transform_run(ctx, (const float *)I[f], C, H, W, k, k, (u64 *)sig[f]);
        if (rc) return rc;
    }
    return DFE_OK;
}

namespace {

// the one call behind its device guard
int census_pair(dfe_ctx *ctx, const char *fn, const void *I0, const void *I1, bool bytes, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                float foe_y, float *flow, float *match, float *depth, float *depth_conf) {
    DfeCensusPair p;
    int rc = dfe_census_pair_check(ctx, fn, I0 && I1 && flow && match, (depth == nullptr) == (depth_conf == nullptr), C, H, W, k, hWin, wWin, agg, &p);
    if (rc) return rc;
    CensusGeom g{};
    rc = census_geom(ctx, fn, C, p.Hp, p.Wp, hWin, wWin, agg, &g);   // (checked above: the sweep's form of it)
    if (rc) return rc;
    u64 *sig0 = nullptr, *sig1 = nullptr;
    const size_t n = (size_t)C * g.Hp * g.Wp;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        sig0 = c.take<u64>(n);
        sig1 = c.take<u64>(n);
    });
    if (rc) return rc;
    g.s0 = sig0; g.s1 = sig1;
    rc = dfe_census_pair_transforms(ctx, I0, I1, bytes, C, H, W, k, (uint64_t *)sig0, (uint64_t *)sig1);
    if (rc) return rc;
    {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        rc = census_sweep_run(ctx, g, k * k - 1, nullptr, nullptr, match, flow, flow + (long long)H * W, W, p.pad_t, p.pad_l);
        if (rc) return rc;
    }
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    return dfe_pair_border_depth(ctx, flow, match, H, W, p.pad_t, p.pad_l, g.Ha, g.Wa, foe_x, foe_y, depth, depth_conf);
}

}  // namespace

extern "C" {

int dfe_census_transform_f32(dfe_ctx *ctx, const float *I, int C, int H, int W, int kh, int kw, uint64_t *sig) {
    DFE_ENTER(ctx);
    return census_transform_entry(ctx, "dfe_census_transform_f32", I, C, H, W, kh, kw, sig);
}

int dfe_census_transform_u8(dfe_ctx *ctx, const uint8_t *I, int C, int H, int W, int kh, int kw, uint64_t *sig) {
    DFE_ENTER(ctx);
    return census_transform_entry(ctx, "dfe_census_transform_u8", I, C, H, W, kh, kw, sig);
}

int dfe_census_cost_volume_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int Wp, int hWin, int wWin, int agg, float *out) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, sig0 && sig1 && out, DFE_E_ARG, "dfe_census_cost_volume_f32: NULL tensor");
    CensusGeom g{};
    int rc = census_geom(ctx, "dfe_census_cost_volume_f32", C, Hp, Wp, hWin, wWin, agg, &g);
    if (rc) return rc;
    g.s0 = (const u64 *)sig0; g.s1 = (const u64 *)sig1;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    DfeProfScope prof(ctx);
    const long long n = (long long)g.Ha * g.Wa * hWin * wWin;
    hipLaunchKernelGGL(census_volume_kernel, dim3((unsigned)dfe_grid1d(n, 256, 256 * 256)), dim3(256), 0, ctx->stream, g, out);
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "census_volume_kernel";
    return DFE_OK;
}

int dfe_census_flow_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int Wp, int nbits, int hWin, int wWin, int agg, int64_t *idx,
                        float *best, float *match, float *flow_y, float *flow_x) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, sig0 && sig1, DFE_E_ARG, "dfe_census_flow_f32: NULL signatures");
    DFE_REQUIRE(ctx, nbits >= 1 && nbits <= 63, DFE_E_ARG, "dfe_census_flow_f32: nbits=%d (1 .. 63: the patch's cells less its centre)", nbits);
    CensusGeom g{};
    int rc = census_geom(ctx, "dfe_census_flow_f32", C, Hp, Wp, hWin, wWin, agg, &g);
    if (rc) return rc;
    g.s0 = (const u64 *)sig0; g.s1 = (const u64 *)sig1;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    return census_sweep_run(ctx, g, nbits, idx, best, match, flow_y, flow_x, g.Wa, 0, 0);
}

int dfe_census_flow_depth_pair_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                                   float foe_y, float *flow, float *match, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    return census_pair(ctx, "dfe_census_flow_depth_pair_f32", I0, I1, false, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, flow, match, depth, depth_conf);
}

int dfe_census_flow_depth_pair_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                                  float foe_y, float scale, float *flow, float *match, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, scale > 0, DFE_E_ARG, "dfe_census_flow_depth_pair_u8: scale=%g must be positive", (double)scale);
    return census_pair(ctx, "dfe_census_flow_depth_pair_u8", I0, I1, true, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, flow, match, depth, depth_conf);
}

}  // extern "C"
