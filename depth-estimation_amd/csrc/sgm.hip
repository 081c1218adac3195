// sgm.hip -- semi-global aggregation (Hirschmueller's path sums) of a cost volume with a one-dimensional label axis: the radial
// matcher's [H][W][D] volume, D <= 32 (NOT in the reference, whose matchers are all winner-takes-all).
// The definition -- directions, the step, the ring, the order of the sum, the first-minimum flow -- is in include/dfe.h and restated
// in numpy in tests/sgm_ref.py; the device is tested against that bit for bit.
//   sgm_path_kernel<LPL>   ONE launch for all the directions asked for (blockIdx.y), each into a plane of its own.  A chain is a
//       sequence of dependent steps of some 60 instructions, and one direction has only H or W chains, 4 to a wave: 320 waves for the
//       1280 columns of the 720p polar image, on 1024 SIMDs.  One direction after the other took 0.17 - 0.21 ms EACH at 720p, every wave
//       alone on its SIMD at one instruction per four or five cycles; side by side the directions share the SIMDs.
//       A LINE is the chain of pixels a path walks: a row for the horizontal directions; for the others the W chains that start on the
//       top (or bottom) row and, on a ring, wind round it -- on the plane a chain that leaves through a side comes back in through the
//       other one and STARTS AGAIN there (L = C), which is the definition's "the predecessor lies outside the plane" for every pixel of
//       the side columns, so every direction has H or W lines of equal length and nothing is ragged.  A line belongs to one 16-lane DPP
//       row, the labels across its lanes (LPL = 1: label = lane, D <= 16; LPL = 2: labels 2 lane and 2 lane + 1, D <= 32), the label
//       axis padded with +Inf cells, which change no bit of a real cell and stay +Inf.  Per step: min_k L by four DPP row steps,
//       L(d -+ 1) by one row shift each (a lane without a neighbour keeps the +Inf it is given as `old`), six more VALU operations,
//       nothing through LDS.  The loads of the next kSgmAhead steps are in flight (a chain's addresses are known from its first step:
//       the walk is SgmCursor of sgm_common.h, which sgm_plane.hip's path kernel shares, as it does the row minimum).
//   guided_sgm_path_kernel<LPL>   the same body with the step's P2 taken from the direction's penalty plane (sgm_penalty.hip; DESIGN.md
//       section 4.38): one value per 16-lane row, fetched with the step's costs through the same look-ahead.
//   sgm_sum_kernel<LPL, FLOW>   agg = ((L_a + L_b) + L_c) + ... in ascending direction order, 16 lanes a pixel as above; the first
//       minimum over the labels by a row reduction on (value, label); the aggregate is stored only if somebody reads it.
#include "sgm_common.h"

namespace {

constexpr int kSgmAhead = 8;   // steps of a line whose loads are in flight

struct SgmJob {
    const float *C;      // [H][W][D]
    float *L[8];         // [H][W][D] each: L of the n directions asked for, in ascending bit order
    int dy[8], dx[8];    // their directions: p's predecessor is p - (dy, dx)
    int n;
    int H, W, D;
    int ring;            // G: 0 = plane
    float P1, P2;
};

__device__ __forceinline__ float sgm_row_shr1(float v, float edge) {   // lane j: lane j - 1's v; lane 0 of the row: edge
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ float sgm_row_shl1(float v, float edge) {   // lane j: lane j + 1's v; lane 15 of the row: edge
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x101, 0xf, 0xf, false));
}

// the body of the two path kernels.  GUIDED: the step's P2 is a cell of the direction's penalty plane (sgm_penalty.hip), one value per
// 16-lane row, fetched with the step's costs through the same look-ahead, so a step's dependent chain keeps its length
template <int LPL, bool GUIDED>
__device__ __forceinline__ void sgm_path_body(const SgmJob &a, const SgmPen *pen) {
#pragma clang fp contract(off)
    const float inf = __builtin_inff();
    const int k = blockIdx.y;                    // which of the directions
    const int dy = a.dy[k], dx = a.dx[k];
    float *__restrict__ out = a.L[k];
    const bool horizontal = dy == 0;
    const int nlines = horizontal ? a.H : a.W;   // lines of this direction
    const int warm = horizontal ? a.ring : 0;    // leading steps of a horizontal line on a ring that are walked and not kept
    const int nsteps = horizontal ? a.W + a.ring : a.H;   // (run in whole groups of kSgmAhead: a short line wastes up to 7 of 8 steps, a row
                                                          //  beyond the last line all of them -- in-bounds loads, no store)
    if ((int)blockIdx.x * 4 >= nlines) return;   // (the grid is sized for the longer side)
    const int lane = threadIdx.x & 15;
    const int line = blockIdx.x * 4 + (int)(threadIdx.x >> 4);
    const bool live = line < nlines;             // a row beyond the last line walks the last line again and stores nothing
    const int ln = live ? line : nlines - 1;
    const int d0 = lane * LPL;
    bool in[LPL];
    int dc[LPL];                                 // a padding lane loads the last real label (and takes +Inf): no load under a branch
#pragma unroll
    for (int j = 0; j < LPL; ++j) {
        in[j] = d0 + j < a.D;
        dc[j] = in[j] ? d0 + j : a.D - 1;
    }

    // the fetch cursor: the pixel of step `fs`, and whether the chain starts (again) there.  Past the last step it stays on the last
    // pixel: the step loop runs whole groups of kSgmAhead steps, and the surplus ones of the last group keep nothing.
    SgmCursor f(dy, dx, ln, a.H, a.W, a.ring);
    int fs = 0;
    float cb[kSgmAhead][LPL];
    int pixb[kSgmAhead];
    bool stb[kSgmAhead];
    float penb[GUIDED ? kSgmAhead : 1];
    const float *__restrict__ pplane = nullptr;
    bool atq = false;
    int qpix = 0;                                // the pixel fetched before this one: the step's predecessor (the first step has none and starts)
    if constexpr (GUIDED) {
        pplane = pen->plane[k];
        atq = pen->atq[k] != 0;
        qpix = f.y * a.W + f.x;
    }
    auto fetch = [&](int slot) {
        const int pix = f.y * a.W + f.x;
        const long long e = (long long)pix * a.D;
#pragma unroll
        for (int j = 0; j < LPL; ++j) cb[slot][j] = a.C[e + dc[j]];
        if constexpr (GUIDED) {
            penb[slot] = pplane[atq ? qpix : pix];
            qpix = pix;
        }
        pixb[slot] = pix;
        stb[slot] = f.start;
        ++fs;
        if (fs < nsteps) f.advance(dy, dx, a.W, a.ring);   // (wave-uniform; integer work only)
    };
#pragma unroll
    for (int u = 0; u < kSgmAhead; ++u) fetch(u);

    float l[LPL];
#pragma unroll
    for (int j = 0; j < LPL; ++j) l[j] = 0.f;
    for (int s = 0; s < nsteps; s += kSgmAhead) {
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u) {
            float c[LPL];
#pragma unroll
            for (int j = 0; j < LPL; ++j) c[j] = in[j] ? cb[u][j] : inf;
            const int pix = pixb[u];
            const bool start = stb[u];
            float P2 = a.P2;
            if constexpr (GUIDED) P2 = penb[u];
            fetch(u);
            // L_r(p, d) = C(p, d) + (min(L(q, d), L(q, d - 1) + P1, L(q, d + 1) + P1, m + P2) - m), m = min_k L(q, k)
            float m = l[0];
            if constexpr (LPL == 2) m = fminf(m, l[1]);
            m = sgm_row_min(m);
            const float far = m + P2;
            float lo[LPL], hi[LPL];              // L(q, d - 1), L(q, d + 1)
            if constexpr (LPL == 1) {
                lo[0] = sgm_row_shr1(l[0], inf);
                hi[0] = sgm_row_shl1(l[0], inf);
            } else {
                lo[0] = sgm_row_shr1(l[1], inf);
                hi[0] = l[1];
                lo[1] = l[0];
                hi[1] = sgm_row_shl1(l[0], inf);
            }
#pragma unroll
            for (int j = 0; j < LPL; ++j) {
                const float t = fminf(fminf(fminf(l[j], lo[j] + a.P1), hi[j] + a.P1), far);
                const float n = c[j] + (t - m);
                l[j] = start ? c[j] : n;
            }
            const bool keep = live && s + u >= warm && s + u < nsteps;
#pragma unroll
            for (int j = 0; j < LPL; ++j)
                if (keep && in[j]) out[(long long)pix * a.D + d0 + j] = l[j];
        }
    }
}

template <int LPL>
__global__ __launch_bounds__(64) void sgm_path_kernel(const SgmJob a) {
    sgm_path_body<LPL, false>(a, nullptr);
}
template <int LPL>
__global__ __launch_bounds__(64) void guided_sgm_path_kernel(const SgmJob a, const SgmPen pen) {
    sgm_path_body<LPL, true>(a, &pen);
}

// agg = the n planes summed in order; flow = its first minimum.  16 lanes a pixel, 16 pixels a block
template <int LPL, bool FLOW>
__global__ __launch_bounds__(256) void sgm_sum_kernel(const SgmJob a, float *__restrict__ agg, float *__restrict__ flow) {
#pragma clang fp contract(off)
    const int P = a.H * a.W;
    const int lane = threadIdx.x & 15;
    const int px = blockIdx.x * 16 + (int)(threadIdx.x >> 4);
    const bool live = px < P;                    // a row beyond the last pixel sums the last pixel again and stores nothing
    const long long e = (long long)(live ? px : P - 1) * a.D;
    const int d0 = lane * LPL;
    float v[LPL];
#pragma unroll
    for (int j = 0; j < LPL; ++j) {
        const bool in = d0 + j < a.D;
        const long long ej = e + (in ? d0 + j : a.D - 1);
        float t = a.L[0][ej];
        for (int k = 1; k < a.n; ++k) t = t + a.L[k][ej];
        v[j] = in ? t : __builtin_inff();
        if (agg && live && in) agg[ej] = t;
    }
    if constexpr (FLOW) {                        // the first minimum: the smallest value, and among equal ones the smallest label
        float b = v[0];
        int bi = d0;
        if constexpr (LPL == 2)
            if (v[1] < b) { b = v[1]; bi = d0 + 1; }
#define DFE_STEP(ctrl)                                                                                                  \
    {                                                                                                                   \
        const float ob = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(b), ctrl, 0xf, 0xf, false));      \
        const int oi = __builtin_amdgcn_update_dpp(0, bi, ctrl, 0xf, 0xf, false);                                       \
        const bool take = (ob < b) | ((ob == b) & (oi < bi));                                                           \
        b = take ? ob : b;                                                                                              \
        bi = take ? oi : bi;                                                                                            \
    }
        DFE_STEP(0x128); DFE_STEP(0x124); DFE_STEP(0x4E); DFE_STEP(0xB1);   // row_ror:8, row_ror:4, quad_perm [2,3,0,1], [1,0,3,2]
#undef DFE_STEP
        if (live && lane == 0) flow[px] = (float)bi;
    }
}

}  // namespace

// planes of H * W * D floats that dfe_sgm_run (and the plane family's jobs) take as `work`: one per direction, unless the only direction
// goes straight to agg
size_t dfe_sgm_work_planes(unsigned paths, bool agg_given) {
    const int n = __builtin_popcount(paths & 255u);
    return n == 1 && agg_given ? 0 : (size_t)n;
}

// The launches of dfe_sgm_aggregate_f32 behind its argument checks.  work: dfe_sgm_work_planes(paths, agg != NULL) planes;
// agg [H][W][D] or NULL; flow [H][W] or NULL.
int dfe_sgm_run(dfe_ctx *ctx, const float *volume, int H, int W, int D, float P1, float P2, unsigned paths, int ring, float *work, float *agg,
                float *flow, const SgmPen *pen) {
    const bool direct = dfe_sgm_work_planes(paths, agg != nullptr) == 0;   // one direction, and its L is the aggregate the caller wants
    SgmJob a{};
    a.C = volume;
    a.H = H; a.W = W; a.D = D;
    a.ring = ring;
    a.P1 = P1; a.P2 = P2;
    a.n = sgm_directions(paths, a.dy, a.dx);
    for (int k = 0; k < a.n; ++k) a.L[k] = direct ? agg : work + (size_t)k * H * W * D;
    DfeProfScope prof(ctx);
    const dim3 grid((unsigned)dfe_cdiv(H > W ? H : W, 4), (unsigned)a.n);
    if (pen) {
        if (D <= 16) hipLaunchKernelGGL(guided_sgm_path_kernel<1>, grid, dim3(64), 0, ctx->stream, a, *pen);
        else hipLaunchKernelGGL(guided_sgm_path_kernel<2>, grid, dim3(64), 0, ctx->stream, a, *pen);
    } else if (D <= 16) hipLaunchKernelGGL(sgm_path_kernel<1>, grid, dim3(64), 0, ctx->stream, a);
    else hipLaunchKernelGGL(sgm_path_kernel<2>, grid, dim3(64), 0, ctx->stream, a);
    DFE_LAUNCH_CHECK(ctx);
    float *aout = direct ? nullptr : agg;
    if (aout || flow) {
        const dim3 sgrid((unsigned)dfe_cdiv((long long)H * W, 16));
#define DFE_SGM_SUM(LPL, FLOW) hipLaunchKernelGGL((sgm_sum_kernel<LPL, FLOW>), sgrid, dim3(256), 0, ctx->stream, a, aout, flow)
        if (D <= 16) { if (flow) DFE_SGM_SUM(1, true); else DFE_SGM_SUM(1, false); }
        else { if (flow) DFE_SGM_SUM(2, true); else DFE_SGM_SUM(2, false); }
#undef DFE_SGM_SUM
        DFE_LAUNCH_CHECK(ctx);
    }
    ctx->last_kernel = "sgm_path_kernel";
    return DFE_OK;
}

int dfe_sgm_check(dfe_ctx *ctx, const char *fn, int H, int W, int D, float P1, float P2, unsigned paths, int ring) {
    DFE_REQUIRE(ctx, H >= 1 && W >= 1 && D >= 1 && (long long)H * W <= INT_MAX, DFE_E_SHAPE, "%s: H=%d W=%d D=%d", fn, H, W, D);
    DFE_REQUIRE(ctx, D <= 32, DFE_E_UNSUPPORTED, "%s: D=%d labels (32 at most)", fn, D);
    const int rc = sgm_params_check(ctx, fn, P1, P2, paths);
    if (rc) return rc;
    DFE_REQUIRE(ctx, ring >= 0 && ring <= W, DFE_E_ARG, "%s: ring=%d must be 0 .. W=%d", fn, ring, W);
    return DFE_OK;
}

namespace {

// the two aggregate entries behind DFE_ENTER (g: NULL for the unguided one)
int sgm_aggregate(dfe_ctx *ctx, const char *fn, const float *volume, int H, int W, int D, float P1, float P2, unsigned paths, int ring, float *agg, float *flow,
                  const SgmGuide *g) {
    DFE_REQUIRE(ctx, volume && (agg || flow), DFE_E_ARG, "%s: %s", fn, volume ? "agg and flow are both NULL" : "volume is NULL");
    DFE_REQUIRE(ctx, agg != volume, DFE_E_ARG, "%s: agg must not be the volume (every direction reads it)", fn);
    int rc = dfe_sgm_check(ctx, fn, H, W, D, P1, P2, paths, ring);
    if (!rc && g) rc = sgm_guide_check(ctx, fn, P1, P2, *g);
    if (rc) return rc;
    const bool guided = g && sgm_guided(*g);
    float *work = nullptr, *planes = nullptr;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        work = c.take<float>(dfe_sgm_work_planes(paths, agg != nullptr) * H * W * D);
        if (guided) planes = c.take<float>(sgm_penalty_floats(paths, H, W));
    });
    if (rc) return rc;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    SgmPen pen{};
    if (guided) {
        rc = sgm_penalty_run(ctx, *g, H, W, P2, paths, planes, &pen);
        if (rc) return rc;
    }
    return dfe_sgm_run(ctx, volume, H, W, D, P1, P2, paths, ring, work, agg, flow, guided ? &pen : nullptr);
}

}  // namespace

extern "C" {

int dfe_sgm_aggregate_f32(dfe_ctx *ctx, const float *volume, int H, int W, int D, float P1, float P2, unsigned paths, int ring, float *agg,
                          float *flow) {
    DFE_ENTER(ctx);
    return sgm_aggregate(ctx, "dfe_sgm_aggregate_f32", volume, H, W, D, P1, P2, paths, ring, agg, flow, nullptr);
}

int dfe_sgm_aggregate_guided_f32(dfe_ctx *ctx, const float *volume, int H, int W, int D, float P1, float P2, unsigned paths, int ring, float *agg,
                                 float *flow, const float *guide, int Cg, float sigma, float P2_edge) {
    DFE_ENTER(ctx);
    const SgmGuide g{guide, false, 1.f, Cg, (size_t)H * W, W, sigma, P2_edge};
    return sgm_aggregate(ctx, "dfe_sgm_aggregate_guided_f32", volume, H, W, D, P1, P2, paths, ring, agg, flow, &g);
}

}  // extern "C"
