// sgm_plane.hip -- semi-global aggregation of a cost volume with a TWO-dimensional label plane: the [H][W][hWin][wWin] volumes of the
// Cartesian matchers (SSD, census, nn.SpatialMatching), up to 1096 cells (NOT in the reference, whose matchers are all
// winner-takes-all).  The definition -- directions, the step with its four label neighbours, the order of the
// sum, the first minimum with the centre rule -- is in include/dfe.h and restated in numpy in tests/sgm_plane_ref.py; the device is
// tested against that bit for bit.
//   sgmp_path_kernel<J, AHEAD>   ONE launch for all the directions asked for (blockIdx.y), each into a plane of its own (sgm.hip measured
//       why).  A chain is sequential along its line and wide across the label plane -- the opposite shape from sgm.hip -- so a LINE (a
//       row for the horizontal directions; for the others the W chains that start on the top or bottom row and start AGAIN, L = C,
//       where they come back in through the other side) belongs to ONE wave: cell c = j 64 + lane, J cells a lane, the cell axis padded
//       with +Inf cells, which change no bit of a real cell and stay +Inf.  L_r(q, .) lives in registers (a lane's own cells) AND in a
//       double-buffered LDS plane of (hWin + 2) x (wWin + 2) floats with a +Inf frame, from which the four neighbour reads need no edge
//       test; one barrier a step.  m = a register min over j and one wave reduction.  C(p, .) is loaded along the class axis, the loads
//       of the next AHEAD steps in flight (a line's addresses are wave-uniform integers, known from its first step).
//   sgmp_sum_kernel<FLOW>   a wave a pixel: agg = ((L_a + L_b) + L_c) + ... in ascending direction order, stored only if somebody
//       reads it; the first minimum in class order by a wave reduction on (value, class), the centre class winning an exact tie; the
//       decoded flow and, for the census one call, the match score of the RAW cost at the chosen class, at the pasted positions.
#include "dfe_internal.h"
#include <cmath>
#include <climits>

namespace {

constexpr int kSgmpMaxCells = 1096;   // the single-scale step's ceiling
constexpr int kSgmpMaxJ = 18;         // cells a lane at that ceiling

// the smallest value of the wave in every lane of it (no NaNs: path costs, +Inf in the padding cells): four DPP steps inside each
// 16-lane row -- the float form of the reductions in dfe_wave.h -- then the four rows' values through scalar registers
__device__ __forceinline__ float sgmp_wave_min(float v) {
#define DFE_STEP(ctrl) v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false)))
    DFE_STEP(0x128); DFE_STEP(0x124); DFE_STEP(0x4E); DFE_STEP(0xB1);   // row_ror:8, row_ror:4, quad_perm [2,3,0,1], [1,0,3,2]
#undef DFE_STEP
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}

template <int J, int AHEAD>
__global__ __launch_bounds__(64) void sgmp_path_kernel(const SgmpJob a) {
#pragma clang fp contract(off)
    extern __shared__ float sgmp_lds[];          // two planes of (hWin + 2) x (wWin + 2): L_r(q, .) inside a +Inf frame
    const float inf = __builtin_inff();
    const int k = blockIdx.y;                    // which of the directions
    const int dy = a.dy[k], dx = a.dx[k];
    float *__restrict__ out = a.L[k];
    const bool horizontal = dy == 0;
    const int nlines = horizontal ? a.H : a.W;   // lines of this direction
    const int nsteps = horizontal ? a.W : a.H;
    const int line = blockIdx.x;
    if (line >= nlines) return;                  // (the grid is sized for the longer side)
    const int lane = threadIdx.x;
    const int pitch = a.wWin + 2, plane = (a.hWin + 2) * pitch;
    for (int i = lane; i < 2 * plane; i += 64) sgmp_lds[i] = inf;

    bool in[J];
    int cl[J], off[J];                           // a padding cell loads and reads as the last real cell, takes +Inf and stores nothing
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = j * 64 + lane;
        in[j] = c < a.cells;
        cl[j] = in[j] ? c : a.cells - 1;
        const int y = cl[j] / a.wWin;
        off[j] = (y + 1) * pitch + cl[j] - y * a.wWin + 1;
    }

    // the fetch cursor (wave-uniform integers): the pixel of step `fs`, and whether the chain starts (again) there
    int fy, fx, fs = 0;
    bool fstart = true;
    if (horizontal) {
        fy = line;
        fx = dx > 0 ? 0 : a.W - 1;
    } else {
        fy = dy > 0 ? 0 : a.H - 1;
        fx = line;
    }
    float cb[AHEAD][J];
    int pixb[AHEAD];
    bool stb[AHEAD];
    auto fetch = [&](int slot) {
        const int pix = fy * a.W + fx;
        const float *__restrict__ src = a.C + (size_t)pix * a.cells;
#pragma unroll
        for (int j = 0; j < J; ++j) cb[slot][j] = src[cl[j]];
        pixb[slot] = pix;
        stb[slot] = fstart;
        ++fs;
        fy += dy;
        fx += dx;
        const bool wrapped = fx < 0 || fx >= a.W;   // through a side: the predecessor of the pixel it comes back in at lies outside
        fx = fx < 0 ? a.W - 1 : (fx >= a.W ? 0 : fx);
        fstart = wrapped;
    };
#pragma unroll
    for (int u = 0; u < AHEAD; ++u)
        if (fs < nsteps) fetch(u);
    __syncthreads();                             // the frame is there

    float l[J];
#pragma unroll
    for (int j = 0; j < J; ++j) l[j] = inf;
    int cur = 0;                                 // the LDS plane that holds L_r(q, .)
    for (int s = 0; s < nsteps; s += AHEAD) {
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            if (s + u >= nsteps) break;          // (wave-uniform, as every branch of this loop)
            float c[J];
#pragma unroll
            for (int j = 0; j < J; ++j) c[j] = in[j] ? cb[u][j] : inf;
            const int pix = pixb[u];
            const bool start = stb[u];
            if (fs < nsteps) fetch(u);
            if (start) {
#pragma unroll
                for (int j = 0; j < J; ++j) l[j] = c[j];
            } else {
                // L_r(p, c) = C(p, c) + (min(L(q, c), L(q, c's four neighbours) + P1, m + P2) - m), m = min over the cells of L(q, .)
                float m = l[0];
#pragma unroll
                for (int j = 1; j < J; ++j) m = fminf(m, l[j]);
                m = sgmp_wave_min(m);
                const float far = m + a.P2;
                const float *q = sgmp_lds + cur * plane;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const float *qc = q + off[j];
                    float t = l[j];
                    t = fminf(t, qc[-1] + a.P1);
                    t = fminf(t, qc[1] + a.P1);
                    t = fminf(t, qc[-pitch] + a.P1);
                    t = fminf(t, qc[pitch] + a.P1);
                    t = fminf(t, far);
                    l[j] = c[j] + (t - m);
                }
            }
            cur ^= 1;
            float *w = sgmp_lds + cur * plane;
            float *__restrict__ dst = out + (size_t)pix * a.cells + lane;
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (in[j]) {
                    w[off[j]] = l[j];
                    dst[j * 64] = l[j];
                }
            __syncthreads();                     // one wave: orders its LDS stores before the next step's neighbour reads
        }
    }
}

// agg = the n planes summed in order; its first minimum with the centre rule.  A wave a pixel, four pixels a block
template <bool FLOW>
__global__ __launch_bounds__(256) void sgmp_sum_kernel(const SgmpJob a, const SgmpOut o) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long P = (long long)a.H * a.W;
    const long long px = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (px >= P) return;                         // (wave-uniform; no barrier below)
    const size_t e = (size_t)px * a.cells;
    float b = __builtin_inff(), cen = __builtin_inff();
    int bi = INT_MAX;
    for (int c = lane; c < a.cells; c += 64) {
        float t = a.L[0][e + c];
        for (int k = 1; k < a.n; ++k) t = t + a.L[k][e + c];
        if (o.agg) o.agg[e + c] = t;
        if constexpr (FLOW) {
            if (t < b) { b = t; bi = c; }        // (a lane's classes ascend: strict `<` keeps its first minimum)
            if (c == o.mid0) cen = t;
        }
    }
    if constexpr (FLOW) {
        // the smallest value, and among equal ones the smallest class; the centre's value to every lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float ob = __shfl_xor(b, d, 64);
            const int oi = __shfl_xor(bi, d, 64);
            const bool take = (ob < b) | ((ob == b) & (oi < bi));
            b = take ? ob : b;
            bi = take ? oi : bi;
            cen = fminf(cen, __shfl_xor(cen, d, 64));
        }
        if (lane != 0) return;
        if (cen == b || bi >= a.cells) bi = o.mid0;   // the centre wins an exact tie with the best (and a volume that is not finite reads in bounds)
        const int y = (int)(px / a.W), x = (int)(px - (long long)y * a.W);
        const size_t op = (size_t)(y + o.pad_t) * o.pitch + x + o.pad_l;
        if (o.idx) o.idx[px] = bi + 1;
        if (o.match) o.match[op] = 1.0f - o.raw[e + bi] / o.den;
        const int fl = bi / a.wWin;              // dfe_x2yx
        if (o.fy) o.fy[op] = (float)(fl - (a.hWin - 1) / 2);
        if (o.fx) o.fx[op] = (float)(bi - fl * a.wWin - (a.wWin - 1) / 2);
    }
}

}  // namespace

// (declared in dfe_internal.h: sgm_pick.hip launches the path kernel through them)
// planes of H * W * cells floats that sgmp_run takes as `work`: one per direction, unless the only direction goes straight to agg
size_t sgmp_work_planes(unsigned paths, bool agg_given) {
    const int n = __builtin_popcount(paths & 255u);
    return n == 1 && agg_given ? 0 : (size_t)n;
}

int sgmp_check(dfe_ctx *ctx, const char *fn, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths) {
    DFE_REQUIRE(ctx, H >= 1 && W >= 1 && hWin >= 1 && wWin >= 1 && (long long)H * W <= INT_MAX, DFE_E_SHAPE, "%s: H=%d W=%d window %dx%d", fn, H, W, hWin,
                wWin);
    DFE_REQUIRE(ctx, (long long)hWin * wWin <= kSgmpMaxCells, DFE_E_UNSUPPORTED, "%s: window %dx%d has more than %d cells", fn, hWin, wWin, kSgmpMaxCells);
    DFE_REQUIRE(ctx, paths >= 1u && paths <= 255u, DFE_E_ARG, "%s: paths=0x%x must be 1 .. 255 (bit r = direction r)", fn, paths);
    DFE_REQUIRE(ctx, std::isfinite(P1) && std::isfinite(P2) && P1 >= 0.f && P1 <= P2, DFE_E_ARG, "%s: P1=%g P2=%g must be finite with 0 <= P1 <= P2", fn,
                (double)P1, (double)P2);
    return DFE_OK;
}

// The two launches behind the checks.  work: sgmp_work_planes(paths, o.agg != NULL) planes; o: where the results go
int sgmp_run(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, float *work, SgmpOut o) {
    static const int dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};   // (dy, dx) of bit r
    const bool direct = sgmp_work_planes(paths, o.agg != nullptr) == 0;   // one direction, and its L is the aggregate the caller wants
    SgmpJob a{};
    a.C = volume;
    a.H = H; a.W = W; a.hWin = hWin; a.wWin = wWin; a.cells = hWin * wWin;
    a.P1 = P1; a.P2 = P2;
    const size_t plane = (size_t)H * W * a.cells;
    for (int r = 0; r < 8; ++r) {
        if (!(paths >> r & 1u)) continue;
        a.L[a.n] = direct ? o.agg : work + (size_t)a.n * plane;
        a.dy[a.n] = dirs[r][0]; a.dx[a.n] = dirs[r][1];
        ++a.n;
    }
    DfeProfScope prof(ctx);
    const dim3 grid((unsigned)(H > W ? H : W), (unsigned)a.n);
    const size_t lds = (size_t)2 * (hWin + 2) * (wWin + 2) * sizeof(float);   // 26352 bytes at the most (1 x 1096)
    const int J = dfe_cdiv(a.cells, 64);
#define DFE_SGMP_PATH(JJ, AA) hipLaunchKernelGGL((sgmp_path_kernel<JJ, AA>), grid, dim3(64), lds, ctx->stream, a)
    if (J <= 1) DFE_SGMP_PATH(1, 8);
    else if (J <= 2) DFE_SGMP_PATH(2, 8);
    else if (J <= 5) DFE_SGMP_PATH(5, 4);
    else if (J <= 9) DFE_SGMP_PATH(9, 4);
    else DFE_SGMP_PATH(kSgmpMaxJ, 2);
#undef DFE_SGMP_PATH
    DFE_LAUNCH_CHECK(ctx);
    const bool flow = o.idx || o.fy || o.fx || o.match;
    if (direct) o.agg = nullptr;
    if (o.agg || flow) {
        o.mid0 = dfe_window_middle(hWin, wWin) - 1;
        const dim3 sgrid((unsigned)dfe_cdiv((long long)H * W, 4));
        if (flow) hipLaunchKernelGGL(sgmp_sum_kernel<true>, sgrid, dim3(256), 0, ctx->stream, a, o);
        else hipLaunchKernelGGL(sgmp_sum_kernel<false>, sgrid, dim3(256), 0, ctx->stream, a, o);
        DFE_LAUNCH_CHECK(ctx);
    }
    ctx->last_kernel = "sgmp_path_kernel";
    return DFE_OK;
}

namespace {

// the census one call behind its device guard: T = float or uint8_t
template <class T>
int sgmp_census_pair(dfe_ctx *ctx, const char *fn, const T *I0, const T *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x, float foe_y,
                     float P1, float P2, unsigned paths, float *flow, float *match, float *depth, float *depth_conf) {
    // census.hip's checks of its one call, in its order, then the aggregation's: everything is refused before any launch
    DFE_REQUIRE(ctx, I0 && I1 && flow && match, DFE_E_ARG, "%s: NULL tensor", fn);
    DFE_REQUIRE(ctx, (depth == nullptr) == (depth_conf == nullptr), DFE_E_ARG, "%s: depth and depth_conf go together", fn);
    DFE_REQUIRE(ctx, k >= 3 && (k & 1) && k * k <= 64, DFE_E_ARG, "%s: patch %dx%d: odd sides of at least 3 with at most 64 cells expected", fn, k, k);
    DFE_REQUIRE(ctx, H >= 1 && W >= 1 && H <= 32768 && W <= 32768, DFE_E_SHAPE, "%s: frame %dx%d (1 .. 32768 each)", fn, H, W);
    DFE_REQUIRE(ctx, H >= k && W >= k, DFE_E_SHAPE, "%s: frame %dx%d too small for a %dx%d patch", fn, H, W, k, k);
    DFE_REQUIRE(ctx, C >= 1 && C <= 4, DFE_E_ARG, "%s: C=%d channels (1 .. 4)", fn, C);
    DFE_REQUIRE(ctx, agg == 1 || agg == 3 || agg == 5, DFE_E_ARG, "%s: agg=%d must be 1, 3 or 5", fn, agg);
    DFE_REQUIRE(ctx, hWin >= 1 && wWin >= 1, DFE_E_ARG, "%s: window %dx%d", fn, hWin, wWin);
    DFE_REQUIRE(ctx, (long long)hWin * wWin <= kSgmpMaxCells, DFE_E_UNSUPPORTED, "%s: window %dx%d has more than %d cells", fn, hWin, wWin, kSgmpMaxCells);
    const int Hp = H - k + 1, Wp = W - k + 1;
    const int Ha = Hp - hWin + 1 - agg + 1, Wa = Wp - wWin + 1 - agg + 1;
    DFE_REQUIRE(ctx, Ha >= 1 && Wa >= 1, DFE_E_SHAPE, "%s: %dx%d patch positions leave no pixel for a %dx%d window summed over %dx%d", fn, Hp, Wp, hWin, wWin,
                agg, agg);
    int rc = sgmp_check(ctx, fn, Ha, Wa, hWin, wWin, P1, P2, paths);
    if (rc) return rc;
    uint64_t *sig0 = nullptr, *sig1 = nullptr;
    float *vol = nullptr, *work = nullptr;
    const size_t n = (size_t)C * Hp * Wp, plane = (size_t)Ha * Wa * hWin * wWin;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        sig0 = c.take<uint64_t>(n);
        sig1 = c.take<uint64_t>(n);
        vol = c.take<float>(plane);
        work = c.take<float>(sgmp_work_planes(paths, false) * plane);
    });
    if (rc) return rc;
    {   // the staged public calls themselves (they carve nothing): the same kernels, the same bits
        DfeStageScope st(ctx, DFE_STAGE_FILTER);
        if constexpr (sizeof(T) == 1) {
            rc = dfe_census_transform_u8(ctx, I0, C, H, W, k, k, sig0);
            if (!rc) rc = dfe_census_transform_u8(ctx, I1, C, H, W, k, k, sig1);
        } else {
            rc = dfe_census_transform_f32(ctx, I0, C, H, W, k, k, sig0);
            if (!rc) rc = dfe_census_transform_f32(ctx, I1, C, H, W, k, k, sig1);
        }
        if (rc) return rc;
    }
    const int pad_t = (H - Ha) / 2, pad_l = (W - Wa) / 2;   // the rule of flow_step.hip
    {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        rc = dfe_census_cost_volume_f32(ctx, sig0, sig1, C, Hp, Wp, hWin, wWin, agg, vol);
        if (rc) return rc;
        SgmpOut o{};
        o.fy = flow; o.fx = flow + (size_t)H * W;
        o.match = match; o.raw = vol;
        o.den = (float)((k * k - 1) * C * agg * agg);
        o.pitch = W; o.pad_t = pad_t; o.pad_l = pad_l;
        rc = sgmp_run(ctx, vol, Ha, Wa, hWin, wWin, P1, P2, paths, work, o);
        if (rc) return rc;
    }
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    return dfe_pair_border_depth(ctx, flow, match, H, W, pad_t, pad_l, Ha, Wa, foe_x, foe_y, depth, depth_conf);
}

}  // namespace

extern "C" {

int dfe_sgm_plane_aggregate_f32(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, float *agg,
                                int64_t *idx, float *flow_y, float *flow_x) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_sgm_plane_aggregate_f32";
    DFE_REQUIRE(ctx, volume && (agg || idx || flow_y || flow_x), DFE_E_ARG, "%s: %s", fn, volume ? "every output is NULL" : "volume is NULL");
    DFE_REQUIRE(ctx, agg != volume, DFE_E_ARG, "%s: agg must not be the volume (every direction reads it)", fn);
    int rc = sgmp_check(ctx, fn, H, W, hWin, wWin, P1, P2, paths);
    if (rc) return rc;
    float *work = nullptr;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) { work = c.take<float>(sgmp_work_planes(paths, agg != nullptr) * H * W * (size_t)(hWin * wWin)); });
    if (rc) return rc;
    SgmpOut o{};
    o.agg = agg;
    o.idx = (long long *)idx; o.fy = flow_y; o.fx = flow_x;
    o.pitch = W;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    return sgmp_run(ctx, volume, H, W, hWin, wWin, P1, P2, paths, work, o);
}

int dfe_census_flow_depth_pair_sgm_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                                       float foe_y, float P1, float P2, unsigned paths, float *flow, float *match, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    return sgmp_census_pair(ctx, "dfe_census_flow_depth_pair_sgm_f32", I0, I1, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths, flow, match, depth,
                            depth_conf);
}

int dfe_census_flow_depth_pair_sgm_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                                      float foe_y, float scale, float P1, float P2, unsigned paths, float *flow, float *match, float *depth,
                                      float *depth_conf) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, scale > 0, DFE_E_ARG, "dfe_census_flow_depth_pair_sgm_u8: scale=%g must be positive", (double)scale);
    return sgmp_census_pair(ctx, "dfe_census_flow_depth_pair_sgm_u8", I0, I1, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths, flow, match, depth,
                            depth_conf);
}

}  // extern "C"
