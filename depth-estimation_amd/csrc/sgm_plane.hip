// sgm_plane.hip -- semi-global aggregation of a cost volume with a TWO-dimensional label plane: the [H][W][hWin][wWin] volumes of the
// Cartesian matchers (SSD, census, nn.SpatialMatching), up to 1096 cells (NOT in the reference, whose matchers are all
// winner-takes-all).  The definition -- directions, the step with its four label neighbours, the order of the
// sum, the first minimum with the centre rule -- is in include/dfe.h and restated in numpy in tests/sgm_plane_ref.py; the device is
// tested against that bit for bit.
//   sgmp_path_kernel<J, AHEAD>   ONE launch for all the directions asked for (blockIdx.y), each into a plane of its own (sgm.hip measured
//       why).  A chain is sequential along its line and wide across the label plane -- the opposite shape from sgm.hip -- so a LINE (a
//       row for the horizontal directions; for the others the W chains that start on the top or bottom row and start AGAIN, L = C,
//       where they come back in through the other side: SgmCursor of sgm_common.h, the walk sgm.hip's path kernel takes, with no ring)
//       belongs to ONE wave: cell c = j 64 + lane, J cells a lane, the cell axis padded with +Inf cells, which change no bit of a
//       real cell and stay +Inf.  L_r(q, .) lives in registers (a lane's own cells) AND in a
//       double-buffered LDS plane of (hWin + 2) x (wWin + 2) floats with a +Inf frame, from which the four neighbour reads need no edge
//       test; one barrier a step.  m = a register min over j and one wave reduction.  C(p, .) is loaded along the class axis, the loads
//       of the next AHEAD steps in flight (a line's addresses are wave-uniform integers, known from its first step).
//   guided_sgmp_path_kernel<J, AHEAD>   the same body with the step's P2 taken from the direction's penalty plane (sgm_penalty.hip;
//       DESIGN.md section 4.38): a wave-uniform value, fetched a chunk of up to 64 steps at a time into LDS behind the two planes.
//   sgmp_sum_kernel<FLOW>   a wave a pixel: agg = ((L_a + L_b) + L_c) + ... in ascending direction order, stored only if somebody
//       reads it; the first minimum in class order by a wave reduction on (value, class), the centre class winning an exact tie; the
//       decoded flow and, for the census one call, the match score of the RAW cost at the chosen class, at the pasted positions.  Its
//       steps are the functions of sgm_common.h that sgm_pick.hip's kernel is made of too.
// The census one calls that aggregate (dfe_census_flow_depth_pair_sgm_*) are in sgm_pick.hip, one body with the _sgm2_ entries.
#include "sgm_common.h"

namespace {

constexpr int kSgmpMaxJ = (kDfeMaxWindowCells + 63) / 64;   // cells a lane at the ceiling: 18

// the smallest value of the wave in every lane of it (no NaNs: path costs, +Inf in the padding cells): the minimum of each 16-lane
// row, then the four rows' values through scalar registers
__device__ __forceinline__ float sgmp_wave_min(float v) {
    v = sgm_row_min(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}

extern __shared__ float sgmp_lds[];              // two planes of (hWin + 2) x (wWin + 2): L_r(q, .) inside a +Inf frame

// the body of the two path kernels.  GUIDED: the step's P2 is a cell of the direction's penalty plane (sgm_penalty.hip), a wave-uniform
// value.  The wave fetches the penalties of 64 steps at once, lane i that of step s + i (a line's pixels have a closed form), into 64
// floats of LDS behind the two planes, and a step reads its own from there with its neighbour cells: no register is held across
// steps, where a slot per step of the look-ahead, in VGPRs or SGPRs, cost the 5- and 9-cell forms an occupancy class; a step's
// dependent chain keeps its length
template <int J, int AHEAD, bool GUIDED>
__device__ __forceinline__ void sgmp_path_body(const SgmpJob &a, const SgmPen *pen) {
#pragma clang fp contract(off)
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
    SgmCursor f(dy, dx, line, a.H, a.W, /*ring*/ 0);
    int fs = 0;
    float cb[AHEAD][J];
    int pixb[AHEAD];
    bool stb[AHEAD];
    constexpr int kChunk = 64 / AHEAD * AHEAD;   // steps a fetch of penalties serves: whole groups of the look-ahead
    float *pen_lds = sgmp_lds + 2 * plane;       // P2 of step cbase + i at [i], for the chunk of the line that is being walked
    int cbase = -kChunk;
    auto pen_fetch = [&](int first) {            // the penalties of the steps first + lane (past the line: the last step's again)
        int st = first + lane;
        st = st < nsteps ? st : nsteps - 1;
        if (pen->atq[k]) st = st > 0 ? st - 1 : 0;   // the plane's cell is the predecessor's: the pixel of the step before (step 0 starts)
        int y, x;
        if (horizontal) {
            y = line;
            x = dx > 0 ? st : a.W - 1 - st;
        } else {                                 // SgmCursor's walk: down or up from x = line, through the sides modulo W
            y = dy > 0 ? st : a.H - 1 - st;
            x = (line + st * dx) % a.W;
            x = x < 0 ? x + a.W : x;
        }
        return pen->plane[k][(size_t)y * a.W + x];
    };
    auto fetch = [&](int slot) {
        const int pix = f.y * a.W + f.x;
        const float *__restrict__ src = a.C + (size_t)pix * a.cells;
#pragma unroll
        for (int j = 0; j < J; ++j) cb[slot][j] = src[cl[j]];
        pixb[slot] = pix;
        stb[slot] = f.start;
        ++fs;
        f.advance(dy, dx, a.W, /*ring*/ 0);
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
        if constexpr (GUIDED) {
            if (s - cbase == kChunk) {           // a chunk begins (the last step's barrier is behind the reads of the chunk before)
                cbase = s;
                pen_lds[lane] = pen_fetch(s);
                __syncthreads();
            }
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            if (s + u >= nsteps) break;          // (wave-uniform, as every branch of this loop)
            float c[J];
#pragma unroll
            for (int j = 0; j < J; ++j) c[j] = in[j] ? cb[u][j] : inf;
            const int pix = pixb[u];
            const bool start = stb[u];
            float P2 = a.P2;
            if constexpr (GUIDED) P2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pen_lds[s + u - cbase])));   // (uniform: into an SGPR, as a.P2 is)
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
                const float far = m + P2;
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

template <int J, int AHEAD>
__global__ __launch_bounds__(64) void sgmp_path_kernel(const SgmpJob a) {
    sgmp_path_body<J, AHEAD, false>(a, nullptr);
}
template <int J, int AHEAD>
__global__ __launch_bounds__(64) void guided_sgmp_path_kernel(const SgmpJob a, const SgmPen pen) {
    sgmp_path_body<J, AHEAD, true>(a, &pen);
}

// agg = the n planes summed in order; its first minimum with the centre rule.  A wave a pixel, four pixels a block
template <bool FLOW>
__global__ __launch_bounds__(256) void sgmp_sum_kernel(const SgmpJob a, const SgmpOut o) {
    const int lane = threadIdx.x & 63;
    const long long P = (long long)a.H * a.W;
    const long long px = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (px >= P) return;                         // (wave-uniform; no barrier below)
    const size_t e = (size_t)px * a.cells;
    float b = __builtin_inff(), cen = __builtin_inff();
    int bi = INT_MAX;
    sgmp_lane_sum<FLOW, false>(a, o.agg, e, lane, nullptr, b, bi, cen);
    if constexpr (FLOW) {
        sgmp_wave_first_min(b, bi, cen);
        if (lane != 0) return;
        bi = sgmp_centre_rule(a, b, bi, cen);
        const int fl = bi / a.wWin;              // dfe_x2yx
        sgmp_store_winner(o, px, e, sgmp_pasted(a, o, px), bi, (float)(fl - (a.hWin - 1) / 2), (float)(bi - fl * a.wWin - (a.wWin - 1) / 2));
    }
}

}  // namespace

// (declared in sgm_common.h: sgm_pick.hip launches the path kernel through them)
int sgmp_check(dfe_ctx *ctx, const char *fn, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths) {
    DFE_REQUIRE(ctx, H >= 1 && W >= 1 && hWin >= 1 && wWin >= 1 && (long long)H * W <= INT_MAX, DFE_E_SHAPE, "%s: H=%d W=%d window %dx%d", fn, H, W, hWin,
                wWin);
    DFE_REQUIRE(ctx, (long long)hWin * wWin <= kDfeMaxWindowCells, DFE_E_UNSUPPORTED, "%s: window %dx%d has more than %d cells", fn, hWin, wWin,
                kDfeMaxWindowCells);
    return sgm_params_check(ctx, fn, P1, P2, paths);
}

SgmpJob sgmp_job(const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, float *work, float *&agg) {
    SgmpJob a{};
    a.C = volume;
    a.H = H; a.W = W; a.hWin = hWin; a.wWin = wWin; a.cells = hWin * wWin;
    a.mid0 = dfe_window_middle(hWin, wWin) - 1;
    a.P1 = P1; a.P2 = P2;
    a.n = sgm_directions(paths, a.dy, a.dx);
    const bool direct = paths && dfe_sgm_work_planes(paths, agg != nullptr) == 0;   // one direction, and its L is the aggregate the caller wants
    for (int k = 0; k < a.n; ++k) a.L[k] = direct ? agg : work + (size_t)k * H * W * a.cells;
    if (direct) agg = nullptr;
    if (!paths) {                                // nothing is aggregated: the sum reads the volume as it is (and writes no L)
        a.L[0] = const_cast<float *>(volume);
        a.n = 1;
    }
    return a;
}

int sgmp_launch_paths(dfe_ctx *ctx, const SgmpJob &a, const SgmPen *pen) {
    DfeProfScope prof(ctx);
    const dim3 grid((unsigned)(a.H > a.W ? a.H : a.W), (unsigned)a.n);
    const size_t lds = (size_t)2 * (a.hWin + 2) * (a.wWin + 2) * sizeof(float) + (pen ? 64 * sizeof(float) : 0);   // 26352 bytes at the most (1 x 1096), and a chunk of penalties
    const int J = dfe_cdiv(a.cells, 64);
    // (GA: the guided form's look-ahead -- one step less at 9 cells a lane, which came out three registers above the 96 of its twin's
    //  five waves a SIMD at four)
#define DFE_SGMP_PATH(JJ, AA, GA)                                                                                \
    do {                                                                                                         \
        if (pen) hipLaunchKernelGGL((guided_sgmp_path_kernel<JJ, GA>), grid, dim3(64), lds, ctx->stream, a, *pen); \
        else hipLaunchKernelGGL((sgmp_path_kernel<JJ, AA>), grid, dim3(64), lds, ctx->stream, a);                  \
    } while (0)
    if (J <= 1) DFE_SGMP_PATH(1, 8, 8);
    else if (J <= 2) DFE_SGMP_PATH(2, 8, 8);
    else if (J <= 5) DFE_SGMP_PATH(5, 4, 4);
    else if (J <= 9) DFE_SGMP_PATH(9, 4, 3);
    else DFE_SGMP_PATH(kSgmpMaxJ, 2, 2);
#undef DFE_SGMP_PATH
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "sgmp_path_kernel";
    return DFE_OK;
}

// The two launches behind the checks.  work: dfe_sgm_work_planes(paths, o.agg != NULL) planes; o: where the results go
int sgmp_run(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, float *work, SgmpOut o,
             const SgmPen *pen) {
    const SgmpJob a = sgmp_job(volume, H, W, hWin, wWin, P1, P2, paths, work, o.agg);
    DfeProfScope prof(ctx);
    int rc = sgmp_launch_paths(ctx, a, pen);
    if (rc) return rc;
    const bool flow = o.idx || o.fy || o.fx || o.match;
    if (o.agg || flow) {
        const dim3 sgrid((unsigned)dfe_cdiv((long long)H * W, 4));
        if (flow) hipLaunchKernelGGL(sgmp_sum_kernel<true>, sgrid, dim3(256), 0, ctx->stream, a, o);
        else hipLaunchKernelGGL(sgmp_sum_kernel<false>, sgrid, dim3(256), 0, ctx->stream, a, o);
        DFE_LAUNCH_CHECK(ctx);
    }
    return DFE_OK;
}

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
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) { work = c.take<float>(dfe_sgm_work_planes(paths, agg != nullptr) * H * W * (size_t)(hWin * wWin)); });
    if (rc) return rc;
    SgmpOut o{};
    o.agg = agg;
    o.idx = (long long *)idx; o.fy = flow_y; o.fx = flow_x;
    o.pitch = W;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    return sgmp_run(ctx, volume, H, W, hWin, wWin, P1, P2, paths, work, o);
}

}  // extern "C"
