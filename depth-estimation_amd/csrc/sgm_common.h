// sgm_common.h -- what the semi-global files (sgm.hip, sgm_plane.hip, sgm_pick.hip, sgm_penalty.hip; nobody else includes this) hold to ONE definition,
// because the device is tested against the numpy definitions bit for bit and a fix made in one copy only would be a silent divergence:
//   host    the direction table, the paths / P1 / P2 check (the work-planes rule is dfe_sgm_work_planes, dfe_internal.h)
//           the guide and the penalty planes of the edge-aware entries (sgm_penalty.hip)
//   device  the 16-lane row minimum; the line cursor of the two path kernels; the summed arg-min of the plane family -- the ordered sum,
//           the (value, class) reduction, the centre rule, the stores of the winner -- which sgmp_sum_kernel and sgpk_pick_kernel share
// (not in dfe_wave.h: that file is hashed whole into the traffic profiles, and nothing here touches the kernels they describe)
#pragma once
#include "dfe_internal.h"
#include <cmath>
#include <climits>

// ---- host ----

// the directions `paths` asks for, in ascending bit order: p's predecessor on direction i is p - (dy[i], dx[i]).  Returns how many
inline int sgm_directions(unsigned paths, int *dy, int *dx) {
    static const int dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};   // (dy, dx) of bit r
    int n = 0;
    for (int r = 0; r < 8; ++r) {
        if (!(paths >> r & 1u)) continue;
        dy[n] = dirs[r][0]; dx[n] = dirs[r][1];
        ++n;
    }
    return n;
}

// the parameter rules every aggregation shares (fn: the entry's name for the message)
inline int sgm_params_check(dfe_ctx *ctx, const char *fn, float P1, float P2, unsigned paths) {
    DFE_REQUIRE(ctx, paths >= 1u && paths <= 255u, DFE_E_ARG, "%s: paths=0x%x must be 1 .. 255 (bit r = direction r)", fn, paths);
    DFE_REQUIRE(ctx, std::isfinite(P1) && std::isfinite(P2) && P1 >= 0.f && P1 <= P2, DFE_E_ARG, "%s: P1=%g P2=%g must be finite with 0 <= P1 <= P2", fn,
                (double)P1, (double)P2);
    return DFE_OK;
}

// ---- the guided penalty (sgm_penalty.hip defines the functions) ----
// Where P2(p, r) comes from: a guide image on the volume's pixel grid, as floats or as bytes read as float(byte) * scale
struct SgmGuide {
    const void *g;         // channel c's pixel (y, x) at g[c chan + y pitch + x]; NULL: no guide
    bool bytes;
    float scale;           // (bytes only)
    int Cg;
    size_t chan;
    int pitch;
    float sigma, P2_edge;
};
// what the guided path kernels take beside their job: for the job's direction k the [H][W] plane of its AXIS, which holds P2(p, r) at p
// for the axis' even bit r -- and, (a - b)^2 and (b - a)^2 having the same bits, P2(p, -r) at p's predecessor p + r for the odd bit
struct SgmPen {
    const float *plane[8];
    int atq[8];            // 1: direction k reads its plane at the predecessor's pixel
};
inline bool sgm_guided(const SgmGuide &g) { return g.g && g.sigma > 0.f; }   // (sigma NaN: not guided)
// the rules of the guided entries on top of the unguided ones'
DFE_HIDDEN int sgm_guide_check(dfe_ctx *ctx, const char *fn, float P1, float P2, const SgmGuide &g);
// floats of the penalty planes of a guided call: H * W per axis that `paths` touches
DFE_HIDDEN size_t sgm_penalty_floats(unsigned paths, int H, int W);
// one launch: every cell of the planes of the axes `paths` touches, the predecessor's column taken modulo W (the ring's wrap pair; on the
// plane such a step is a chain start and its cell is written and not used), P2 where the predecessor's row lies outside.  Fills `pen`
DFE_HIDDEN int sgm_penalty_run(dfe_ctx *ctx, const SgmGuide &g, int H, int W, float P2, unsigned paths, float *planes, SgmPen *pen);

// ---- the plane family's job and outputs (sgm_plane.hip defines the functions; sgm_pick.hip launches the path kernel through them) ----
struct SgmpJob {
    const float *C;      // [H][W][cells]
    float *L[8];         // [H][W][cells] each: the planes to sum, in order -- L of the n directions asked for, in ascending bit order
    int dy[8], dx[8];    // their directions
    int n;
    int H, W, hWin, wWin, cells;
    float P1, P2;
    int mid0;            // the centre class, 0-based (behind what the path kernel reads: its argument loads stay as they were)
};
struct SgmpOut {
    float *agg;            // [H][W][cells] or NULL
    long long *idx;        // [H][W], 1-based; or NULL
    // each of the following at [(y + pad_t) pitch + x + pad_l], or NULL
    float *fy, *fx;
    float *best, *second, *unique;   // the pick only (NULL for the plain aggregate); unique is 0 below min_unique
    float *match;          // 1 - raw(p, idx) / den (the census one calls)
    const float *raw;      // the volume the match score reads (match != NULL)
    float den, min_unique;
    int pitch, pad_t, pad_l;
};
// dfe_sgm_plane_aggregate_f32's checks of the sizes and parameters (fn: the entry's name for the message)
DFE_HIDDEN int sgmp_check(dfe_ctx *ctx, const char *fn, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths);
// The job of a call: direction k into work + k planes of H * W * cells floats (dfe_sgm_work_planes(paths, agg != NULL) of them), or the
// only direction straight into agg, which is then set to NULL: nothing is left to store.  paths == 0 (the pick): the volume is the one plane
DFE_HIDDEN SgmpJob sgmp_job(const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, float *work, float *&agg);
DFE_HIDDEN int sgmp_launch_paths(dfe_ctx *ctx, const SgmpJob &a, const SgmPen *pen = nullptr);   // sgmp_path_kernel for the job's directions (pen: its guided form)
// the two launches behind the checks: the paths, then the sum kernel for whatever `o` asks for
DFE_HIDDEN int sgmp_run(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, float *work, SgmpOut o,
                        const SgmPen *pen = nullptr);

// ---- device ----

// the smallest value of a 16-lane DPP row in every lane of it (no NaNs: path costs, +Inf in the padding lanes) -- the float form of the
// reductions in dfe_wave.h, in their step order
__device__ __forceinline__ float sgm_row_min(float v) {
#define DFE_STEP(ctrl) v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false)))
    DFE_STEP(0x128); DFE_STEP(0x124); DFE_STEP(0x4E); DFE_STEP(0xB1);   // row_ror:8, row_ror:4, quad_perm [2,3,0,1], [1,0,3,2]
#undef DFE_STEP
    return v;
}

// The walk of a LINE (wave-uniform integers): a row for the horizontal directions; for the others the chain that starts on the top or
// bottom row at x = line and, where it leaves through a side, comes back in through the other one -- on the plane (ring == 0) it STARTS
// AGAIN there, which is the definition's "the predecessor lies outside".  On a ring of G columns a horizontal line begins G steps early.
struct SgmCursor {
    int y, x;
    bool start;          // the chain starts (again) at this pixel: L = C
    __device__ __forceinline__ SgmCursor(int dy, int dx, int line, int H, int W, int ring) : start(true) {
        if (dy == 0) {
            const int lead = (W - ring) % W;     // (0 on the plane)
            y = line;
            x = dx > 0 ? lead : W - 1 - lead;
        } else {
            y = dy > 0 ? 0 : H - 1;
            x = line;
        }
    }
    __device__ __forceinline__ void advance(int dy, int dx, int W, int ring) {
        y += dy;
        x += dx;
        const bool left = x < 0, right = x >= W;   // through a side
        x = left ? W - 1 : (right ? 0 : x);
        start = (left || right) && ring == 0;
    }
};

// ---- the summed arg-min of the plane family: a wave a pixel, a lane's classes c = lane, lane + 64, ... ----

// A lane's cells of A(p, .) = ((L_a + L_b) + L_c) + ... in ascending direction order, stored if somebody reads the aggregate and, with KEEP,
// left in `row`; with ARGMIN the lane's first minimum (b, bi) and the centre's value
template <bool ARGMIN, bool KEEP>
__device__ __forceinline__ void sgmp_lane_sum(const SgmpJob &a, float *agg, size_t e, int lane, float *row, float &b, int &bi, float &cen) {
#pragma clang fp contract(off)
    for (int c = lane; c < a.cells; c += 64) {
        float t = a.L[0][e + c];
        for (int k = 1; k < a.n; ++k) t = t + a.L[k][e + c];
        if (agg) agg[e + c] = t;
        if constexpr (KEEP) row[c] = t;
        if constexpr (ARGMIN) {
            if (t < b) { b = t; bi = c; }        // (a lane's classes ascend: strict `<` keeps its first minimum)
            if (c == a.mid0) cen = t;
        }
    }
}
// the lanes' minima to the wave's: the smallest value, and among equal ones the smallest class; the centre's value to every lane
__device__ __forceinline__ void sgmp_wave_first_min(float &b, int &bi, float &cen) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float ob = __shfl_xor(b, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        const bool take = (ob < b) | ((ob == b) & (oi < bi));
        b = take ? ob : b;
        bi = take ? oi : bi;
        cen = fminf(cen, __shfl_xor(cen, d, 64));
    }
}
// the centre wins an exact tie with the best (and a volume that is not finite reads in bounds)
__device__ __forceinline__ int sgmp_centre_rule(const SgmpJob &a, float b, int bi, float cen) { return (cen == b || bi >= a.cells) ? a.mid0 : bi; }
// where pixel px's results go in the pasted planes
__device__ __forceinline__ size_t sgmp_pasted(const SgmpJob &a, const SgmpOut &o, long long px) {
    const int y = (int)(px / a.W), x = (int)(px - (long long)y * a.W);
    return (size_t)(y + o.pad_t) * o.pitch + x + o.pad_l;
}
// the winner's class and the match score of the RAW cost there; the flow the caller decoded (and refined)
__device__ __forceinline__ void sgmp_store_winner(const SgmpOut &o, long long px, size_t e, size_t op, int bi, float fy, float fx) {
#pragma clang fp contract(off)
    if (o.idx) o.idx[px] = bi + 1;
    if (o.match) o.match[op] = 1.0f - o.raw[e + bi] / o.den;
    if (o.fy) o.fy[op] = fy;
    if (o.fx) o.fx[op] = fx;
}
