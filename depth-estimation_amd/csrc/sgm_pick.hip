// sgm_pick.hip -- what a caller reads off the aggregate of sgm_plane.hip besides its arg-min: a uniqueness confidence and a sub-pixel
// flow taken on the surface that was minimised (NOT in the reference).  The definition -- the far cells, the
// uniqueness ratio, the per-axis parabola with cost := A -- is in include/dfe.h and restated in numpy in tests/sgm_pick_ref.py; the
// device is tested against that bit for bit.
//   sgpk_pick_kernel<SUB>   sgmp_sum_kernel's shape and its steps, the functions of sgm_common.h: a wave a pixel, four pixels a block,
//       agg = ((L_a + L_b) + L_c) + ... in ascending direction order, the first minimum in class order by a wave reduction on
//       (value, class), the centre class winning an exact tie.
//       A lane also leaves each sum in the wave's own LDS row (1096 floats a wave, 17.5 KB a block: the registers, not the LDS, bound
//       the waves a CU holds), so the second pass -- the smallest sum outside the winner's 3 x 3 neighbourhood -- and the parabola's
//       four neighbours read A itself: no plane is read twice and no sum is formed twice, so their bits are A's by construction.
//   The path launch is sgm_plane.hip's, unchanged (sgmp_launch_paths on sgmp_job's job); paths == 0 skips it and A = the volume.
//   The one calls: dfe_flow_depth_pair_sgm_f32 / _u8 (the SSD step) and, in ONE body on census.hip's front end, the census entries
//   dfe_census_flow_depth_pair_sgm_f32 / _u8 (sgmp_run: the plain aggregate) and dfe_census_flow_depth_pair_sgm2_f32 / _u8 (sgpk_run).
//   The guided entries are the same bodies with a guide: dfe_sgm_plane_pick_guided_f32 and the one calls
//   dfe_flow_depth_pair_sgm_guided_* / dfe_census_flow_depth_pair_sgm_guided_*, whose guide is frame 0 on the pasted region; the penalty
//   planes (sgm_penalty.hip) are carved behind the direction planes and handed to the path launch.
#include "sgm_common.h"
#include "subpixel_offset.h"   // the parabola's vertex on one axis (include/dfe.h: this order, IEEE division)

namespace {

template <bool SUB>
__global__ __launch_bounds__(256) void sgpk_pick_kernel(const SgmpJob a, const SgmpOut o) {
#pragma clang fp contract(off)
    __shared__ float sums[4][kDfeMaxWindowCells];   // A(p, .) of the wave's pixel
    const float inf = __builtin_inff();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *A = sums[wave];
    const long long P = (long long)a.H * a.W;
    const long long px = (long long)blockIdx.x * 4 + wave;
    const bool live = px < P;                    // (wave-uniform; a wave past the end still meets the barrier)
    const size_t e = live ? (size_t)px * a.cells : 0;
    float b = inf, cen = inf;
    int bi = INT_MAX;
    if (live) sgmp_lane_sum<true, true>(a, o.agg, e, lane, A, b, bi, cen);
    sgmp_wave_first_min(b, bi, cen);
    __syncthreads();                             // the wave's sums are in its row
    if (!live) return;
    bi = sgmp_centre_rule(a, b, bi, cen);
    const int r = bi / a.wWin, s = bi - r * a.wWin;
    // the smallest sum at Chebyshev distance 2 or more from the winner: +Inf if the window has no such cell
    float sec = inf;
    if (o.second || o.unique) {
        int cy = lane / a.wWin, cx = lane - cy * a.wWin;
        const int sy = 64 / a.wWin, sx = 64 - sy * a.wWin;   // 64 cells further on
        for (int c = lane; c < a.cells; c += 64) {
            const int ey = cy > r ? cy - r : r - cy, ex = cx > s ? cx - s : s - cx;
            const float t = A[c];
            sec = ((ey >= 2) | (ex >= 2)) ? fminf(sec, t) : sec;
            cy += sy; cx += sx;
            if (cx >= a.wWin) { cx -= a.wWin; ++cy; }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) sec = fminf(sec, __shfl_xor(sec, d, 64));
    }
    if (lane != 0) return;
    const float c0 = A[bi];
    const size_t op = sgmp_pasted(a, o, px);
    if (o.best) o.best[op] = c0;
    if (o.second) o.second[op] = sec;
    if (o.unique) {
        const float u = (sec == inf || !(sec > 0.f)) ? 0.f : (sec - c0) / sec;   // (not clamped)
        o.unique[op] = u >= o.min_unique ? u : 0.f;
    }
    float fy = (float)(r - (a.hWin - 1) / 2), fx = (float)(s - (a.wWin - 1) / 2);   // dfe_x2yx
    if constexpr (SUB) {
        // a neighbour outside the window is not read: its cell is replaced by the winner's and the axis gives off = 0
        const bool inx = s >= 1 && s + 1 < a.wWin, iny = r >= 1 && r + 1 < a.hWin;
        const float cxm = A[inx ? bi - 1 : bi], cxp = A[inx ? bi + 1 : bi];
        const float cym = A[iny ? bi - a.wWin : bi], cyp = A[iny ? bi + a.wWin : bi];
        fy = fy + subpixel_offset(iny, cym, c0, cyp);
        fx = fx + subpixel_offset(inx, cxm, c0, cxp);
    }
    sgmp_store_winner(o, px, e, op, bi, fy, fx);
}

// dfe_sgm_plane_pick_f32's parameter rules on top of sgmp_check's (paths == 0 allowed: P1 / P2 are checked all the same)
int sgpk_check(dfe_ctx *ctx, const char *fn, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, float min_unique) {
    int rc = sgmp_check(ctx, fn, H, W, hWin, wWin, P1, P2, paths ? paths : 1u);
    if (rc) return rc;
    DFE_REQUIRE(ctx, min_unique >= 0.f && min_unique <= 1.f, DFE_E_ARG, "%s: min_unique=%g must be in [0, 1]", fn, (double)min_unique);
    return DFE_OK;
}

// The launches behind the checks: sgm_plane.hip's path kernel (paths != 0), then the pick.  work: dfe_sgm_work_planes(paths, o.agg != NULL)
// planes; o: where the results go, and min_unique
int sgpk_run(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, int subpixel, float *work, SgmpOut o,
             const SgmPen *pen = nullptr) {
    const SgmpJob a = sgmp_job(volume, H, W, hWin, wWin, P1, P2, paths, work, o.agg);
    if (paths) {
        int rc = sgmp_launch_paths(ctx, a, pen);
        if (rc) return rc;
    }
    DfeProfScope prof(ctx);
    const dim3 grid((unsigned)dfe_cdiv((long long)H * W, 4));
    if (subpixel) hipLaunchKernelGGL(sgpk_pick_kernel<true>, grid, dim3(256), 0, ctx->stream, a, o);
    else hipLaunchKernelGGL(sgpk_pick_kernel<false>, grid, dim3(256), 0, ctx->stream, a, o);
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "sgpk_pick_kernel";
    return DFE_OK;
}

// The guide of a one call: its own frame 0 [C][H][W], all channels, cropped to the Hr x Wr pixels at (pad_t, pad_l) the volume's plane is
// pasted at; bytes read as float(byte) * scale
SgmGuide sgm_frame_guide(const void *I0, bool bytes, float scale, int C, int H, int W, int pad_t, int pad_l, float sigma, float P2_edge) {
    const size_t off = (size_t)pad_t * W + pad_l;
    const void *g = bytes ? (const void *)((const uint8_t *)I0 + off) : (const void *)((const float *)I0 + off);
    return SgmGuide{g, bytes, scale, C, (size_t)H * W, W, sigma, P2_edge};
}

// the penalty planes of a guided call into `planes` (sgm_penalty_floats of them) and `pen`; *use = pen, or NULL where the call is not guided
int sgm_guide_planes(dfe_ctx *ctx, const SgmGuide *gd, int H, int W, float P2, unsigned paths, float *planes, SgmPen *pen, const SgmPen **use) {
    *use = nullptr;
    if (!gd || !paths || !sgm_guided(*gd)) return DFE_OK;
    const int rc = sgm_penalty_run(ctx, *gd, H, W, P2, paths, planes, pen);
    if (!rc) *use = pen;
    return rc;
}

// the SSD one call behind its device guard, on float frames (gd: sigma and P2_edge of the guided entries, else NULL)
int sgpk_ssd_pair(dfe_ctx *ctx, const char *fn, const float *I0, const float *I1, const uint8_t *B0, const uint8_t *B1, float scale, int C, int H, int W, int k,
                  int hWin, int wWin, float foe_x, float foe_y, float P1, float P2, unsigned paths, int subpixel, float min_unique, float *flow, float *scores,
                  float *depth, float *depth_conf, const SgmGuide *gd = nullptr) {
    // the single-scale step's checks, in its order, then the aggregation's and the pick's: everything is refused before any launch
    const bool bytes = B0 || B1;
    DFE_REQUIRE(ctx, (bytes ? B0 && B1 : I0 && I1) && flow && scores, DFE_E_ARG, "%s: NULL tensor", fn);
    DFE_REQUIRE(ctx, C > 0 && k > 0 && hWin > 0 && wWin > 0, DFE_E_ARG, "%s: C=%d k=%d win=%dx%d", fn, C, k, hWin, wWin);
    DFE_REQUIRE(ctx, (depth == nullptr) == (depth_conf == nullptr), DFE_E_ARG, "%s: depth and depth_conf go together", fn);
    const int Ho = H - k + 1 - hWin + 1, Wo = W - k + 1 - wWin + 1;
    DFE_REQUIRE(ctx, Ho > 0 && Wo > 0, DFE_E_SHAPE, "%s: frame %dx%d too small for kernel %d + window %dx%d", fn, H, W, k, hWin, wWin);
    DFE_REQUIRE(ctx, paths != 0u, DFE_E_ARG, "%s: paths=0x%x must be 1 .. 255 (bit r = direction r)", fn, paths);
    int rc = sgpk_check(ctx, fn, Ho, Wo, hWin, wWin, P1, P2, paths, min_unique);
    if (!rc && gd) rc = sgm_guide_check(ctx, fn, P1, P2, *gd);
    if (rc) return rc;
    float *f0 = nullptr, *f1 = nullptr, *vol = nullptr, *work = nullptr, *planes = nullptr;
    const size_t n = (size_t)C * H * W, plane = (size_t)Ho * Wo * hWin * wWin;
    // The whole volume: the vertical paths need every row, so there are no bands.  In the PLAIN arena: the volume and the n planes lie a
    // fixed distance apart, and in physically contiguous memory the build and the path launch are slower for it (VGA, 17 x 17, 4 paths:
    // the build 163 against 90 us, the paths 810 against 755 us; the call 1.41 against 1.06 ms -- DESIGN.md section 4.32)
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        if (bytes) { f0 = c.take<float>(n); f1 = c.take<float>(n); }
        vol = c.take<float>(plane);
        work = c.take<float>(dfe_sgm_work_planes(paths, false) * plane);
        if (gd && gd->sigma > 0.f) planes = c.take<float>(sgm_penalty_floats(paths, Ho, Wo));
    }, /*plain*/ true);
    if (rc) return rc;
    if (bytes) {   // float(byte) * scale, as dfe_flow_depth_pair_u8 converts
        DfeStageScope st(ctx, DFE_STAGE_LOAD);
        rc = dfe_u8_to_f32(ctx, B0, (int64_t)n, scale, f0);
        if (!rc) rc = dfe_u8_to_f32(ctx, B1, (int64_t)n, scale, f1);
        if (rc) return rc;
        I0 = f0; I1 = f1;
    }
    const int pad_t = (H - Ho) / 2, pad_l = (W - Wo) / 2;   // the rule of flow_step.hip
    {   // the staged public call itself (it carves nothing): the same kernel, the same bits
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        rc = dfe_ssd_cost_volume_f32(ctx, I0, I1, C, H, W, k, k, hWin, wWin, vol);
        if (rc) return rc;
        SgmpOut o{};
        o.fy = flow; o.fx = flow + (size_t)H * W;
        o.unique = scores; o.min_unique = min_unique;
        o.pitch = W; o.pad_t = pad_t; o.pad_l = pad_l;
        SgmPen pen{};
        const SgmPen *use = nullptr;
        if (gd) {   // (the float frame 0, converted above for the byte entry)
            const SgmGuide g = sgm_frame_guide(I0, false, 1.f, C, H, W, pad_t, pad_l, gd->sigma, gd->P2_edge);
            rc = sgm_guide_planes(ctx, &g, Ho, Wo, P2, paths, planes, &pen, &use);
            if (rc) return rc;
        }
        rc = sgpk_run(ctx, vol, Ho, Wo, hWin, wWin, P1, P2, paths, subpixel, work, o, use);
        if (rc) return rc;
    }
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    return dfe_pair_border_depth(ctx, flow, scores, H, W, pad_t, pad_l, Ho, Wo, foe_x, foe_y, depth, depth_conf);
}

// The census one calls behind their device guard, on census.hip's front end: the staged volume, then the plain aggregate (pick == false:
// sgmp_run) or the pick (sgpk_run).  Everything is refused before any launch: the census checks, then the aggregation's, then the pick's
int sgm_census_pair(dfe_ctx *ctx, const char *fn, bool pick, const void *I0, const void *I1, bool bytes, int C, int H, int W, int k, int hWin, int wWin, int agg,
                    float foe_x, float foe_y, float P1, float P2, unsigned paths, int subpixel, float min_unique, float *flow, float *match, float *unique,
                    float *depth, float *depth_conf, const SgmGuide *gd = nullptr) {
    DfeCensusPair g;
    int rc = dfe_census_pair_check(ctx, fn, I0 && I1 && flow && match, (depth == nullptr) == (depth_conf == nullptr), C, H, W, k, hWin, wWin, agg, &g);
    if (rc) return rc;
    if (pick) DFE_REQUIRE(ctx, paths != 0u, DFE_E_ARG, "%s: paths=0x%x must be 1 .. 255 (bit r = direction r)", fn, paths);
    rc = pick ? sgpk_check(ctx, fn, g.Ha, g.Wa, hWin, wWin, P1, P2, paths, min_unique) : sgmp_check(ctx, fn, g.Ha, g.Wa, hWin, wWin, P1, P2, paths);
    if (!rc && gd) rc = sgm_guide_check(ctx, fn, P1, P2, *gd);
    if (rc) return rc;
    uint64_t *sig0 = nullptr, *sig1 = nullptr;
    float *vol = nullptr, *work = nullptr, *planes = nullptr;
    SgmGuide fg{};                               // the guide of a guided entry: frame 0 on the region (scale: gd's)
    if (gd) fg = sgm_frame_guide(I0, bytes, gd->scale, C, H, W, g.pad_t, g.pad_l, gd->sigma, gd->P2_edge);
    const size_t n = (size_t)C * g.Hp * g.Wp, plane = (size_t)g.Ha * g.Wa * hWin * wWin;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        sig0 = c.take<uint64_t>(n);
        sig1 = c.take<uint64_t>(n);
        vol = c.take<float>(plane);
        work = c.take<float>(dfe_sgm_work_planes(paths, false) * plane);
        if (gd && sgm_guided(fg)) planes = c.take<float>(sgm_penalty_floats(paths, g.Ha, g.Wa));
    });
    if (rc) return rc;
    rc = dfe_census_pair_transforms(ctx, I0, I1, bytes, C, H, W, k, sig0, sig1);
    if (rc) return rc;
    {
        DfeStageScope st(ctx, DFE_STAGE_MATCH);
        rc = dfe_census_cost_volume_f32(ctx, sig0, sig1, C, g.Hp, g.Wp, hWin, wWin, agg, vol);   // the staged public call itself: the same kernel, the same bits
        if (rc) return rc;
        if (unique) DFE_HIP(ctx, hipMemsetAsync(unique, 0, (size_t)H * W * sizeof(float), ctx->stream));   // its border: 0, as match's
        SgmpOut o{};
        o.fy = flow; o.fx = flow + (size_t)H * W;
        o.match = match; o.raw = vol;
        o.den = (float)((k * k - 1) * C * agg * agg);
        o.unique = unique; o.min_unique = min_unique;
        o.pitch = W; o.pad_t = g.pad_t; o.pad_l = g.pad_l;
        SgmPen pen{};
        const SgmPen *use = nullptr;
        rc = sgm_guide_planes(ctx, gd ? &fg : nullptr, g.Ha, g.Wa, P2, paths, planes, &pen, &use);
        if (rc) return rc;
        rc = pick ? sgpk_run(ctx, vol, g.Ha, g.Wa, hWin, wWin, P1, P2, paths, subpixel, work, o, use)
                  : sgmp_run(ctx, vol, g.Ha, g.Wa, hWin, wWin, P1, P2, paths, work, o, use);
        if (rc) return rc;
    }
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    return dfe_pair_border_depth(ctx, flow, match, H, W, g.pad_t, g.pad_l, g.Ha, g.Wa, foe_x, foe_y, depth, depth_conf);
}

// the two pick entries behind DFE_ENTER (g: NULL for the unguided one; paths == 0 aggregates nothing and ignores the guide)
int sgpk_entry(dfe_ctx *ctx, const char *fn, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, int subpixel,
               float min_unique, float *agg, int64_t *idx, float *flow_y, float *flow_x, float *best, float *second, float *unique, const SgmGuide *g) {
    DFE_REQUIRE(ctx, volume && (agg || idx || flow_y || flow_x || best || second || unique), DFE_E_ARG, "%s: %s", fn,
                volume ? "every output is NULL" : "volume is NULL");
    DFE_REQUIRE(ctx, agg != volume, DFE_E_ARG, "%s: agg must not be the volume (every direction reads it)", fn);
    int rc = sgpk_check(ctx, fn, H, W, hWin, wWin, P1, P2, paths, min_unique);
    if (!rc && g) rc = sgm_guide_check(ctx, fn, P1, P2, *g);
    if (rc) return rc;
    const bool guided = g && paths && sgm_guided(*g);
    float *work = nullptr, *planes = nullptr;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        work = c.take<float>(dfe_sgm_work_planes(paths, agg != nullptr) * H * W * (size_t)(hWin * wWin));
        if (guided) planes = c.take<float>(sgm_penalty_floats(paths, H, W));
    });
    if (rc) return rc;
    SgmpOut o{};
    o.agg = agg;
    o.idx = (long long *)idx; o.fy = flow_y; o.fx = flow_x;
    o.best = best; o.second = second; o.unique = unique; o.min_unique = min_unique;
    o.pitch = W;
    DfeStageScope st(ctx, DFE_STAGE_MATCH);
    SgmPen pen{};
    const SgmPen *use = nullptr;
    rc = sgm_guide_planes(ctx, g, H, W, P2, paths, planes, &pen, &use);
    if (rc) return rc;
    return sgpk_run(ctx, volume, H, W, hWin, wWin, P1, P2, paths, subpixel, work, o, use);
}

}  // namespace

extern "C" {

int dfe_sgm_plane_pick_f32(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, int subpixel,
                           float min_unique, float *agg, int64_t *idx, float *flow_y, float *flow_x, float *best, float *second, float *unique) {
    DFE_ENTER(ctx);
    return sgpk_entry(ctx, "dfe_sgm_plane_pick_f32", volume, H, W, hWin, wWin, P1, P2, paths, subpixel, min_unique, agg, idx, flow_y, flow_x, best, second,
                      unique, nullptr);
}

int dfe_sgm_plane_pick_guided_f32(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths, int subpixel,
                                  float min_unique, float *agg, int64_t *idx, float *flow_y, float *flow_x, float *best, float *second, float *unique,
                                  const float *guide, int Cg, float sigma, float P2_edge) {
    DFE_ENTER(ctx);
    const SgmGuide g{guide, false, 1.f, Cg, (size_t)H * W, W, sigma, P2_edge};
    return sgpk_entry(ctx, "dfe_sgm_plane_pick_guided_f32", volume, H, W, hWin, wWin, P1, P2, paths, subpixel, min_unique, agg, idx, flow_y, flow_x, best,
                      second, unique, &g);
}

int dfe_flow_depth_pair_sgm_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x, float foe_y,
                                float P1, float P2, unsigned paths, int subpixel, float min_unique, float *flow, float *scores, float *depth,
                                float *depth_conf) {
    DFE_ENTER(ctx);
    return sgpk_ssd_pair(ctx, "dfe_flow_depth_pair_sgm_f32", I0, I1, nullptr, nullptr, 1.f, C, H, W, k, hWin, wWin, foe_x, foe_y, P1, P2, paths, subpixel,
                         min_unique, flow, scores, depth, depth_conf);
}

int dfe_flow_depth_pair_sgm_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x, float foe_y,
                               float scale, float P1, float P2, unsigned paths, int subpixel, float min_unique, float *flow, float *scores, float *depth,
                               float *depth_conf) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_flow_depth_pair_sgm_u8";
    DFE_REQUIRE(ctx, I0 && I1, DFE_E_ARG, "%s: NULL frame", fn);
    DFE_REQUIRE(ctx, C > 0 && H > 0 && W > 0 && scale > 0, DFE_E_ARG, "%s: C=%d %dx%d scale=%g", fn, C, H, W, (double)scale);
    return sgpk_ssd_pair(ctx, fn, nullptr, nullptr, I0, I1, scale, C, H, W, k, hWin, wWin, foe_x, foe_y, P1, P2, paths, subpixel, min_unique, flow, scores, depth,
                         depth_conf);
}

int dfe_census_flow_depth_pair_sgm_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                                       float foe_y, float P1, float P2, unsigned paths, float *flow, float *match, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    return sgm_census_pair(ctx, "dfe_census_flow_depth_pair_sgm_f32", false, I0, I1, false, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths, 0, 0.f, flow,
                           match, nullptr, depth, depth_conf);
}

int dfe_census_flow_depth_pair_sgm_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                                      float foe_y, float scale, float P1, float P2, unsigned paths, float *flow, float *match, float *depth,
                                      float *depth_conf) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, scale > 0, DFE_E_ARG, "dfe_census_flow_depth_pair_sgm_u8: scale=%g must be positive", (double)scale);
    return sgm_census_pair(ctx, "dfe_census_flow_depth_pair_sgm_u8", false, I0, I1, true, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths, 0, 0.f, flow,
                           match, nullptr, depth, depth_conf);
}

int dfe_census_flow_depth_pair_sgm2_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, int agg, float foe_x,
                                        float foe_y, float P1, float P2, unsigned paths, int subpixel, float min_unique, float *flow, float *match,
                                        float *unique, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    return sgm_census_pair(ctx, "dfe_census_flow_depth_pair_sgm2_f32", true, I0, I1, false, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths, subpixel,
                           min_unique, flow, match, unique, depth, depth_conf);
}

int dfe_census_flow_depth_pair_sgm2_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, int agg,
                                       float foe_x, float foe_y, float scale, float P1, float P2, unsigned paths, int subpixel, float min_unique, float *flow,
                                       float *match, float *unique, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, scale > 0, DFE_E_ARG, "dfe_census_flow_depth_pair_sgm2_u8: scale=%g must be positive", (double)scale);
    return sgm_census_pair(ctx, "dfe_census_flow_depth_pair_sgm2_u8", true, I0, I1, true, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths, subpixel,
                           min_unique, flow, match, unique, depth, depth_conf);
}

int dfe_flow_depth_pair_sgm_guided_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x, float foe_y,
                                       float P1, float P2, unsigned paths, int subpixel, float min_unique, float sigma, float P2_edge, float *flow,
                                       float *scores, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    const SgmGuide gd{nullptr, false, 1.f, C, 0, 0, sigma, P2_edge};
    return sgpk_ssd_pair(ctx, "dfe_flow_depth_pair_sgm_guided_f32", I0, I1, nullptr, nullptr, 1.f, C, H, W, k, hWin, wWin, foe_x, foe_y, P1, P2, paths, subpixel,
                         min_unique, flow, scores, depth, depth_conf, &gd);
}

int dfe_flow_depth_pair_sgm_guided_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                                      float foe_y, float scale, float P1, float P2, unsigned paths, int subpixel, float min_unique, float sigma,
                                      float P2_edge, float *flow, float *scores, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    const char *fn = "dfe_flow_depth_pair_sgm_guided_u8";
    DFE_REQUIRE(ctx, I0 && I1, DFE_E_ARG, "%s: NULL frame", fn);
    DFE_REQUIRE(ctx, C > 0 && H > 0 && W > 0 && scale > 0, DFE_E_ARG, "%s: C=%d %dx%d scale=%g", fn, C, H, W, (double)scale);
    const SgmGuide gd{nullptr, false, 1.f, C, 0, 0, sigma, P2_edge};
    return sgpk_ssd_pair(ctx, fn, nullptr, nullptr, I0, I1, scale, C, H, W, k, hWin, wWin, foe_x, foe_y, P1, P2, paths, subpixel, min_unique, flow, scores, depth,
                         depth_conf, &gd);
}

int dfe_census_flow_depth_pair_sgm_guided_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, int agg,
                                              float foe_x, float foe_y, float P1, float P2, unsigned paths, int subpixel, float min_unique, float sigma,
                                              float P2_edge, float *flow, float *match, float *unique, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    const SgmGuide gd{nullptr, false, 1.f, C, 0, 0, sigma, P2_edge};
    return sgm_census_pair(ctx, "dfe_census_flow_depth_pair_sgm_guided_f32", true, I0, I1, false, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths,
                           subpixel, min_unique, flow, match, unique, depth, depth_conf, &gd);
}

int dfe_census_flow_depth_pair_sgm_guided_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin, int agg,
                                             float foe_x, float foe_y, float scale, float P1, float P2, unsigned paths, int subpixel, float min_unique,
                                             float sigma, float P2_edge, float *flow, float *match, float *unique, float *depth, float *depth_conf) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, scale > 0, DFE_E_ARG, "dfe_census_flow_depth_pair_sgm_guided_u8: scale=%g must be positive", (double)scale);
    const SgmGuide gd{nullptr, true, scale, C, 0, 0, sigma, P2_edge};
    return sgm_census_pair(ctx, "dfe_census_flow_depth_pair_sgm_guided_u8", true, I0, I1, true, C, H, W, k, hWin, wWin, agg, foe_x, foe_y, P1, P2, paths,
                           subpixel, min_unique, flow, match, unique, depth, depth_conf, &gd);
}

}  // extern "C"
