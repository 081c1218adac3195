// temporal_splat.hip -- the temporal depth filter's sub-pixel forward warp: a four-tap (bilinear) splat on INTEGER accumulators (not in the
// reference; the definition: include/dfe.h).
//   dfe_forward_splat_f32         values [C][H][W] and weights [H][W] spread along flow [2][H][W] over a region R: every source goes to the
//                                 four pixels around where it lands, a target is the weighted mean of what reached it
//   dfe_temporal_step_splat_f32   that and dfe_temporal_fuse_f32 in one call: the prior stays in registers
//
// Layout: per pixel of R, (C + 2) 64-bit sums as PLANES [C + 2][n] (A_0 .. A_{C-1}, B, U) and one 32-bit front word, in the ctx's side
// buffer.  Clear = one kernel of 16-byte stores (zeros; all-ones on the front).  Front = a thread per pixel of R, one no-return 32-bit
// integer minimum per tap.  Accumulate = the same thread per pixel, per tap the front read back and (C + 2) no-return 64-bit integer adds;
// neighbouring lanes add to neighbouring words of one plane, whole runs per wave instruction.  In the LDS form of either pass a workgroup
// owns 8 x 64 sources and a 14 x 70 window of cells laid where the tile's CENTRE source goes (a smooth flow carries the whole tile there,
// however long the flow is); taps inside the window are combined in LDS, the others go to global memory, and every touched cell is sent
// once.  Integer sums and minima do not depend on the order or the grouping of their terms: both forms, and every run, give the same bits.
// Resolve = a thread per pixel of the FRAME as in temporal.hip; the fused resolve runs temporal_fuse_px on the quotients in registers.
#include "temporal_common.h"

namespace {

constexpr int kSplatAxis = 128, kSplatUnit = kSplatAxis * kSplatAxis;   // tent weights per axis; the four of a source sum to 16384
constexpr int kSplatTileH = 8, kSplatMargin = 3;                        // the LDS form: 8 x 64 sources, a margin of 3 cells on every side
constexpr int kSplatWinH = kSplatTileH + 2 * kSplatMargin, kSplatWinW = 64 + 2 * kSplatMargin, kSplatWin = kSplatWinH * kSplatWinW;
constexpr bool kSplatLdsDefault = true;                                 // option "splat_lds" left automatic: the LDS forms (measured)

struct SplatArgs {
    float ztol, quant;
    int min_u;                // max(1, ceil(min_cover 16384))
    long long *acc;           // [C + 2][n]
    unsigned *front;          // [n]; null without a key
    long long n;              // pixels of R
    float *cover;             // [H][W] or null
};

template <int C> struct SplatSource {
    float k, by, bx;          // key + 0, the floor of the position
    int uy1, ux1;             // the far taps' weights per axis, 0 .. 128
    long long V[C], Wf;
};

__device__ __forceinline__ float splat_unordered(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

__device__ __forceinline__ void splat_add(long long *p, long long v) {
    (void)__hip_atomic_fetch_add((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void splat_add_lds(long long *p, long long v) {
    (void)__hip_atomic_fetch_add((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the source at frame pixel (Y, X) of R in fixed point; false: there is none (no sample, a flow or key that is not finite, a value
// outside the quant range, a weight that rounds to 0)
template <int C> __device__ __forceinline__ bool splat_source(const TemporalFrame &f, const WarpArgs &a, float quant, int Y, int X, SplatSource<C> *s) {
#pragma clang fp contract(off)
    const long long HW = (long long)f.H * f.W, p = (long long)Y * f.W + X;
    float val[C];
    if (dfe_sample_read<C>(a.v, a.w, HW, p, val) == 0.f) return false;
    const float fy = a.flow[p], fx = a.flow[HW + p];
    if (!(dfe_finite(fy) && dfe_finite(fx))) return false;
    s->k = 0.f;
    if (a.key) {
        const float k = a.key[p];
        if (!dfe_finite(k)) return false;
        s->k = k + 0.0f;   // -0 counts as +0
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float t = val[c];
        if (a.has_gain) t = a.gain[c] * t;
        if (a.has_bias) t = t + a.bias[c];
        const float q = t * quant;
        if (!(fabsf(q) <= 16777216.0f)) return false;   // (false for NaN)
        s->V[c] = (long long)rintf(q);
    }
    const float w = a.w[p], wd = a.decay == 1.f ? w : w * a.decay;
    s->Wf = (long long)rintf(fminf(wd, 256.0f) * 256.0f);
    if (s->Wf == 0) return false;
    const float py = (float)Y + fy, px = (float)X + fx;
    s->by = floorf(py);
    s->bx = floorf(px);
    s->uy1 = (int)floorf((py - s->by) * 128.0f + 0.5f);
    s->ux1 = (int)floorf((px - s->bx) * 128.0f + 0.5f);
    return true;
}

// tap (i, j) of a source: its weight and its target (yt, xt) in R's coordinates; false: the tap does not exist or lies outside R
template <int C> __device__ __forceinline__ bool splat_tap(const TemporalFrame &f, const SplatSource<C> &s, int i, int j, int *u, int *yt, int *xt) {
#pragma clang fp contract(off)
    *u = (i ? s.uy1 : kSplatAxis - s.uy1) * (j ? s.ux1 : kSplatAxis - s.ux1);
    if (*u == 0) return false;
    const float ty = s.by + (float)i, tx = s.bx + (float)j;
    // decided on the floats: only a target inside R (inside the frame) is converted to int
    if (!(ty >= (float)f.y0 && ty <= (float)(f.y0 + f.Ho - 1) && tx >= (float)f.x0 && tx <= (float)(f.x0 + f.Wo - 1))) return false;
    *yt = (int)ty - f.y0;
    *xt = (int)tx - f.x0;
    return (unsigned)*yt < (unsigned)f.Ho && (unsigned)*xt < (unsigned)f.Wo;   // (a bound above 2^24 that moved when it became a float)
}

// whether a tap of a source with key k contributes to target t: within ztol behind the front
__device__ __forceinline__ bool splat_in_front(const SplatArgs &sa, float k, long long t) {
#pragma clang fp contract(off)
    return !sa.front || (k - splat_unordered(sa.front[t])) <= sa.ztol;
}

// ---- clear: zeros on the sums, all-ones on the front, 16 bytes per thread (the buffers' ends are padded to 256 bytes) ----
__global__ __launch_bounds__(256) void splat4_clear_kernel(uint4 *acc, long long nacc, uint4 *front, long long nfront) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nacc) acc[i] = make_uint4(0u, 0u, 0u, 0u);
    else if (i < nacc + nfront) front[i - nacc] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// ---- front: one thread per pixel of R ----
template <int C> __global__ __launch_bounds__(256) void splat4_front_kernel(TemporalFrame f, WarpArgs a, SplatArgs sa) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= f.Wo || y >= f.Ho) return;
    SplatSource<C> s;
    if (!splat_source<C>(f, a, sa.quant, f.y0 + y, f.x0 + x, &s)) return;
    const unsigned word = temporal_ordered(s.k);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        int u, yt, xt;
        if (splat_tap<C>(f, s, t >> 1, t & 1, &u, &yt, &xt))
            (void)__hip_atomic_fetch_min(sa.front + ((long long)yt * f.Wo + xt), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the origin, in R's coordinates, of the LDS window of the tile at (ty0, tx0): the tile's, moved by the floor of the flow at the tile's
// centre (0 where that is not a number of a few thousand pixels: the window is a matter of speed, never of the result)
__device__ __forceinline__ void splat_window(const TemporalFrame &f, const WarpArgs &a, int ty0, int tx0, long long *wy0, long long *wx0) {
    const long long HW = (long long)f.H * f.W;
    const long long pc = (long long)(f.y0 + min(ty0 + kSplatTileH / 2, f.Ho - 1)) * f.W + (f.x0 + min(tx0 + 32, f.Wo - 1));
    const float cfy = a.flow[pc], cfx = a.flow[HW + pc];
    *wy0 = (long long)ty0 - kSplatMargin + (fabsf(cfy) <= 32768.f ? (int)floorf(cfy) : 0);
    *wx0 = (long long)tx0 - kSplatMargin + (fabsf(cfx) <= 32768.f ? (int)floorf(cfx) : 0);
}

// ---- front through LDS: a workgroup per 8 x 64 sources, the minimum of a window cell taken in LDS, every touched cell sent once ----
template <int C> __global__ __launch_bounds__(256) void splat4_front_lds_kernel(TemporalFrame f, WarpArgs a, SplatArgs sa) {
    __shared__ unsigned cell[kSplatWin];
    const int ty0 = blockIdx.y * kSplatTileH, tx0 = blockIdx.x * 64;
    long long wy0, wx0;
    splat_window(f, a, ty0, tx0, &wy0, &wx0);
    for (int i = threadIdx.x; i < kSplatWin; i += 256) cell[i] = ~0u;
    __syncthreads();
    const int x = tx0 + (threadIdx.x & 63);
#pragma unroll
    for (int r = 0; r < kSplatTileH / 4; ++r) {
        const int y = ty0 + 4 * r + (threadIdx.x >> 6);
        SplatSource<C> s;
        if (x >= f.Wo || y >= f.Ho || !splat_source<C>(f, a, sa.quant, f.y0 + y, f.x0 + x, &s)) continue;
        const unsigned word = temporal_ordered(s.k);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int u, yt, xt;
            if (!splat_tap<C>(f, s, t >> 1, t & 1, &u, &yt, &xt)) continue;
            const long long wy = yt - wy0, wx = xt - wx0;
            if ((unsigned long long)wy < (unsigned long long)kSplatWinH && (unsigned long long)wx < (unsigned long long)kSplatWinW)
                (void)__hip_atomic_fetch_min(cell + ((int)wy * kSplatWinW + (int)wx), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else
                (void)__hip_atomic_fetch_min(sa.front + ((long long)yt * f.Wo + xt), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    // a touched cell is no longer all-ones (no finite key maps there) and lies in R
    for (int i = threadIdx.x; i < kSplatWin; i += 256) {
        const unsigned word = cell[i];
        if (word != ~0u)
            (void)__hip_atomic_fetch_min(sa.front + ((wy0 + i / kSplatWinW) * f.Wo + (wx0 + i % kSplatWinW)), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the (C + 2) sums of one tap on planes of `stride` words
template <int C, bool Lds> __device__ __forceinline__ void splat_tap_add(long long *cell, long long stride, const SplatSource<C> &s, int u) {
    const long long omega = (long long)u * s.Wf;
    long long term[C + 2];
#pragma unroll
    for (int c = 0; c < C; ++c) term[c] = omega * s.V[c];
    term[C] = omega;
    term[C + 1] = (long long)u;
#pragma unroll
    for (int c = 0; c < C + 2; ++c) {
        if constexpr (Lds) splat_add_lds(cell + c * stride, term[c]);
        else splat_add(cell + c * stride, term[c]);
    }
}

// ---- accumulate, every tap to global memory: one thread per pixel of R ----
template <int C> __global__ __launch_bounds__(256) void splat4_accum_kernel(TemporalFrame f, WarpArgs a, SplatArgs sa) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= f.Wo || y >= f.Ho) return;
    SplatSource<C> s;
    if (!splat_source<C>(f, a, sa.quant, f.y0 + y, f.x0 + x, &s)) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        int u, yt, xt;
        if (!splat_tap<C>(f, s, t >> 1, t & 1, &u, &yt, &xt)) continue;
        const long long q = (long long)yt * f.Wo + xt;
        if (splat_in_front(sa, s.k, q)) splat_tap_add<C, false>(sa.acc + q, sa.n, s, u);
    }
}

// ---- accumulate through LDS: a workgroup per 8 x 64 sources, two per thread ----
template <int C> __global__ __launch_bounds__(256) void splat4_accum_lds_kernel(TemporalFrame f, WarpArgs a, SplatArgs sa) {
    __shared__ long long cell[(C + 2) * kSplatWin];
    const int ty0 = blockIdx.y * kSplatTileH, tx0 = blockIdx.x * 64;
    long long wy0, wx0;
    splat_window(f, a, ty0, tx0, &wy0, &wx0);
    for (int i = threadIdx.x; i < (C + 2) * kSplatWin; i += 256) cell[i] = 0;
    __syncthreads();
    const int x = tx0 + (threadIdx.x & 63);
#pragma unroll
    for (int r = 0; r < kSplatTileH / 4; ++r) {
        const int y = ty0 + 4 * r + (threadIdx.x >> 6);
        SplatSource<C> s;
        if (x >= f.Wo || y >= f.Ho || !splat_source<C>(f, a, sa.quant, f.y0 + y, f.x0 + x, &s)) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int u, yt, xt;
            if (!splat_tap<C>(f, s, t >> 1, t & 1, &u, &yt, &xt)) continue;
            const long long q = (long long)yt * f.Wo + xt;
            if (!splat_in_front(sa, s.k, q)) continue;
            const long long wy = yt - wy0, wx = xt - wx0;
            if ((unsigned long long)wy < (unsigned long long)kSplatWinH && (unsigned long long)wx < (unsigned long long)kSplatWinW)
                splat_tap_add<C, true>(cell + ((int)wy * kSplatWinW + (int)wx), kSplatWin, s, u);
            else
                splat_tap_add<C, false>(sa.acc + q, sa.n, s, u);
        }
    }
    __syncthreads();
    // a touched cell has U != 0 and lies in R (taps outside R were dropped before they were added)
    for (int i = threadIdx.x; i < kSplatWin; i += 256) {
        if (cell[(C + 1) * kSplatWin + i] == 0) continue;
        const long long q = (wy0 + i / kSplatWinW) * f.Wo + (wx0 + i % kSplatWinW);
#pragma unroll
        for (int c = 0; c < C + 2; ++c) splat_add(sa.acc + c * sa.n + q, cell[c * kSplatWin + i]);
    }
}

// ---- what the resolve leaves at a pixel of R: the quotients, the weight, the cover ----
template <int C> __device__ __forceinline__ void splat_quotient(const TemporalFrame &f, const SplatArgs &sa, int Y, int X, float (&val)[C], float *wv, float *cov) {
#pragma clang fp contract(off)
    const long long q = (long long)(Y - f.y0) * f.Wo + (X - f.x0);
    const long long B = sa.acc[C * sa.n + q], U = sa.acc[(C + 1) * sa.n + q];
    *wv = 0.f;
    *cov = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = 0.f;
    if (!(B > 0 && U >= (long long)sa.min_u)) return;
    const float fb = (float)B;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = ((float)sa.acc[c * sa.n + q] / fb) / sa.quant;
    *wv = fb / (256.0f * (float)(U > kSplatUnit ? U : (long long)kSplatUnit));
    *cov = (float)U / 16384.0f;
}

// ---- resolve: one thread per pixel of the frame ----
template <int C> __global__ __launch_bounds__(256) void splat4_resolve_kernel(TemporalFrame f, WarpArgs a, SplatArgs sa) {
    int Y, X;
    bool inR;
    if (!temporal_pixel(f, &Y, &X, &inR)) return;
    const long long HW = (long long)f.H * f.W, p = (long long)Y * f.W + X;
    float val[C], wv = 0.f, cov = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = 0.f;
    if (inR) splat_quotient<C>(f, sa, Y, X, val, &wv, &cov);
#pragma unroll
    for (int c = 0; c < C; ++c) a.out[c * HW + p] = val[c];
    a.wout[p] = wv;
    if (sa.cover) sa.cover[p] = cov;
}

// ---- the fused resolve: divide, fuse in registers; the prior reaches memory only where it is asked for ----
template <int C> __global__ __launch_bounds__(256) void splat4_step_kernel(TemporalFrame f, WarpArgs a, SplatArgs sa, FuseArgs u) {
    int Y, X;
    bool inR;
    if (!temporal_pixel(f, &Y, &X, &inR)) return;
    const long long HW = (long long)f.H * f.W, p = (long long)Y * f.W + X;
    float z[C], m[C], wp = 0.f, wm = 0.f, cov = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = m[c] = 0.f;
    if (inR) {
        splat_quotient<C>(f, sa, Y, X, z, &wp, &cov);
#pragma unroll
        for (int c = 0; c < C; ++c) m[c] = u.meas[c * HW + p];
        wm = u.wm[p];
    }
    if (a.out) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.out[c * HW + p] = z[c];
    }
    if (a.wout) a.wout[p] = wp;
    if (sa.cover) sa.cover[p] = cov;
    temporal_fuse_store<C>(f, u, p, inR, z, wp, m, wm);
}

// ---- host ----
int splat_check(dfe_ctx *ctx, const char *fn, float ztol, float quant, float min_cover, SplatArgs *sa) {
    DFE_REQUIRE(ctx, temporal_finite(ztol) && ztol >= 0.f, DFE_E_ARG, "%s: ztol=%g must be finite and >= 0", fn, (double)ztol);
    DFE_REQUIRE(ctx, temporal_finite(quant) && quant > 0.f, DFE_E_ARG, "%s: quant=%g must be finite and > 0", fn, (double)quant);
    DFE_REQUIRE(ctx, min_cover >= 0.f && min_cover <= 1.f, DFE_E_ARG, "%s: min_cover=%g must lie in [0, 1]", fn, (double)min_cover);   // (false for NaN)
    const int mu = (int)ceilf(min_cover * 16384.0f);
    sa->ztol = ztol; sa->quant = quant; sa->min_u = mu > 1 ? mu : 1;
    return DFE_OK;
}

// the accumulators in the ctx's side buffer (grown once, then no allocation per call), the clear, the front and the accumulate pass
template <int C> int splat_passes(dfe_ctx *ctx, const TemporalFrame &f, const WarpArgs &a, SplatArgs *sa) {
    const size_t n = (size_t)f.Ho * f.Wo;
    auto layout = [&](DfeCarve &carve) {
        sa->acc = carve.take<long long>((C + 2) * n);
        sa->front = a.key ? carve.take<unsigned>(n) : nullptr;
    };
    DfeCarve size;
    layout(size);
    void *aux = nullptr;
    if (int rc = dfe_aux_scratch(ctx, size.off, &aux)) return rc;
    DfeCarve carve(aux);
    layout(carve);
    sa->n = (long long)n;
    {
        DfeProfScope prof(ctx);
        const long long nacc = (long long)(((C + 2) * n * sizeof(long long) + 15) / 16), nfront = a.key ? (long long)((n * sizeof(unsigned) + 15) / 16) : 0;
        hipLaunchKernelGGL(splat4_clear_kernel, dim3((unsigned)((nacc + nfront + 255) / 256)), dim3(256), 0, ctx->stream, (uint4 *)sa->acc, nacc, (uint4 *)sa->front, nfront);
        DFE_LAUNCH_CHECK(ctx);
    }
    const bool lds = ctx->opt_bool(DFE_OPT_SPLAT_LDS, kSplatLdsDefault);
    const dim3 tiles((unsigned)dfe_cdiv(f.Wo, 64), (unsigned)dfe_cdiv(f.Ho, kSplatTileH));
    if (a.key) {
        DfeProfScope prof(ctx);
        if (lds) hipLaunchKernelGGL((splat4_front_lds_kernel<C>), tiles, dim3(256), 0, ctx->stream, f, a, *sa);
        else hipLaunchKernelGGL((splat4_front_kernel<C>), temporal_grid(f.Ho, f.Wo), dim3(256), 0, ctx->stream, f, a, *sa);
        DFE_LAUNCH_CHECK(ctx);
    }
    DfeProfScope prof(ctx);
    if (lds)
        hipLaunchKernelGGL((splat4_accum_lds_kernel<C>), tiles, dim3(256), 0, ctx->stream, f, a, *sa);
    else
        hipLaunchKernelGGL((splat4_accum_kernel<C>), temporal_grid(f.Ho, f.Wo), dim3(256), 0, ctx->stream, f, a, *sa);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_forward_splat_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key, int y0, int x0, int Ho,
                          int Wo, const float *gain, const float *bias, float decay, float ztol, float quant, float min_cover, float *out, float *wout,
                          float *cover) {
    static const char *fn = "dfe_forward_splat_f32";
    DFE_ENTER(ctx);
    WarpArgs a{};
    SplatArgs sa{};
    if (int rc = temporal_warp_check(ctx, fn, v, C, H, W, w, flow, gain, bias, decay, &a)) return rc;
    if (int rc = splat_check(ctx, fn, ztol, quant, min_cover, &sa)) return rc;
    DFE_REQUIRE(ctx, out && wout, DFE_E_ARG, "%s: NULL tensor", fn);
    if (int rc = dfe_region_check(ctx, fn, H, W, y0, x0, Ho, Wo)) return rc;
    const long long HW = (long long)H * W;
    const TemporalSpan outs[] = {{out, C * HW}, {wout, HW}, {cover, HW}}, ins[] = {{v, C * HW}, {w, HW}, {flow, 2 * HW}, {key, HW}};
    if (int rc = temporal_overlap_check(ctx, fn, outs, 3, ins, 4)) return rc;
    a.key = key; a.out = out; a.wout = wout; sa.cover = cover;
    const TemporalFrame f{H, W, y0, x0, Ho, Wo};
    return dfe_dispatch_1to4(C, [&](auto c) {
        constexpr int Cc = decltype(c)::value;
        DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
        if (int rc = splat_passes<Cc>(ctx, f, a, &sa)) return rc;
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((splat4_resolve_kernel<Cc>), temporal_grid(H, W), dim3(256), 0, ctx->stream, f, a, sa);
        DFE_LAUNCH_CHECK(ctx);
        return (int)DFE_OK;
    });
}

int dfe_temporal_step_splat_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key, int y0, int x0,
                                int Ho, int Wo, const float *gain, const float *bias, float decay, float ztol, float quant, float min_cover,
                                const float *meas, const float *wm, float tol, float wmax, float *out, float *wout, float *flag, float *prior,
                                float *wprior, float *cover) {
    static const char *fn = "dfe_temporal_step_splat_f32";
    DFE_ENTER(ctx);
    WarpArgs a{};
    SplatArgs sa{};
    if (int rc = temporal_warp_check(ctx, fn, v, C, H, W, w, flow, gain, bias, decay, &a)) return rc;
    if (int rc = splat_check(ctx, fn, ztol, quant, min_cover, &sa)) return rc;
    DFE_REQUIRE(ctx, meas && wm && out && wout, DFE_E_ARG, "%s: NULL tensor", fn);
    if (int rc = temporal_fuse_check(ctx, fn, tol, wmax)) return rc;
    if (int rc = dfe_region_check(ctx, fn, H, W, y0, x0, Ho, Wo)) return rc;
    const long long HW = (long long)H * W;
    // the rules of dfe_temporal_step_f32: no output on the state or on another output; out / wout may be meas / wm (pointwise)
    const TemporalSpan outs[] = {{out, C * HW}, {wout, HW}, {flag, HW}, {prior, C * HW}, {wprior, HW}, {cover, HW}};
    const TemporalSpan ins[] = {{v, C * HW}, {w, HW}, {flow, 2 * HW}, {key, HW}};
    if (int rc = temporal_overlap_check(ctx, fn, outs, 6, ins, 4)) return rc;
    const TemporalSpan late[] = {{flag, HW}, {prior, C * HW}, {wprior, HW}, {cover, HW}}, pointwise[] = {{meas, C * HW}, {wm, HW}};
    if (int rc = temporal_overlap_check(ctx, fn, late, 4, pointwise, 2)) return rc;
    a.key = key; a.out = prior; a.wout = wprior; sa.cover = cover;
    const TemporalFrame f{H, W, y0, x0, Ho, Wo};
    const FuseArgs u{nullptr, nullptr, meas, wm, tol * tol, wmax, out, wout, flag};
    return dfe_dispatch_1to4(C, [&](auto c) {
        constexpr int Cc = decltype(c)::value;
        DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
        if (int rc = splat_passes<Cc>(ctx, f, a, &sa)) return rc;
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((splat4_step_kernel<Cc>), temporal_grid(H, W), dim3(256), 0, ctx->stream, f, a, sa, u);
        DFE_LAUNCH_CHECK(ctx);
        return (int)DFE_OK;
    });
}

}  // extern "C"
