// fill.hip -- hole filling: a dense field from the confident pixels of a sparse one by a confidence-weighted push-pull (not in the
// reference).
//   dfe_fill_holes_f32      values [C][H][W] and weights [H][W] over a region R -> filled values and the filled mask (the definition:
//                           include/dfe.h)
//
// The definition is per cell with a fixed order of operations, and the two forms below run the SAME device functions (fill_push_cell,
// fill_pull_px), so they give the same bits:
//   per-level kernels   push: one thread per coarse cell, its 2 x 2 children loaded from the finer level; pull: one thread per fine pixel,
//                       up to four taps of the coarser level.  A wave = 64 consecutive cells of one row.  Level 0 is read from the caller's
//                       planes (validity decided there) and its pull writes out / filled with the zero border of the frame in the same launch.
//   the apex kernel     ONE workgroup takes every level from the first one whose pyramid fits LDS: one read of that level, the pushes to
//                       the top and the pulls back down in LDS with a barrier per level, one write.  The planes are small (R of the VGA
//                       step: 3 MB), the cost is launch boundaries, and the upper levels are the ones with nothing to do per launch.
// A level is C + 1 planes [h][w]: the values, then the weight a; its pull overwrites them in place with f and the mask g (a pull reads
// the coarser level and the pixel's own cell only).  The top needs no pass: g = (a > 0) is what a tap's test `!= 0` reads off a.
#include "dfe_field.h"

#pragma clang fp contract(off)

namespace {

constexpr int kFillMaxLevels = 32;               // halvings of an int-sized grid
constexpr int kFillApexThreads = 1024;
constexpr size_t kFillApexLds = 160 * 1024;      // LDS of a CU: the one workgroup may take it all

template <int C> struct FillPx { float v[C]; float a; };

// a level's planes in memory (global or LDS): v_0 .. v_{C-1}, then a (g once pulled), each [h][w]
struct FillLevel { float *p; int h, w; };
// the caller's planes: level 0 is R inside them
struct FillFrame {
    const float *v, *w;            // [C][H][W], [H][W]
    float *out, *filled;           // [C][H][W], [H][W] or null
    int H, W, y0, x0, Ho, Wo;
};

template <int C> __device__ __forceinline__ FillPx<C> fill_zero() {
    FillPx<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) r.v[c] = 0.f;
    r.a = 0.f;
    return r;
}

// level 0 at (y, x) of R: the sample rule of dfe_field.h; where the sample does not exist the values read as 0 (what is under a zero
// weight never enters arithmetic)
template <int C> __device__ __forceinline__ FillPx<C> fill_read0(const FillFrame &f, int y, int x) {
    FillPx<C> r;
    r.a = dfe_sample_read<C>(f.v, f.w, (long long)f.H * f.W, (long long)(f.y0 + y) * f.W + f.x0 + x, r.v);
    return r.a != 0.f ? r : fill_zero<C>();
}

template <int C> __device__ __forceinline__ FillPx<C> fill_load(const float *p, long long plane, long long i) {
    FillPx<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) r.v[c] = p[c * plane + i];
    r.a = p[C * plane + i];
    return r;
}
template <int C> __device__ __forceinline__ void fill_store(float *p, long long plane, long long i, const FillPx<C> &r) {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c * plane + i] = r.v[c];
    p[C * plane + i] = r.a;
}

// PUSH: coarse cell (i, j) from its children (2i + dy, 2j + dx) of the h x w finer level, in the order (0,0) (0,1) (1,0) (1,1)
template <int C, class Child> __device__ __forceinline__ FillPx<C> fill_push_cell(int i, int j, int h, int w, Child child) {
    float s = 0.f, n[C];
#pragma unroll
    for (int c = 0; c < C; ++c) n[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * i + (k >> 1), x = 2 * j + (k & 1);
        if (y < h && x < w) {
            const FillPx<C> q = child(y, x);
            if (q.a != 0.f) {
                s += q.a;
#pragma unroll
                for (int c = 0; c < C; ++c) n[c] += q.a * q.v[c];
            }
        }
    }
    if (!(s > 0.f)) return fill_zero<C>();
    FillPx<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) r.v[c] = n[c] / s;
    r.a = fminf(s, 1.f);
    return r;
}

// PULL: pixel (y, x), own = (v, a), from the hp x wp coarser level: taps (i, j) 9/16, (i, j') 3/16, (i', j) 3/16, (i', j') 1/16 in this
// order, those outside the level or with g == 0 skipped.  Returns (f, g)
template <int C, class Par> __device__ __forceinline__ FillPx<C> fill_pull_px(const FillPx<C> &own, int y, int x, int hp, int wp, Par par) {
    const int i = y >> 1, j = x >> 1, i2 = i + ((y & 1) ? 1 : -1), j2 = j + ((x & 1) ? 1 : -1);
    float S = 0.f, U[C];
#pragma unroll
    for (int c = 0; c < C; ++c) U[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ii = (k >> 1) ? i2 : i, jj = (k & 1) ? j2 : j;
        const float t = k == 0 ? 0.5625f : k == 3 ? 0.0625f : 0.1875f;
        if (ii >= 0 && ii < hp && jj >= 0 && jj < wp) {
            const FillPx<C> q = par(ii, jj);
            if (q.a != 0.f) {
                S += t;
#pragma unroll
                for (int c = 0; c < C; ++c) U[c] += t * q.v[c];
            }
        }
    }
    if (!(S > 0.f)) return fill_zero<C>();
    FillPx<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float u = U[c] / S;
        // a == 1: the pixel's bits; a == 0: its value is not read
        r.v[c] = own.a == 1.f ? own.v[c] : own.a == 0.f ? u : own.a * own.v[c] + (1.f - own.a) * u;
    }
    r.a = 1.f;
    return r;
}
// L == 0 (R is one pixel): f = v, g = (a > 0)
template <int C> __device__ __forceinline__ FillPx<C> fill_top_px(FillPx<C> own) {
    if (own.a != 0.f) own.a = 1.f;
    return own;
}

// ---- per-level kernels ----
template <int C, bool L0> __global__ __launch_bounds__(256) void fill_push_kernel(FillFrame f, FillLevel fine, FillLevel coarse) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= coarse.w || i >= coarse.h) return;
    const int h = L0 ? f.Ho : fine.h, w = L0 ? f.Wo : fine.w;
    const long long fplane = (long long)h * w;
    const FillPx<C> r = fill_push_cell<C>(i, j, h, w, [&](int y, int x) {
        if constexpr (L0) return fill_read0<C>(f, y, x);
        else return fill_load<C>(fine.p, fplane, (long long)y * w + x);
    });
    fill_store<C>(coarse.p, (long long)coarse.h * coarse.w, (long long)i * coarse.w + j, r);
}

// level l > 0: in place over `fine`
template <int C> __global__ __launch_bounds__(256) void fill_pull_kernel(FillLevel fine, FillLevel par) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= fine.w || y >= fine.h) return;
    const long long plane = (long long)fine.h * fine.w, pplane = (long long)par.h * par.w, p = (long long)y * fine.w + x;
    const FillPx<C> own = fill_load<C>(fine.p, plane, p);
    const FillPx<C> r = fill_pull_px<C>(own, y, x, par.h, par.w, [&](int ii, int jj) { return fill_load<C>(par.p, pplane, (long long)ii * par.w + jj); });
    fill_store<C>(fine.p, plane, p, r);
}

// what level 0 leaves in the caller's planes at frame pixel p: (f, g) inside R, zeros outside
template <int C> __device__ __forceinline__ void fill_store0(const FillFrame &f, long long p, const FillPx<C> &r) {
    const long long HW = (long long)f.H * f.W;
#pragma unroll
    for (int c = 0; c < C; ++c) f.out[c * HW + p] = r.v[c];
    if (f.filled) f.filled[p] = r.a;
}

// level 0: one thread per pixel of the FRAME (the border zeros included); par.p == nullptr: L == 0, no coarser level
template <int C> __global__ __launch_bounds__(256) void fill_pull0_kernel(FillFrame f, FillLevel par) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= f.W || Y >= f.H) return;
    const int y = Y - f.y0, x = X - f.x0;
    FillPx<C> r = fill_zero<C>();
    if (y >= 0 && y < f.Ho && x >= 0 && x < f.Wo) {
        const FillPx<C> own = fill_read0<C>(f, y, x);
        const long long pplane = (long long)par.h * par.w;
        r = par.p ? fill_pull_px<C>(own, y, x, par.h, par.w, [&](int ii, int jj) { return fill_load<C>(par.p, pplane, (long long)ii * par.w + jj); })
                  : fill_top_px<C>(own);
    }
    fill_store0<C>(f, (long long)Y * f.W + X, r);
}

// ---- the apex: one workgroup, levels base .. base + nlev in LDS ----
// size of level l above an h x w base and the offset (floats) of its planes in the LDS image
template <int C> __device__ __forceinline__ void fill_apex_level(int h, int w, int l, int *hl, int *wl, int *off) {
    int o = 0;
    for (int k = 0; k < l; ++k) {
        o += (C + 1) * h * w;
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    *hl = h; *wl = w; *off = o;
}

// base.p == nullptr: the base is level 0, read from and written to the caller's planes (f.H * f.W < 2^31, the launcher's condition);
// else a level in scratch, read and left pulled in place.  nlev >= 1 levels above the base
template <int C> __global__ __launch_bounds__(kFillApexThreads) void fill_apex_kernel(FillFrame f, FillLevel base, int nlev) {
    extern __shared__ __attribute__((aligned(16))) float fill_lds[];
    const int tid = threadIdx.x;
    const bool l0 = base.p == nullptr;
    const int h0 = l0 ? f.Ho : base.h, w0 = l0 ? f.Wo : base.w, n0 = h0 * w0;
    for (int c = tid; c < n0; c += kFillApexThreads)
        fill_store<C>(fill_lds, n0, c, l0 ? fill_read0<C>(f, c / w0, c % w0) : fill_load<C>(base.p, n0, c));
    __syncthreads();
    for (int l = 0; l < nlev; ++l) {
        int h, w, off;
        fill_apex_level<C>(h0, w0, l, &h, &w, &off);
        const float *fine = fill_lds + off;
        float *coarse = fill_lds + off + (C + 1) * h * w;
        const int hc = (h + 1) / 2, wc = (w + 1) / 2, nc = hc * wc, n = h * w;
        for (int c = tid; c < nc; c += kFillApexThreads)
            fill_store<C>(coarse, nc, c, fill_push_cell<C>(c / wc, c % wc, h, w, [&](int y, int x) { return fill_load<C>(fine, n, y * w + x); }));
        __syncthreads();
    }
    for (int l = nlev - 1; l > 0; --l) {
        int h, w, off;
        fill_apex_level<C>(h0, w0, l, &h, &w, &off);
        float *fine = fill_lds + off;
        const float *par = fill_lds + off + (C + 1) * h * w;
        const int hp = (h + 1) / 2, wp = (w + 1) / 2, np = hp * wp, n = h * w;
        for (int c = tid; c < n; c += kFillApexThreads) {
            const int y = c / w, x = c % w;
            fill_store<C>(fine, n, c, fill_pull_px<C>(fill_load<C>(fine, n, c), y, x, hp, wp, [&](int ii, int jj) { return fill_load<C>(par, np, ii * wp + jj); }));
        }
        __syncthreads();
    }
    // the base: from its LDS copy and level 1 to memory
    const float *par = fill_lds + (C + 1) * n0;
    const int hp = (h0 + 1) / 2, wp = (w0 + 1) / 2, np = hp * wp;
    if (l0) {
        const int N = f.H * f.W;
        for (int p = tid; p < N; p += kFillApexThreads) {
            const int y = p / f.W - f.y0, x = p % f.W - f.x0;
            FillPx<C> r = fill_zero<C>();
            if (y >= 0 && y < h0 && x >= 0 && x < w0)
                r = fill_pull_px<C>(fill_load<C>(fill_lds, n0, y * w0 + x), y, x, hp, wp, [&](int ii, int jj) { return fill_load<C>(par, np, ii * wp + jj); });
            fill_store0<C>(f, p, r);
        }
    } else {
        for (int c = tid; c < n0; c += kFillApexThreads) {
            const int y = c / w0, x = c % w0;
            fill_store<C>(base.p, n0, c, fill_pull_px<C>(fill_load<C>(fill_lds, n0, c), y, x, hp, wp, [&](int ii, int jj) { return fill_load<C>(par, np, ii * wp + jj); }));
        }
    }
}

// ---- host ----
struct FillPlan {
    int L;                                   // levels above level 0
    int h[kFillMaxLevels + 1], w[kFillMaxLevels + 1];
    size_t off[kFillMaxLevels + 1];          // level l >= 1: offset (floats) of its planes in the scratch block
    size_t floats;                           // of the block
    int apex;                                // the apex's base level, or -1: per-level kernels only
    size_t apex_lds;                         // bytes of its LDS image
};

// levels: 0 = down to 1 x 1.  budget: option "fill_apex" (-1: from LDS; 0: no apex; n > 0: the apex's base level has at most n cells)
FillPlan fill_plan(int C, int H, int W, int Ho, int Wo, int levels, int budget) {
    FillPlan p{};
    p.h[0] = Ho; p.w[0] = Wo;
    int lfull = 0;
    while (p.h[lfull] > 1 || p.w[lfull] > 1) {
        p.h[lfull + 1] = (p.h[lfull] + 1) / 2;
        p.w[lfull + 1] = (p.w[lfull] + 1) / 2;
        ++lfull;
    }
    p.L = levels == 0 || levels > lfull ? lfull : levels;
    for (int l = 1; l <= p.L; ++l) {
        p.off[l] = p.floats;
        p.floats += DfeCarve::up((size_t)(C + 1) * p.h[l] * p.w[l] * sizeof(float)) / sizeof(float);
    }
    // the apex's base: the first level below the top whose levels up to the top fit LDS (and the cell budget).  Level 0 only where the
    // one workgroup would not have a far larger frame's border to zero
    p.apex = -1;
    if (budget != 0) {
        size_t above = 0;   // bytes of levels s + 1 .. L
        int best = -1;
        size_t best_lds = 0;
        for (int s = p.L - 1; s >= 0; --s) {
            above += (size_t)(C + 1) * p.h[s + 1] * p.w[s + 1] * sizeof(float);
            const size_t cells = (size_t)p.h[s] * p.w[s], lds = above + (C + 1) * cells * sizeof(float);
            if (lds > kFillApexLds || (budget > 0 && cells > (size_t)budget)) break;
            if (s == 0 && (long long)H * W > 2 * (long long)cells) break;
            best = s;
            best_lds = lds;
        }
        p.apex = best;
        p.apex_lds = best_lds;
    }
    return p;
}

template <int C> int fill_launch(dfe_ctx *ctx, const FillFrame &f, const FillPlan &p, float *scr) {
    auto level = [&](int l) { return FillLevel{l >= 1 ? scr + p.off[l] : nullptr, p.h[l], p.w[l]}; };
    auto grid = [](int h, int w) { return dim3((unsigned)dfe_cdiv(w, 64), (unsigned)dfe_cdiv(h, 4)); };
    DfeStageScope ex(ctx, DFE_STAGE_EXTRACT);
    const int down = p.apex >= 0 ? p.apex : p.L;   // levels 0 .. down - 1 are pushed and pulled by a launch each
    for (int l = 0; l < down; ++l) {
        DfeProfScope prof(ctx);
        if (l == 0) hipLaunchKernelGGL((fill_push_kernel<C, true>), grid(p.h[1], p.w[1]), dim3(256), 0, ctx->stream, f, level(0), level(1));
        else hipLaunchKernelGGL((fill_push_kernel<C, false>), grid(p.h[l + 1], p.w[l + 1]), dim3(256), 0, ctx->stream, f, level(l), level(l + 1));
        DFE_LAUNCH_CHECK(ctx);
    }
    if (p.apex >= 0) {
        if (p.apex_lds > 64 * 1024)
            DFE_HIP(ctx, hipFuncSetAttribute((const void *)fill_apex_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.apex_lds));
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((fill_apex_kernel<C>), dim3(1), dim3(kFillApexThreads), p.apex_lds, ctx->stream, f, level(p.apex), p.L - p.apex);
        DFE_LAUNCH_CHECK(ctx);
    }
    for (int l = down - 1; l >= 0; --l) {
        DfeProfScope prof(ctx);
        if (l == 0) hipLaunchKernelGGL((fill_pull0_kernel<C>), grid(f.H, f.W), dim3(256), 0, ctx->stream, f, level(1));
        else hipLaunchKernelGGL((fill_pull_kernel<C>), grid(p.h[l], p.w[l]), dim3(256), 0, ctx->stream, level(l), level(l + 1));
        DFE_LAUNCH_CHECK(ctx);
    }
    if (p.L == 0) {   // R is one pixel: nothing above it
        DfeProfScope prof(ctx);
        hipLaunchKernelGGL((fill_pull0_kernel<C>), grid(f.H, f.W), dim3(256), 0, ctx->stream, f, FillLevel{nullptr, 0, 0});
        DFE_LAUNCH_CHECK(ctx);
    }
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_fill_holes_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, int y0, int x0, int Ho, int Wo, int levels, float *out,
                       float *filled) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, v && w && out, DFE_E_ARG, "dfe_fill_holes_f32: NULL tensor");
    if (int rc = dfe_channels_check(ctx, "dfe_fill_holes_f32", C)) return rc;
    DFE_REQUIRE(ctx, levels >= 0, DFE_E_ARG, "dfe_fill_holes_f32: levels=%d must be >= 0", levels);
    if (int rc = dfe_region_check(ctx, "dfe_fill_holes_f32", H, W, y0, x0, Ho, Wo)) return rc;
    const FillPlan p = fill_plan(C, H, W, Ho, Wo, levels, ctx->opt[DFE_OPT_FILL_APEX]);
    float *scr = nullptr;
    if (p.floats) {   // the ctx's side buffer: grown once, then no allocation per call
        void *aux = nullptr;
        int rc = dfe_aux_scratch(ctx, p.floats * sizeof(float), &aux);
        if (rc) return rc;
        scr = (float *)aux;
    }
    FillFrame f{v, w, out, filled, H, W, y0, x0, Ho, Wo};
    return dfe_dispatch_1to4(C, [&](auto c) { return fill_launch<decltype(c)::value>(ctx, f, p, scr); });
}

}  // extern "C"
