// sgm_penalty.hip -- the edge-aware P2 of the guided semi-global entries (NOT in the reference).  The definition
// -- d2 over the guide's channels, w = max(0, 1 - d2 / sigma^2), P2(p, r) = P2_edge + (P2 - P2_edge) w, P2 itself where w == 1 -- is in
// include/dfe.h and restated in numpy in tests/sgm_guided_ref.py; the device is tested against that bit for bit.
//   sgm_penalty_kernel<T>   ONE launch before the path launch: a thread a pixel p writes P2(p, r) for the even bit r of every AXIS the
//       call's directions lie on -- 0 (0, +1), 2 (+1, 0), 4 (+1, +1), 6 (+1, -1) -- into that axis' [H][W] plane.  The odd bit of the
//       axis is the same pair of pixels seen from the other end, and (a - b)^2 has the bits of (b - a)^2, so direction -r reads the
//       plane at its predecessor: four planes at the most serve eight directions, 4 H W floats beside the (n + 1) H W cells of the
//       path launch.  The predecessor's column is taken modulo W, so the ring's wrap pair (x = 0, x = W - 1) has its own penalty; on
//       the plane that step is a chain start, whose cell is written all the same: the path kernels fetch it with the step's costs and
//       no cell of the planes is read unwritten.  Where the predecessor's row lies outside, P2.
//       T = float, or uint8_t read as float(byte) * scale (dfe_u8_to_f32's bits): the census byte one calls guide with no float copy.
#include "sgm_common.h"

namespace {

struct SgmPenJob {
    const void *g;
    long long chan;
    int pitch, Cg;
    int H, W;
    float scale, inv_s2, P2, P2_edge, span;
    float *plane[4];     // per axis, or NULL
};

template <typename T>
__device__ __forceinline__ float sgm_guide_at(const SgmPenJob &a, int c, int y, int x) {
#pragma clang fp contract(off)
    const T v = ((const T *)a.g)[(long long)c * a.chan + (long long)y * a.pitch + x];
    if constexpr (sizeof(T) == 1) return (float)v * a.scale;
    else return v;
}

template <typename T>
__global__ __launch_bounds__(256) void sgm_penalty_kernel(const SgmPenJob a) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.H * a.W) return;
    const int y = (int)(i / a.W), x = (int)(i - (long long)y * a.W);
    const int xm = x > 0 ? x - 1 : a.W - 1, xp = x + 1 < a.W ? x + 1 : 0;   // the columns a predecessor has, modulo W
    const int qy[4] = {y, y - 1, y - 1, y - 1};                              // q = p - r for r = (0, +1), (+1, 0), (+1, +1), (+1, -1)
    const int qx[4] = {xm, x, xm, xp};
#pragma unroll
    for (int ax = 0; ax < 4; ++ax) {
        if (!a.plane[ax]) continue;              // (uniform)
        float pen = a.P2;
        if (qy[ax] >= 0) {
            float d2 = 0.f;
            for (int c = 0; c < a.Cg; ++c) {
                const float d = sgm_guide_at<T>(a, c, y, x) - sgm_guide_at<T>(a, c, qy[ax], qx[ax]);
                const float sq = d * d;
                d2 = c == 0 ? sq : d2 + sq;      // (in channel order, starting from the first square)
            }
            float w = 1.0f - d2 * a.inv_s2;
            w = w > 0.f ? w : 0.f;               // max(0, .); a w that is not finite (NaN here: w <= 1 otherwise) counts as 0
            if (w != 1.0f) pen = a.P2_edge + a.span * w;
        }
        a.plane[ax][i] = pen;
    }
}

inline unsigned sgm_axes(unsigned paths) { return (paths | paths >> 1) & 0x55u; }   // bit 2 ax: an axis some direction of `paths` lies on

}  // namespace

int sgm_guide_check(dfe_ctx *ctx, const char *fn, float P1, float P2, const SgmGuide &g) {
    DFE_REQUIRE(ctx, std::isfinite(g.P2_edge) && P1 <= g.P2_edge && g.P2_edge <= P2, DFE_E_ARG, "%s: P2_edge=%g must be finite with P1=%g <= P2_edge <= P2=%g",
                fn, (double)g.P2_edge, (double)P1, (double)P2);
    DFE_REQUIRE(ctx, !g.g || g.Cg >= 1, DFE_E_ARG, "%s: Cg=%d guide channels (1 at least)", fn, g.Cg);
    return DFE_OK;
}

size_t sgm_penalty_floats(unsigned paths, int H, int W) { return (size_t)__builtin_popcount(sgm_axes(paths)) * H * W; }

int sgm_penalty_run(dfe_ctx *ctx, const SgmGuide &g, int H, int W, float P2, unsigned paths, float *planes, SgmPen *pen) {
    SgmPenJob a{};
    a.g = g.g;
    a.chan = (long long)g.chan; a.pitch = g.pitch; a.Cg = g.Cg;
    a.H = H; a.W = W;
    a.scale = g.scale;
    a.inv_s2 = 1.0f / (g.sigma * g.sigma);
    a.P2 = P2; a.P2_edge = g.P2_edge;
    a.span = P2 - g.P2_edge;
    const unsigned axes = sgm_axes(paths);
    size_t used = 0;
    for (int ax = 0; ax < 4; ++ax)
        if (axes >> (2 * ax) & 1u) a.plane[ax] = planes + used++ * (size_t)H * W;
    int k = 0;
    for (int r = 0; r < 8; ++r) {                // the job's directions: ascending bit order (sgm_directions)
        if (!(paths >> r & 1u)) continue;
        pen->plane[k] = a.plane[r >> 1];
        pen->atq[k] = r & 1;
        ++k;
    }
    DfeProfScope prof(ctx);
    const dim3 grid((unsigned)dfe_cdiv((long long)H * W, 256));
    if (g.bytes) hipLaunchKernelGGL(sgm_penalty_kernel<uint8_t>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(sgm_penalty_kernel<float>, grid, dim3(256), 0, ctx->stream, a);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}
