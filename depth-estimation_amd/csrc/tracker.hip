// tracker.hip -- next-row N4, the step in front of the pose: the sparse corner tracker that `sfm2.getEgoMotion{im1, im2, K, maxPoints,
// pointsQuality, pointsMinDistance}` runs on the two IMAGES (radial/radial_opticalflow_data.lua:211-217, depth_estimation_api.lua:141,
// test_opticalflow.lua:282, groundtruth_opticalflow.lua:283, version2/data.lua:96).  sfm2 is an un-vendored OpenCV wrapper, so parity
// is unpinned: this is the library's own tracker, with the arithmetic of every stage fixed in DESIGN section 4 (corner response,
// corner selection, 5-tap pyramid, pyramidal Lucas-Kanade) so that a float64 reference can be written from the definitions.
//   response  : smaller eigenvalue of the 3 x 3 structure tensor of central-difference gradients, LDS tile with a halo of 2
//   selection : threshold against quality * max, dominance inside the min_dist disc, then the max_points best in (response
//               descending, index ascending) order -- a 64-bit key per kept corner, a bitwise search for the max_points-th key and
//               a rank count of the survivors: the result does not depend on the order the blocks ran in
//   pyramid   : (1 4 6 4 1) / 16 separable, reflected borders
//   tracker   : one wave per point, the (win + 2)^2 template patch in LDS, T / Tx / Ty in registers, fixed lane <-> sample map
//               and reduction tree (same call, same bits)
// Every image read goes through a clamped index; every loop is bounded by a constant or by a checked argument; no block waits
// on another.
#include "dfe_internal.h"
#include "dfe_wave.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

// ------------------------------------------------------------------------------------------------------------- corner response
constexpr int CR_TW = 64, CR_TH = 4;   // output tile: 4 rows of 64 floats = two whole 128-B lines per row store

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(CR_TW * CR_TH) void corner_response_kernel(const float *__restrict__ Y, int H, int W, float *__restrict__ resp) {
#pragma clang fp contract(off)
    __shared__ float sy[CR_TH + 4][CR_TW + 4];          // Y at clamped positions, halo 2
    __shared__ float sgx[CR_TH + 2][CR_TW + 2];         // gradients AT the clamped positions of the halo-1 region
    __shared__ float sgy[CR_TH + 2][CR_TW + 2];
    const int x0 = blockIdx.x * CR_TW, y0 = blockIdx.y * CR_TH;
    const int tid = threadIdx.y * CR_TW + threadIdx.x;
    for (int e = tid; e < (CR_TH + 4) * (CR_TW + 4); e += CR_TW * CR_TH) {
        const int r = e / (CR_TW + 4), c = e - r * (CR_TW + 4);
        sy[r][c] = Y[(long long)clampi(y0 - 2 + r, 0, H - 1) * W + clampi(x0 - 2 + c, 0, W - 1)];
    }
    __syncthreads();
    // entry (r, c) of the gradient tile belongs to frame position q = clamp(y0 - 1 + r, x0 - 1 + c); its taps are clamp(q +- 1),
    // which lie inside the Y tile (q is inside the frame and inside the tile's halo-1 region, or clamped towards it)
    const int xhi = min(x0 + CR_TW + 1, W - 1), yhi = min(y0 + CR_TH + 1, H - 1);   // last frame column / row the Y tile holds
    for (int e = tid; e < (CR_TH + 2) * (CR_TW + 2); e += CR_TW * CR_TH) {
        const int r = e / (CR_TW + 2), c = e - r * (CR_TW + 2);
        const int qy = clampi(y0 - 1 + r, 0, yhi), qx = clampi(x0 - 1 + c, 0, xhi);
        const int ty = qy - (y0 - 2), tx = qx - (x0 - 2);
        const int txp = min(qx + 1, xhi) - (x0 - 2), txm = max(qx - 1, 0) - (x0 - 2);
        const int typ = min(qy + 1, yhi) - (y0 - 2), tym = max(qy - 1, 0) - (y0 - 2);
        sgx[r][c] = (sy[ty][txp] - sy[ty][txm]) * 0.5f;
        sgy[r][c] = (sy[typ][tx] - sy[tym][tx]) * 0.5f;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float gx = sgx[threadIdx.y + dy][threadIdx.x + dx], gy = sgy[threadIdx.y + dy][threadIdx.x + dx];
            a += gx * gx;
            b += gx * gy;
            c += gy * gy;
        }
    // (the eigenvalue in double from the float sums: (a - c)^2 + 4 b^2 cancels against (a + c)^2 where the tensor is nearly of rank 1, and a
    //  float32 square root there is wrong by 2^-24 (a + c), many ulps of the small result; one double sqrt per pixel is free here)
    const double d = (double)a - (double)c;
    resp[(long long)y * W + x] = (float)(0.5 * (((double)a + (double)c) - sqrt(d * d + 4.0 * ((double)b * (double)b))));
}

// ------------------------------------------------------------------------------------------------------------ corner selection
// workspace: [0] bit pattern of the maximum (positive floats order as unsigned integers), [1] kept corners, then their keys
constexpr int SEL_MAX_POINTS = 4096;

__global__ __launch_bounds__(256) void sel_max_kernel(const float *__restrict__ resp, long long P, unsigned *__restrict__ head) {
    unsigned m = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256) {
        const float v = resp[p];
        if (v > 0.f) m = max(m, (unsigned)__float_as_int(v));      // (NaN: the comparison is false)
    }
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(head, m);
}

// q dominates p: a larger response, or the same response at a smaller linear index
__device__ __forceinline__ bool sel_dominates(float vq, int q, float vp, int p) { return vq > vp || (vq == vp && q < p); }

__global__ __launch_bounds__(256) void sel_keep_kernel(const float *__restrict__ resp, int H, int W, float quality, int r, int R2, unsigned *__restrict__ head,
                                                       unsigned long long *__restrict__ keys) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float M = __int_as_float((int)head[0]);
    if (!(M > 0.f)) return;
    const int p = y * W + x;
    const float v = resp[p], thr = quality * M;
    if (!(v > 0.f && v >= thr)) return;
    const int ya = max(y - r, 0), yb = min(y + r, H - 1), xa = max(x - r, 0), xb = min(x + r, W - 1);
    // the 3 x 3 neighbourhood first (inside every disc: R2 >= 1; its corners only when R2 >= 2): most candidates end here
    for (int qy = max(y - 1, ya); qy <= min(y + 1, yb); ++qy)
        for (int qx = max(x - 1, xa); qx <= min(x + 1, xb); ++qx) {
            const int q = qy * W + qx;
            if (q != p && (qy - y) * (qy - y) + (qx - x) * (qx - x) <= R2 && sel_dominates(resp[q], q, v, p)) return;
        }
    for (int qy = ya; qy <= yb; ++qy) {
        const int dy2 = (qy - y) * (qy - y);
        for (int qx = xa; qx <= xb; ++qx) {
            const int q = qy * W + qx;
            if (q != p && dy2 + (qx - x) * (qx - x) <= R2 && sel_dominates(resp[q], q, v, p)) return;
        }
    }
    const unsigned slot = atomicAdd(head + 1, 1u);       // (the order of the list is arbitrary; the keys are unique and get sorted)
    keys[slot] = ((unsigned long long)(unsigned)__float_as_int(v) << 32) | (unsigned)~(unsigned)p;
}

// one block: the max_points largest keys of the list in descending order -> pts / resp_out.  More than max_points kept: the
// max_points-th largest key by a bitwise binary search (63 counting passes over the list), then the survivors, at most 4096, are
// gathered in LDS and every one counts the keys above it: its place.
__global__ __launch_bounds__(1024) void sel_top_kernel(const unsigned *__restrict__ head, const unsigned long long *__restrict__ keys, int W, int max_points,
                                                       float *__restrict__ pts, float *__restrict__ resp_out) {
    __shared__ unsigned long long sk[SEL_MAX_POINTS];
    __shared__ unsigned cnt[16];
    __shared__ unsigned nsurv;
    const unsigned n = head[1];
    const int tid = threadIdx.x;
    unsigned long long thr = 0;
    if (n > (unsigned)max_points) {
        for (int bit = 62; bit >= 0; --bit) {               // (bit 63 is the sign of a positive float: never set)
            const unsigned long long cand = thr | (1ull << bit);
            unsigned c = 0;
            for (unsigned i = tid; i < n; i += 1024) c += keys[i] >= cand;
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor((int)c, off);
            __syncthreads();                                // (cnt of the previous pass has been read)
            if ((tid & 63) == 0) cnt[tid >> 6] = c;
            __syncthreads();
            unsigned tot = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) tot += cnt[w];
            if (tot >= (unsigned)max_points) thr = cand;    // (block-uniform)
        }
    }
    if (tid == 0) nsurv = 0;
    __syncthreads();
    for (unsigned i = tid; i < n; i += 1024) {
        const unsigned long long k = keys[i];
        if (k >= thr) {
            const unsigned s = atomicAdd(&nsurv, 1u);
            if (s < (unsigned)SEL_MAX_POINTS) sk[s] = k;     // (keys are unique: exactly min(n, max_points) pass)
        }
    }
    __syncthreads();
    const unsigned ns = min(nsurv, (unsigned)max_points);
    for (unsigned i = tid; i < ns; i += 1024) {
        const unsigned long long k = sk[i];
        unsigned rank = 0;
        for (unsigned j = 0; j < ns; ++j) rank += sk[j] > k;
        const unsigned p = ~(unsigned)(k & 0xffffffffull);
        const unsigned y = p / (unsigned)W, x = p - y * (unsigned)W;
        pts[2 * rank] = (float)x;
        pts[2 * rank + 1] = (float)y;
        if (resp_out) resp_out[rank] = __int_as_float((int)(k >> 32));
    }
}

// the selection's workspace: the list's head and one key per pixel
struct SelWs { unsigned *head; unsigned long long *keys; };
SelWs sel_layout(DfeCarve &c, int H, int W) {
    SelWs ws;
    ws.head = c.take<unsigned>(1);
    ws.keys = c.take<unsigned long long>((size_t)H * W);
    return ws;
}

int select_run(dfe_ctx *ctx, const float *resp, int H, int W, float quality, float min_dist, int max_points, float *pts, float *resp_out, int *n_out, const SelWs &ws) {
    unsigned *head = ws.head;
    unsigned long long *keys = ws.keys;
    // floor(min_dist^2) as the integer the kernel compares with, capped at the frame's diagonal (a larger disc holds the same pixels)
    const double diag2 = (double)(H - 1) * (H - 1) + (double)(W - 1) * (W - 1);
    const double md2 = floor((double)min_dist * (double)min_dist);
    const int R2 = (int)(md2 < diag2 ? md2 : diag2 < 1 ? 1 : diag2);
    int r = (int)floor(sqrt((double)R2));
    while ((long long)(r + 1) * (r + 1) <= R2) ++r;
    while ((long long)r * r > R2) --r;
    DFE_HIP(ctx, hipMemsetAsync(head, 0, 256, ctx->stream));
    const long long P = (long long)H * W;
    hipLaunchKernelGGL(sel_max_kernel, dim3((unsigned)std::min<long long>(1024, (P + 255) / 256)), dim3(256), 0, ctx->stream, resp, P, head);
    hipLaunchKernelGGL(sel_keep_kernel, dim3(dfe_cdiv(W, 64), dfe_cdiv(H, 4)), dim3(256), 0, ctx->stream, resp, H, W, quality, r, R2, head, keys);
    hipLaunchKernelGGL(sel_top_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned *)head, (const unsigned long long *)keys, W, max_points, pts, resp_out);
    DFE_LAUNCH_CHECK(ctx);
    unsigned hh[2] = {0, 0};
    DFE_HIP(ctx, hipMemcpyAsync(hh, head, 8, hipMemcpyDeviceToHost, ctx->stream));
    DFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = (int)(hh[1] < (unsigned)max_points ? hh[1] : (unsigned)max_points);
    return DFE_OK;
}

// --------------------------------------------------------------------------------------------------------------------- pyramid
// reflection about the first and the last sample (-1 -> 1, n -> n - 2), for any index: period 2 (n - 1); n = 1: always 0
__device__ __forceinline__ int reflecti(int i, int n) {
    if (n == 1) return 0;
    const int per = 2 * (n - 1);
    int m = i % per;
    if (m < 0) m += per;
    return m < n ? m : per - m;
}

__global__ __launch_bounds__(256) void pyr_down_kernel(const float *__restrict__ in, int H, int W, float *__restrict__ out, int Ho, int Wo) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= Wo || y >= Ho) return;
    const float w[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    int cx[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) cx[j] = reflecti(2 * x + j - 2, W);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float *row = in + (long long)reflecti(2 * y + i - 2, H) * W;
        float h = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) h += w[j] * row[cx[j]];
        acc += w[i] * h;
    }
    out[(long long)y * Wo + x] = acc;
}

void pyr_down_run(dfe_ctx *ctx, const float *in, int H, int W, float *out) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    hipLaunchKernelGGL(pyr_down_kernel, dim3(dfe_cdiv(Wo, 64), dfe_cdiv(Ho, 4)), dim3(256), 0, ctx->stream, in, H, W, out, Ho, Wo);
}

// --------------------------------------------------------------------------------------------------------------------- tracker
constexpr int LK_MAX_LEVELS = 8, LK_MAX_WIN = 31;
constexpr int LK_PATCH = (LK_MAX_WIN + 2) * (LK_MAX_WIN + 2);          // 1089 floats per wave
constexpr int LK_SPL = (LK_MAX_WIN * LK_MAX_WIN + 63) / 64;            // 16 template samples per lane
constexpr int LK_FILL = (LK_PATCH + 63) / 64;                          // 18 patch samples per lane

struct LkArgs {
    const float *y0[LK_MAX_LEVELS], *y1[LK_MAX_LEVELS];
    int H[LK_MAX_LEVELS], W[LK_MAX_LEVELS];
    int N, win, levels, max_iters;
    float eps2, min_eig, max_err;
    const float *pts0;
    float *pts1, *err, *wts;
    int *status;
};

// bilinear sample at (x, y), the coordinates clamped to the frame first (NaN clamps to 0: fmaxf returns its other operand)
__device__ __forceinline__ float lk_sample(const float *__restrict__ I, int H, int W, float x, float y) {
#pragma clang fp contract(off)
    x = fminf(fmaxf(x, 0.f), (float)(W - 1));
    y = fminf(fmaxf(y, 0.f), (float)(H - 1));
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = x - xf, fy = y - yf;
    const float *r0 = I + (long long)y0 * W, *r1 = I + (long long)y1 * W;
    const float top = r0[x0] + fx * (r0[x1] - r0[x0]), bot = r1[x0] + fx * (r1[x1] - r1[x0]);
    return top + fy * (bot - top);
}

__device__ __forceinline__ float lk_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// One wave per point, four per block (a wave past the last point repeats the last point and writes nothing, so that every wave
// reaches the block's barriers).  Template sample s = 64 k + lane <-> window cell (s / win, s % win), k < 16; sums: per-lane partial
// sums in k order, then wave_sum_f32_ordered.  The 2 x 2 solve and the eigenvalue are taken in double from the float sums.
__global__ __launch_bounds__(256) void lk_track_kernel(const LkArgs A) {
#pragma clang fp contract(off)
    __shared__ float patch_all[4][LK_PATCH];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *patch = patch_all[wv];
    const int pt_raw = blockIdx.x * 4 + wv;
    const bool active = pt_raw < A.N;
    const int pt = active ? pt_raw : A.N - 1;
    const float px_in = A.pts0[2 * pt], py_in = A.pts0[2 * pt + 1];
    const bool finite_p = isfinite(px_in) && isfinite(py_in);
    const float px = finite_p ? px_in : 0.f, py = finite_p ? py_in : 0.f;
    const int win = A.win, h = (win - 1) >> 1, pw = win + 2, nsamp = win * win, npatch = pw * pw;
    const int q64 = 64 / win, r64 = 64 - q64 * win, i_first = lane / win, j_first = lane - i_first * win;
    const double inv_n = 1.0 / (double)nsamp;
    float gx = 0.f, gy = 0.f, vx = 0.f, vy = 0.f, errsum = 0.f;
    bool lost = false;
    for (int L = A.levels - 1; L >= 0; --L) {
        const float *__restrict__ I0 = A.y0[L];
        const float *__restrict__ I1 = A.y1[L];
        const int HL = A.H[L], WL = A.W[L];
        const float sc = 1.0f / (float)(1 << L);
        const float cx = px * sc, cy = py * sc;
        // the (win + 2)^2 patch of frame 0 around c
#pragma unroll 1
        for (int m = 0; m < LK_FILL; ++m) {
            const int t = m * 64 + lane;
            if (t < npatch) {
                const int r = t / pw, c = t - r * pw;
                patch[t] = lk_sample(I0, HL, WL, cx + (float)(c - h - 1), cy + (float)(r - h - 1));
            }
        }
        __syncthreads();
        float T[LK_SPL], Tx[LK_SPL], Ty[LK_SPL];
        float sa = 0.f, sb = 0.f, scc = 0.f;
        {
            int i = i_first, j = j_first;
#pragma unroll
            for (int k = 0; k < LK_SPL; ++k) {
                T[k] = Tx[k] = Ty[k] = 0.f;
                if (k * 64 < nsamp) {                                  // (wave-uniform)
                    if (k * 64 + lane < nsamp) {
                        const float *c = patch + (i + 1) * pw + j + 1;
                        T[k] = c[0];
                        Tx[k] = (c[1] - c[-1]) * 0.5f;
                        Ty[k] = (c[pw] - c[-pw]) * 0.5f;
                        sa += Tx[k] * Tx[k];
                        sb += Tx[k] * Ty[k];
                        scc += Ty[k] * Ty[k];
                    }
                    j += r64; i += q64;
                    if (j >= win) { j -= win; ++i; }
                }
            }
        }
        const double a = (double)wave_sum_f32_ordered(sa), b = (double)wave_sum_f32_ordered(sb), cc = (double)wave_sum_f32_ordered(scc);
        const double lam = 0.5 * ((a + cc) - sqrt((a - cc) * (a - cc) + 4.0 * b * b)) * inv_n;
        const bool weak = __builtin_amdgcn_readfirstlane((int)(lam < (double)A.min_eig)) != 0;
        vx = 0.f; vy = 0.f;
        if (weak) {
            if (L == 0) lost = true;
        } else {
            const double det = a * cc - b * b;
            for (int it = 0; it < A.max_iters; ++it) {
                const float bxp = cx + (gx + vx) - (float)h, byp = cy + (gy + vy) - (float)h;
                float sbx = 0.f, sby = 0.f, sr = 0.f;
                int i = i_first, j = j_first;
#pragma unroll
                for (int k = 0; k < LK_SPL; ++k) {
                    if (k * 64 < nsamp) {
                        if (k * 64 + lane < nsamp) {
                            const float r = T[k] - lk_sample(I1, HL, WL, bxp + (float)j, byp + (float)i);
                            sbx += r * Tx[k];
                            sby += r * Ty[k];
                            sr += fabsf(r);
                        }
                        j += r64; i += q64;
                        if (j >= win) { j -= win; ++i; }
                    }
                }
                const double bx = (double)wave_sum_f32_ordered(sbx), by = (double)wave_sum_f32_ordered(sby);
                if (L == 0) errsum = wave_sum_f32_ordered(sr);
                const float dx = lk_uniform((float)((cc * bx - b * by) / det)), dy = lk_uniform((float)((a * by - b * bx) / det));
                vx += dx; vy += dy;
                if (dx * dx + dy * dy < A.eps2) break;
            }
        }
        if (L > 0) { gx = 2.f * (gx + vx); gy = 2.f * (gy + vy); }
        __syncthreads();                                               // (the patch is rewritten at the next level)
    }
    const float dx = gx + vx, dy = gy + vy;
    const float qx = px + dx, qy = py + dy;
    float e = (float)((double)errsum * inv_n);
    const bool inside = qx >= 0.f && qx <= (float)(A.W[0] - 1) && qy >= 0.f && qy <= (float)(A.H[0] - 1);   // (false for NaN)
    lost = lost || !finite_p || !isfinite(dx) || !isfinite(dy) || !inside || (A.max_err > 0.f && e > A.max_err);
    if (active && lane == 0) {
        A.pts1[2 * pt] = lost ? px_in : qx;
        A.pts1[2 * pt + 1] = lost ? py_in : qy;
        A.status[pt] = lost ? 0 : 1;
        if (A.err) A.err[pt] = lost ? 0.f : e;
        if (A.wts) A.wts[pt] = lost ? 0.f : 1.f;
    }
}

// the tracker's workspace: the pyramid levels 1 .. levels - 1 of both frames
struct LkWs { float *lev[2][LK_MAX_LEVELS]; };
LkWs lk_layout(DfeCarve &c, int H, int W, int levels) {
    LkWs ws{};
    for (int k = 0; k < 2; ++k)
        for (int L = 1, h = H, w = W; L < levels; ++L) {
            h = (h + 1) / 2; w = (w + 1) / 2;
            ws.lev[k][L] = c.take<float>((size_t)h * w);
        }
    c.take<char>(256);   // (slack behind the last level, as the first layout had it)
    return ws;
}

int lk_check_params(dfe_ctx *ctx, const dfe_tracker_params *p, const char *who) {
    DFE_REQUIRE(ctx, p, DFE_E_ARG, "%s: params is NULL", who);
    DFE_REQUIRE(ctx, p->win >= 3 && p->win <= LK_MAX_WIN && (p->win & 1) && p->levels >= 1 && p->levels <= LK_MAX_LEVELS && p->max_iters >= 1 && p->max_iters <= 64 &&
                         p->eps >= 0.f, DFE_E_ARG, "%s: win=%d (odd, 3..31) levels=%d (1..8) max_iters=%d (1..64) eps=%g (>= 0)", who, p->win, p->levels, p->max_iters,
                (double)p->eps);
    return DFE_OK;
}

// wts (or NULL): status as float weights, what dfe_ego_motion_from_points_f32 takes
int track_run(dfe_ctx *ctx, const float *Y0, const float *Y1, int H, int W, const float *pts0, int N, const dfe_tracker_params *p, float *pts1, int *status,
              float *err, float *wts, const LkWs &ws) {
    LkArgs A;
    memset(&A, 0, sizeof(A));
    const float *src[2] = {Y0, Y1};
    for (int k = 0; k < 2; ++k) {
        int h = H, w = W;
        const float *prev = src[k];
        for (int L = 0; L < p->levels; ++L) {
            if (L > 0) {
                pyr_down_run(ctx, prev, h, w, ws.lev[k][L]);
                prev = ws.lev[k][L];
                h = (h + 1) / 2; w = (w + 1) / 2;
            }
            (k == 0 ? A.y0 : A.y1)[L] = prev;
            A.H[L] = h; A.W[L] = w;
        }
    }
    A.N = N; A.win = p->win; A.levels = p->levels; A.max_iters = p->max_iters;
    A.eps2 = p->eps * p->eps; A.min_eig = p->min_eig; A.max_err = p->max_err;
    A.pts0 = pts0; A.pts1 = pts1; A.err = err; A.wts = wts; A.status = status;
    hipLaunchKernelGGL(lk_track_kernel, dim3(dfe_cdiv(N, 4)), dim3(256), 0, ctx->stream, A);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

int check_select_args(dfe_ctx *ctx, float quality, float min_dist, int max_points, const char *who) {
    DFE_REQUIRE(ctx, min_dist >= 1.f && max_points >= 1 && max_points <= SEL_MAX_POINTS && quality >= 0.f && quality <= 1.f, DFE_E_ARG,
                "%s: min_dist=%g (>= 1) max_points=%d (1..4096) quality=%g (0..1)", who, (double)min_dist, max_points, (double)quality);
    return DFE_OK;
}

void corner_response_run(dfe_ctx *ctx, const float *Y, int H, int W, float *resp) {
    hipLaunchKernelGGL(corner_response_kernel, dim3(dfe_cdiv(W, CR_TW), dfe_cdiv(H, CR_TH)), dim3(CR_TW, CR_TH), 0, ctx->stream, Y, H, W, resp);
}

}  // namespace

extern "C" {

int dfe_corner_response_f32(dfe_ctx *ctx, const float *Y, int H, int W, float *resp) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, Y && resp, DFE_E_ARG, "dfe_corner_response_f32: NULL tensor");
    DFE_REQUIRE(ctx, H > 0 && W > 0 && dfe_cdiv(H, CR_TH) <= 65535, DFE_E_SHAPE, "dfe_corner_response_f32: %dx%d", H, W);
    corner_response_run(ctx, Y, H, W, resp);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

int dfe_select_corners_f32(dfe_ctx *ctx, const float *resp, int H, int W, float quality, float min_dist, int max_points, float *pts, float *resp_out, int *n_out) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, resp && pts && n_out, DFE_E_ARG, "dfe_select_corners_f32: NULL argument");
    DFE_REQUIRE(ctx, H > 0 && W > 0 && H <= 32768 && W <= 32768 && (long long)H * W < (1ll << 31), DFE_E_SHAPE, "dfe_select_corners_f32: %dx%d", H, W);
    int rc = check_select_args(ctx, quality, min_dist, max_points, "dfe_select_corners_f32");
    if (rc) return rc;
    SelWs ws;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) { ws = sel_layout(c, H, W); });
    if (rc) return rc;
    return select_run(ctx, resp, H, W, quality, min_dist, max_points, pts, resp_out, n_out, ws);
}

int dfe_pyr_down_f32(dfe_ctx *ctx, const float *in, int H, int W, float *out) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, in && out, DFE_E_ARG, "dfe_pyr_down_f32: NULL tensor");
    DFE_REQUIRE(ctx, H > 0 && W > 0 && H < (1 << 29) && W < (1 << 29) && dfe_cdiv((H + 1) / 2, 4) <= 65535, DFE_E_SHAPE, "dfe_pyr_down_f32: %dx%d", H, W);
    pyr_down_run(ctx, in, H, W, out);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

int dfe_track_points_lk_f32(dfe_ctx *ctx, const float *Y0, const float *Y1, int H, int W, const float *pts0, int N, const dfe_tracker_params *params, float *pts1,
                            int *status, float *err) {
    DFE_ENTER(ctx);
    int rc = lk_check_params(ctx, params, "dfe_track_points_lk_f32");
    if (rc) return rc;
    DFE_REQUIRE(ctx, N >= 0, DFE_E_ARG, "dfe_track_points_lk_f32: N=%d", N);
    if (N == 0) return DFE_OK;
    DFE_REQUIRE(ctx, Y0 && Y1 && pts0 && pts1 && status, DFE_E_ARG, "dfe_track_points_lk_f32: NULL argument");
    DFE_REQUIRE(ctx, H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24) && dfe_cdiv((H + 1) / 2, 4) <= 65535, DFE_E_SHAPE, "dfe_track_points_lk_f32: %dx%d", H, W);
    LkWs ws;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) { ws = lk_layout(c, H, W, params->levels); });
    if (rc) return rc;
    return track_run(ctx, Y0, Y1, H, W, pts0, N, params, pts1, status, err, nullptr, ws);
}

int dfe_ego_motion_from_images_f32(dfe_ctx *ctx, const float *im0, const float *im1, int C, int H, int W, const double *K9, const dfe_tracker_params *params,
                                   double ransac_max_dist, int iterations, unsigned seed, double *R9, double *T3, int *n_found, int *n_inliers, double *F9,
                                   float *pts0_out, float *pts1_out, int *status_out, int *n_corners) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, im0 && im1 && K9 && R9 && T3, DFE_E_ARG, "dfe_ego_motion_from_images_f32: NULL argument");
    DFE_REQUIRE(ctx, C == 1 || C == 3, DFE_E_SHAPE, "dfe_ego_motion_from_images_f32: C=%d (1 or 3)", C);
    DFE_REQUIRE(ctx, H > 0 && W > 0 && H <= 32768 && W <= 32768 && (long long)H * W < (1ll << 31), DFE_E_SHAPE, "dfe_ego_motion_from_images_f32: %dx%d", H, W);
    int rc = lk_check_params(ctx, params, "dfe_ego_motion_from_images_f32");
    if (rc) return rc;
    rc = check_select_args(ctx, params->quality, params->min_dist, params->max_points, "dfe_ego_motion_from_images_f32");
    if (rc) return rc;
    DFE_REQUIRE(ctx, iterations >= 1 && iterations <= 65536 && ransac_max_dist > 0, DFE_E_ARG, "dfe_ego_motion_from_images_f32: iterations=%d (1..65536) ransac_max_dist=%g",
                iterations, ransac_max_dist);
    const int mp = params->max_points;
    // arena: luminance of both frames (C = 3), the response, the selection's list, the pyramids.  The point lists live in the side
    // buffer: the pose step lays its own data out from the arena's start.
    const size_t HW = (size_t)H * W;
    float *y0, *y1, *resp;
    SelWs sel;
    LkWs lk;
    rc = dfe_scratch_carve(ctx, [&](DfeCarve &c) {
        y0 = c.take<float>(C == 3 ? HW : 0); y1 = c.take<float>(C == 3 ? HW : 0); resp = c.take<float>(HW);
        sel = sel_layout(c, H, W);
        lk = lk_layout(c, H, W, params->levels);
    });
    if (rc) return rc;
    void *aux = nullptr;
    rc = dfe_aux_scratch(ctx, (size_t)mp * 24, &aux);
    if (rc) return rc;
    float *p0 = (float *)aux, *p1 = p0 + 2 * (size_t)mp, *wts = p1 + 2 * (size_t)mp;
    int *status = (int *)(wts + mp);
    const float *Y0 = im0, *Y1 = im1;
    if (C == 3) {
        rc = dfe_rgb2y_f32(ctx, im0, H, W, y0);
        if (rc) return rc;
        rc = dfe_rgb2y_f32(ctx, im1, H, W, y1);
        if (rc) return rc;
        Y0 = y0; Y1 = y1;
    }
    corner_response_run(ctx, Y0, H, W, resp);
    int n = 0;
    rc = select_run(ctx, resp, H, W, params->quality, params->min_dist, mp, p0, nullptr, &n, sel);
    if (rc) return rc;
    // dfe_stream_push_* (stream.hip) tells the two "fewer than 8" refusals below from an argument error by the counts: *n_corners and
    // *n_found are written BEFORE the refusal they explain, every argument error returns before *n_corners is written, and nothing
    // behind the second refusal returns DFE_E_ARG with a count under 8.  Keep that order, or give the refusals a code of their own.
    if (n_corners) *n_corners = n;
    if (n_found) *n_found = 0;
    DFE_REQUIRE(ctx, n >= 8, DFE_E_ARG, "dfe_ego_motion_from_images_f32: only %d corners", n);
    rc = track_run(ctx, Y0, Y1, H, W, p0, n, params, p1, status, nullptr, wts, lk);
    if (rc) return rc;
    std::vector<int> hs(n);
    DFE_HIP(ctx, hipMemcpyAsync(hs.data(), status, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (pts0_out) DFE_HIP(ctx, hipMemcpyAsync(pts0_out, p0, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (pts1_out) DFE_HIP(ctx, hipMemcpyAsync(pts1_out, p1, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (status_out) DFE_HIP(ctx, hipMemcpyAsync(status_out, status, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    DFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int found = 0;
    for (int i = 0; i < n; ++i) found += hs[i] != 0;
    if (n_found) *n_found = found;
    DFE_REQUIRE(ctx, found >= 8, DFE_E_ARG, "dfe_ego_motion_from_images_f32: only %d of %d corners tracked", found, n);
    return dfe_ego_motion_from_points_f32(ctx, p0, p1, wts, n, K9, ransac_max_dist, iterations, seed, R9, T3, n_inliers, F9);
}

}  // extern "C"
