// subpixel_costs.h -- the five SSD costs a sub-pixel refinement needs (the arg-min cell and its two neighbours on either axis), formed
// from the frames with shared reads; used by the single-scale refinement (subpixel.hip) and the pyramid's (multiscale_subpixel.hip).
#pragma once
#include <hip/hip_runtime.h>

// A: frame-0 patch of the pixel, channel 0 (row i at A + i W); B: frame 1, channel 0, at the pixel's window origin plus the arg-min
// cell's column s (row t of cell row r at B + (r + t) W); rows W, channels `plane` floats apart.  r: the cell's row, rm / rp: the rows of
// its y neighbours, dsm / dsp: the columns of its x neighbours relative to s -- the caller replaces a neighbour outside the window by
// the cell itself (in bounds), and ignores that axis.
// Per channel, frame 1's k + 2 rows around the cell are read once, k + 2 values each (the x neighbours are the same row shifted by
// one), and each frame-0 row once, kept in a ring of three rows (row t of frame 1 meets frame-0 rows t - 1, t, t + 1 for the y+1 cost,
// the centre row and the y-1 cost): C (kh kw + (kh + 2)(kw + 2)) loads -- 390 at k = 7, C = 3 -- against 5 C kh kw = 735 for five
// independent sums.  The sums run in the (c, i, j) order with separately rounded multiply and add (ssd_cv_ref_kernel), so each cost is
// the bit pattern the cost volume's reference kernel gives for that cell.
// K > 0: a K x K patch, known at compile time: the frame-0 rows stay in registers and the row loop unrolls, so that a channel's loads
// are in flight together; K == 0: any kh x kw patch, each term read where it is used (6 loads per term).
template <int K>
__device__ __forceinline__ void subpixel_five_costs(const float *A, const float *B, long long plane, int W, int C, int kh, int kw, int r, int rm,
                                                    int rp, int dsm, int dsp, float &c0, float &cxm, float &cxp, float &cym, float &cyp) {
#pragma clang fp contract(off)
    c0 = 0.f; cxm = 0.f; cxp = 0.f; cym = 0.f; cyp = 0.f;
    for (int c = 0; c < C; ++c, A += plane, B += plane) {
        if constexpr (K > 0) {
            constexpr int KW = K;
            float ap[KW], ac[KW], an[KW];   // frame-0 rows t - 1, t, t + 1
#pragma unroll
            for (int j = 0; j < KW; ++j) { ap[j] = 0.f; ac[j] = 0.f; an[j] = 0.f; }
#pragma unroll
            for (int t = -1; t <= K; ++t) {
                // frame-1 row r + t (rows -1 and K only feed the y-1 / y+1 costs: rm, rp stand in for them at the window's edge),
                // columns s - 1 .. s + KW (the end columns only feed the x costs: dsm, dsp at the edge)
                const int row = t < 0 ? rm : t >= K ? rp + K - 1 : r + t;
                const float *bp = B + (long long)row * W;
                float b[KW + 2];
                b[0] = bp[dsm];
#pragma unroll
                for (int j = 0; j < KW; ++j) b[j + 1] = bp[j];
                b[KW + 1] = bp[dsp + KW - 1];
#pragma unroll
                for (int j = 0; j < KW; ++j) { ap[j] = ac[j]; ac[j] = an[j]; }
                if (t + 1 < K) {
#pragma unroll
                    for (int j = 0; j < KW; ++j) an[j] = A[(long long)(t + 1) * W + j];
                }
                // ap / ac / an now hold frame-0 rows t - 1, t, t + 1
                if (t >= 0 && t < K) {
#pragma unroll
                    for (int j = 0; j < KW; ++j) {
                        float d = ac[j] - b[j + 1]; float d2 = d * d; c0 = c0 + d2;
                        d = ac[j] - b[j]; d2 = d * d; cxm = cxm + d2;
                        d = ac[j] - b[j + 2]; d2 = d * d; cxp = cxp + d2;
                    }
                }
                if (t + 1 < K) {   // row t of frame 1 against frame-0 row t + 1: the cell one row up
#pragma unroll
                    for (int j = 0; j < KW; ++j) { const float d = an[j] - b[j + 1]; const float d2 = d * d; cym = cym + d2; }
                }
                if (t >= 1) {         // against frame-0 row t - 1: the cell one row down
#pragma unroll
                    for (int j = 0; j < KW; ++j) { const float d = ap[j] - b[j + 1]; const float d2 = d * d; cyp = cyp + d2; }
                }
            }
        } else {
            for (int i = 0; i < kh; ++i) {
                const float *ar = A + (long long)i * W;
                const float *b0 = B + (long long)(r + i) * W, *bm = B + (long long)(rm + i) * W, *bq = B + (long long)(rp + i) * W;
                for (int j = 0; j < kw; ++j) {
                    const float v = ar[j];
                    float d = v - b0[j]; float d2 = d * d; c0 = c0 + d2;
                    d = v - b0[j + dsm]; d2 = d * d; cxm = cxm + d2;
                    d = v - b0[j + dsp]; d2 = d * d; cxp = cxp + d2;
                    d = v - bm[j]; d2 = d * d; cym = cym + d2;
                    d = v - bq[j]; d2 = d * d; cyp = cyp + d2;
                }
            }
        }
    }
}
