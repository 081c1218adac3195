// cv_records.h -- device code and kernel-argument layouts that the fused cost-volume epilogue (ssd_cost_volume.hip) and the tail kernels
// (postops.hip) share: what the sweep leaves behind, where the finalize puts its results, and the finalize of one pixel.  No launcher is
// declared here: tools/kernel_hash.py hashes this file whole.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// sorting networks of extract_output.cpp:17-61: a comparator swaps value AND index iff v[b] > v[a]
__device__ __forceinline__ void dfe_sortswap(float *v, float *ix, int a, int b) {
    if (v[b] > v[a]) {
        float t = v[b]; v[b] = v[a]; v[a] = t;
        t = ix[b]; ix[b] = ix[a]; ix[a] = t;
    }
}
__device__ __forceinline__ void dfe_sort4(float *v, float *ix) {   // :27-33
    dfe_sortswap(v, ix, 0, 2); dfe_sortswap(v, ix, 1, 3); dfe_sortswap(v, ix, 0, 1); dfe_sortswap(v, ix, 2, 3); dfe_sortswap(v, ix, 1, 2);
}
__device__ __forceinline__ void dfe_sort8(float *v, float *ix) {   // :35-61
    dfe_sortswap(v, ix, 0, 1); dfe_sortswap(v, ix, 2, 3); dfe_sortswap(v, ix, 4, 5); dfe_sortswap(v, ix, 6, 7);
    dfe_sortswap(v, ix, 0, 2); dfe_sortswap(v, ix, 1, 3); dfe_sortswap(v, ix, 4, 6); dfe_sortswap(v, ix, 5, 7);
    dfe_sortswap(v, ix, 1, 2); dfe_sortswap(v, ix, 5, 6); dfe_sortswap(v, ix, 0, 4); dfe_sortswap(v, ix, 3, 7);
    dfe_sortswap(v, ix, 1, 5); dfe_sortswap(v, ix, 2, 6);
    dfe_sortswap(v, ix, 1, 4); dfe_sortswap(v, ix, 3, 6);
    dfe_sortswap(v, ix, 2, 4); dfe_sortswap(v, ix, 3, 5);
    dfe_sortswap(v, ix, 3, 4);
}

// what the cost-volume kernel's fused epilogue leaves behind for flow_finalize_kernel
#define DFE_LEAD 16   // leading cells of every pixel kept for extractOutput
struct CvFuseArgs {
    float2 *part;          // [nchunks][Ptot]: per (chunk, pixel) the chunk's minimum cost and the 0-based index (int bits) of
                           // the first cell that attains it
    float *centre;         // [Ptot]: cost of the centre cell
    float *lead;           // [Ptot][DFE_LEAD]: the pixel's first cells
    long long Ptot;
    int cmid, lmid;        // chunk / lane of the centre cell
    int row_off;           // output-row offset of this launch inside the pair
    float *rec;            // the role-split row-image kernels leave their per-pixel results here instead of in the planes above:
                           // [column group = tile column][output row of the pair][DFE_REC floats] -- one 128-B line per TILE ROW:
                           // 8 x (minimum, first index as int bits) | 8 x centre cost | 8 x 0 | lead cells -- whole lines, written by ONE store of one wave,
                           // a block sweeping down its column writes consecutive lines.  (The planes took four partial-line stores per
                           // PIXEL and row step -- 8 B + 8 B + 64 B + 4 B, lines shared with neighbouring blocks on other XCDs -- and made
                           // the fused 1080p kernel take 1.78 .. 2.21 ms depending on the process; a 128-B record per pixel, 251 MB at
                           // 1080p, cost 0.8 ms: DESIGN section 5.)  Behind the first line: [pixel][DFE_REC_NLEAD] the pixels' first cells
                           // (extractOutput's input; read back from the volume at first -- that doubled the finalize kernel and, at 1080p,
                           // left volume lines in the memory-side cache that slowed the next launch's stores by 10 %).
    int rec_rows;          // output rows of the pair (the record's row pitch)
};
#define DFE_REC_NLEAD 8    // a pixel's first cells kept in its tile row's record
#define DFE_REC (32 + 8 * DFE_REC_NLEAD)   // floats per tile-row record (3 whole 128-B lines)
#define DFE_REC_CENTRE 16  // (entries 0..15: (minimum, index) of the 8 pixels; 16..23: their centre costs; 24..31: 0 or the fallback flags)
#define DFE_REC_FLAG 24    // (entries 24..31, volume-free sweep only: 1 = fewer than M lead cells pass, extractOutput's hits are in the fallback plane)
#define DFE_REC_LEAD 32    // (entries 32..: [pixel][DFE_REC_NLEAD] the pixels' first cells)
// Volume-free flow sweep (ssd_cv_rowimg_flow_kernel): extractOutput's rare fall-back is taken inside the kernel, from the row image in
// LDS.  A pixel whose first DFE_REC_NLEAD cells hold fewer than M values above the threshold gets its first M hits over all cells, in
// index order, in the fallback plane [column group][output row][8 pixels][DFE_FB] floats = (value, 1-based index as a float) pairs,
// zero-padded; the pixel's record flag says so.  Other pixels' entries are never written nor read.
#define DFE_FB 16          // floats per pixel of the fallback plane: 8 (value, index) pairs, 64 B
struct CvNovolArgs {
    float *fb;             // the fallback plane
    float thr;             // the largest float <= the extractOutput threshold: v > thr <=> (double)v > threshold for every float v
    int M;                 // hits extractOutput keeps (8 if threshold < 0.2, else 4)
};
// ---- the finalize of a pixel from its tile row's record: flow_finalize_kernel's record path (postops.hip), kept here next to the record layout it reads
// (round 4 also ran it at the end of the fused sweep: no gain, ssd_cost_volume.hip) ----
// replaces: radial/radial_opticalflow_groundtruth.lua:87-105 (min(3), tie-break, decode, extractOutput)
struct TailOut {
    long long *idx;      // [P] or null
    float *best;         // [P] or null
    float *fy, *fx;      // decoded displacement, written at (y+pad_t)*pitch + x+pad_l  (pad-back :108), or null
    float *scores;       // extractOutput score, same addressing as fy/fx when padded != 0, else [P]
    long long *imaxs;    // [P] or null (goes with scores)
    int Wo;              // pixels per volume row
    int pitch, pad_t, pad_l;   // full-frame addressing for fy/fx/(scores if padded)
    int padded;          // scores addressed full-frame (1) or [P] (0)
    long long p_off;     // pixel offset of this band inside the [P] outputs
    int row_off;         // output-row offset of this band
    // frame mode (flow_finalize_kernel, one band only): the threads cover the whole H x W frame -- interior pixels run the
    // pipeline's tail and the flow -> depth formula, border pixels are zeroed -- so the pair step needs no third launch
    int frame_H, frame_W;     // 0 = off
    float *depth, *conf;      // [H][W] or null
    float mw, mh, infty;      // focus of expansion, depth clamp (test_opticalflow.lua:143-216)
};
// frame mode of the finalize (one band only): it also zeroes the frame border and makes depth / confidence
struct DfePairDepth { int H, W; float cx, cy; float *depth, *conf; };
// The one description of where a flow step's results go, made by the entry point: whatever the arguments do not name is zero (first band,
// frame mode off).  The pipelines set row_off / p_off per band, the finalize the frame-mode fields from a DfePairDepth.
inline TailOut dfe_tailout(int64_t *idx, float *best, float *fy, float *fx, float *scores, int64_t *imaxs, int Wo, int pitch, int pad_t, int pad_l,
                           int scores_padded) {
    TailOut o{};
    o.idx = (long long *)idx; o.best = best; o.fy = fy; o.fx = fx; o.scores = scores; o.imaxs = (long long *)imaxs;
    o.Wo = Wo; o.pitch = pitch; o.pad_t = pad_t; o.pad_l = pad_l; o.padded = scores_padded;
    return o;
}

// flow -> depth of one pixel (i, j) with displacement (dy, dx): the quirk-preserving cartesian formula of
// test_opticalflow.lua:143-216 (same arithmetic as flow_to_depth_cartesian_kernel)
__device__ __forceinline__ void pair_depth_px(int i, int j, float dy, float dx, float mw, float mh, float infty, float *r_out, float *c_out) {
#pragma clang fp contract(off)   // products rounded one by one, as the reference's C (and the oracle) do
    const float py = (float)i - mh, px = (float)j - mw;
    const float pn = (float)sqrt((double)(px * px + py * py));
    const float dn = (float)sqrt((double)(dx * dx + dy * dy));
    float r = 0.f, c = 0.f;
    if (dn >= 0.2f) {
        const float q = pn / dn;
        r = q < infty ? q : infty;
        if (px * dx + dy * dy > 0.125f) c = 1.0f;   // test_opticalflow.lua:181 (sic)
    } else {
        c = 1.0f;
        r = infty;
    }
    *r_out = r;
    *c_out = c;
}

// A6: the record's (minimum, first index), centre override.  A9: decode.  A7: extractOutput over the pixel's first DFE_REC_NLEAD cells
// (in the record), walking on through the volume itself only if fewer than M of them pass the threshold (extract_output.cpp:99-112 stops
// at M as well).  p: pixel index inside the band (row-major over Wo); (fi, fj): its frame position (frame mode).
// fb != nullptr (the volume-free sweep; vol is nullptr then): pixels whose record flag is set take their hits from the fallback plane.
template <int M>
__device__ __forceinline__ void dfe_finalize_rec_pixel(const float *__restrict__ rec, int rec_rows, const float *__restrict__ vol, long long p, int N,
                                                       int hWin, int wWin, int middle, double threshold, const TailOut &o, int fi, int fj,
                                                       int iy = -1, int ix = -1, const float *__restrict__ fb = nullptr) {
    // (iy, ix): the pixel's row / column inside the band where the caller has them (frame mode) -- else from p, as a 32-bit division
    // (the 64-bit quotient and remainder of the first version were a hundred instructions of a kernel that has few others)
    const long long pg = o.p_off + p;
    const int yb = iy >= 0 ? iy : (int)((unsigned)p / (unsigned)o.Wo), x = ix >= 0 ? ix : (int)((unsigned)p - (unsigned)yb * (unsigned)o.Wo);
    const int y = yb + o.row_off;
    const int ncols = (o.Wo + 7) >> 3;
    const int g = min(x >> 3, ncols - 1), xb = g == ncols - 1 ? o.Wo - 8 : g << 3;   // (the last tile column is shifted inwards)
    const float *rp = rec + ((long long)g * rec_rows + y) * DFE_REC;
    // (non-temporal: what is read here is REWRITTEN by the next frame's cost-volume launch -- lines left in the memory-side cache by
    //  these reads made that launch's stores slower: 1080p 2.4 against 1.8 ms)
    // (the pixel's (minimum, index) pair as ONE 8-byte load and its eight lead cells as two 16-byte loads -- the record is 128-B aligned
    //  and both pieces are naturally aligned inside it: four load instructions per pixel instead of eleven)
    typedef float dfe_f2v __attribute__((ext_vector_type(2)));
    typedef float dfe_f4v __attribute__((ext_vector_type(4)));
    float2 b;
    {
        const dfe_f2v bv = __builtin_nontemporal_load(reinterpret_cast<const dfe_f2v *>(rp + 2 * (x - xb)));
        b.x = bv[0]; b.y = bv[1];
    }
    const float cen = __builtin_nontemporal_load(rp + DFE_REC_CENTRE + x - xb);
    long long id = (long long)__float_as_int(b.y) + 1;
    if (middle > 0 && b.x == cen) id = middle;
    if (o.idx) o.idx[pg] = id;
    if (o.best) o.best[pg] = b.x;
    const long long fo = (long long)(y + o.pad_t) * o.pitch + x + o.pad_l;
    const int id0 = (int)id - 1, fl = id0 / wWin;                               // (id <= hWin * wWin: 32-bit)
    const float dyf = (float)(fl - (hWin - 1) / 2), dxf = (float)(id0 - fl * wWin - (wWin - 1) / 2);
    if (o.fy) o.fy[fo] = dyf;
    if (o.fx) o.fx[fo] = dxf;
    if (o.frame_H && o.depth) pair_depth_px(fi, fj, dyf, dxf, o.mw, o.mh, o.infty, &o.depth[fo], &o.conf[fo]);
    if (o.scores) {
        static_assert(DFE_REC_NLEAD == 8, "the record holds a pixel's first 8 cells");
        float hv[M], hi[M];
#pragma unroll
        for (int j = 0; j < M; ++j) { hv[j] = 0.f; hi[j] = 0.f; }
        int n = 0;
        if (fb && __builtin_nontemporal_load(rp + DFE_REC_FLAG + x - xb) != 0.f) {   // rare: the kernel found fewer than M hits in the lead cells
            const float *fp = fb + (((long long)g * rec_rows + y) * 8 + (x - xb)) * DFE_FB;
#pragma unroll
            for (int j = 0; j < M; ++j) { hv[j] = fp[2 * j]; hi[j] = fp[2 * j + 1]; }
        } else {
            float qq[DFE_REC_NLEAD];
            const float *lv = rp + DFE_REC_LEAD + (x - xb) * DFE_REC_NLEAD;
            {
                const dfe_f4v q0 = __builtin_nontemporal_load(reinterpret_cast<const dfe_f4v *>(lv)), q1 = __builtin_nontemporal_load(reinterpret_cast<const dfe_f4v *>(lv) + 1);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) { qq[kk] = q0[kk]; qq[4 + kk] = q1[kk]; }
            }
#pragma unroll
            for (int kk = 0; kk < DFE_REC_NLEAD; ++kk) {
                if (kk < N && n < M && (double)qq[kk] > threshold) {
#pragma unroll
                    for (int j = 0; j < M; ++j)
                        if (j == n) { hv[j] = qq[kk]; hi[j] = (float)(kk + 1); }
                    ++n;
                }
            }
            if (!fb && n < M && N > DFE_REC_NLEAD) {   // rare: keep scanning the volume itself (with fb: flag clear, n == M here)
                const float *v = vol + p * N;
                for (int kk = DFE_REC_NLEAD; kk < N && n < M; ++kk) {
                    const float t = v[kk];
                    if ((double)t > threshold) {
#pragma unroll
                        for (int j = 0; j < M; ++j)
                            if (j == n) { hv[j] = t; hi[j] = (float)(kk + 1); }
                        ++n;
                    }
                }
            }
        }
        if (hv[0] > 0) {
            if (M == 4) dfe_sort4(hv, hi); else dfe_sort8(hv, hi);
            if (o.imaxs) o.imaxs[pg] = (long long)hi[0];
#pragma unroll
            for (int j = 1; j < M; ++j) hv[j] += hv[j - 1];
            double acc = 0;
#pragma unroll
            for (int j = 0; j < M; ++j) acc += hv[j];
            o.scores[o.padded ? fo : pg] = (float)acc;
        } else if (o.padded) {
            o.scores[fo] = 0.f;   // pair mode: the caller's buffer is not pre-zeroed (pixels without a hit read 0)
        }
    }
}
