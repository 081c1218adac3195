// fm_select.h -- WHICH kernel matches a pair of K-plane feature maps (nn.SpatialMatching on learned features), decided in one place.
// No HIP header: a plain host program can include it (tests/fm_select_check.cpp).
//   * a planner (version2.hip, single_scale.hip) asks fm_select whether the volume needs a place in its arena;
//   * dfe_fm_run (feat_matching_dispatch.hip) asks it again for the same job and launches the pick.
// A kernel is chosen here and nowhere else; a launcher never declines.  Every condition a kernel family puts on a shape -- options, cost-
// volume mode, window sizes, offset limits, pointer alignment, LDS budgets -- is in fm_select, with the tile constants and the LDS formulas
// it reads; the launchers take the geometry from the FmPick.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FM_HD __host__ __device__
#else
#define FM_HD
#endif

// ---- tile constants and geometry of the matcher families (the kernels are in feat_matching*.hip) ----
// flat tiles (feat_matching_flat.hip)
constexpr int FF_PX = 4;                     // pixels per lane
constexpr int FF_GROUPS = 64;                // groups (lanes) per tile
template <int MW> struct FfGeom {
    static constexpr int PITCH = (64 * FF_PX + 2 * (MW - 1) + 8 + 3) / 4 * 4;   // floats per LDS tile row (piece A | piece B)
    static constexpr int NLOAD = (PITCH + 63) / 64;                             // LDS-DMA loads per tile row
    static constexpr int NB4 = (FF_PX + MW - 1 + 3) / 4;                        // b128 reads of a lane's window row
};
// floats per window slot of the copy-out image: a multiple of 4 with room for the alignment shift (<= 3 floats) of a window whose
// place in the output is not 16-B aligned, and not a multiple of 8 (the 64 lanes' 16-B writes then fall on different banks)
FM_HD inline int ff_wnp(int WN) {
    int w = (WN + 3 + 3) & ~3;
    return (w & 7) ? w : w + 4;
}
// chunk, row and one-chunk kernels (feat_matching.hip)
constexpr int FM_TX = 8, FM_TY = 8, FM_NW = 8, FM_MAXT = 8;   // tile, waves, max tasks per wave
constexpr int F64_TY = 16;
// banded GEMM on the matrix cores (feat_matching_mfma.hip)
constexpr int FMM_R = 8;     // output rows per block (= waves)
constexpr int FMM_KC = 8;    // planes per stage (two MFMA k-steps); the arg-min form takes 16 where K % 16 == 0

// what getModel's tail + processOutput leave per pair (opticalflow_model.lua:201-252): the centre-pasted full-frame flow and confidences,
// optionally the per-pixel class index and extractOutput score over the model's own output region
struct DfeSoftOut {
    int use_threshold;             // 0: processOutput(geometry, out, true, nil);  1: ...(geometry, out, true, threshold)
    float threshold;
    int hFull, wFull;              // geometry.hImg, geometry.wImg
    float *full, *full_conf;       // [2][hFull][wFull] (plane 0 = y), [hFull][wFull]: ZEROED by the caller; the kernel writes the pasted region
    long long *index;              // [H1][W1] or NULL
    float *scores;                 // [H1][W1] or NULL
};

// what the choice reads from the context: dfe_set_cost_volume_kernel's mode and the options (-1 = automatic)
struct FmEnv { int cv_mode, fm_flat, fm64, fm_rows, fm_mfma, fm_split; };

// FM_VOLUME: out [H1][W1][maxh][maxw].  FM_ARGMIN: no volume -- `min` over the window and the decode of version2/test.lua:45-51 (idx /
// xflow / yflow, each may be NULL).  FM_SOFT / FM_MEAN: no volume -- Minus -> SoftMax over the window -> processOutput, its arg-max or
// its 'mean' branch (soft; FM_MEAN does not read use_threshold, threshold and scores)
enum FmForm { FM_VOLUME = 0, FM_ARGMIN = 1, FM_SOFT = 2, FM_MEAN = 3 };
// one single-pair match.  in1 is a view: rows pitch1 floats apart, planes plane1 floats apart (prepareInput's narrow of a feature map,
// opticalflow_model.lua:147-149; W1 and H1 * W1 for a contiguous map); in2 is [K][H1 + maxh - 1][W1 + maxw - 1].  fm_select uses the
// pointers only for their alignment bits and for being null or not: a planner whose maps will be arena buffers (256-byte aligned)
// leaves in1 / in2 null
struct FmJob {
    const float *in1, *in2;
    int pitch1;
    long long plane1;
    int K, H1, W1, maxh, maxw;
    FmForm form;
    float *out;
    long long *idx;
    float *xflow, *yflow;
    const DfeSoftOut *soft;
    float *norms;        // matrix-core matcher: fm_mfma_scratch floats for |a|^2 [H1][W1] | |b|^2 [H2][W2]; NULL: dfe_fm_run takes the ctx's side buffer
    bool norms_ready;    // ... already there (left by the convolution that made the features)
};
inline FmJob fm_job(FmForm form, const float *in1, const float *in2, int K, int H1, int W1, int maxh, int maxw) {
    FmJob j{};
    j.in1 = in1; j.in2 = in2; j.pitch1 = W1; j.plane1 = (long long)H1 * W1;
    j.K = K; j.H1 = H1; j.W1 = W1; j.maxh = maxh; j.maxw = maxw; j.form = form;
    return j;
}
// floats of scratch the matrix-core matcher needs for the two norm planes
inline size_t fm_mfma_scratch(const FmJob &j) { return (size_t)j.H1 * j.W1 + (size_t)(j.H1 + j.maxh - 1) * (j.W1 + j.maxw - 1); }

enum FmKernel { FM_K_NONE = 0, FM_K_MFMA, FM_K_WIN64, FM_K_FLAT, FM_K_ROWS, FM_K_CHUNK, FM_K_REF };
// the kernel and the launch geometry its launcher needs, computed once
struct FmPick {
    FmKernel kernel;
    size_t lds;          // dynamic LDS bytes of a block (REF: 0)
    int S, nd, WNP;      // FLAT: blocks per tile, window rows of a block, floats per window slot of the copy-out image
    int extra;           // FLAT: 17 window rows on 16 waves
    int pitch;           // WIN64, CHUNK: floats per LDS tile row
    int KB;              // CHUNK: planes per slab
    int KC;              // MFMA: planes per stage
};

// the name dfe_last_kernel reports for a pick
inline const char *fm_kernel_name(FmKernel k, FmForm form) {
    switch (k) {
    case FM_K_MFMA: return form == FM_VOLUME ? "fmm_kernel" : "fmm_kernel+argmin";
    case FM_K_WIN64: return "feat_matching_win64_kernel";
    case FM_K_FLAT:
        return form == FM_MEAN ? "feat_matching_flat_mean_kernel" : form == FM_SOFT ? "feat_matching_flat_kernel+softmax"
               : form == FM_ARGMIN ? "feat_matching_flat_kernel+argmin" : "feat_matching_flat_kernel";
    case FM_K_ROWS: return "feat_matching_rows_kernel";
    case FM_K_CHUNK: return "feat_matching_kernel";
    case FM_K_REF: return "ssd_cv_ref_kernel";
    default: return "";
    }
}

// The one-chunk matcher's window-level conditions and tile geometry (maxh * maxw == 64, K <= 16 planes resident in LDS): the single-pair
// pick below, the multi-pair launcher dfe_feat_matching_win64_batch and the multiscale plan (dfe_feat_matching_win64_ok) all read it
// here, so a plan never meets a refusal (round-3 advisor: with dfe_set_cost_volume_kernel(1) or fm64 = 0 the fused second scale was
// planned and then refused).
inline bool fm_win64_geom(const FmEnv &e, int K, int maxh, int maxw, int *pitch_out, size_t *lds_out) {
    if (maxh * maxw != 64 || K < 1 || K > 16 || e.cv_mode == 1 || e.fm64 == 0) return false;
    const int tcols = FM_TX + maxw - 1, trows = F64_TY + maxh - 1;
    if (tcols > 16) return false;                          // (the staging deals 16 columns per tile row)
    int pitch = tcols;
    while ((pitch - maxw) % 32 != 0) ++pitch;              // pitch == maxw (mod 32): conflict-free for the lane <-> (dy, dx) reads
    size_t lds = (size_t)K * trows * pitch * sizeof(float);
    if (lds < (size_t)8 * FM_TX * 64 * sizeof(float)) lds = (size_t)8 * FM_TX * 64 * sizeof(float);   // the copy-out scratch reuses the tile
    if (lds > 64 * 1024) return false;
    if (pitch_out) *pitch_out = pitch;
    if (lds_out) *lds_out = lds;
    return true;
}

// ---- one try per kernel family: true = the family takes the job, with its geometry in p ----

// the banded GEMM on the matrix cores (opt-in, fm_mfma = 1): 16 x 16 and 17 x 17 windows, the volume or its first minimum, contiguous maps
inline bool fm_try_mfma(const FmEnv &e, const FmJob &j, FmPick &p) {
    const int K = j.K, H1 = j.H1, W1 = j.W1, maxh = j.maxh, maxw = j.maxw;
    if (e.fm_mfma <= 0 || e.cv_mode == 1 || j.form > FM_ARGMIN) return false;
    if (!((maxh == 17 && maxw == 17) || (maxh == 16 && maxw == 16))) return false;
    if (K < 1 || K > 256 || H1 < 1 || W1 < 1) return false;
    // the LDS-DMA requests address in2 as 32-bit BYTE offsets 4 * (k plane2 + row W2 + col) from the map's base: below 2^30 floats they do
    // not wrap (in1 and the norm planes are smaller)
    if ((long long)K * (H1 + maxh - 1) * (W1 + maxw - 1) >= (1ll << 30)) return false;
    const int BROWS = (FMM_R + maxh - 1 + 3) & ~3;
    // the arg-min form stages 16 planes at a time where K allows it: three of four k-steps then have their operands requested behind MFMAs
    p.KC = (j.form == FM_ARGMIN && K % 16 == 0) ? 16 : FMM_KC;
    p.lds = ((size_t)2 * (p.KC * (BROWS * 32 + 16) + p.KC * (FMM_R * 16)) + (size_t)2 * BROWS * 32) * sizeof(float);
    return true;
}

// one-chunk windows (the pyramid's 8 x 8), the volume only: the prefetching, transposing matcher -- whole 16 x 8 tiles of a 4-byte aligned
// in1 into a 16-byte aligned volume
inline bool fm_try_win64(const FmEnv &e, const FmJob &j, FmPick &p) {
    if (e.cv_mode == 2 || j.H1 < F64_TY || j.W1 < FM_TX || ((uintptr_t)j.in1 & 3) || ((uintptr_t)j.out & 15)) return false;
    if ((long long)j.K * j.H1 * j.W1 * 4 >= (1ll << 32)) return false;           // (32-bit plane offsets of the frame-1 scalar loads)
    return fm_win64_geom(e, j.K, j.maxh, j.maxw, &p.pitch, &p.lds);
}

// flat tiles: 16- / 17-wide windows of 4 .. 17 rows on frames at least 64 groups wide, every form, in1 as a view
inline bool fm_try_flat(const FmEnv &e, const FmJob &j, FmPick &p) {
    const int K = j.K, H1 = j.H1, W1 = j.W1, maxh = j.maxh, maxw = j.maxw;
    const bool volume = j.form == FM_VOLUME;
    if (e.cv_mode == 1 || e.cv_mode == 2 || e.fm_flat == 0) return false;
    if (maxw != 16 && maxw != 17) return false;
    if (maxh < 4 || maxh > 17 || (maxh == 17 && maxw != 17)) return false;
    const int G = (W1 + FF_PX - 1) / FF_PX;
    if (G < FF_GROUPS || K < 1 || H1 < 1) return false;                    // (a tile must not touch more than two image rows)
    if ((long long)H1 * G > (1ll << 30) || (long long)H1 * W1 * maxh * maxw >= (1ll << 40)) return false;
    if (j.pitch1 < W1 || j.plane1 < (long long)(H1 - 1) * j.pitch1 + W1 || j.plane1 >= (1ll << 29)) return false;
    if (((uintptr_t)j.in1 | (uintptr_t)j.in2 | (volume ? (uintptr_t)j.out : 0)) & 3) return false;
    if (j.soft && (j.soft->full || j.soft->full_conf) && (j.soft->hFull < H1 || j.soft->wFull < W1)) return false;   // (the centre paste needs room)
    const bool extra = maxh == 17;
    // two half blocks per tile and CU where the window's rows split evenly into halves of >= 4 waves (the arg-min and soft-max forms need
    // the whole window in one block; 17 rows = 17 waves do not fit a CU's registers as 9 + 8)
    // (option fm_split: 0 whole tiles, 1 / 2 halves, 4 quarters; the launcher's own choice: quarters for few planes -- the copy-out is
    //  then a larger share of a tile, K = 10: 0.102 -> 0.098 ms, time_matching.lua's shape 0.024 -> 0.022 -- else halves, which cost
    //  less staging: profiles/r04_ao_fm_quarters.txt)
    const int want = e.fm_split < 0 ? (K <= 16 ? 4 : 2) : e.fm_split == 1 ? 2 : e.fm_split;
    const bool can = volume && !extra;
    p.S = can && want >= 4 && maxh == 16 ? 4 : can && want >= 2 && maxh >= 8 && maxh % 2 == 0 ? 2 : 1;
    p.nd = extra ? 16 : maxh / p.S;
    p.extra = extra;
    const int PITCH = maxw == 17 ? FfGeom<17>::PITCH : FfGeom<16>::PITCH;
    p.WNP = ff_wnp((extra ? 17 : p.nd) * maxw);
    // the copy-out image [64][WNP]; the arg-min form keeps its candidates there instead -- cv[256][NC] and ci[256][NC], NC = 16 (20 with
    // the extra task) whatever the window's height: larger than the image of a window of fewer than 8 rows; the soft-max form reads its
    // windows in 16-B pieces up to cell 4 * 16 * ceil(WN / 64) of the last window and keeps extractOutput's candidates [64][16] behind
    const size_t image = (size_t)64 * p.WNP, cand = j.form == FM_ARGMIN ? (size_t)2 * 256 * (extra ? 20 : 16) : 0;
    const size_t img_floats = j.form >= FM_SOFT ? image + 64 * 16 + 64 : image > cand ? image : cand;
    p.lds = ((size_t)3 * (extra ? 18 : p.nd + 1) * PITCH + 3 * 64 * FF_PX + 64 + img_floats) * sizeof(float);
    // (holds for every shape that gets here: 146368 bytes at most, the 17 x 17 soft-max -- the sweep of tests/fm_select_check.cpp prints it)
    return p.lds * p.S <= 160 * 1024;
}

// The row kernel pays a barrier and a tile refill per plane and only fills its 256-column blocks on wide frames: measured
// 625 x 465, 16 x 16: K = 32 0.37 ms against 0.55 ms for the chunk kernel below, K = 10 0.168 against 0.194 (with the next plane's
// loads in flight behind the arithmetic; 0.46 / 0.23 before); K = 10, 293 x 153: 0.064 against 0.039 ms.
// (W1 == 1: the patch-mode call of the trainers, any K -- the chunk kernel needs 8 x 8 pixels.)
inline bool fm_try_rows(const FmEnv &e, const FmJob &j, FmPick &p) {
    bool rows_pays = (j.K >= 8 && j.W1 >= 400) || j.W1 < FM_TX || j.H1 < FM_TY;
    if (e.fm_rows >= 0) rows_pays = e.fm_rows != 0;   // tuning
    if (!rows_pays || (j.maxw != 16 && j.maxw != 8) || j.maxh < 4 || j.maxh > 16 || e.cv_mode == 2 || ((uintptr_t)j.out & 15)) return false;
    const int TC = 256 + j.maxw;
    p.lds = ((size_t)2 * j.maxh * TC + 2 * 256 + (size_t)64 * j.maxh * j.maxw) * sizeof(float);
    return true;
}

// chunk: lane <-> window cell, whole 8 x 8 tiles, at most FM_MAXT (row, chunk) tasks per wave, a slab of KB planes in 48 KiB of LDS
inline bool fm_try_chunk(const FmEnv &, const FmJob &j, FmPick &p) {
    const int nchunks = (j.maxh * j.maxw + 63) / 64;
    if (j.W1 < FM_TX || j.H1 < FM_TY || FM_TY * nchunks > FM_MAXT * FM_NW) return false;
    if (((uintptr_t)j.in1 & 3) != 0) return false;
    p.pitch = (FM_TX + j.maxw - 1) | 1;                    // odd pitch: the lanes behind a dy-row jump land on other banks
    const size_t per_plane = (size_t)(FM_TY + j.maxh - 1) * p.pitch * sizeof(float);
    const int kb = (int)((48 * 1024) / per_plane);
    if (kb < 1) return false;
    p.KB = kb < j.K ? kb : j.K;
    p.lds = (size_t)p.KB * per_plane;
    return true;
}

// The order of the tries: matrix cores (opt-in), one-chunk, flat tiles, rows, chunk, reference order.  Only the flat tiles read in1 as a
// view, and only they and the matrix cores have forms without the volume: FM_VOLUME on a contiguous in1 always ends at FM_K_REF (the
// reference-order kernel takes every shape; mode 1 asks for it); a strided in1 that the flat tiles do not want is FM_K_NONE (the caller
// copies and asks again); the other forms are FM_K_MFMA, FM_K_FLAT or FM_K_NONE (the caller goes through the volume).
inline FmPick fm_select(const FmEnv &e, const FmJob &j) {
    const bool volume = j.form == FM_VOLUME, contig = j.pitch1 == j.W1 && j.plane1 == (long long)j.H1 * j.W1;
    const auto tried = [&](FmKernel k, bool (*fn)(const FmEnv &, const FmJob &, FmPick &), FmPick &p) {
        p = FmPick{};
        p.kernel = fn(e, j, p) ? k : FM_K_NONE;
        return p.kernel != FM_K_NONE;
    };
    FmPick p{};
    if (contig && tried(FM_K_MFMA, fm_try_mfma, p)) return p;
    if (contig && volume && tried(FM_K_WIN64, fm_try_win64, p)) return p;
    if (tried(FM_K_FLAT, fm_try_flat, p)) return p;
    if (!contig || !volume) return FmPick{};
    if (e.cv_mode != 1 && (tried(FM_K_ROWS, fm_try_rows, p) || tried(FM_K_CHUNK, fm_try_chunk, p))) return p;
    p = FmPick{};
    p.kernel = FM_K_REF;
    return p;
}
