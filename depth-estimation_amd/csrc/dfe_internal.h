// dfe_internal.h -- shared by the translation units of libdfe.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_ext.h>
#include "../../include/dfe.h"
#include "dfe_carve.h"
#include "fm_select.h"

// Behaviour switches of the launchers (dfe_set_option / dfe_get_option, include/dfe.h).  -1 = automatic: the launcher's own choice
// per shape.  The environment is read ONCE, in dfe_ctx_create (tuning scripts), never inside a launcher.
enum DfeOpt {
    DFE_OPT_CASCADE_PX = 0,   // lane <-> pixel cascade kernels (0: keep the lane <-> cell kernels)
    DFE_OPT_FINE_FUSE,        // finest pyramid scale inside its volume / matcher kernel (0 / 1 forces)
    DFE_OPT_MID_FUSE,         // the second scale the same way
    DFE_OPT_FINE_NQ,          // tile-height code of the fused finest kernel
    DFE_OPT_MID_NQ,           // ... of the fused second scale
    DFE_OPT_PREP_TILES,       // every scale from one read of the frames (0: one launch per scale set)
    DFE_OPT_XPOSE,            // 1-KB transposed stores of one-chunk windows (0: 256-B pieces)
    DFE_OPT_XPOSE_NT,         // their non-temporal hint (0 / 1 forces)
    DFE_OPT_SOFT_EPILOGUE,    // soft-min inside the pyramid's volume kernel (0 / 1 forces)
    DFE_OPT_CONV_BATCH,       // batched LDS-tiled convolution (0: one direct launch per layer and input)
    DFE_OPT_CONV_NT10,        // 10 output planes per thread where nOut % 10 == 0 (0: two groups of 5)
    DFE_OPT_FM64,             // one-chunk feature matcher (0: chunk kernel per scale)
    DFE_OPT_FM_ROWS,          // feature matcher: the row kernels (0 / 1 forces)
    DFE_OPT_SWEEP_OVH,        // cost model of the persistent column sweep: per-piece overhead in rows
    DFE_OPT_SWEEP_BLOCKS,     // ... number of blocks
    DFE_OPT_DEBUG_ARENA,      // print where the scratch arena lands
    DFE_OPT_FM_FLAT,          // feature matcher: the flat-tile kernel for 16- / 17-wide windows (0: the round-3 row / chunk kernels)
    DFE_OPT_FM_SPLIT,         // ... a tile's window rows dealt to two co-resident half blocks (0: one block per tile)
    DFE_OPT_CONV_NARROW,      // batched convolution: 64 x 16 output tiles (0: 128 x 8; automatic: for kernels of 9 x 9 and larger)
    DFE_OPT_CONV_MFMA,        // one-call models: filter layers as implicit GEMMs on the matrix cores (fused multiply-adds; default 0 = exact kernels)
    DFE_OPT_FM_MFMA,          // feature matcher as a banded GEMM on the matrix cores, |a|^2 + |b|^2 - 2 a.b (default 0 = exact k-ordered sums)
    DFE_OPT_ARENA_CONTIG,     // scratch arena from physically contiguous memory (hipDeviceMallocContiguous; 0: plain hipMalloc)
    DFE_OPT_CV_NOVOL,         // single-scale flow step without its cost volume (volume-free sweep; 0: build the volume, finalize reads it)
    DFE_OPT_CONV_NT,          // batched convolution: n > 0 = n output planes per thread where nOut % n == 0 and <kW, n> is instantiated (tests)
    DFE_OPT_CV_I8,            // volume-free flow step on the int8 matrix cores where the frames turn out byte-valued (ssd_flow_i8.hip; 0: the float sweep only)
    DFE_OPT_I8_SLOTS,         // int8 flow sweep: the number of waves its item plan takes the device to hold at once (tests; automatic: from the device)
    DFE_OPT_FILL_APEX,        // hole filling: the one-workgroup apex kernel (fill.hip; 0: per-level kernels only; n > 0: its base level has at most n cells, tests)
    DFE_OPT_SPLAT_LDS,        // four-tap temporal splat: the front and the accumulate pass with a workgroup's taps combined in LDS first (temporal_splat.hip; 0: every tap straight to global memory)
    DFE_NOPT
};
struct DfeOptName { const char *key; const char *env; bool env_presence_means_zero; };
extern const DfeOptName dfe_opt_names[DFE_NOPT];

constexpr int DFE_NSLOT = 3;   // device slots of the pipelined ingest (ingest.hip)
// a grow-only device buffer that a ctx owns: grown by dfe_grow and by nothing else, freed with the ctx; empty = {nullptr, 0}
struct DfeBuf { void *p = nullptr; size_t bytes = 0; };
struct dfe_ctx {
    int opt[DFE_NOPT];
    dfe_ctx() { for (int i = 0; i < DFE_NOPT; ++i) opt[i] = -1; }
    // the launcher's own choice `autov` unless the option was set (>= 0)
    bool opt_bool(int o, bool autov) const { return opt[o] < 0 ? autov : opt[o] != 0; }
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int cv_mode = 0;                  // dfe_set_cost_volume_kernel
    int cv_chunk0 = 0;                // tiled kernel covers chunks >= this (set by the row-image launcher for its tail)
    int cv_tyq = 0;                   // 0 = pick the tile height per shape; else dfe_set_cost_volume_tile's code (tuning / tests)
    int ncu = 256;                    // compute units of the device
    const char *last_kernel = "";
    const char *ms_prep = "", *ms_cascade = "";   // the pyramid matcher's last preparation / cascade kernel (dfe_multiscale_last_path)
    const char *ms_census = "";       // ... and its census volume kernel ("" where the last run scored by SSD)
    char ms_path[96] = "";
    DfeBuf scratch;                   // grow-only device arena (never shrinks; freed with the ctx), physically contiguous where the driver grants it
    DfeBuf scratch_plain;             // the arena of the paths that run learned filter stacks: a plain hipMalloc (dfe_scratch's `plain`)
    size_t scratch_limit = (size_t)16 << 30;   // cost-volume bands are sized to fit (dfe_set_scratch_limit)
    DfeBuf ingest;                    // fp32 copy of a uint8 frame pair (ingest.hip)
    // pipelined ingest (ingest.hip): a copy stream of the ctx's own and DFE_NSLOT device slots for frame pairs -- the upload (+ conversion)
    // of pair i+1 runs beside the step of pair i; copied[s] / consumed[s] order the two streams per slot
    hipStream_t copy_stream = nullptr;
    DfeBuf slot[DFE_NSLOT];           // two uint8 frames each
    size_t slot_bytes = 0;            // bytes of ONE frame of a slot
    hipEvent_t copied[DFE_NSLOT] = {}, consumed[DFE_NSLOT] = {};
    bool slot_used[DFE_NSLOT] = {};
    int slot_next = 0;
    DfeBuf aux;                       // side buffer for small per-call planes (the matrix-core matcher's norms): NOT the arena, whose carved
                                      // pointers a nested launcher must not invalidate
    // nn.SpatialContrastiveNormalization's border-correction plane (the estimator of a tensor of ones): a function of the frame size, the
    // plane count and the kernel only -- kept from call to call (filters.hip)
    DfeBuf cn_coef;
    int cn_key[4] = {0, 0, 0, 0};     // H, W, C, k of the plane that is there (k = 0: none)
    float cn_key_kn[33] = {};
    int *dflag = nullptr;             // one device int for error flags raised by kernels
    DfeBuf i8_verdict;                // three device words taken in turn: word (i8_seq % 3) != 0 = the frames of int8 flow step i8_seq were NOT byte-valued
                                      // (ssd_flow_i8.hip; a step's pack kernel clears the next step's word, so no launch resets them); the ctx's
                                      // own, so that dfe_flow_last_path can read it whatever has carved the arena since
    unsigned i8_seq = 0;              // number of the last int8 flow step
    int i8_slots = 0;                 // waves of the int8 sweep that the device holds at once (0: not asked yet)
    int flow_gated_lds = 0;           // dynamic LDS that the gated float sweep has been allowed on this ctx (set when a step needs more)
    bool i8_last = false;            // the last flow step launched the int8 kernel (and the gated float sweep behind it)
    char err[512] = {0};
    // optional per-launch timing of the cost-volume kernel (dfe_profile_enable)
    bool profile = false;
    int prof_depth = 0;               // only the outermost DfeProfScope records (a launcher may nest another)
    std::vector<hipEvent_t> prof_events;   // start/stop pairs, resolved by dfe_profile_read
    // launch-bound one-call pipelines (the multiscale matcher: 4-6 launches of 9-33 us) can be replayed as a hipGraph when
    // they are called again with the same arguments (same buffers, same shapes): the second such call captures, later ones
    // replay.  OFF unless DFE_GRAPHS=1 is in the environment when the ctx is created: on ROCm 7.2 / MI355X the replay
    // measured SLOWER than the direct launches (VGA 3-level pyramid 0.0857 against 0.0803 ms per pair, 1080p 0.543 against
    // 0.537 ms: the graph launch costs more than four back-to-back kernel launches on one stream).  Profiling and the
    // legacy null stream (not capturable) also turn it off.
    // stage timers with the reference's names (depth_estimation_opticalflow.lua:144-148: load / filter / match / extract): event
    // pairs per stage on the ctx stream, resolved by dfe_stage_timers_read
    bool stage_timers = false;
    int stage_depth = 0;                     // only the outermost DfeStageScope records
    struct StageEvent { int stage; hipEvent_t a, b; };
    std::vector<StageEvent> stage_events;
    struct GraphSlot {
        std::vector<unsigned char> key;
        int hits = 0;
        hipGraphExec_t exec = nullptr;
    };
    GraphSlot ms_graph;
    bool graphs = false;
};

// brackets the cost-volume kernel launch with events on the ctx stream when profiling is on
struct DfeProfScope {
    dfe_ctx *ctx;
    // attach mode (a scope around ONE launch): the pair of events rides on the kernel's own dispatch packet (hipExtLaunchKernelGGL(...,
    // prof.a, prof.b, 0, ...)) instead of being recorded on the stream in front of and behind it.  A recorded event is a barrier packet:
    // the two of them cost the VGA step 3.9 us (0.2472 against 0.2433 ms per step with and without the brackets) -- of a measurement
    // that bench.py has to make inside its timed region.  a == b == nullptr: not profiling (or nested), a plain launch.
    hipEvent_t a = nullptr, b = nullptr;
    bool attach;
    explicit DfeProfScope(dfe_ctx *c, bool attach_to_launch = false) : ctx(c), attach(attach_to_launch) {
        if (ctx->profile && ctx->prof_depth++ == 0) {
            hipEvent_t e;
            if (attach) {
                if (hipEventCreate(&a) != hipSuccess) a = nullptr;
                if (a && hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); a = b = nullptr; }
            } else if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, ctx->stream); ctx->prof_events.push_back(e); }
        }
    }
    ~DfeProfScope() {
        if (ctx->profile && --ctx->prof_depth == 0) {
            if (attach) {
                if (a && b) { ctx->prof_events.push_back(a); ctx->prof_events.push_back(b); }
            } else if (ctx->prof_events.size() & 1) {
                hipEvent_t e;
                if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, ctx->stream); ctx->prof_events.push_back(e); }
            }
        }
    }
    DfeProfScope(const DfeProfScope &) = delete;
    DfeProfScope &operator=(const DfeProfScope &) = delete;
};

// brackets the launches of one pipeline stage (DFE_STAGE_*) with events when the stage timers are on
struct DfeStageScope {
    static constexpr size_t kMaxStageEvents = 4096;   // event pairs kept until dfe_stage_timers_read collects them
    dfe_ctx *ctx;
    bool rec = false;
    dfe_ctx::StageEvent ev{};
    DfeStageScope(dfe_ctx *c, int stage) : ctx(c) {
        if (ctx->stage_timers && ctx->stage_depth++ == 0 && ctx->stage_events.size() < kMaxStageEvents) {   // (unread regions beyond the cap are dropped)
            ev.stage = stage;
            rec = hipEventCreate(&ev.a) == hipSuccess && hipEventCreate(&ev.b) == hipSuccess;
            if (rec) (void)hipEventRecord(ev.a, ctx->stream);
        }
    }
    ~DfeStageScope() {
        if (ctx->stage_timers) --ctx->stage_depth;
        if (rec) { (void)hipEventRecord(ev.b, ctx->stream); ctx->stage_events.push_back(ev); }
    }
    DfeStageScope(const DfeStageScope &) = delete;
    DfeStageScope &operator=(const DfeStageScope &) = delete;
};

int dfe_fail(dfe_ctx *ctx, int code, const char *fmt, ...);   // (dfe_ctx.hip)

#define DFE_HIP(ctx, expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return dfe_fail((ctx), DFE_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                        \
    } while (0)

#define DFE_REQUIRE(ctx, cond, code, ...)                    \
    do {                                                     \
        if (!(cond)) return dfe_fail((ctx), (code), __VA_ARGS__); \
    } while (0)

#define DFE_LAUNCH_CHECK(ctx) DFE_HIP(ctx, hipGetLastError())

// Every extern "C" entry point runs on ITS ctx's device whatever the caller's current device is (one ctx per GPU, several
// ctxs per host thread are legal: include/dfe.h), and leaves the caller's current device as it found it.
struct DfeDeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DfeDeviceGuard(const dfe_ctx *c) {
        if (c && hipGetDevice(&prev) == hipSuccess && prev != c->device) switched = hipSetDevice(c->device) == hipSuccess;
    }
    ~DfeDeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DfeDeviceGuard(const DfeDeviceGuard &) = delete;
    DfeDeviceGuard &operator=(const DfeDeviceGuard &) = delete;
};
// first statement of an entry point: NULL check + device guard for the rest of the call
#define DFE_ENTER(ctx)                                          \
    DFE_REQUIRE((ctx), (ctx), DFE_E_ARG, "ctx is NULL");        \
    DfeDeviceGuard dfe_device_guard_(ctx)

static inline int dfe_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// blocks of a grid-stride launch over n elements: ceil(n / per_block), at least 1, at most cap
static inline int dfe_grid1d(long long n, int per_block = 256, int cap = 256 * 32) {
    const long long b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}
// rows of the output volume that fit one scratch band (ctx->scratch_limit, 16 GiB by default:
// one launch per pair up to 1080p/33x33; 288 GB of HBM make the whole volume the natural unit)
static inline int band_rows(const dfe_ctx *ctx, int Ho, int Wo, int D, int elem = (int)sizeof(float)) {
    long long row_bytes = (long long)Wo * D * elem;
    long long band = (long long)ctx->scratch_limit / row_bytes;
    if (band < 1) band = 1;
    if (band > Ho) band = Ho;
    // balanced: the same number of bands, rows dealt evenly (band i = rows [i Ho / nb, (i+1) Ho / nb)), so that no short last
    // band is left over -- the fast kernels need at least a tile of rows, and the fp16 pipeline has no other kernel to fall back to
    const long long nb = (Ho + band - 1) / band;
    return (int)((Ho + nb - 1) / nb);
}
static inline int band_count(int Ho, int band) { return (Ho + band - 1) / band; }
// 0-based offset of the centre in a window side of n cells, ceil(n / 2) - 1: datap.lWin / tWin (version2/test.lua:18-21), and the first
// row / column that prepareInput's narrow(2, ceil(maxh / 2), ..) keeps of patch 1 (opticalflow_model.lua)
static inline int dfe_window_lead(int n) { return (n + 1) / 2 - 1; }
// 1-based class of the centre cell of an hWin x wWin window: getMiddleIndex = yx2x(centered2onebased(0, 0)) (opticalflow_model.lua:12-14,
// 28-43), yx2xMulti(0, 0) of the pyramid, the centre override of radial/radial_opticalflow_groundtruth.lua:91
static inline int dfe_window_middle(int hWin, int wWin) { return (wWin + 1) / 2 + wWin * dfe_window_lead(hWin); }
// window cells the census and the semi-global entries take at the most: the single-scale step's ceiling (class ids fit census.hip's 11-bit key)
constexpr int kDfeMaxWindowCells = 1096;
// o = a b and o = m^-1 (false: singular) of row-major 3 x 3 matrices on the host (egomotion.hip, egopose.hip)
static inline void dfe_mat3_mul(const double *a, const double *b, double *o) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}
static inline bool dfe_mat3_inv(const double *m, double *o) {
    const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (fabs(d) < 1e-300) return false;
    o[0] = (m[4] * m[8] - m[5] * m[7]) / d; o[1] = (m[2] * m[7] - m[1] * m[8]) / d; o[2] = (m[1] * m[5] - m[2] * m[4]) / d;
    o[3] = (m[5] * m[6] - m[3] * m[8]) / d; o[4] = (m[0] * m[8] - m[2] * m[6]) / d; o[5] = (m[2] * m[3] - m[0] * m[5]) / d;
    o[6] = (m[3] * m[7] - m[4] * m[6]) / d; o[7] = (m[1] * m[6] - m[0] * m[7]) / d; o[8] = (m[0] * m[4] - m[1] * m[3]) / d;
    return true;
}

// multiscale class-id geometry and decode, shared by postops.hip (x2yxMulti, on the host too) and multiscale.hip (fused cascade -> flow)
struct MultiGeom {
    int maxh, maxw, nratios;
    int ratios[DFE_MAX_RATIOS];
    int d[DFE_MAX_RATIOS];   // ring width per scale (index >= 1)
};

// (I = int on the device's per-block decode tables: a 64-bit divide costs ~100 instructions there)
template <class I> __host__ __device__ inline int multi_decode_t(const MultiGeom &g, I id, I *oy, I *ox) {
    // replaces: x2yxMultiNumber opticalflow_model_multiscale.lua:83-132
    const int maxh = g.maxh, maxw = g.maxw;
    const int chh = (maxh + 1) / 2, chw = (maxw + 1) / 2;
    I x = id;
    if (x < 1) return -1;
    if (x <= (I)maxh * maxw) {
        *oy = (x - 1) / maxw + 1 - chh;
        *ox = (x - 1) % maxw + 1 - chw;
        return 0;
    }
    x -= (I)maxh * maxw;
    for (int i = 1; i < g.nratios; ++i) {
        const int d = g.d[i];
        const I len = (I)2 * d * maxw + (I)2 * (maxh - 2 * d) * d;
        I ty, tx;
        if (x <= len) {
            if (x <= (I)d * maxw) {
                ty = (x - 1) / maxw + 1; tx = (x - 1) % maxw + 1;
            } else {
                x -= (I)d * maxw;
                if (x <= (I)(maxh - 2 * d) * d) {
                    ty = (x - 1) / d + 1 + d; tx = (x - 1) % d + 1;
                } else {
                    x -= (I)(maxh - 2 * d) * d;
                    if (x <= (I)(maxh - 2 * d) * d) {
                        ty = (x - 1) / d + 1 + d; tx = (x - 1) % d + 1 + maxw - d;
                    } else {
                        x -= (I)(maxh - 2 * d) * d;
                        if (x > (I)d * maxw) return -1;
                        ty = (x - 1) / maxw + 1 + maxh - d; tx = (x - 1) % maxw + 1;
                    }
                }
            }
            *oy = (ty - chh) * g.ratios[i];
            *ox = (tx - chw) * g.ratios[i];
            return 0;
        }
        x -= len;
    }
    return -1;
}

__host__ __device__ inline int multi_decode(const MultiGeom &g, long long id, long long *oy, long long *ox) {
    return multi_decode_t<long long>(g, id, oy, ox);
}

// ---- argument structs of the launchers below.  The kernel-argument layouts they take by reference or pointer are defined with the device
// code that reads them: CvFuseArgs, CvNovolArgs, TailOut and DfePairDepth in cv_records.h, CvFineArgs in cv_fine_epilogue.h ----
struct CvFuseArgs;
struct CvNovolArgs;
struct TailOut;
struct DfePairDepth;
struct CvFineArgs;
// the pyramid's sub-pixel refinement (multiscale_subpixel.hip): from the class map and every scale's padded frames to the refined flow
struct MsSubpixelArgs {
    const float *p0[DFE_MAX_RATIOS], *p1[DFE_MAX_RATIOS];   // padded scale frames [C][Hp][Wp] (frame 0, frame 1)
    int r[DFE_MAX_RATIOS], Hp[DFE_MAX_RATIOS], Wp[DFE_MAX_RATIOS];
    int base[DFE_MAX_RATIOS];   // 0-based class id of the scale's first class in the joined vector
    int d[DFE_MAX_RATIOS];      // ring width of scale s >= 1
    int nratios, ncls, C, H, W, k, maxh, maxw;
    const long long *idx;       // [H][W], 1-based class ids
    float *fy, *fx;             // [H][W] each, written where idx is a class id
};
// one description of a learned filter stack (filters.hip), the one rule of every entry that takes dfe_filter_layer[]: every layer complete
// (DFE_E_ARG); layer 0 reads the frames' C planes, a full layer the planes of the layer before it, a connection-table layer at most those
// (DFE_E_SHAPE).  nlayers == 0: {1, 1, C, C}
struct DfeStackGeom { int hk, wk, K, maxplanes; };   // receptive field, planes of the last layer, the widest layer (>= C)

// ---- the cross-file launchers, by the file that defines them ----
// kept out of libdfe.so's dynamic symbol table, which is the C ABI's: every cross-file function added from now on (the older ones are
// still exported under their mangled names)
#define DFE_HIDDEN __attribute__((visibility("hidden")))

// dfe_ctx.hip
// key = the bytes of a POD describing the call; returns 0 = launch directly, 1 = capture this call, 2 = replay slot.exec
int dfe_graph_lookup(dfe_ctx *ctx, dfe_ctx::GraphSlot &slot, const void *key, size_t bytes);
// ends a capture begun after dfe_graph_lookup returned 1 (rc = the launcher's result), instantiates and launches the graph
int dfe_graph_finish(dfe_ctx *ctx, dfe_ctx::GraphSlot &slot, int rc);
// arena of at least `bytes`.  plain = false: physically contiguous memory if the driver has it (the volume sweeps' arena); plain = true: a
// plain hipMalloc, for the paths whose convolutions write many feature planes side by side (see dfe_scratch in dfe_ctx.hip for both measurements)
int dfe_scratch(dfe_ctx *ctx, size_t bytes, void **out, bool plain = false);
int dfe_aux_scratch(dfe_ctx *ctx, size_t bytes, void **out);   // the ctx's side buffer, grown to at least `bytes`
// grows `b` to at least `bytes`: no-op when it is large enough; else drains ctx->stream (and the copy stream with
// DFE_GROW_COPY_STREAM), releases the old block (hipFree; a physically contiguous one goes idle in the process's pool instead,
// dfe_contig_pool.h), allocates (with DFE_GROW_CONTIG and option arena_contig: an idle contiguous block of the pool that holds `bytes`,
// else a new contiguous one, else hipMalloc; b.bytes is the block's size, which may exceed `bytes`).  On failure `b` is empty, HIP's last
// error is cleared and DFE_E_ALLOC names the buffer
enum { DFE_GROW_CONTIG = 1, DFE_GROW_COPY_STREAM = 2 };
int dfe_grow(dfe_ctx *ctx, DfeBuf &b, size_t bytes, const char *name, int flags = 0, bool *contig_out = nullptr);
// A launcher's layout `lay` (a function over a DfeCarve & that takes its buffers in order, dfe_carve.h) run for the size, the arena grown
// to it, and `lay` run again on the arena
template <class L> int dfe_scratch_carve(dfe_ctx *ctx, L &&lay, bool plain = false) {
    DfeCarve plan;
    lay(plan);
    void *scr = nullptr;
    int rc = dfe_scratch(ctx, plan.off, &scr, plain);
    if (rc) return rc;
    DfeCarve c(scr);
    lay(c);
    return DFE_OK;
}

// rows and columns that the volume-free flow step (k = 7, 33 x 33: the float sweep, its gated copy, the int8 sweep) takes off a frame
constexpr int DFE_FLOW_MARGIN = 7 - 1 + 33 - 1;

// ssd_flow_i8.hip -- the int8 flow step's kernels and its host state (the ctx's verdict ring); flow_step.hip carves the buffers and calls
// device buffers of the int8 flow step: packed frames and patch-sum planes (carved by the caller), this call's verdict word and the next one's
struct DfeFlowI8Bufs {
    unsigned *pk0, *pk1, *verdict, *verdict_next;
    int *s0, *s1k;
    size_t px;            // elements of each of pk0, pk1, s0, s1k
    int Wp, nstrips;
    void take(DfeCarve &c) {
        pk0 = c.take<unsigned>(px);
        pk1 = c.take<unsigned>(px);
        s0 = c.take<int>(px);
        s1k = c.take<int>(px);
    }
};
// the sizes for an H x W frame (k = 7, 33 x 33) into *b; 0 = the kernel does not take this shape
size_t dfe_flow_i8_plan(int H, int W, DfeFlowI8Bufs *b);
// one more int8 step on this ctx: the verdict ring (ctx->i8_verdict, allocated and cleared at first use) turns, b->verdict / verdict_next
// are this step's word and the next one's
DFE_HIDDEN int dfe_flow_i8_turn(dfe_ctx *ctx, DfeFlowI8Bufs *b);
// pack + patch sums + the int8 sweep, whose waves finish their own pixels into `out` (pd: frame mode, the interior of the pair's planes)
// IF the frames are byte-valued (else nothing: *b.verdict says so to the gated float sweep that the caller launches behind it,
// cv_flow_sweep_gated).  out: one band, the whole pair.  Sets ctx->i8_last
int dfe_flow_i8_launch(dfe_ctx *ctx, const float *I0, const float *I1, int H, int W, const DfeFlowI8Bufs &b, const CvNovolArgs &nv, const TailOut &out,
                       const DfePairDepth *pd);
// the same on frames of bytes (the byte entries at scale 1): the pack kernel reads the bytes as they are, raises no verdict and writes the
// frame's border (pd: required), so these two launches are the whole step
int dfe_flow_i8_launch_bytes(dfe_ctx *ctx, const unsigned char *I0, const unsigned char *I1, int H, int W, const DfeFlowI8Bufs &b, const CvNovolArgs &nv,
                             const TailOut &out, const DfePairDepth *pd);
// flow_step.hip -- dfe_flow_depth_pair_f32 on frames of bytes without the float copy, where the step may take int8 (*done; else nothing
// has been launched and the caller converts and goes the float way)
int dfe_flow_depth_pair_bytes(dfe_ctx *ctx, const unsigned char *I0, const unsigned char *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                              float foe_y, double extract_threshold, float scale, float *flow, float *scores, float *depth, float *depth_conf, bool *done);

// ssd_cost_volume.hip -- the raw-frame cost-volume kernels, their planners and launchers; the host pipeline of the flow step that
// calls them is flow_step.hip
// cost volume of raw frames into `out`; H = rows visible to this call, plane = channel stride
int cv_frames_dispatch(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, long long plane, int kh,
                       int kw, int hWin, int wWin, float *out);
// the fp16 volume (cost * scale) of raw frames, with the fused epilogue's results beside it when fa != NULL; *handled = false: no fast kernel
int cv_frames_dispatch_f16(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, long long plane, int k, int hWin, int wWin,
                           float scale, void *out, const CvFuseArgs *fa, bool *handled, bool *recs);
// the fused builds of this shape leave per-pixel RECORDS (fa.rec) instead of the three planes
DFE_HIDDEN bool cv_writes_records(int C, int hWin, int wWin);
// The volume-free flow sweep (3 channels, k = 7, 33 x 33): records into fa.rec, the fallback plane into nv.fb, no volume.
// cv_flow_sweep: the plain sweep; the caller finalizes its records (dfe_flow_finalize).  *handled = false: no launch.
// cv_flow_sweep_gated_ok: the gated form takes an H x W frame (a caller asks before it launches the int8 kernel in front of it).
// cv_flow_sweep_gated: the ONE launch behind the int8 kernel -- the frame's border (pd: frame mode) whatever *verdict says, and, unless
// *verdict == 0, the sweep and the finalize of its records into `out`, each block its own
DFE_HIDDEN bool cv_flow_sweep_gated_ok(const dfe_ctx *ctx, int H, int W);
DFE_HIDDEN int cv_flow_sweep(dfe_ctx *ctx, const float *I0, const float *I1, int H, int W, const CvFuseArgs &fa, const CvNovolArgs &nv, bool *handled);
DFE_HIDDEN int cv_flow_sweep_gated(dfe_ctx *ctx, const float *I0, const float *I1, int H, int W, const CvFuseArgs &fa, const CvNovolArgs &nv,
                                   const unsigned *verdict, double threshold, const TailOut &out, const DfePairDepth *pd);
// the volumes of n independent pairs (pyramid scales) in one launch where a common block shape exists (*handled)
// prob (may be NULL): per pair, non-null = leave soft-min probabilities there instead of the costs in out[i] -- if the
// launcher finds that worthwhile for the shape (*prob_used)
int cv_frames_dispatch_multi(dfe_ctx *ctx, int n, const float *const *I0, const float *const *I1, int C, const int *H, const int *W, int k,
                             int hWin, int wWin, float *const *out, float *const *prob, bool *handled, bool *prob_used, float f16_scale = 0.f, int nq_hint = 0);
// the volume with the fused epilogue's per-pixel results (CvFuseArgs) beside it
int cv_frames_dispatch_fused(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, long long plane, int k, int hWin,
                             int wWin, float *out, const CvFuseArgs &fa, bool *handled, int *nparts, bool *recs = nullptr);
// the finest scale of the multiscale matcher WITHOUT its volume (CvFineArgs, cv_fine_epilogue.h)
int cv_frames_finest_fused(dfe_ctx *ctx, const float *I0p, const float *I1p, int C, int Hp, int Wp, int k, int maxh, int maxw, const CvFineArgs &fine,
                           bool *handled);
bool cv_finest_plan_ok(dfe_ctx *ctx, int Hp, int Wp, int maxh, int maxw);   // cv_frames_finest_fused (with a parent scale) would take this frame
int dfe_fm_launch_ref(dfe_ctx *ctx, const FmJob &j);   // the reference-order kernel on feature maps (FM_K_REF)

// postops.hip
// Finishes `rows` rows of a fused build from what it left in fa: the tile-row records (recs; part / centre / lead are ignored then) or the
// three planes with nchunks entries per pixel.  vol: the band's volume, for the rare pixels that walk on through it; nv: the volume-free
// sweep's fallback plane (records only, no vol), or NULL.  `out` says where the results go, row_off / p_off set to the band's;
// pd != NULL is frame mode (one band only): the launch also zeroes the frame border and makes depth / confidence
int dfe_flow_finalize(dfe_ctx *ctx, const CvFuseArgs &fa, bool recs, int nchunks, const float *vol, const CvNovolArgs *nv, double threshold, int rows,
                      int hWin, int wWin, const TailOut &out, const DfePairDepth *pd = nullptr);
// the full pass over a band's volume (the public dfe_flow_tail behind its argument checks)
int dfe_flow_tail_run(dfe_ctx *ctx, const float *vol, int rows, int hWin, int wWin, double threshold, const TailOut &out);
int dfe_pair_border_depth(dfe_ctx *ctx, float *flow, float *scores, int H, int W, int pad_t, int pad_l, int Ho, int Wo, float cx,
                          float cy, float *depth, float *conf);

// consistency.hip
// the pair step forwards (subpixel != 0: its refined form), the backward flow (flow_bw, or the ctx's side buffer when NULL) and the
// consistency kernel behind them: dfe_flow_depth_pair_fb_f32 behind its device guard, and _fb_u8 on the frames it has converted once
int dfe_flow_pair_fb_run(dfe_ctx *ctx, const char *fn, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin, float foe_x,
                         float foe_y, double extract_threshold, int subpixel, float tol, int gate, float *flow, float *scores, float *depth,
                         float *depth_conf, float *flow_bw, float *mask, float *err);

// feat_matching_dispatch.hip -- nn.SpatialMatching on feature maps.  The one rule: a kernel is chosen by fm_select (fm_select.h); a launcher
// (dfe_fm_launch_*, one per kernel family, geometry from the FmPick) never declines
static inline FmEnv dfe_fm_env(const dfe_ctx *c) {
    return FmEnv{c->cv_mode, c->opt[DFE_OPT_FM_FLAT], c->opt[DFE_OPT_FM64], c->opt[DFE_OPT_FM_ROWS], c->opt[DFE_OPT_FM_MFMA], c->opt[DFE_OPT_FM_SPLIT]};
}
// fm_select on the job, then the pick's launch.  FM_K_NONE launches nothing: with `picked` the caller sees it there (and goes through a
// contiguous copy or the volume), without it the call fails
int dfe_fm_run(dfe_ctx *ctx, const FmJob &j, FmPick *picked = nullptr);
// the volume of contiguous maps behind dfe_spatial_matching_f32's argument checks
int dfe_spatial_matching_dispatch(dfe_ctx *ctx, const float *in1, const float *in2, int K, int H1, int W1, int maxh, int maxw, float *out);

// feat_matching.hip, feat_matching_flat.hip, feat_matching_mfma.hip
int dfe_fm_launch_win64(dfe_ctx *ctx, const FmJob &j, const FmPick &pk);
int dfe_fm_launch_rows(dfe_ctx *ctx, const FmJob &j, const FmPick &pk);
int dfe_fm_launch_chunk(dfe_ctx *ctx, const FmJob &j, const FmPick &pk);
int dfe_fm_launch_flat(dfe_ctx *ctx, const FmJob &j, const FmPick &pk);
int dfe_fm_launch_mfma(dfe_ctx *ctx, const FmJob &j, const FmPick &pk);
// the one-chunk matcher on n pairs (pyramid scales) in one launch, or on one pair through the fused pyramid epilogue (fine)
bool dfe_feat_matching_win64_ok(const dfe_ctx *ctx, int K, int maxh, int maxw);   // the ctx / window conditions of the launcher below
int dfe_feat_matching_win64_batch(dfe_ctx *ctx, int n, const float *const *in1, const float *const *in2, int K, const int *H1, const int *W1, int maxh,
                                  int maxw, float *const *out, float f16_scale, bool *handled, const CvFineArgs *fine = nullptr);

// filters.hip
int dfe_filter_stack_geom(dfe_ctx *ctx, const char *entry, const dfe_filter_layer *layers, int nlayers, int C, DfeStackGeom *g);
// one layer of a filter stack: in [nIn][H][W] -> out [nOut][H-kH+1][W-kW+1], nn.Tanh fused behind it when
// L.tanh_after (the same tanhf as dfe_tanh_f32: bit-identical to the two separate calls)
int dfe_filter_layer_forward(dfe_ctx *ctx, const float *in, const dfe_filter_layer &L, int H, int W, float *out);
// the same layer position of n independent inputs (both frames of every pyramid scale) in ONE launch where a batched kernel exists
int dfe_filter_layer_forward_batch(dfe_ctx *ctx, int n, const float *const *in, const dfe_filter_layer *const *L, const int *H, const int *W,
                                   float *const *out);
int dfe_filter_layer_forward_batch_view(dfe_ctx *ctx, int n, const float *const *in, const dfe_filter_layer *const *L, const int *H, const int *W, const int *in_pitch,
                                        const long long *in_plane, float *const *out, bool *done);
// nn.SpatialContrastiveNormalization with caller-provided scratch ((C + 3) * H * W floats): for the one-call pipelines
int dfe_contrastive_normalization_run(dfe_ctx *ctx, const float *in, int C, int H, int W, const float *kernel_host, int k, float threshold,
                                      float thresval, float *scratch, float *out);
// ... of two frames of one size in the same two launches; out0 only the crop window cw x ch at (cx, cy) when cw > 0 (scratch: 4 * H * W floats)
int dfe_contrastive_normalization_run2(dfe_ctx *ctx, const float *in0, const float *in1, int C, int H, int W, const float *kernel_host, int k,
                                       float threshold, float thresval, float *scratch, float *out0, float *out1, int cx, int cy, int cw, int ch);

// conv_mfma.hip
// a filter layer of up to two inputs (views allowed) as an implicit GEMM on the matrix cores, weights resident in LDS:
// fused multiply-adds in the reference's (input plane, ky, kx) order -- results differ from the exact kernels by that fusing only
// nrm[e] (or NULL): the kernel also leaves the per-pixel squared norm of its output over the planes there ([Ho][Wo])
int dfe_conv_mfma_res_batch(dfe_ctx *ctx, int n, const float *const *in, const int *H, const int *W, const int *in_pitch, const long long *in_plane,
                            const dfe_filter_layer &L, float *const *out, bool *handled, float *const *nrm = nullptr);

// sgm.hip -- semi-global aggregation of a [H][W][D] volume
// dfe_sgm_aggregate_f32's checks of the sizes and parameters (fn: the entry's name for the message)
DFE_HIDDEN int dfe_sgm_check(dfe_ctx *ctx, const char *fn, int H, int W, int D, float P1, float P2, unsigned paths, int ring);
// ... and its launches behind them, for a caller that has carved the arena itself.  work: dfe_sgm_work_planes(paths, agg != NULL) planes of
// H * W * D floats (one per direction; none when the only direction goes straight to agg); agg [H][W][D] or NULL; flow [H][W] or NULL
DFE_HIDDEN size_t dfe_sgm_work_planes(unsigned paths, bool agg_given);
struct SgmPen;   // (sgm_common.h: the penalty planes of a guided call; NULL: one P2 for the whole frame)
DFE_HIDDEN int dfe_sgm_run(dfe_ctx *ctx, const float *volume, int H, int W, int D, float P1, float P2, unsigned paths, int ring, float *work, float *agg,
                           float *flow, const SgmPen *pen = nullptr);

// radial_pipeline.hip -- the stages around the matcher that the radial one calls and the census radial one call (census_radial.hip) share
// the warp's buffers: two polar frames [C][H][Wp], the radius table (H floats), the angle's sine and cosine (W doubles each), and the
// channel-interleaved copies of the frames (hImg * wImg float4 each; i0 == NULL: the planar taps)
struct DfeRadialWarpBufs { float *pol0, *pol1, *rt; double *sn, *cs; float4 *i0, *i1; };
DFE_HIDDEN double dfe_radial_rmax(double h, double w, double ex, double ey);   // getRMax
DFE_HIDDEN int dfe_radial_warp_pair(dfe_ctx *ctx, const float *prev, const float *cur, int C, int hImg, int wImg, int H, int W, int lpad, int Wp,
                                    float alpha_polar, double e2x, double e2y, double rmax, const DfeRadialWarpBufs &b);
// the P2C sample of the polar flow [hm][W] and flow2depth; kH2 = hKernel of getP2CMaskOF / getKOutput
DFE_HIDDEN int dfe_radial_p2c_depth(dfe_ctx *ctx, const float *pflow, int hImg, int wImg, int H, int W, int hm, int kH2, int hWin, float alpha_polar,
                                    double kinfty, double e2x, double e2y, double rmax, int hOut, int wOut, float *cart_flow, float *depth, float *conf);
// dfe_radial_refine_subpixel_f32's launch behind its checks (fout may be fin)
DFE_HIDDEN int dfe_radial_refine_run(dfe_ctx *ctx, const float *vol, const float *fin, long long P, int hWin, float *fout);

// census.hip -- the front end of every census one call (census.hip's own, and the two that aggregate in sgm_pick.hip)
struct DfeCensusPair { int Hp, Wp, Ha, Wa, pad_t, pad_l; };   // patch positions, the aggregated cost's region, where it is pasted
// the one call's checks in their order -- tensors / depth_pair: what the entry found of its pointers -- and the geometry behind them
DFE_HIDDEN int dfe_census_pair_check(dfe_ctx *ctx, const char *fn, bool tensors, bool depth_pair, int C, int H, int W, int k, int hWin, int wWin, int agg,
                                     DfeCensusPair *g);
// the two transforms under DFE_STAGE_FILTER: float frames, or bytes, into sig0 and sig1 ([C][Hp][Wp] each)
DFE_HIDDEN int dfe_census_pair_transforms(dfe_ctx *ctx, const void *I0, const void *I1, bool bytes, int C, int H, int W, int k, uint64_t *sig0, uint64_t *sig1);

// multiscale.hip, multiscale_subpixel.hip
// the raw-patch pyramid on uint8 frames, converted inside its preparation kernels (f16_scale 0 = fp32 volumes)
// subpixel: the sub-pixel refinement behind the matcher (dfe_multiscale_flow_pair_subpixel_u8)
int dfe_multiscale_flow_pair_bytes(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int maxh, int maxw,
                                   const int *ratios, int nratios, float u8_scale, float f16_scale, float *flow, int64_t *idx, bool subpixel = false);
int dfe_multiscale_subpixel_launch(dfe_ctx *ctx, const MsSubpixelArgs &a);
// one scale's two frames, staged: box down-sample by r into d (2 * C * H/r * W/r floats; untouched for r = 1), zero-pad into p (2 * C * Hp * Wp)
DFE_HIDDEN int dfe_pyramid_prep_scale(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int r, int pl, int pt, int Hp, int Wp, float *d,
                                      float *p);
// the one-call pyramid matcher in its census mode (dfe_multiscale_census_flow_pair_*); bytes: I0 / I1 are uint8 frames, taken as float(byte)
// refine: the vee fit on the raw census cost behind the matcher (census_subpixel.hip; flow required)
DFE_HIDDEN int dfe_multiscale_census_pair(dfe_ctx *ctx, const void *I0, const void *I1, bool bytes, int C, int H, int W, int k, int maxh, int maxw,
                                          const int *ratios, int nratios, int agg, float beta, float *flow, int64_t *idx, const char *entry,
                                          bool refine = false);

// census_pyramid.hip -- the census cost of the pyramid's scales, from the padded scale frames that ms_prep_raw leaves to the volumes the
// cascade stages read
struct DfeCensusPyramid {
    int ns, C, k, maxh, maxw, agg;
    float beta;
    const float *p0[DFE_MAX_RATIOS], *p1[DFE_MAX_RATIOS];   // padded scale frames [C][Hp][Wp]
    int Hp[DFE_MAX_RATIOS], Wp[DFE_MAX_RATIOS];
    uint64_t *sig0[DFE_MAX_RATIOS], *sig1[DFE_MAX_RATIOS];  // signature planes [C][Hp - k + 1][Wp - k + 1]
    float *cost[DFE_MAX_RATIOS];                            // volumes [Hs][Ws][maxh][maxw]
};
// k, C, agg and beta of every census pyramid entry (DFE_E_ARG)
DFE_HIDDEN int dfe_census_pyramid_check(dfe_ctx *ctx, const char *fn, int C, int k, int agg, float beta);
DFE_HIDDEN bool dfe_census_pyramid_fast(int maxh, int maxw);   // the window has the one-launch volume kernel
DFE_HIDDEN int dfe_census_pyramid_signatures(dfe_ctx *ctx, const DfeCensusPyramid &a);   // every scale, both frames, one launch
// every scale's volume: one launch where dfe_census_pyramid_fast, else the staged kernels scale by scale; names the route in ctx->ms_census
DFE_HIDDEN int dfe_census_pyramid_volumes(dfe_ctx *ctx, const DfeCensusPyramid &a);

// census_subpixel.hip -- the census pyramid's sub-pixel refinement: from the class map and every scale's signature planes to the refined flow
struct DfeCenfitPyramid {
    const uint64_t *s0[DFE_MAX_RATIOS], *s1[DFE_MAX_RATIOS];   // signature planes [C][Hg][Wg] (frame 0, frame 1)
    int r[DFE_MAX_RATIOS], Hg[DFE_MAX_RATIOS], Wg[DFE_MAX_RATIOS];
    int base[DFE_MAX_RATIOS];   // 0-based class id of the scale's first class in the joined vector
    int d[DFE_MAX_RATIOS];      // ring width of scale s >= 1
    int nratios, ncls, C, H, W, maxh, maxw, agg;
    const long long *idx;       // [H][W], 1-based class ids
    float *fy, *fx;             // [H][W] each, written where idx is a class id
};
DFE_HIDDEN int dfe_census_pyramid_subpixel_launch(dfe_ctx *ctx, const DfeCenfitPyramid &a);
