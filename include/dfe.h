/*
 * dfe.h -- C ABI of libdfe.so: the MI355X (gfx950) implementation of the dense
 * patch-correlation flow->depth hot path of MichaelMathieu/depth-estimation.
 *
 * This is the drop-in boundary.  Each entry point replaces one operator the
 * reference reaches through Torch7's nn.Module protocol or through its two
 * native Lua C modules; the replaced reference interface is cited as
 * "replaces: file:line" (paths relative to the reference repository).  A
 * LuaJIT-FFI caller binds exactly these prototypes.
 *
 * Conventions
 *  - plain C types only; every tensor is a dense row-major buffer, sizes in elements;
 *  - all tensor pointers are DEVICE pointers (hipMalloc / dfe_malloc / any allocator of the
 *    same HIP runtime, e.g. torch).  dfe_memcpy_* stage host data for callers without one;
 *  - the caller allocates inputs AND outputs (the reference's ops also write into
 *    caller-allocated tensors, extract_output.cpp:63-81); the library owns only ctx scratch;
 *  - class ids are 1-based int64 exactly as the reference's LongTensors;
 *  - every function returns DFE_OK or a negative DFE_E_*; dfe_last_error(ctx) gives the text
 *    (the Lua skin turns that into error(), matching CascadingAddTable.lua:111,115,123);
 *  - work is enqueued on the ctx's HIP stream and NOT synchronised unless stated;
 *  - a ctx is single-threaded; use one ctx per GPU / host thread;
 *  - there is no CPU fallback: without a gfx950 device dfe_ctx_create fails with DFE_E_HIP.
 */
#ifndef DFE_H
#define DFE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DFE_OK 0
#define DFE_E_ARG (-1)
#define DFE_E_SHAPE (-2)
#define DFE_E_ALLOC (-3)
#define DFE_E_HIP (-4)
#define DFE_E_UNSUPPORTED (-5)

#define DFE_MAX_RATIOS 10 /* x2yxMulti2.c:1 N_MAX_RATIOS */

typedef struct dfe_ctx dfe_ctx;

/* ---- context, memory --------------------------------------------------- */
int dfe_version(void);
/* revision tag of the cost-volume kernels (profiles/traffic_*.json records the one its HBM counters were measured with) */
const char *dfe_kernel_revision(void);
/* own_stream != 0: the ctx creates (and owns) a private non-blocking stream, `stream` is ignored;
 * own_stream == 0: work is enqueued on the caller's hipStream_t `stream` (NULL = the HIP default
 * stream, which is what torch's default stream is) so it is ordered with the caller's other work */
int dfe_ctx_create(int device, void *stream, int own_stream, dfe_ctx **out);
void dfe_ctx_destroy(dfe_ctx *ctx);
const char *dfe_last_error(const dfe_ctx *ctx); /* ctx may be NULL: last creation error */
int dfe_ctx_synchronize(dfe_ctx *ctx);
void *dfe_ctx_stream(dfe_ctx *ctx);
int dfe_malloc(dfe_ctx *ctx, size_t bytes, void **dptr);
int dfe_free(dfe_ctx *ctx, void *dptr);
int dfe_memcpy_h2d(dfe_ctx *ctx, void *dst, const void *src, size_t bytes); /* synchronous */
int dfe_memcpy_d2h(dfe_ctx *ctx, void *dst, const void *src, size_t bytes); /* synchronous */
/* Pins a host range the caller keeps passing to dfe_memcpy_h2d / _d2h (the storage of a Torch tensor that is reused from
 * frame to frame): copies from / to it then run as direct DMA instead of through the runtime's pageable staging.
 * Registering a range twice, or unregistering an unknown one, is not an error.  Unregister before the memory is freed. */
int dfe_host_register(dfe_ctx *ctx, void *ptr, size_t bytes);
int dfe_host_unregister(dfe_ctx *ctx, void *ptr);
/* Library-owned pinned host memory (hipHostMalloc): the bounce buffer a binding stages its tensors through, so that it never
 * has to pin memory it does not own (garbage-collected temporaries, storage that is resized or freed behind its back). */
int dfe_host_alloc(dfe_ctx *ctx, size_t bytes, void **hptr);
int dfe_host_free(dfe_ctx *ctx, void *hptr);
/* cost-volume kernel selection (tuning / tests; also the DFE_CV_MODE environment variable at context creation):
 * 0 = auto (default: the row-image kernel where it applies -- C=3, 7x7 patch, 769..1096 window cells, e.g. 33x33 --
 * else the tiled kernel, else the reference-order kernel), 1 = force the reference-order kernel (bit-identical float
 * summation order to the CPU path), 2 = force the tiled kernel, 3 = force the row-image kernel
 * (2/3: DFE_E_UNSUPPORTED from the op when the shape has no such kernel) */
int dfe_set_cost_volume_kernel(dfe_ctx *ctx, int mode);
/* tile height of the tiled / row-image kernels: 0 = chosen per shape (default); 2..7 = force NQ (a tile sweeps
 * NQ groups of 6 image rows at k = 7: 6 NQ - 6 output rows); 100 + ty (101..164) = row-image tiles of ty output
 * rows (ty a multiple of 6 at k = 7); 1 = force the row-image kernel's column sweep (unfused build only).  For tuning and for testing.
 * The row-image kernel takes every code.  The tiled kernels (the single-scale one, its fused build and the pyramid's merged volume
 * launch) are built for NQ = 2..5 only: there 6, 7, 1 and 100 + ty mean 0, the launcher's own choice.  A forced height that does not
 * fit the frame makes the tiled launcher decline: the next kernel in line builds the volume, the same values (with kernel mode 2,
 * which leaves no other kernel, the op returns DFE_E_UNSUPPORTED). */
int dfe_set_cost_volume_tile(dfe_ctx *ctx, int tyq);
/* Behaviour switches of the launchers (tuning and tests; none is needed for correct results -- every choice has a parity test or is
 * a pure scheduling choice).  value >= 0 forces, -1 restores the launcher's own choice per shape.  Keys: "cascade_px", "fine_fuse",
 * "mid_fuse", "fine_nq", "mid_nq", "prep_tiles", "xpose", "xpose_nt", "soft_epilogue", "conv_batch", "conv_nt10", "fm64", "fm_rows",
 * "sweep_ovh", "sweep_blocks", "debug_arena", "fm_flat", "fm_split", "conv_narrow", "conv_mfma", "fm_mfma", "arena_contig", "graphs", "cv_novol", "conv_nt", "cv_i8", "i8_slots", "fill_apex", "splat_lds".  The library reads the environment ONCE, in dfe_ctx_create
 * (DFE_<KEY> variables of the tuning scripts) -- never inside an op, so an op's behaviour depends on its ctx only.
 * Two keys trade the exact arithmetic for the matrix cores, both OFF unless set to 1: "conv_mfma" (the one-call models' filter layers as
 * implicit GEMMs, v_mfma_f32_16x16x4_f32: the reference's (input plane, ky, kx) order with FUSED multiply-adds, <= 1e-5 relative to
 * sum |terms|) and "fm_mfma" (nn.SpatialMatching as a banded GEMM, |a|^2 + |b|^2 - 2 a.b: each cost within 4 u (K + 2) (|a|^2 + |b|^2)
 * of the exact sum of squared differences, u = 2^-24 -- an error ABSOLUTE in the squared norms of the two feature vectors, not relative
 * to the cost, so features with a common offset lose the small costs' digits; arg-min indices equal except where the two best costs lie
 * within twice that band; maps of K (H1 + maxh - 1) (W1 + maxw - 1) >= 2^30 floats take the exact kernels).
 * replaces: the option tables the reference's drivers pass down (opticalflow.lua:138-198 `geometry`), for the switches that have no
 * counterpart there.  "cv_novol" (default 1): the single-scale flow step (dfe_ssd_flow_f32, dfe_flow_depth_pair_f32) of 3-channel frames,
 * 7 x 7 patch, 33 x 33 window builds no cost volume -- one launch whatever the frame size, bit-identical outputs; 0 materialises the
 * volume in ctx scratch (bands of dfe_set_scratch_limit) and the finalize reads it.  "conv_nt" (tests): n > 0 makes the batched convolution
 * give a thread n output planes in every layer whose plane count n divides and whose kernel width is built with n; other layers keep the
 * automatic choice.  "cv_i8" (default 1; only where "cv_novol" applies): the volume-free step packs both float frames to bytes on the
 * device, checking every value; frames that hold nothing but integers in 0..255 are matched by an int8 matrix-core kernel (exact integer
 * arithmetic: the float sweep's bits), any other frame by the float sweep, decided on the device without a host round trip
 * (dfe_flow_last_path tells which); 0 runs the float sweep alone.  "i8_slots" (tests): the number of waves that the int8
 * kernel's split of the rows into two-row and one-row wave items takes the device to hold at once (automatic: compute units x resident
 * blocks x 4, from the device); a pure scheduling choice.  "fill_apex" (dfe_fill_holes_f32): automatic = the upper pyramid levels, from
 * the first one whose levels up to the top fit the 160 KB of LDS, run in one workgroup's single launch; 0 = a launch per level and
 * direction only; n > 0 (tests) = the apex takes over at the first level of at most n cells (that also fits).  The same bits either way.
 * "splat_lds" (dfe_forward_splat_f32, dfe_temporal_step_splat_f32): 1 = the front and the accumulate pass combine the taps of a
 * workgroup's 8 x 64 sources that land in a 14 x 70 window around where the tile's centre goes in LDS and send every touched cell to
 * global memory once; 0 = every tap straight to global memory; automatic = 1, the faster one at the VGA and the 1080p step's region
 * (DESIGN section 4.36).  Integer minima and sums: the same bits.
 * Unknown key: DFE_E_ARG. */
int dfe_set_option(dfe_ctx *ctx, const char *key, int value);
int dfe_get_option(dfe_ctx *ctx, const char *key, int *value);
/* name of the kernel the last cost-volume call launched (static string) */
const char *dfe_last_kernel(const dfe_ctx *ctx);
/* the preparation and cascade kernels of the last one-call pyramid matcher run on this ctx, "<prep> <cascade>" -- prep_scales_kernel or
 * prep_tiles_kernel (prep_frames_kernel with learned filters); cascade_px_kernel, cascade_argmax_kernel<fast> (one cell per lane) or
 * cascade_argmax_kernel<slow>, or the fused volume kernel's name where the finest scale has no launch of its own.  After a census
 * run (dfe_multiscale_census_flow_pair_*) a third word follows, "<prep> <cascade> <volume>": census_pyramid_volume_kernel (the
 * one-launch kernel) or census_volume_kernel (the staged kernel, scale by scale).  A graph replay
 * keeps the names of its capture.  The string lives in the ctx and is rewritten by this call.  For tests and tuning. */
const char *dfe_multiscale_last_path(dfe_ctx *ctx);
/* which kernel produced the last single-scale flow step's result: *i8_taken = 1 the int8 matrix-core kernel (option "cv_i8": the frames
 * were byte-valued), 0 the float kernels.  Synchronises the ctx stream.  For tests and tuning. */
int dfe_flow_last_path(dfe_ctx *ctx, int *i8_taken);

/* upper bound for the ctx scratch arena that holds a materialised cost volume inside the one-call
 * pipelines (default 16 GiB); larger volumes are processed in bands of output rows (the volume-free flow step, option "cv_novol", has
 * no volume and no bands) */
int dfe_set_scratch_limit(dfe_ctx *ctx, size_t bytes);
/* device memory for a caller-owned cost volume (the `out` of dfe_ssd_cost_volume_f32 and friends): physically contiguous where the driver
 * grants it (hipExtMallocWithFlags + hipDeviceMallocContiguous), a plain hipMalloc otherwise; *contiguous (may be NULL) says which.  The
 * sweeps write a volume at up to 10 % more bytes per second into contiguous memory than into an unlucky plain allocation (the ctx's own arena is
 * allocated the same way, option "arena_contig").  Any device pointer works as `out`; this is the allocation that is fastest to fill.
 * replaces: torch.Tensor():resize() of the matcher's output on the reference side (SpatialMatching.lua:24), for callers that want the
 * placement.  dfe_device_free releases it (NULL is allowed).
 * A contiguous block is NOT handed back to the driver when it is released -- by dfe_device_free, by a growth of the ctx's arena or by
 * dfe_ctx_destroy: it goes idle in a pool of the process and serves the next contiguous request on its device that it can hold (the
 * smallest such block; freeing such memory is not safe on the driver this was developed on).  Hence: the block
 * behind *ptr may be larger than `bytes` (the caller owns all of it until it frees it) and holds whatever its last user left; a second
 * dfe_device_free of the same pointer fails with DFE_E_HIP and changes nothing; memory that the process's contexts took as contiguous
 * stays with the process until dfe_contig_pool_trim. */
int dfe_device_alloc(dfe_ctx *ctx, size_t bytes, void **ptr, int *contiguous);
int dfe_device_free(dfe_ctx *ctx, void *ptr);
/* Gives idle blocks of that pool on the ctx's device back to the driver (hipFree), largest first, until at most keep_bytes of them stay;
 * *idle_bytes (may be NULL) = what stays.  keep_bytes = SIZE_MAX frees nothing and only reports.  Synchronises the ctx stream.  For a
 * process that needs the memory more than it fears the driver's defect: allocations made after a trim are exposed to it again. */
int dfe_contig_pool_trim(dfe_ctx *ctx, size_t keep_bytes, size_t *idle_bytes);
/* per-launch HIP-event timing of the cost-volume kernel on the ctx stream (bench.py's roofline):
 * enable, run, then read the summed kernel time and launch count (read synchronises and resets) */
int dfe_profile_enable(dfe_ctx *ctx, int on);
int dfe_profile_read(dfe_ctx *ctx, double *total_ms, int *launches);
/* the same, and the first `cap` launches' durations one by one (each_ms[cap], in launch order): where inside a timed region the time went
 * (bench.py reports minimum / median / maximum next to the average) */
int dfe_profile_read_each(dfe_ctx *ctx, double *total_ms, int *launches, float *each_ms, int cap);

/* Stage timers with the reference's names -- `load / filter / match / extract` printed per frame by the dense driver
 * (depth_estimation_opticalflow.lua:44-47,112-117,144-148): HIP events around the launches of each stage inside the
 * one-call pipelines and the staging copies.  load = dfe_memcpy_h2d (the driver's image load + upload); filter = down-sampling,
 * padding, polar warps and the learned filter stacks (its `filter:forward`); match = cost volumes, soft-min and cascade
 * (`model:forward`); extract = arg-best / extractOutput / decode / border / depth passes (`processOutput`; where the arg-best
 * is fused into the matching kernel -- the multiscale cascade, the fused cost-volume build -- that part counts as match).
 * The single-scale flow step with option "cv_i8" on: match = the pack kernel and the int8 sweep; the ONE launch behind them counts as
 * extract.  On byte-valued frames that launch is the frame's border; on frames that fail the gate it is also the float sweep, which is
 * then counted under extract ("cv_i8" = 0 gives the true split).  The byte entries at scale 1 (dfe_flow_depth_pair_u8, _u8_slot) on the
 * int8 route launch nothing under load or extract: pack-from-bytes (with the border) and the sweep both count as match.
 * enable, run, read: ms[s] = summed GPU time of stage s, launches[s] = number of bracketed regions; read synchronises and resets. */
#define DFE_STAGE_LOAD 0
#define DFE_STAGE_FILTER 1
#define DFE_STAGE_MATCH 2
#define DFE_STAGE_EXTRACT 3
#define DFE_NSTAGES 4
int dfe_stage_timers_enable(dfe_ctx *ctx, int on);
int dfe_stage_timers_read(dfe_ctx *ctx, double *ms /* [DFE_NSTAGES] */, int *regions /* [DFE_NSTAGES] */);

/* ---- A0+A1: dense SSD cost volume from raw frames ----------------------- */
/* replaces: unfold + SpatialPadding crop + nn.SpatialMatching(hWin,wWin,false):forward
 *   radial/radial_opticalflow_groundtruth.lua:79-84 (= version2/groundtruth.lua:77-82),
 *   the raw-patch (identity filter) case of opticalflow_model.lua:81-99.
 * I0,I1 [C][H][W] f32.  out [Ho][Wo][hWin][wWin] f32,
 *   Ho = H-kh+1-hWin+1, Wo = W-kw+1-wWin+1,
 *   out[y][x][dy][dx] = sum_{c,i,j} (I0[c][y+oy+i][x+ox+j] - I1[c][y+dy+i][x+dx+j])^2,
 *   oy = floor((hWin-1)/2), ox = floor((wWin-1)/2). */
int dfe_ssd_cost_volume_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W,
                            int kh, int kw, int hWin, int wWin, float *out);

/* ---- A0+A1 with an fp16 volume (BASELINE configs[4]; SURVEY 7 "fp16 cost volume", 8(c) numeric contract) ------ */
/* Same sums as dfe_ssd_cost_volume_f32 (fp32 accumulation); the volume is stored as IEEE half, out[..] =
 * half(cost * scale), round to nearest even.  Raw SSD overflows half (147 * 255^2 = 9.56e6 > 65504), hence the scale:
 * 2^-8 for uint8-valued frames (max 37 344), 1 for frames in [0, 1].  out [Ho][Wo][hWin][wWin] of uint16 (half bits).
 * Stored values are within rel 2^-11 of the fp32 volume (bit-exact against half(oracle * scale) on integer-valued frames). */
int dfe_ssd_cost_volume_f16(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int kh, int kw, int hWin,
                            int wWin, float scale, void *out);
/* dfe_flow_depth_pair_f32 with the volume materialised as fp16: arg-min (+ centre tie-break) is taken on the fp32 sums
 * BEFORE the down-convert, so idx / best / flow / depth are identical to the fp32 path's.  idx, best [Ho][Wo] (may be NULL),
 * flow [2][H][W] centre-pasted, depth / depth_conf [H][W] (both or neither).  No extractOutput scores (their rare
 * fall-back reads the volume).  Shapes: C in {1,3}, 7x7 patch, 769..1096 window cells (else DFE_E_UNSUPPORTED). */
int dfe_flow_depth_pair_f16(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                            float foe_x, float foe_y, float scale, int64_t *idx, float *best, float *flow, float *depth,
                            float *depth_conf);

/* ---- A1: nn.SpatialMatching(maxh,maxw,false):updateOutput on feature maps -- */
/* replaces: nnx SpatialMatching call sites opticalflow_model_multiscale.lua:216,
 *   opticalflow_model.lua:93, version2/network.lua:30, tests/time_matching.lua:18.
 * in1 [K][H1][W1], in2 [K][H1+maxh-1][W1+maxw-1] -> out [H1][W1][maxh][maxw]. */
int dfe_spatial_matching_f32(dfe_ctx *ctx, const float *in1, const float *in2, int K, int H1,
                             int W1, int maxh, int maxw, float *out);

/* ---- A1r: nn.SpatialRadialMatching(hWin):updateOutput --------------------- */
/* replaces: radial/radial_opticalflow_network.lua:33,71-72.
 * in1 [K][H1][W], in2 [K][H1+hWin-1][W] -> out [H1][W][hWin]. */
int dfe_radial_matching_f32(dfe_ctx *ctx, const float *in1, const float *in2, int K, int H1,
                            int W, int hWin, float *out);

/* ---- A1r + arg-min, and the radial path in one call (BASELINE configs[2]) ------------------ */
/* replaces: SpatialRadialMatching(hWin):forward followed by `_, idx = output:min(3); idx:add(-1)`
 *   (radial/train_radial_opticalflow.lua:161-168, radial/test_radial_opticalflow.lua:204-207).  in1 [K][in1_plane_rows][W]
 *   (only the first H1 rows of a plane are read: the previous frame cropped by hWin-1 rows, network.lua:59;
 *   0 = H1), in2 [K][H1+hWin-1][W]; volume [H1][W][hWin] or NULL; flow [H1][W] = first-minimum index - 1 as float
 *   (TH min keeps the first minimum), its last row zeroed when zero_last_row (train_radial:178-180: the trainer's display
 *   code does that; the inference script test_radial:204-207 does not).
 *   hWin in {8, 12, 15, 16}. */
int dfe_radial_match_argmin_f32(dfe_ctx *ctx, const float *in1, int in1_plane_rows, const float *in2, int K, int H1, int W,
                                int hWin, float *volume, float *flow, int zero_last_row);
/* not in the reference: dfe_radial_match_argmin_f32 with a sub-pixel radial flow.  Same arguments,
 *   same volume, same hWin set {8, 12, 15, 16} (DFE_E_UNSUPPORTED otherwise).  For a pixel with costs c[0 .. hWin-1] (its
 *   volume cells, fp32):
 *     bi  = the first minimum, by strict `<` scan from 0 (as dfe_radial_match_argmin_f32);
 *     off = 0 if bi == 0 or bi == hWin - 1 (a neighbour lies outside the searched window); otherwise, with
 *           c0 = c[bi], cm = c[bi-1], cp = c[bi+1], den = (cm - c0) + (cp - c0):
 *           off = (cm - cp) / (2 * den) clamped to [-0.5, 0.5] if den > 0, else 0;
 *     flow = (float)bi + off.
 *   Every operation is fp32, separately rounded, in exactly this order, with IEEE division -- the per-axis rule of
 *   dfe_flow_refine_subpixel_f32.  The last row is 0 when zero_last_row.  The arithmetic is an epilogue on the costs the
 *   matcher's thread already holds: no second pass over the features. */
int dfe_radial_match_subpixel_f32(dfe_ctx *ctx, const float *in1, int in1_plane_rows, const float *in2, int K, int H1, int W,
                                  int hWin, float *volume, float *flow, int zero_last_row);
/* not in the reference: the same rule as a stage of its own, for any hWin >= 1 and any filter stack.  volume [P][hWin]
 *   (dfe_radial_matching_f32's output, P = H1 * W), flow_in [P] the integer radial flow as float (first-minimum index - 1,
 *   i.e. bi) -> flow_out [P] = flow_in + off.  Pixels whose flow_in is 0, hWin - 1 or no index of the window keep their
 *   value.  flow_out may be flow_in (in place).  Bit-identical to dfe_radial_match_subpixel_f32 on the same volume. */
int dfe_radial_refine_subpixel_f32(dfe_ctx *ctx, const float *volume, const float *flow_in, int64_t P, int hWin,
                                   float *flow_out);

/* networkp of the radial scripts (radial/train_radial_opticalflow.lua:83-97) for the default separable filter stack
 * {{C,1,kW1,n1},{n1,kH2,1,n2}} (train_radial:27), optionally with 'tanh' between the two convolutions. */
typedef struct dfe_radial_params {
    int C, hImg, wImg;     /* cartesian frames [C][hImg][wImg] */
    int hInput, wInput;    /* polar image size before the wKernel-1 wrap-around columns */
    int hWin;              /* radial search window */
    int n1, kW1;           /* layer 1: C -> n1 planes, 1 x kW1 (wKernel = kW1) */
    int n2, kH2;           /* layer 2: n1 -> n2 planes, kH2 x 1 (hKernel = kH2) */
    int tanh_between;      /* non-zero: nn.Tanh between the layers */
    float alpha_polar;     /* radial exponent of the polar grid (1 = linear) */
    double kinfty;         /* flow2depth's infinity factor (0.65 in test_radial:225; a Lua number, i.e. a double) */
    int zero_last_row;     /* 0 = radial/test_radial_opticalflow.lua:204-207 as shipped (idx = min(3) - 1, nothing else);
                              non-zero = also `test:sub(h,h,1,w):zero()` of the trainer's display path (train_radial:178-180) */
} dfe_radial_params;
/* rows of the matcher output (hInput - hKernel - hWin + 2) and size of the cartesian flow / depth images
 * (floor(hImg * kOutput) x floor(wImg * kOutput), getP2CMaskOF radial/radial_opticalflow_polar.lua:18-30). */
int dfe_radial_out_shape(const dfe_radial_params *p, int *hMatch, int *hOut, int *wOut);
/* replaces, composed: radial/test_radial_opticalflow.lua:186-225 (= train_radial:161-182 + flow2depth):
 *   getC2PMask + cartesian2polar of both frames -> getTesterNetwork(networkp):forward -> min(3) - 1 -> getP2CMaskOF +
 *   cartesian2polar of the flow -> flow2depth(networkp, flow, e2 * getKOutput(networkp), kinfty).
 *   prev (ego-motion-corrected by the caller) / cur [C][hImg][wImg]; (e2x, e2y) the epipole = focus of expansion in
 *   frame pixels (doubles, like the Lua numbers they replace: they are scaled before the reference rounds them to float); w1 [n1][C][1][kW1], b1 [n1], w2 [n2][n1][kH2][1], b2 [n2] (biases may be NULL).
 *   Outputs (each may be NULL): volume [hMatch][wInput][hWin], polar_flow [hMatch][wInput], cart_flow / depth / conf
 *   [hOut][wOut].  Bit-identical to the staged calls (dfe_polar_grid_c2p_f32, dfe_warp_bilinear_f32,
 *   dfe_spatial_convolution_f32, dfe_radial_matching_f32, ...). */
int dfe_radial_flow_depth_pair_f32(dfe_ctx *ctx, const dfe_radial_params *p, const float *prev, const float *cur, double e2x,
                                   double e2y, const float *w1, const float *b1, const float *w2, const float *b2,
                                   float *volume, float *polar_flow, float *cart_flow, float *depth, float *conf);
/* not in the reference: dfe_radial_flow_depth_pair_f32 with the sub-pixel polar flow of dfe_radial_match_subpixel_f32
 *   (DESIGN section 4.21).  Same arguments and outputs; everything after the matcher is unchanged -- the P2C bilinear
 *   sample, `f < 0.1 -> infty`, d / f, conf and the infty normalisation see a fractional polar flow instead of one of
 *   {0 .. hWin-1}.  Bit-identical to the staged calls with dfe_radial_refine_subpixel_f32 after the arg-min. */
int dfe_radial_flow_depth_pair_subpixel_f32(dfe_ctx *ctx, const dfe_radial_params *p, const float *prev, const float *cur,
                                            double e2x, double e2y, const float *w1, const float *b1, const float *w2,
                                            const float *b2, float *volume, float *polar_flow, float *cart_flow, float *depth,
                                            float *conf);

/* ---- semi-global aggregation of a cost volume with one label axis: a smoothed polar flow (NOT in the reference, whose matchers
 * are all winner-takes-all) ------------------------------------------------------------------------------- */
/* Hirschmueller's path aggregation.  volume [H][W][D] (dfe_radial_matching_f32's layout, D = hWin), agg [H][W][D] or NULL,
 * flow [H][W] or NULL.  With C = volume, every operation fp32, separately rounded, in exactly this order:
 *   Directions: bit r of `paths` is the direction (dy, dx): 0 (0, +1), 1 (0, -1), 2 (+1, 0), 3 (-1, 0), 4 (+1, +1), 5 (-1, -1),
 *     6 (+1, -1), 7 (-1, +1).
 *   Step: for a pixel p with predecessor q = p - r and m = min_k L_r(q, k), cells outside 0 .. D-1 taken as +Inf:
 *     t = min(min(min(L_r(q, d), L_r(q, d-1) + P1), L_r(q, d+1) + P1), m + P2);   L_r(p, d) = C(p, d) + (t - m).
 *   Start: L_r(p, .) = C(p, .) where q lies outside the plane.
 *   ring = G > 0: the columns are a ring, as the polar image's angle is.  The predecessor's column is taken modulo W, so a diagonal
 *     path only ever starts on the top or bottom row.  Direction 0 of a row starts at column W - G with L = C, walks the G warm-up
 *     columns up to W - 1 and then the columns 0 .. W - 1: only this second stretch is its L_0.  Direction 1 is the mirror image:
 *     it starts at G - 1, goes down to 0, then W - 1 .. 0.  G = 0 is the plane.
 *   Sum: agg = L_r of the lowest set bit, then agg = agg + L_r for each further set bit in ascending r.
 *   flow = the first minimum of agg over d, by strict `<` scan from 0, as a float (the matcher's rule).
 * 1 <= D <= 32 (a larger D: DFE_E_UNSUPPORTED); H, W >= 1 with H * W < 2^31 (DFE_E_SHAPE); paths in 1 .. 255, P1 and P2 finite
 * with 0 <= P1 <= P2, 0 <= ring <= W, agg and flow not both NULL, agg != volume, volume not NULL (DFE_E_ARG).  The volume must be
 * finite; for anything else (NaN, Inf, sums that overflow) the result is unspecified.
 * Two launches.  All directions at once, each into a plane of its own in the ctx's scratch arena (H * W * D floats per set bit): a
 * path's chain runs in one 16-lane DPP row, the labels across the lanes (two per lane above 16), the label axis padded with +Inf
 * cells, which change no bit of a real cell.  Then the planes are summed in order and the first minimum taken; with agg == NULL
 * the aggregate is never stored.  (A single direction with agg given writes its L straight there.)  Asynchronous on the ctx's
 * stream; runs under DFE_STAGE_MATCH. */
int dfe_sgm_aggregate_f32(dfe_ctx *ctx, const float *volume, int H, int W, int D, float P1, float P2, unsigned paths, int ring,
                          float *agg, float *flow);
/* dfe_radial_flow_depth_pair_f32 with the aggregation between the matcher and the P2C sample.  Same arguments and outputs, plus
 * P1, P2, paths, ring (dfe_sgm_aggregate_f32's; 0 <= ring <= wInput), subpixel (non-zero: dfe_radial_refine_subpixel_f32's rule on the
 * AGGREGATE) and agg_volume [hMatch][wInput][hWin] or NULL.  Order of work: the matcher writes the volume (to scratch when `volume` is
 * NULL); dfe_sgm_aggregate_f32 gives the aggregate and polar_flow = its first minimum; with subpixel the refinement; with
 * p->zero_last_row the last polar flow row is zeroed; the unchanged P2C sample and flow2depth.  hWin in {8, 12, 15, 16}.
 * Bit-identical to the same steps as staged public calls. */
int dfe_radial_flow_depth_pair_sgm_f32(dfe_ctx *ctx, const dfe_radial_params *p, const float *prev, const float *cur, double e2x,
                                       double e2y, const float *w1, const float *b1, const float *w2, const float *b2, float P1,
                                       float P2, unsigned paths, int ring, int subpixel, float *volume, float *agg_volume,
                                       float *polar_flow, float *cart_flow, float *depth, float *conf);

/* ---- the census matching cost: an exposure-robust single-scale matcher (NOT in the reference, whose raw-frame matchers all score
 * by the sum of squared differences) ------------------------------------------------------------------------ */
/* Integers only up to the match score, so every result below is exact.
 *   Signature.  kh, kw odd, at least 3, kh kw <= 64.  Patch positions Hp = H - kh + 1 by Wp = W - kw + 1, a patch indexed by its
 *     top-left corner as in dfe_ssd_cost_volume_f32.  S[c][y][x] is a uint64_t: walk the patch row-major over (i, j) and skip the
 *     centre (floor(kh / 2), floor(kw / 2)); the b-th visited cell sets bit b iff I[c][y+i][x+j] < I[c][y+floor(kh/2)][x+floor(kw/2)].
 *     The comparison is strict and on the stored values; with a NaN on either side it is false; the unused high bits are 0.  The
 *     byte entry compares the bytes themselves: the bits of the float entry on float(byte) * scale for any scale > 0.
 *   Hamming.  h[y][x][dy][dx] = sum_c popcount(S0[c][y+oy][x+ox] ^ S1[c][y+dy][x+dx]), oy = floor((hWin - 1) / 2),
 *     ox = floor((wWin - 1) / 2), y < Ho = Hp - hWin + 1, x < Wo = Wp - wWin + 1: the geometry and class order of the SSD volume,
 *     for odd and even windows alike.
 *   Aggregated cost.  agg = a in {1, 3, 5}: cost[y][x][dy][dx] = sum_{u < a, v < a} h[y+u][x+v][dy][dx], Ha = Ho - a + 1 by
 *     Wa = Wo - a + 1.  At most 63 C a^2, so exact in fp32: the volume is stored as float, and dfe_flow_tail, dfe_argbest_center and
 *     dfe_extract_output read it as they read any other.
 *   Flow.  The first minimum in class order (class = dy wWin + dx + 1); the centre class wins an exact tie with the best: the rule
 *     and the middle index of dfe_ssd_flow_f32 / dfe_argbest_center (getMiddleIndex).  Decoded as dfe_x2yx decodes.
 *   Match score.  match = 1.0f - (float)best / (float)(nbits C a^2), nbits = kh kw - 1: one rounded fp32 division, one rounded
 *     subtraction.  Above 0 unless every bit disagrees.
 *   Paste.  The full-frame outputs hold the Ha x Wa region at pad_t = (H - Ha) / 2, pad_l = (W - Wa) / 2 (integer divisions, the
 *     single-scale step's rule) and 0 elsewhere; depth and depth_conf are made from the pasted flow as dfe_flow_depth_pair_f32
 *     makes them (dfe_flow_to_depth_cartesian, fix_dot = 0).
 * Limits: 1 <= C <= 4, kh / kw as above, agg in {1, 3, 5}, nbits in 1 .. 63, no NULL input (DFE_E_ARG); hWin wWin <= 1096
 * (DFE_E_UNSUPPORTED); every frame side and Hp, Wp at most 32768 and Ha, Wa >= 1 (DFE_E_SHAPE).  Refused before any launch.
 * Asynchronous on the ctx's stream.
 * dfe_census_transform_*: I [C][H][W] -> sig [C][Hp][Wp].  One launch, a 4 x 64 tile of positions with its halo in LDS. */
int dfe_census_transform_f32(dfe_ctx *ctx, const float *I, int C, int H, int W, int kh, int kw, uint64_t *sig);
int dfe_census_transform_u8(dfe_ctx *ctx, const uint8_t *I, int C, int H, int W, int kh, int kw, uint64_t *sig);
/* The staged route: out [Ha][Wa][hWin][wWin], for tests and for callers who want the volume.  A thread per cell. */
int dfe_census_cost_volume_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int Wp, int hWin,
                               int wWin, int agg, float *out);
/* The fused route: no volume reaches memory.  idx (1-based class), best (the cost), match, flow_y, flow_x, all [Ha][Wa], any may be
 * NULL.  Equal to dfe_census_cost_volume_f32 -> dfe_argbest_center(middle = getMiddleIndex) -> dfe_x2yx.  A workgroup stages
 * frame 1's signatures of a band of window rows in LDS (at most 64 KB), a lane keeps frame 0's signatures of its column in
 * registers and walks down it once per class; the box sum is DPP row shifts across and register adds down. */
int dfe_census_flow_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int Wp, int nbits, int hWin,
                        int wWin, int agg, int64_t *idx, float *best, float *match, float *flow_y, float *flow_x);
/* The one call: two transforms (k x k patch) into the ctx's scratch arena, the fused sweep storing at the pasted positions, then
 * the border and depth pass of the single-scale step.  flow [2][H][W] (y, x), match [H][W], depth / depth_conf [H][W] (both or
 * neither).  Bit-identical to the staged public calls plus the paste.  scale only has to be positive: it changes no bit. */
int dfe_census_flow_depth_pair_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                                   int agg, float foe_x, float foe_y, float *flow, float *match, float *depth, float *depth_conf);
int dfe_census_flow_depth_pair_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin,
                                  int agg, float foe_x, float foe_y, float scale, float *flow, float *match, float *depth,
                                  float *depth_conf);

/* ---- semi-global aggregation on a two-dimensional label plane: smoothed labels for the Cartesian matchers (NOT in the reference;
 * DESIGN section 4.31) ------------------------------------------------------------------------------------------------------------ */
/* dfe_sgm_aggregate_f32's path aggregation for the volumes whose label is a cell of a search window.  volume [H][W][hWin][wWin]: the
 * geometry and class order of the SSD and census volumes, class = dy wWin + dx + 1.  agg [H][W][hWin][wWin] or NULL; idx [H][W]
 * (int64, 1-based class), flow_y, flow_x [H][W], each or NULL.  With C = volume, every operation fp32, rounded on its own, not
 * contracted, in exactly this order:
 *   Labels: a label is a cell (dy, dx) of the window; its neighbours are the four cells at city-block distance 1; a cell outside
 *     the window counts as +Inf.
 *   Directions: bit r of `paths` is the direction (dy, dx) of dfe_sgm_aggregate_f32: 0 (0, +1), 1 (0, -1), 2 (+1, 0), 3 (-1, 0),
 *     4 (+1, +1), 5 (-1, -1), 6 (+1, -1), 7 (-1, +1).  There is no ring: these are Cartesian frames.
 *   Step: for a pixel p with predecessor q = p - r and m = the minimum of L_r(q, .) over all cells:
 *     t = L_r(q, (dy, dx));
 *     t = min(t, L_r(q, (dy, dx-1)) + P1);  t = min(t, L_r(q, (dy, dx+1)) + P1);
 *     t = min(t, L_r(q, (dy-1, dx)) + P1);  t = min(t, L_r(q, (dy+1, dx)) + P1);
 *     t = min(t, m + P2);   L_r(p, (dy, dx)) = C(p, (dy, dx)) + (t - m).
 *   Start: L_r(p, .) = C(p, .) where q lies outside the plane.
 *   Sum: agg = L_r of the lowest set bit, then agg = agg + L_r for each further set bit in ascending r.
 *   Flow: idx = what dfe_argbest_center gives on agg with middle = getMiddleIndex: the first minimum in class order, the centre
 *     class winning an exact tie; flow_y, flow_x decoded as dfe_x2yx decodes, as floats.
 * hWin, wWin >= 1 with hWin wWin <= 1096, the single-scale step's ceiling (more: DFE_E_UNSUPPORTED); H, W >= 1 with H * W < 2^31
 * (DFE_E_SHAPE, as a window side below 1); paths in 1 .. 255, P1 and P2 finite with 0 <= P1 <= P2, volume not NULL, outputs not all
 * NULL, agg != volume (DFE_E_ARG).  Refused before any launch.  The volume must be finite; for anything else the result is unspecified.
 * Two launches.  All directions at once, each into a plane of its own in the ctx's scratch arena (H * W * hWin * wWin floats per set
 * bit): a line of pixels belongs to one wave, cell j 64 + lane in lane `lane`, the cell axis padded with +Inf cells, which change no
 * bit of a real cell; L_r(q, .) is exchanged through a double-buffered LDS plane with a +Inf frame.  Then a wave a pixel sums the
 * planes in order and takes the first minimum; with agg == NULL the aggregate is never stored.  (A single direction with agg given
 * writes its L straight there.)  Asynchronous on the ctx's stream; runs under DFE_STAGE_MATCH. */
int dfe_sgm_plane_aggregate_f32(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2,
                                unsigned paths, float *agg, int64_t *idx, float *flow_y, float *flow_x);
/* dfe_census_flow_depth_pair_* with the aggregation between the cost and the arg-min.  Same arguments and outputs, plus P1, P2, paths
 * (dfe_sgm_plane_aggregate_f32's, on the Ha x Wa plane of the aggregated census cost).  Order of work: two transforms, the staged
 * census volume (dfe_census_cost_volume_f32) into the scratch arena, the aggregation with no aggregate stored, the flow at the pasted
 * positions, the border and depth pass of the single-scale step.  match = 1 - C(p, idx) / (nbits C agg^2): the census match score of the
 * RAW cost at the chosen class, on the scale of dfe_census_flow_depth_pair_*'s.  Every argument is checked before any launch, with
 * the codes of the two entries it joins.  Bit-identical to the staged public calls plus the paste. */
int dfe_census_flow_depth_pair_sgm_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                                       int agg, float foe_x, float foe_y, float P1, float P2, unsigned paths, float *flow,
                                       float *match, float *depth, float *depth_conf);
int dfe_census_flow_depth_pair_sgm_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin,
                                      int agg, float foe_x, float foe_y, float scale, float P1, float P2, unsigned paths, float *flow,
                                      float *match, float *depth, float *depth_conf);

/* ---- what is read off the aggregate besides its arg-min: a uniqueness confidence and a sub-pixel flow (NOT in the reference; DESIGN
 * section 4.32) ---------------------------------------------------------------------------------------------------------------------- */
/* volume, H, W, hWin, wWin, P1, P2, paths, agg, idx: dfe_sgm_plane_aggregate_f32's.  paths == 0 is also accepted here and means no
 * aggregation: A = volume, no path launch, P1 and P2 ignored but still checked -- uniqueness and the sub-pixel rule then serve any
 * winner-takes-all volume.  flow_y, flow_x, best, second, unique: [H][W] floats, each or NULL; at least one output must be given.
 * A is the aggregate exactly as dfe_sgm_plane_aggregate_f32 sums it and (r, s) the cell it picks, centre rule included.  Every
 * operation is fp32, rounded on its own, not contracted:
 *   best   = A(r, s).
 *   second = the smallest A(r', s') over the cells with max(|r' - r|, |s' - s|) >= 2; +Inf if the window has no such cell.  (The
 *     winner's 3 x 3 neighbourhood is left out because a true minimum drags its neighbours down with it.)
 *   u      = (second == +Inf || !(second > 0)) ? 0 : (second - best) / second: one rounded subtraction, one IEEE division.  u is NOT
 *     clamped: with costs of mixed sign (second > 0 > best) it exceeds 1.  unique = u >= min_unique ? u : 0, min_unique in [0, 1]
 *     (else DFE_E_ARG).  idx and the flow are written whatever the gate says.
 *   subpixel != 0: the per-axis parabola of dfe_flow_refine_subpixel_f32 with cost := A (x shown; y alike with r -+ 1):
 *     c0 = A(r, s), cm = A(r, s-1), cp = A(r, s+1); off = 0 if s-1 < 0 or s+1 >= wWin; else den = (cm - c0) + (cp - c0),
 *     off = den > 0 ? clamp((cm - cp) / (2 den), -0.5, 0.5) : 0;  flow_x = (float)dx + off_x, flow_y = (float)dy + off_y.
 *   subpixel == 0: flow_y, flow_x have the bits of dfe_sgm_plane_aggregate_f32's; idx and agg have them always, for every non-zero paths.
 * Errors: dfe_sgm_plane_aggregate_f32's, with paths in 0 .. 255.  Refused before any launch.
 * The path launch is dfe_sgm_plane_aggregate_f32's; then a wave a pixel sums the planes in order, keeps the sums in LDS, takes the
 * first minimum and, in a second reduction over the sums it has kept, the far minimum; the parabola reads the same sums.  With
 * agg == NULL the aggregate is never stored.  Asynchronous on the ctx's stream; runs under DFE_STAGE_MATCH. */
int dfe_sgm_plane_pick_f32(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2, unsigned paths,
                           int subpixel, float min_unique, float *agg, int64_t *idx, float *flow_y, float *flow_x, float *best,
                           float *second, float *unique);
/* The single-scale SSD step with the aggregation between the cost and the arg-min: the arguments of dfe_flow_depth_pair_f32 / _u8
 * without extract_threshold, plus P1, P2, paths (1 .. 255), subpixel, min_unique (dfe_sgm_plane_pick_f32's, on the Ho x Wo plane).
 * Order of work: the WHOLE SSD volume (dfe_ssd_cost_volume_f32) into the ctx's scratch arena -- no row bands, the vertical paths need
 * every row; an arena that cannot be had returns the arena's own error --, the aggregation with no aggregate stored, the pick storing
 * at the pasted positions: flow [2][H][W] (y, x), scores [H][W] = unique; then the border and depth pass of the single-scale step
 * (depth / depth_conf both or neither).  The byte entry converts with float(byte) * scale, as dfe_flow_depth_pair_u8 does.  Every
 * argument is refused before any launch, with the codes of the entries it joins.  Bit-identical to the staged public calls plus the
 * paste. */
int dfe_flow_depth_pair_sgm_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                                float foe_x, float foe_y, float P1, float P2, unsigned paths, int subpixel, float min_unique,
                                float *flow, float *scores, float *depth, float *depth_conf);
int dfe_flow_depth_pair_sgm_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin,
                               float foe_x, float foe_y, float scale, float P1, float P2, unsigned paths, int subpixel,
                               float min_unique, float *flow, float *scores, float *depth, float *depth_conf);
/* dfe_census_flow_depth_pair_sgm_* with subpixel and min_unique (dfe_sgm_plane_pick_f32's) and one more output: unique [H][W] or NULL,
 * the uniqueness of the AGGREGATE at the pasted positions, 0 elsewhere.  match keeps its meaning (the raw cost at the chosen class).
 * With subpixel == 0 and unique == NULL every output has the bits of dfe_census_flow_depth_pair_sgm_*'s. */
int dfe_census_flow_depth_pair_sgm2_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                                        int agg, float foe_x, float foe_y, float P1, float P2, unsigned paths, int subpixel,
                                        float min_unique, float *flow, float *match, float *unique, float *depth, float *depth_conf);
int dfe_census_flow_depth_pair_sgm2_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin,
                                       int wWin, int agg, float foe_x, float foe_y, float scale, float P1, float P2, unsigned paths,
                                       int subpixel, float min_unique, float *flow, float *match, float *unique, float *depth,
                                       float *depth_conf);

/* ---- edge-aware semi-global aggregation: P2 adapted to a guide image, for both label families (NOT in the reference; DESIGN section
 * 4.38) ------------------------------------------------------------------------------------------------------------------------------- */
/* Everything is as dfe_sgm_aggregate_f32 / dfe_sgm_plane_aggregate_f32 / dfe_sgm_plane_pick_f32 define it, except the term m + P2 of a
 * step: for a pixel p whose predecessor on direction r is q = p - r it is m + P2(p, r).  guide [Cg][H][W], float32, Cg >= 1, on the
 * volume's own pixel grid; on a ring q's column is taken modulo W, so the pair (x = 0, x = W - 1) has a penalty of its own.
 *   Host:    inv_s2 = 1.0f / (sigma * sigma);  span = P2 - P2_edge;  both in float.
 *   Device:  fp32, rounded on its own, not contracted:
 *            d2 = sum over c of (g_c(p) - g_c(q))^2, in channel order, starting from the first square;
 *            w = max(0, 1 - d2 * inv_s2); a w that is not finite counts as 0.
 *   Penalty: P2(p, r) = P2_edge + span * w; where w == 1 exactly P2(p, r) = P2 with no arithmetic, so a flat guide gives the unguided
 *            bits.  This is the range term of dfe_weighted_median_f32 and dfe_guided_upsample_f32 applied to P2.
 *   Unguided: guide == NULL, or sigma <= 0 or NaN: P2(p, r) = P2, and the entry returns the bits of the unguided entry with its launches.
 *   Unchanged: a chain start (L = C) uses no penalty; the P1 terms, the order of the sum, the first minimum, the centre rule, the
 *            uniqueness and the sub-pixel rules.  (a - b)^2 and (b - a)^2 have the same bits: direction r at p and direction -r at
 *            p - r use the same number.
 * Errors: the unguided entry's, and P2_edge finite with P1 <= P2_edge <= P2, Cg >= 1 with a guide (DFE_E_ARG).  Refused before any launch.
 * One launch more than the unguided entry: a pre-pass writes P2(p, r) for the even direction of each axis the paths lie on into an
 * [H][W] plane in the ctx's scratch arena (four at the most: the odd direction reads the plane at its predecessor); the path kernels'
 * guided forms fetch a step's penalty with its costs.  A NaN or Inf guide sample gives P2_edge on the steps that touch it. */
int dfe_sgm_aggregate_guided_f32(dfe_ctx *ctx, const float *volume, int H, int W, int D, float P1, float P2, unsigned paths, int ring,
                                 float *agg, float *flow, const float *guide, int Cg, float sigma, float P2_edge);
/* dfe_sgm_plane_pick_f32 under the guided penalty.  It serves the plain aggregate too (best, second, unique NULL and subpixel 0 give
 * dfe_sgm_plane_aggregate_f32's outputs); paths == 0 stays the winner-takes-all read, and the guide is ignored there. */
int dfe_sgm_plane_pick_guided_f32(dfe_ctx *ctx, const float *volume, int H, int W, int hWin, int wWin, float P1, float P2,
                                  unsigned paths, int subpixel, float min_unique, float *agg, int64_t *idx, float *flow_y, float *flow_x,
                                  float *best, float *second, float *unique, const float *guide, int Cg, float sigma, float P2_edge);
/* dfe_flow_depth_pair_sgm_f32 / _u8 and dfe_census_flow_depth_pair_sgm2_f32 / _u8 under the guided penalty: their arguments plus sigma
 * and P2_edge.  The guide is the call's own frame 0, all C channels, cropped to the pixels the volume's plane is pasted at; for the
 * byte entries float(byte) * scale, as dfe_u8_to_f32 gives (the census entry compares the bytes as they are, so scale matters to it
 * only here: sigma is in the units of float(byte) * scale).  Bit-identical to the staged public calls -- the volume, then
 * dfe_sgm_plane_pick_guided_f32 on that crop -- plus the paste. */
int dfe_flow_depth_pair_sgm_guided_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                                       float foe_x, float foe_y, float P1, float P2, unsigned paths, int subpixel, float min_unique,
                                       float sigma, float P2_edge, float *flow, float *scores, float *depth, float *depth_conf);
int dfe_flow_depth_pair_sgm_guided_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin,
                                      int wWin, float foe_x, float foe_y, float scale, float P1, float P2, unsigned paths, int subpixel,
                                      float min_unique, float sigma, float P2_edge, float *flow, float *scores, float *depth,
                                      float *depth_conf);
int dfe_census_flow_depth_pair_sgm_guided_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin,
                                              int wWin, int agg, float foe_x, float foe_y, float P1, float P2, unsigned paths,
                                              int subpixel, float min_unique, float sigma, float P2_edge, float *flow, float *match,
                                              float *unique, float *depth, float *depth_conf);
int dfe_census_flow_depth_pair_sgm_guided_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin,
                                             int wWin, int agg, float foe_x, float foe_y, float scale, float P1, float P2,
                                             unsigned paths, int subpixel, float min_unique, float sigma, float P2_edge, float *flow,
                                             float *match, float *unique, float *depth, float *depth_conf);

/* ---- the census cost for the radial (polar) matcher: an exposure-robust polar flow that needs no trained weights (NOT in the
 * reference, whose radial matcher scores learned features by the sum of squared differences) ---------------- */
/* Integers only up to the score, so every result below is exact.  With W = wInput, lpad = (kw - 1) / 2 and rpad = kw - 1 - lpad (the
 * filter stack's rule for wKernel):
 *   Signatures.  S = dfe_census_transform_f32 of a polar frame [C][hInput][W + kw - 1], as the polar warp makes it with lpad wrap
 *     columns on the left: [C][Hp = hInput - kh + 1][W], column x's patch centred on polar column x.
 *   Hamming.  h[y][x][d] = sum_c popcount(S0[c][y][x] ^ S1[c][y + d][x]), y < H1 = Hp - hWin + 1, 0 <= d < hWin: the geometry of
 *     dfe_radial_matching_f32 (frame 0 is not centred, d = 0 is no motion).
 *   Box.  agg = a in {1, 3, 5}, a <= W: cost[y][x][d] = sum_{u < a} sum_{v < a} h[y + u][(x + v - floor(a / 2)) mod W][d].  The rows
 *     shrink to Ha = H1 - a + 1, indexed from the top-left as the Cartesian census cost is; the columns are a ring, so all W survive.
 *     At most 63 C a^2 <= 6300: stored as an exact float.
 *   Flow.  The first minimum over d by a strict `<` scan from 0, as a float; no centre rule (dfe_radial_match_argmin_f32's rule).
 *   Match score.  match = 1.0f - (float)best / (float)(nbits C a^2): one rounded fp32 division, one rounded subtraction.
 *   Sub-pixel.  dfe_radial_refine_subpixel_f32's rule on the float costs.
 *   zero_last_row.  As in the radial entries: the last flow row is stored as 0 (best, match and the volume keep their values).
 * Limits: 1 <= C <= 4, agg in {1, 3, 5} and agg <= W, nbits in 1 .. 63, hWin >= 1, no NULL input (DFE_E_ARG); Hp, W in 1 .. 32768,
 * hWin <= Hp and Ha >= 1 (DFE_E_SHAPE).  Refused before any launch.  Asynchronous on the ctx's stream, under DFE_STAGE_MATCH.
 * There is no byte entry: the polar warp interpolates, so byte frames have no exactness to offer on this path.
 * The staged route: out [Ha][W][hWin], any hWin >= 1, a thread per cell. */
int dfe_census_radial_cost_volume_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int W, int hWin,
                                      int agg, float *out);
/* The fused matcher, one launch: flow [Ha][W]; volume [Ha][W][hWin], best (the cost at the first minimum) and match [Ha][W] may
 * each be NULL, and no volume reaches memory unless asked for.  hWin in {8, 12, 15, 16} (anything else: DFE_E_UNSUPPORTED, use the
 * staged route + dfe_argbest_center + dfe_radial_refine_subpixel_f32, as with dfe_radial_match_argmin_f32).  A workgroup of four
 * waves stages frame 1's signatures of its tile's rows in LDS; a lane keeps frame 0's signatures of its column (x0 - floor(a / 2) +
 * lane) mod W in registers; the labels are dealt to the waves; the box sum is register adds down and DPP row shifts across; the costs
 * of the tile meet in LDS for the scan, the sub-pixel rule and whole-line stores of the volume. */
int dfe_census_radial_flow_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int W, int nbits, int hWin,
                               int agg, int subpixel, int zero_last_row, float *volume, float *flow, float *best, float *match);
typedef struct dfe_census_radial_params {
    int C, hImg, wImg;     /* cartesian frames [C][hImg][wImg] */
    int hInput, wInput;    /* polar image size before the kw - 1 wrap-around columns */
    int hWin;              /* radial search window */
    int kh, kw;            /* census patch: odd sides of at least 3, kh kw <= 64 */
    int agg;               /* box side a: 1, 3 or 5 */
    float alpha_polar;     /* radial exponent of the polar grid (1 = linear) */
    double kinfty;         /* flow2depth's infinity factor, as in dfe_radial_params */
    int zero_last_row;     /* as in dfe_radial_params */
} dfe_census_radial_params;
/* The radial path in one call with the census matcher in the filter stack's and the matcher's place.  prev / cur [C][hImg][wImg],
 * (e2x, e2y) the epipole.  Order of work: the polar warps of both frames (dfe_radial_flow_depth_pair_f32's kernels, lpad wrap
 * columns on the left), two transforms into the ctx's scratch arena, the fused matcher, the unchanged P2C sample and flow2depth.
 * Geometry: hMatch = hInput - (kh - 1) - (hWin - 1) - (a - 1), and every formula of dfe_radial_flow_depth_pair_f32's last step with
 * kH2 = kh + a - 1 -- dfe_radial_out_shape with that kH2 gives hMatch, hOut and wOut.
 * paths == 0: winner takes all.  paths in 1 .. 255: the matcher runs for its volume (to scratch when `volume` is NULL),
 * dfe_sgm_aggregate_f32 (P1, P2, paths, ring) gives the aggregate and polar_flow = its first minimum, with subpixel the refinement
 * runs on the AGGREGATE, and match is the census score of the RAW cost at the chosen integer label.
 * Outputs (each may be NULL): volume, agg_volume [hMatch][wInput][hWin] (agg_volume only with paths != 0), polar_flow, match
 * [hMatch][wInput], cart_flow / depth / conf [hOut][wOut].  hWin in {8, 12, 15, 16}.  Every argument is checked before any launch:
 * the limits above, kh / kw as for dfe_census_transform_f32, dfe_sgm_aggregate_f32's rules, agg_volume != volume.  Bit-identical
 * to the same steps as staged public calls. */
int dfe_census_radial_flow_depth_pair_f32(dfe_ctx *ctx, const dfe_census_radial_params *p, const float *prev, const float *cur,
                                          double e2x, double e2y, float P1, float P2, unsigned paths, int ring, int subpixel,
                                          float *volume, float *agg_volume, float *polar_flow, float *match, float *cart_flow,
                                          float *depth, float *conf);

/* ---- the census cost in the pyramid matcher: an exposure-robust multiscale flow that needs no trained weights (NOT in the
 * reference, whose pyramid scores raw patches by the sum of squared differences) ----------------------------- */
/* Per scale with ratio r, for frames I0, I1 [C][H][W], H and W multiples of every ratio, k x k census patch, agg = a:
 *   1. Down-sample.  Box down-sample by r with dfe_downsample_box_f32's bits; r = 1 is the frame itself.
 *   2. Pad.  Zero-pad by hp = (maxh - 1) + (k - 1) + (a - 1) rows and wp = (maxw - 1) + (k - 1) + (a - 1) columns, pt = hp / 2 above
 *      and pl = wp / 2 on the left (integer divisions), the rest below and on the right: the SSD pyramid's rule
 *      (dfe_pyramid_scale_volume_f32) with the receptive field k + a - 1 in k's place.
 *   3. Signatures.  dfe_census_transform_f32 with a k x k patch on both padded frames: [C][Hs + maxh - 1 + a - 1][Ws + maxw - 1 + a - 1],
 *      Hs = H / r, Ws = W / r.  Strict comparison on the stored floats; the zero border compares like any value.
 *   4. Cost.  dfe_census_cost_volume_f32(sig0, sig1, C, .., hWin = maxh, wWin = maxw, agg = a): the integer cost [Hs][Ws][maxh][maxw] in
 *      the geometry and class order of the SSD scale volume (frame-0 offset floor((maxh - 1) / 2), floor((maxw - 1) / 2)); the a x a box
 *      ends up centred on the pixel.
 *   5. Stored value.  (float)cost * beta, one rounded fp32 multiply.  beta is the soft-min's temperature: a Hamming sum reaches
 *      (k k - 1) C a^2, and unscaled the soft-min is one-hot, so that the cascade cannot weigh a scale against its parent.
 *   6. Chain.  dfe_softmin_f32 per scale and dfe_cascade_flow_f32, as in dfe_multiscale_flow_pair_f32.
 * Limits, refused before any launch: k odd, k >= 3, k k <= 64; 1 <= C <= 4; agg in {1, 3, 5}; beta finite and > 0; no NULL input
 * (DFE_E_ARG); maxh maxw <= 1096 (DFE_E_UNSUPPORTED); every padded scale at most 32768 a side (DFE_E_SHAPE); and every ratio,
 * ring-geometry and size rule of dfe_multiscale_flow_pair_f32.  Asynchronous on the ctx's stream.
 * dfe_census_pyramid_scale_volume_f32: steps 1 - 5 for one scale, staged from the kernels of the entries named above plus the
 *   multiply; out [H/r][W/r][maxh][maxw].  Any window.  For tests and for callers who want the volume. */
int dfe_census_pyramid_scale_volume_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int r, int k, int maxh,
                                        int maxw, int agg, float beta, float *out);
/* The one call: flow [2][H][W] and / or idx [H][W] as dfe_multiscale_flow_pair_f32 gives them, bit-identical to
 * dfe_census_pyramid_scale_volume_f32 per scale -> dfe_softmin_f32 -> dfe_cascade_flow_f32.  One launch prepares every scale's padded
 * frames (the SSD pyramid's), one takes every scale's signatures, one builds every scale's volume (8 x 8 windows: frame 1's
 * signatures of a tile in LDS, frame 0's of a lane's column in registers, the box sum by DPP row shifts and register adds, whole
 * 128-byte lines stored; any other window: the staged volume kernel scale by scale), then the SSD pyramid's cascade launches.  Every
 * scale's volume is materialised in the ctx's scratch arena.  dfe_multiscale_last_path names the volume kernel behind the other two.
 * The _u8 entry takes byte frames and is the f32 entry on float(byte). */
int dfe_multiscale_census_flow_pair_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int maxh, int maxw,
                                        const int *ratios, int nratios, int agg, float beta, float *flow, int64_t *idx);
int dfe_multiscale_census_flow_pair_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int maxh,
                                       int maxw, const int *ratios, int nratios, int agg, float beta, float *flow, int64_t *idx);

/* ---- sub-pixel flow on the raw census cost: the single-scale matcher and the pyramid (NOT in the reference) --- */
/* For an output pixel (y, x) with chosen cell (r, s) -- the step's first minimum with the centre tie-break, whatever the window's
 * parity; decoded flow dy = r - (hWin-1)/2, dx = s - (wWin-1)/2 -- cost(r', s') is the aggregated integer census cost of
 * dfe_census_cost_volume_f32 for that pixel and cell: exact in fp32, at most 63 C a^2.  A Hamming cost is V-shaped around its
 * minimum, so the fit is the equiangular ("vee") one, not the SSD paths' parabola.  Per axis (x shown; y alike with r -+ 1), in fp32:
 *   c0 = cost(r, s), cm = cost(r, s-1), cp = cost(r, s+1);
 *   off = 0 if s-1 < 0 or s+1 >= wWin (a neighbour outside the searched window);
 *   else m = max(cm - c0, cp - c0); off = m > 0 ? clamp((cm - cp) / (2 m), -0.5, 0.5) : 0   (one IEEE division; everything before
 *     it is an exact integer);
 *   fx = (float)dx + off_x, fy = (float)dy + off_y.
 * Where c0 is the minimum |off| <= 0.5 without the clamp; the clamp and the m > 0 test matter only for a class map from another
 * producer.  Two equal minima side by side give +-0.5, the point between them.  The class, best and match never change.  Because the
 * costs are integers every result is defined bit for bit.  Meant for agg >= 3 or several channels: one channel without a box has too
 * few bits to refine on.
 * dfe_census_refine_subpixel_f32: the refinement alone, from the 1-based idx [Ha][Wa] of dfe_census_flow_f32 and the signatures it
 *   read; fy / fx written at [(y + pad_t) * pitch + x + pad_l].  Pixels whose idx is outside 1 .. hWin wWin keep what fy / fx held.
 *   The limits and error codes of dfe_census_flow_f32; pitch >= pad_l + Wa, pads >= 0 (DFE_E_SHAPE).  One launch, a thread per pixel: the
 *   five costs are re-formed from the two signature planes, frame 0's a x a box shared by all five, frame 1's plus-shaped footprint of
 *   (a + 2)^2 - 4 signatures, a popcount per pair.
 * dfe_census_flow_depth_pair_subpixel_f32 / _u8: the arguments and outputs of dfe_census_flow_depth_pair_f32 / _u8; the step runs
 *   unchanged, then its pasted flow is refined and depth / depth_conf (NULL together, as there) are the step's per-pixel formula on the
 *   refined flow.  match and the zero border are the step's.  Bit-identical to the staged public calls plus the paste. */
int dfe_census_refine_subpixel_f32(dfe_ctx *ctx, const uint64_t *sig0, const uint64_t *sig1, int C, int Hp, int Wp, int hWin, int wWin,
                                   int agg, const int64_t *idx, float *fy, float *fx, int pitch, int pad_t, int pad_l);
int dfe_census_flow_depth_pair_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin,
                                            int wWin, int agg, float foe_x, float foe_y, float *flow, float *match, float *depth,
                                            float *depth_conf);
int dfe_census_flow_depth_pair_subpixel_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin,
                                           int wWin, int agg, float foe_x, float foe_y, float scale, float *flow, float *match,
                                           float *depth, float *depth_conf);
/* The pyramid.  A pixel's class id decodes (x2yxMultiNumber, dfe_x2yx_multi) to a scale with ratio r and a cell (a, b) of the
 * maxh x maxw window, as in dfe_multiscale_refine_subpixel_f32.  The costs are the integer census costs of that scale -- step 4 above,
 * before the multiply by beta, which cancels in the fit and would only add rounding -- at the scale's pixel (y / r, x / r), inside
 * a coarse scale's ring hole too.  The rule above per axis, then
 *   fx = (float)(dx r) + (float)r * off   (product and sum separately rounded).
 * The class id, and with it the integer flow, never changes; the refined flow is within r / 2 of it per axis.
 * dfe_multiscale_census_refine_subpixel_f32: the refinement alone, from any 1-based class map idx [H][W] into flow [2][H][W]; it
 *   prepares the padded scales and their signatures itself.  Pixels whose idx is no class id keep what flow held.  The limits of
 *   dfe_multiscale_census_flow_pair_f32 (no beta).
 * dfe_multiscale_census_flow_pair_subpixel_f32 / _u8: the arguments of dfe_multiscale_census_flow_pair_f32 / _u8; the matcher runs
 *   unchanged, then flow (required) is refined in place from the signatures the call already made; idx (optional) is the matcher's. */
int dfe_multiscale_census_refine_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int maxh,
                                              int maxw, const int *ratios, int nratios, int agg, const int64_t *idx, float *flow);
int dfe_multiscale_census_flow_pair_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int maxh,
                                                 int maxw, const int *ratios, int nratios, int agg, float beta, float *flow,
                                                 int64_t *idx);
int dfe_multiscale_census_flow_pair_subpixel_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k,
                                                int maxh, int maxw, const int *ratios, int nratios, int agg, float beta, float *flow,
                                                int64_t *idx);

/* ---- N2: gradients of the two matchers (training drivers call model:backward through them) ------- */
/* replaces: nn.SpatialMatching:updateGradInput / nn.SpatialRadialMatching:updateGradInput (un-vendored nnx), reached
 *   from radial/train_radial_opticalflow.lua:228-252 and opticalflow.lua:296-338.  gradOut has the forward output's
 *   layout; gradIn1 / gradIn2 the inputs'.  Gather form (no atomics): every input element sums its own terms in
 *   (dy, dx) order. */
int dfe_spatial_matching_backward_f32(dfe_ctx *ctx, const float *in1, const float *in2, const float *gradOut, int K,
                                      int H1, int W1, int maxh, int maxw, float *gradIn1, float *gradIn2);
int dfe_radial_matching_backward_f32(dfe_ctx *ctx, const float *in1, const float *in2, const float *gradOut, int K,
                                     int H1, int W, int hWin, float *gradIn1, float *gradIn2);

/* ---- A6: arg-min / arg-max with the centre tie-break ---------------------- */
/* replaces: output:min(3) + centre override radial/radial_opticalflow_groundtruth.lua:88-94;
 *   input:max(3) + override in getOutputConfidences opticalflow_model.lua:153-161.
 * vol [P][N] -> idx [P] (1-based, first extremum wins, centre wins exact ties with the best),
 *   best [P] (may be NULL).  middle <= 0 disables the override. */
int dfe_argbest_center(dfe_ctx *ctx, const float *vol, int64_t P, int N, int middle, int take_max,
                       int64_t *idx, float *best);

/* ---- A7 / A8: extractoutput.* --------------------------------------------- */
/* replaces: extractoutput.extractOutput(input, scores, threshold, imaxs)
 *   extract_output.cpp:63-155 (Lua registration :357-366); same argument order.
 * input [H][W][N] f32; imaxs [H][W] int64, scores [H][W] f32.  Pixels with no value
 * above threshold are left untouched, as in the reference. */
int dfe_extract_output(dfe_ctx *ctx, const float *input, int H, int W, int N, float *scores,
                       double threshold, int64_t *imaxs);
/* replaces: extractoutput.extractOutputMarginalized(input, threshold, threshold_acc, ret, retgd)
 *   extract_output.cpp:157-255.  retgd is zeroed first (:166). */
int dfe_extract_output_marginalized(dfe_ctx *ctx, const float *input, int H, int W, int N,
                                    double threshold, double threshold_acc, int64_t *ret,
                                    int64_t *retgd);

/* ---- A9 / A10: class id -> displacement ----------------------------------- */
/* replaces: x2yx + centered2onebased opticalflow_model.lua:16-34,209-213;
 *   radial/radial_opticalflow_groundtruth.lua:97-100. */
int dfe_x2yx(dfe_ctx *ctx, const int64_t *idx, int64_t P, int maxh, int maxw, int64_t *y,
             int64_t *x);
/* replaces: x2yxMulti2(geometry, LongTensor) opticalflow_model_multiscale.lua:72-81 (body
 *   x2yxMulti2.c:1-95).  compat_c = 0: the Lua scalar semantics x2yxMultiNumber :83-132 that the
 *   reference's round-trip test pins (tests/test_multiscale.lua:57-80); compat_c = 1: the shipped C
 *   body bug for bug (ids it never matches leave y/x untouched). ratios are the Lua table values
 *   ratios[1..n]. Returns DFE_E_ARG if an id is outside 1..nclasses (compat_c = 0 only; the device
 *   flag is read back, so this call synchronises). */
int dfe_x2yx_multi(dfe_ctx *ctx, int maxh, int maxw, const int *ratios, int nratios,
                   const int64_t *idx, int64_t P, int64_t *y, int64_t *x, int compat_c);
/* The ring layout: scale s >= 1 contributes the blocks top, left, right, bottom of its window, of width
 *   d = round(maxw (r_s - r_{s-1}) / (2 r_s)) on BOTH axes (:296); the side blocks have maxh - 2 d rows.  Every entry
 *   that uses the layout -- the three below, dfe_x2yx_multi, dfe_cascade_ring_f32, dfe_cascade_flow_f32 and the one-call
 *   pyramid matchers -- rejects maxh < 2 d (DFE_E_SHAPE; -1 from the two that return an id or a count).  maxh == 2 d
 *   (empty side blocks) is accepted, which the reference's nn.Narrow is not. */
/* host-side scalar codec (no device work): yx2xMulti :10-52, x2yxMultiNumber :83-132 */
int64_t dfe_yx2x_multi(int maxh, int maxw, const int *ratios, int nratios, double y, double x);
int dfe_x2yx_multi_number(int maxh, int maxw, const int *ratios, int nratios, int64_t id,
                          int64_t *y, int64_t *x);
int64_t dfe_multi_nclasses(int maxh, int maxw, const int *ratios, int nratios);

/* ---- dense single-scale flow in one call (A0+A1+A6+A7+A9; the volume lives only in ctx scratch) --- */
/* replaces: compute_cartesian_groundtruth_cross_correlation radial/radial_opticalflow_groundtruth.lua:66-112
 *   up to (not including) the pad-back :108.
 * Outputs, all [Ho][Wo]: idx = arg-min class with centre tie-break (:88-94), flow_y/flow_x
 *   decoded displacement (:97-100), scores/imaxs = extractOutput(cost, thr) (:105; pixels with
 *   nothing above thr keep the caller's values), best = min cost.  Any output may be NULL. */
int dfe_ssd_flow_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int kh,
                     int kw, int hWin, int wWin, double extract_threshold, int64_t *idx,
                     float *best, float *flow_y, float *flow_x, float *scores, int64_t *imaxs);

/* ---- A6+A7+A9 in one pass over an existing volume (rows x Wo pixels, hWin*wWin cells) ------- */
/* replaces: radial/radial_opticalflow_groundtruth.lua:87-105 (min(3), centre tie-break, decode,
 *   extractOutput) and the pad-back of :108 for the float planes: fy/fx (and scores when
 *   scores_padded != 0) are written at [(row_off+y+pad_t)*pitch + x+pad_l]; idx/best/imaxs (and
 *   scores when scores_padded == 0) at [(row_off+y)*Wo + x].  Any output may be NULL; scores and
 *   imaxs of pixels with nothing above the threshold are left untouched. */
int dfe_flow_tail(dfe_ctx *ctx, const float *vol, int rows, int Wo, int hWin, int wWin,
                  double threshold, int row_off, int64_t *idx, float *best, float *fy, float *fx,
                  float *scores, int64_t *imaxs, int pitch, int pad_t, int pad_l, int scores_padded);

/* ---- A12: flow -> depth ----------------------------------------------------------------- */
/* replaces: the inline-C `radial(geometry, flow, mh, mw)` of test_opticalflow.lua:143-216.
 * flow [2][H][W] (plane 0 = y, plane 1 = x); (cx,cy) = focus of expansion = (mw,mh); infty = W/2.
 * depth = min(|p-c|/|flow|, infty) where |flow| >= 0.2 else infty; conf as shipped uses
 * px*dx + dy*dy (:181); fix_dot != 0 selects px*dx + py*dy. */
int dfe_flow_to_depth_cartesian(dfe_ctx *ctx, const float *flow, int H, int W, float cx, float cy,
                                int fix_dot, float *depth, float *conf);

/* ---- the one-call single-scale pipeline: frames -> flow + confidence + depth ------------- */
/* replaces: the per-frame body of the dense drivers (depth_estimation_opticalflow.lua:113-116 +
 *   test_opticalflow.lua:349-355 flow -> depth) for the single-scale raw-patch matcher.
 * flow [2][H][W], scores [H][W], depth [H][W], depth_conf [H][W]: full-frame, zero outside the
 * centre-pasted Ho x Wo region (opticalflow_model.lua:227-249).  The cost volume is materialised
 * in ctx scratch (bands of output rows within dfe_set_scratch_limit) by dfe_ssd_cost_volume_f32's kernel and consumed by dfe_flow_tail. */
int dfe_flow_depth_pair_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W,
                            int k, int hWin, int wWin, float foe_x, float foe_y,
                            double extract_threshold, float *flow, float *scores, float *depth,
                            float *depth_conf);

/* ---- A2: one pyramid scale on raw frames ------------------------------------------------- */
/* replaces: per-ratio branch of getMultiscalePrefilter + matcher opticalflow_model_multiscale.lua:134-173,196-229
 *   (raw-patch identity filter): box down-sample by r, zero-pad by hPatch2-1 = (maxh-1)+(kh-1) split
 *   floor/ceil, crop frame 0 by maxw-1, SpatialMatching(maxh,maxw).  out [H/r][W/r][maxh][maxw] at native
 *   scale (the x r nearest-neighbour upsampling is applied by the consumer's indexing). */
int dfe_downsample_box_f32(dfe_ctx *ctx, const float *img, int C, int H, int W, int r, float *out);
int dfe_pyramid_scale_volume_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W,
                                 int r, int kh, int kw, int maxh, int maxw, float *out);

/* ---- A3: nn.Minus -> nn.SoftMax over the window cells ------------------------------------ */
/* replaces: cascad_preproc opticalflow_model_multiscale.lua:270-279.  cost, prob [P][N]. */
int dfe_softmin_f32(dfe_ctx *ctx, const float *cost, int64_t P, int N, float *prob);

/* ---- A4: nn.CascadingAddTable:updateOutput ------------------------------------------------ */
/* replaces: CascadingAddTable.lua:108-135.  in[s], out[s]: [P][maxh][maxw] for each of the nratios
 *   scales (arrays of device pointers on the HOST).  out[n-1] = in[n-1];
 *   out[i] = in[i] + replicate(crop(out[i+1])).  DFE_E_SHAPE with the reference's message when ratios
 *   and window size are not compatible (:121-124). */
int dfe_cascading_add_f32(dfe_ctx *ctx, const float *const *in, const int *ratios, int nratios,
                          int64_t P, int maxh, int maxw, float *const *out);

/* ---- A4 + A5 + A6 + A10 fused: cascade -> arg-max -> displacement --------------------------------- */
/* replaces: cascad + middle remover + getOutputConfidences (no threshold) + x2yxMulti of processOutput
 *   (opticalflow_model_multiscale.lua:281-333, opticalflow_model.lua:153-161,205-208) in one pass: the joined
 *   [H][W][nclasses] tensor is never materialised.  prob[s] [H/r_s][W/r_s][maxh][maxw] as for dfe_cascade_ring_f32;
 *   idx [H][W] 1-based class id (first maximum, centre tie-break), best [H][W] its value, flow_y / flow_x [H][W]
 *   the decoded displacement in finest-scale pixels; each output may be NULL (flow_y and flow_x together).
 *   Bit-identical to dfe_cascade_ring_f32 -> dfe_argbest_center(take_max) -> dfe_x2yx_multi. */
int dfe_cascade_flow_f32(dfe_ctx *ctx, const float *const *prob, const int *ratios, int nratios, int H, int W,
                         int maxh, int maxw, int64_t *idx, float *best, float *flow_y, float *flow_x);

/* ---- A2..A6 + A10 in one call: the multiscale matcher of a frame pair ------------------------------ */
/* replaces: getModelMultiscale(geometry, true, false):forward({I0, I1}) + processOutput ('max', no threshold) for
 *   the identity patch filter -- opticalflow_model_multiscale.lua:175-333, opticalflow_model.lua:201-226.
 *   I0, I1 [C][H][W] with H, W multiples of every ratio (the caller pads, :234-248).  Per scale: box down-sample,
 *   zero-pad, k x k raw-patch SSD over a maxh x maxw window, softmin; then the fused cascade / ring / arg-max /
 *   decode.  flow [2][H][W] (plane 0 = y, 1 = x, finest-scale pixels) and / or idx [H][W] (1-based class id). */
int dfe_multiscale_flow_pair_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k,
                                 int maxh, int maxw, const int *ratios, int nratios, float *flow, int64_t *idx);

/* dfe_multiscale_flow_pair_f32 with every scale's cost volume stored as IEEE half (BASELINE configs[4]: "5-level pyramid, fp16
 * cost volume"; SURVEY 8(d): the 4K 5-level volumes are 1.6 GB in fp32).  The SSD sums are fp32; a volume holds
 * half(cost * scale), round to nearest even, and the cascade works on float(stored) * (1 / scale) in fp32 registers: soft-min,
 * cascade adds and arg-max are fp32 as in the f32 entry.  The result is that of the fp32 chain run on volumes rounded to half
 * precision (11 significant bits) where they are stored.  scale: 1 for frames in [0, 1] (and up to a few units), 2^-8 for
 * uint8-valued frames (147 * 255^2 overflows half).  8 x 8 windows with ratios 1, 2, 4, ... (C = 3, k = 7) write and read real
 * half volumes; any other shape builds fp32 volumes and rounds them in place -- the same values. */
int dfe_multiscale_flow_pair_f16(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k,
                                 int maxh, int maxw, const int *ratios, int nratios, float scale, float *flow, int64_t *idx);

/* ---- A2..A6 + A10 + A15 in one call: the multiscale matcher with its LEARNED patch filters ------------------------------- */
/* One layer of getFilter(geometry) (opticalflow_model.lua:45-79): nn.SpatialConvolution(nIn, nOut, kW, kH), or
 * nn.SpatialConvolutionMap over a connection table when conn != NULL, followed by nn.Tanh when tanh_after (getFilter puts
 * one behind every layer but the last).  All pointers are DEVICE pointers.
 * A stack of them is an array in layer order, and every entry that takes one checks it by the same rule: each layer has weight != NULL
 * and kH, kW, nIn, nOut > 0 (else DFE_E_ARG); layers[0].nIn == C, the frames' planes; a later layer has nIn == nOut of the layer before
 * it, or with a connection table nIn <= that nOut -- the table can name no plane the layer before does not make (else DFE_E_SHAPE). */
typedef struct dfe_filter_layer {
    int nIn, nOut, kH, kW;
    const float *weight;   /* [nOut][nIn][kH][kW]; with conn: [nConn][kH][kW] */
    const float *bias;     /* [nOut] or NULL */
    const int32_t *conn;   /* SpatialConvolutionMap: [nConn][2] = (from, to), 1-based int32; NULL = full connection */
    int nConn;
    int tanh_after;
} dfe_filter_layer;
/* replaces: getModelMultiscale(geometry, true, false):forward({I0, I1}) + processOutput ('max', no threshold) with
 *   getFilter(geometry) in front of every scale's nn.SpatialMatching -- opticalflow_model_multiscale.lua:175-333 (the filter
 *   branches :196-211, shared or cloned per scale :219-226), equivalently getMultiscalePrefilter (:134-173) followed by the
 *   prefiltered model: the per-scale computation is the same.  Per scale r: box down-sample by r, zero-pad by hPatch2-1 =
 *   (maxh-1)+(hKernel-1) split floor/ceil (hKernel = sum kH - (nlayers-1), the stack's receptive field: opticalflow.lua:154-189),
 *   frame 0 cropped by maxh-1 / maxw-1 (:198-202), the filter stack on both, SpatialMatching(maxh, maxw) on the K-plane
 *   features, soft-min; then cascade / ring / arg-max / decode as in dfe_multiscale_flow_pair_f32.
 *   layers: HOST array [share_filters ? 1 : nratios][nlayers] (scale-major); share_filters != 0: one stack for every scale
 *   (geometry.share_filters).  I0, I1 [C][H][W], C = layers[0].nIn, H and W multiples of every ratio.
 *   f16_scale != 0: volumes rounded to half precision where they are stored (see dfe_multiscale_flow_pair_f16). */
int dfe_multiscale_flow_pair_filtered_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int maxh, int maxw,
                                          const int *ratios, int nratios, const dfe_filter_layer *layers, int nlayers,
                                          int share_filters, float f16_scale, float *flow, int64_t *idx);

/* ---- the single-scale trained model in one call: A15 + A1 + A3 + A6/A7 + A9 + A11 ------------------------------------------- */
/* replaces: what depth_estimation_opticalflow.lua:66-116 (and depth_estimation_api.lua:164-168, test_opticalflow.lua:347-355) run per
 *   frame pair for a model that is not multiscale --
 *     filter:forward(frame) of both frames          getFilter(geometry), opticalflow_model.lua:45-79
 *     prepareInput(geometry, last_im, im)           :131-151: patch 1 narrowed to rows ceil(maxh/2) .. (H - maxh + 1 of them), columns alike
 *     model:forward(input)                          getModel(geometry, true, true), :81-129: SpatialMatching(maxh, maxw) -> Minus -> SoftMax over the window
 *     processOutput(geometry, moutput, true, thr)   :201-252: without threshold the first maximum with the centre tie-break (:153-161), confidences 1;
 *                                                   with one extractoutput.extractOutput(p, scores, 0.11, imaxs) and confidences = scores > thr (:163-167);
 *                                                   y, x = x2yx(index) - centered2onebased(0, 0); both pasted at floor((hImg - h) / 2), floor((wImg - w) / 2)
 *   I0, I1 [C][H][W] frames; layers: HOST array of the filter stack (C = layers[0].nIn).  nlayers == 0: I0 / I1 ARE the feature maps
 *   (geometry.prefilter: the caller keeps each frame's features for the next pair, as the script does) and patch 1's narrow is taken as a
 *   view of I0, no copy.  The output region is H1 x W1 = (H - hKernel + 1 - maxh + 1) x (W - wKernel + 1 - maxw + 1).
 *   Outputs (each may be NULL): full [2][hImg][wImg] (plane 0 = y, plane 1 = x; zero outside the pasted region), full_conf [hImg][wImg],
 *   index [H1][W1] int64 1-based class ids, scores [H1][W1] extractOutput's score (0 without threshold).  Pixels where no probability
 *   exceeds 0.11 -- imaxs / scores uninitialised in the reference -- get index = the centre class and score 0.
 *   16- / 17-wide windows on maps at least 253 columns wide never write the volume (the matcher's soft-max epilogue); other shapes go
 *   through the stand-alone ops.  Either way the results equal the module path's (getModel():forward + processOutput) bit for bit.
 *   The one-kernel form needs the planes of patch 1 below 2^29 floats (prefilter: H W < 2^29); beyond, the stand-alone ops materialise the
 *   volume (H1 W1 maxh maxw floats, twice) and the call fails with DFE_E_ALLOC where that does not fit the device. */
int dfe_flow_pair_filtered_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, const dfe_filter_layer *layers, int nlayers,
                               int maxh, int maxw, int use_threshold, double threshold, int hImg, int wImg, float *full, float *full_conf,
                               int64_t *index, float *scores);
/* replaces: the same per-pair step for a model built with geometry.output_extraction_method = 'mean' (depth_estimation_api.lua:25-31,
 *   164-182; test_opticalflow.lua:347-353): getModel's SpatialMatching -> Minus -> SoftMax, then processOutput's 'mean' branch
 *   (opticalflow_model.lua:171-199, 218-226) --
 *     y, x        the probability-weighted mean cell of the window, 1-based (OutputExtractor), minus centered2onebased(0, 0): sub-pixel flow
 *     confidence  extractOutput(m, scores, 0.11, imaxs) on the window's row marginals m_r = sum_c p[r][c], then scores > 0 -- i.e. 1 where
 *                 some m_r exceeds 0.11, else 0
 *     index       yx2x(floor(y + 0.5), floor(x + 0.5)) of the uncentred y, x (fp32), int64
 *   Frames, layers, nlayers (0: I0 / I1 are the feature maps, patch 1's narrow a view) and the output region as dfe_flow_pair_filtered_f32.
 *   Outputs (each may be NULL, not all): full [2][hImg][wImg] (plane 0 = y, plane 1 = x, floats; zero outside the pasted region),
 *   full_conf [hImg][wImg], index [H1][W1].  There is no threshold (processOutput's 'mean' branch ignores it).
 *   16- / 17-wide windows on maps at least 253 columns wide never write the volume (the matcher's soft-arg-max epilogue); other shapes go
 *   through the stand-alone ops (dfe_output_extractor_f32, dfe_marginal_sum_f32, dfe_extract_output).  Either way the results equal the
 *   module path's (getModel():forward up to the soft-max + processOutput) bit for bit. */
int dfe_flow_pair_filtered_mean_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, const dfe_filter_layer *layers,
                                    int nlayers, int maxh, int maxw, int hImg, int wImg, float *full, float *full_conf, int64_t *index);
/* replaces: nn.SpatialMatching(maxh, maxw, false):forward({patch1, patch2}) where patch1 is the NARROW of a larger map
 *   (prepareInput, opticalflow_model.lua:147-149: `patch1:narrow(2, ..):narrow(3, ..)` is a view; nnx made it contiguous inside the
 *   module): in1 is read in place, rows in1_pitch floats apart and planes in1_plane floats apart.  Same output as dfe_spatial_matching_f32. */
int dfe_spatial_matching_strided_f32(dfe_ctx *ctx, const float *in1, int in1_pitch, int64_t in1_plane, const float *in2, int K, int H1, int W1,
                                     int maxh, int maxw, float *out);

/* ---- A4b: nn.CascadingAddTable:updateGradInput --------------------------------------------- */
/* replaces: CascadingAddTable.lua:137-154 (HEAD's graph has no trainable parameters in it: Mul2 / Power are
 *   commented out, :29,46,57 -- accGradParameters is a no-op).  gradOut[s], gradIn[s]: [P][maxh][maxw];
 *   g_0 = gradOut_0, g_{i+1} = gradOut_{i+1} + zero-pad(q x q block sums of g_i), gradIn_i = g_i. */
int dfe_cascading_add_backward_f32(dfe_ctx *ctx, const float *const *gradOut, const int *ratios, int nratios,
                                   int64_t P, int maxh, int maxw, float *const *gradIn);

/* ---- A2(upsample)+A4+A5: cascade and ring extraction for a whole frame --------------------- */
/* replaces: nearest upsampling of SpatialPyramid + CascadingAddTable + the "middle remover" +
 *   JoinTable(2) + SmartReshape(hImg,wImg,-2), opticalflow_model_multiscale.lua:227-229,285-333.
 *   prob[s] [H/r_s][W/r_s][maxh][maxw] (native scale).  out [H][W][nclasses]. */
int dfe_cascade_ring_f32(dfe_ctx *ctx, const float *const *prob, const int *ratios, int nratios,
                         int H, int W, int maxh, int maxw, float *out);

/* ---- A13 / A14: polar grids and bilinear warp ------------------------------------------------ */
/* replaces: getC2PMask radial/cartesian2polar.lua:4-49.  mask [2][hdst][wdst+lpadding+rpadding].  rmax > 0 and alpha > 0, as for
 *   the P2C grid (else DFE_E_ARG, nothing is written): alpha < 0 makes row 0 pow(0, alpha) * sin(0) = inf * 0 = NaN coordinates. */
int dfe_polar_grid_c2p_f32(dfe_ctx *ctx, int wsrc, int hsrc, int wdst, int hdst, float xcenter,
                           float ycenter, int lpadding, int rpadding, float rmax, float alpha,
                           float *mask);
/* replaces: getP2CMask radial/cartesian2polar.lua:51-89.  mask [2][hdst][wdst].  rmax is a double: the reference computes
 *   ky = hsrc / rmax^(1/alpha) in Lua numbers (:59) and getP2CMaskOF hands it a scaled, non-integer radius (polar.lua:25);
 *   only the finished ky becomes a float. */
int dfe_polar_grid_p2c_f32(dfe_ctx *ctx, int wsrc, int hsrc, int wdst, int hdst, float xcenter,
                           float ycenter, double rmax, float alpha, float *mask);
/* replaces: cartesian2polar(img, mask) = image.warp(img, mask, 'bilinear', false)
 *   radial/cartesian2polar.lua:91-93.  img [C][H][W], mask [2][Hd][Wd] (plane 0 = y, 1 = x, absolute,
 *   0-based), out [C][Hd][Wd]; coordinates outside the image are clamped, a NaN coordinate samples row / column 0. */
int dfe_warp_bilinear_f32(dfe_ctx *ctx, const float *img, int C, int H, int W, const float *mask,
                          int Hd, int Wd, float *out);

/* ---- A12(ii): radial flow -> depth --------------------------------------------------------- */
/* replaces: flow2depth radial/radial_opticalflow_display.lua:6-58.  rflow [H][W] scalar radial flow;
 *   depth = (d/f or infty)/infty where |p-c| > 10, conf = 0 inside that radius. */
int dfe_flow_to_depth_radial(dfe_ctx *ctx, const float *rflow, int H, int W, float xcenter,
                             float ycenter, float infty, float *depth, float *conf);

/* ---- A12(iii): x-flow -> depth of the drone API ----------------------------------------------- */
/* replaces: ARdroneAPI::computeDepthMapFromFlow ardrone/ardrone_api.cpp:99-140.  xflow, mask [H][W];
 *   mode filter of round(xflow) over the (sic) half-open 6x6 window [i-3,i+3) x [j-3,j+3) of pixels with non-zero
 *   mask (20 bins, values -8..11; samples outside are skipped -- the reference indexes its histogram unchecked),
 *   depth = imu_tx*|j-W/2|/|mode| (100 where |mode| < 1.1), conf = 1 where mask > 0.5 and j != W/2; elsewhere
 *   conf = 0 and depth = 0 (uninitialised in the reference). */
int dfe_flow_to_depth_ardrone(dfe_ctx *ctx, const float *xflow, const float *mask, int H, int W, float imu_tx,
                              float *depth, float *conf);

/* ---- A16: postProcessImage(input, mask, winsize, method) ------------------------------------ */
/* replaces: the inline-C `fmax` (mode) and `fmed` (median) filters and their Lua wrapper
 *   opticalflow_model.lua:323-472.  flow, out [2][H][W] (plane 0 = y, 1 = x), mask [H][W].
 *   method 0 = 'max': floor(flow+0.5), shift by the global minimum m, most frequent (vx,vy) of the masked
 *   k x k window (lowest code on ties), + m everywhere (the untouched border becomes m, as shipped :440);
 *   DFE_E_ARG when the rounded range exceeds the reference's 16 x 16 histogram.  method 1: per-component
 *   masked median tmp[n/2]; DFE_E_ARG when k*k > 32 (the reference's buffer).  Windows run over
 *   i < H-k, j < W-k as shipped.  Synchronises (method 0 reads the range back). */
int dfe_postprocess_image_f32(dfe_ctx *ctx, const float *flow, const float *mask, int H, int W,
                              int winsize, int method, float *out);

/* ---- A17: enlargeMask(mask, ix, iy), in place ------------------------------------------------- */
/* replaces: depth_estimation_api.lua:76-132. */
int dfe_enlarge_mask_f32(dfe_ctx *ctx, float *mask, int H, int W, int ix, int iy);

/* ---- A18: nn.OutputExtractor:updateOutput (soft arg-max) -------------------------------------- */
/* replaces: OutputExtractor.lua:21-35 (used by output_extraction_method = 'mean', opticalflow_model.lua:115-116).
 *   input [P][maxh*maxw] -> x [P] = sum p*j, y [P] = sum p*i with 1-based cell coordinates. */
int dfe_output_extractor_f32(dfe_ctx *ctx, const float *input, int64_t P, int maxh, int maxw,
                             float *x, float *y);

/* ---- A15 (next-row N1): the learned patch-feature stack -------------------------------------------- */
/* replaces: nn.SpatialConvolution / nn.SpatialConvolutionMap / nn.Tanh as used by getFilter
 *   (opticalflow_model.lua:45-79, radial/radial_opticalflow_network.lua:6-30): valid cross-correlation + bias,
 *   in [nIn][H][W] -> out [nOut][H-kH+1][W-kW+1]; weight [nOut][nIn][kH][kW] resp. one [kH][kW] kernel per
 *   connection of conn [nConn][2] = (from, to), 1-based, device int32; bias [nOut] or NULL.  Direct form, one thread
 *   per output, accumulation order (input plane | connection, ky, kx) -- correctness first, not tuned (this is where
 *   an implicit-GEMM MFMA kernel belongs). */
int dfe_spatial_convolution_f32(dfe_ctx *ctx, const float *in, const float *weight, const float *bias, int nIn, int nOut,
                                int H, int W, int kH, int kW, float *out);
/* replaces: nn.SpatialConvolution followed by nn.Tanh, as getFilter chains them (opticalflow_model.lua:48-64), in one launch; results equal
 *   dfe_spatial_convolution_f32 + dfe_tanh_f32 bit for bit. */
int dfe_spatial_convolution_tanh_f32(dfe_ctx *ctx, const float *in, const float *weight, const float *bias, int nIn, int nOut, int H, int W,
                                     int kH, int kW, float *out);
int dfe_spatial_convolution_map_f32(dfe_ctx *ctx, const float *in, const float *weight, const float *bias,
                                    const int32_t *conn, int nConn, int nIn, int nOut, int H, int W, int kH, int kW,
                                    float *out);
int dfe_tanh_f32(dfe_ctx *ctx, const float *in, int64_t n, float *out);
/* nn.SpatialContrastiveNormalization(nIn, kernel1d, threshold, thresval) (version2/network.lua:12, in front of both filter
 * branches): subtractive then divisive local normalisation with a separable 1-D kernel (k <= 33 taps, HOST pointer),
 * border-corrected by the estimator of a ones tensor.  Un-vendored nn, restated from recall: parity unpinned.
 * in / out [C][H][W]. */
int dfe_contrastive_normalization_f32(dfe_ctx *ctx, const float *in, int C, int H, int W, const float *kernel_host, int k,
                                      float threshold, float thresval, float *out);
/* ---- frames as the camera delivers them: uint8 planes ("upload frames as uint8, not fp32") ---------------------- */
/* dst[i] = float(src[i]) * scale (scale = 1: the integer values; 1/255: image.load's [0, 1] range). */
int dfe_u8_to_f32(dfe_ctx *ctx, const uint8_t *src, int64_t n, float scale, float *dst);
/* ---- sub-pixel flow for the single-scale step (NOT in the reference: its flow is the integer arg-min cell) -------------------- */
/* For an output pixel (y, x) with arg-min cell (r, s) -- the cell the step picks, centre tie-break included; decoded flow
 * dy = r - (hWin-1)/2, dx = s - (wWin-1)/2 -- cost(r', s') is the SSD of dfe_ssd_cost_volume_f32 for that pixel and cell (frame 0's
 * patch at (y + (hWin-1)/2, x + (wWin-1)/2), frame 1's at (y + r', x + s')).  Per axis (x shown; y alike with r -+ 1), in fp32:
 *   c0 = cost(r, s), cm = cost(r, s-1), cp = cost(r, s+1);
 *   off = 0 if s-1 < 0 or s+1 >= wWin (a neighbour outside the searched window);
 *   else den = (cm - c0) + (cp - c0); off = den > 0 ? clamp((cm - cp) / (2 den), -0.5, 0.5) : 0   (this order, IEEE division);
 *   fx = (float)dx + off_x, fy = (float)dy + off_y.
 * Costs are recomputed from the frames (C (kh kw + (kh+2)(kw+2)) reads per pixel); on byte-valued frames every cost is an integer
 * below 2^24, so the refined flow is exact and reproducible on the host.
 * dfe_flow_depth_pair_subpixel_f32 / _u8: the arguments and outputs of dfe_flow_depth_pair_f32 / _u8; the step runs unchanged, then
 *   its centre-pasted flow is refined in place and depth / depth_conf (NULL together, as there) are the step's per-pixel formula
 *   (dfe_flow_to_depth_cartesian, fix_dot = 0) on the refined flow.  The border stays zero; scores are the step's.
 * dfe_flow_refine_subpixel_f32: the refinement alone, from the 1-based idx [Ho][Wo] of dfe_ssd_flow_f32 (Ho = H - kh + 1 - hWin + 1,
 *   Wo = W - kw + 1 - wWin + 1); fy / fx written at [(y + pad_t) * pitch + x + pad_l] as dfe_flow_tail does.  Pixels whose idx is
 *   outside 1..hWin*wWin keep their fy / fx. */
int dfe_flow_depth_pair_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                                     float foe_x, float foe_y, double extract_threshold, float *flow, float *scores, float *depth,
                                     float *depth_conf);
int dfe_flow_depth_pair_subpixel_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin,
                                    float foe_x, float foe_y, double extract_threshold, float scale, float *flow, float *scores,
                                    float *depth, float *depth_conf);
int dfe_flow_refine_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int kh, int kw, int hWin,
                                 int wWin, const int64_t *idx, float *fy, float *fx, int pitch, int pad_t, int pad_l);
/* ---- forward-backward flow consistency: an occlusion mask (NOT in the reference) ------------------------------ */
/* fw, bw [2][H][W] (plane 0 = y, plane 1 = x: the layout of dfe_flow_depth_pair_f32's flow): fw maps frame 0 to frame 1, bw frame 1 to
 * frame 0.  The valid region R = rows y0 .. y0+Ho-1, columns x0 .. x0+Wo-1 must lie inside the frame (DFE_E_SHAPE); tol >= 0, not NaN
 * (DFE_E_ARG).  mask, err [H][W]; err may be NULL.  Per pixel p = (y, x), everything in fp32 without fused multiply-adds:
 *   p outside R: mask = 0, err = 0.
 *   q = p + fw(p).  A component of fw(p) not finite: mask = 0, err = +Inf (decided before any float -> int conversion of q).
 *   Reach: fy = floor(q.y), cy = ceil(q.y), fx = floor(q.x), cx = ceil(q.x) (an integral coordinate has floor = ceil).  One of the four
 *     taps (fy|cy, fx|cx) outside R: mask = 0, err = +Inf.  So a q exactly on R's last row or column is inside, a fraction beyond is not.
 *   b = bilinear sample of bw at q: wy = q.y - fy, wx = q.x - fx, uy = 1 - wy, ux = 1 - wx;
 *     b = (uy ux) bw(fy, fx) + (uy wx) bw(fy, cx) + (wy ux) bw(cy, fx) + (wy wx) bw(cy, cx), summed in this order from 0, where a tap
 *     with a factor that is exactly 0 is NOT read and adds nothing: an integral q reads one pixel, and a NaN under a zero weight does
 *     not poison the sum.  A component of b not finite: mask = 0, err = +Inf.
 *   Residual e = fw(p) + b; d2 = e.y e.y + e.x e.x; err = sqrtf(d2); mask = d2 <= tol tol ? 1 : 0 (the squares are compared: integer-valued
 *     flows give an exact mask).
 * One launch, one thread per pixel of the frame (the border zeros included).
 * dfe_flow_depth_pair_fb_f32 / _u8: the pair step in both directions and their consistency in one call.  With gate == 0, flow, scores,
 *   depth, depth_conf (same NULL rules) are bit-identical to dfe_flow_depth_pair_f32 / _u8 -- subpixel != 0: to the _subpixel_ forms;
 *   flow_bw [2][H][W] is the flow of that entry with I0 and I1 swapped (NULL: kept in the ctx's own scratch); mask (required) and err
 *   (may be NULL) are dfe_flow_consistency_f32(flow, flow_bw, H, W, pad_t, pad_l, Ho, Wo, tol) with R the step's centre-pasted region,
 *   Ho = H - k + 1 - hWin + 1, Wo alike, pad_t = (H - Ho) / 2, pad_l = (W - Wo) / 2.  gate != 0: scores and depth_conf (where given)
 *   are multiplied by mask inside R; flow and depth stay.  The backward direction makes its two flow planes only (no extractOutput,
 *   no depth); the _u8 form converts each frame once for both directions. */
int dfe_flow_consistency_f32(dfe_ctx *ctx, const float *fw, const float *bw, int H, int W, int y0, int x0, int Ho, int Wo, float tol,
                             float *mask, float *err);
int dfe_flow_depth_pair_fb_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int hWin, int wWin,
                               float foe_x, float foe_y, double extract_threshold, int subpixel, float tol, int gate, float *flow,
                               float *scores, float *depth, float *depth_conf, float *flow_bw, float *mask, float *err);
int dfe_flow_depth_pair_fb_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin,
                              float foe_x, float foe_y, double extract_threshold, float scale, int subpixel, float tol, int gate,
                              float *flow, float *scores, float *depth, float *depth_conf, float *flow_bw, float *mask, float *err);
/* ---- hole filling: a dense field from the confident pixels (NOT in the reference) ---------------------------- */
/* A confidence-weighted push-pull.  v, out [C][H][W], 1 <= C <= 4 (DFE_E_ARG); w [H][W]; filled [H][W], may be NULL; out may be v itself.
 * The region R = rows y0 .. y0+Ho-1, columns x0 .. x0+Wo-1 must lie inside the frame (DFE_E_SHAPE); levels >= 0 and no NULL tensor
 * (DFE_E_ARG).  Everything in fp32 without fused multiply-adds, sums taken from 0 in the stated order, IEEE division.
 *   Outside R: out = 0, filled = 0.  Every level below is a grid relative to R's origin.
 *   Level 0 (Ho x Wo): a0 = min(w, 1) where w is finite, w >= 1e-6f (the fp32 constant) and every channel of v is finite; else a0 = 0.
 *     Where a0 = 0 the value is never read into arithmetic: a NaN in a hole or under a zero weight does not leak.
 *   Levels: H_{l+1} = (H_l + 1) / 2, W alike; Lfull = the halvings until the grid is 1 x 1; L = Lfull if levels == 0, else
 *     min(levels, Lfull).
 *   Push, l = 0 .. L-1, per coarse cell (i, j): the children (2i + dy, 2j + dx) in the order (0,0) (0,1) (1,0) (1,1), those outside the
 *     level-l grid or with a = 0 skipped; s = sum a, n_c = sum a v_c.  s > 0: v_{l+1,c} = n_c / s, a_{l+1} = min(s, 1); else both 0.
 *   Top: f_L = v_L, g_L = (a_L > 0).
 *   Pull, l = L-1 .. 0, per level-l pixel (y, x): parent (i, j) = (y >> 1, x >> 1), i' = i + (y & 1 ? 1 : -1), j' alike; the taps
 *     (i, j) 9/16, (i, j') 3/16, (i', j) 3/16, (i', j') 1/16 in this order, those outside the level-(l+1) grid or with g = 0 skipped;
 *     S = sum t, U_c = sum t f_c.  S > 0: u_c = U_c / S, g_l = 1 and f_{l,c} = a_l v_{l,c} + (1 - a_l) u_c -- a_l == 1 copies v_{l,c}
 *     (a fully trusted pixel keeps its bits), a_l == 0 copies u_c (the value under it is not read).  S == 0: f = 0, g = 0 (only with
 *     a limited `levels`, or when nothing in R is valid).
 *   out = f_0, filled = g_0.
 * Launches: a push and a pull kernel per level, and from the first level whose pyramid fits LDS one workgroup's apex kernel for all
 * levels above (option "fill_apex"); both run the same per-cell code and give the same bits.  Pyramid levels live in the ctx's side
 * buffer: nothing is allocated per call once it has grown. */
int dfe_fill_holes_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, int y0, int x0, int Ho, int Wo, int levels,
                       float *out, float *filled);
/* ---- guided weighted median: outliers out, motion boundaries kept (NOT in the reference) --------------------- */
/* Per channel the lower weighted median of the k x k window, the weights from a confidence plane and, optionally, from a guide image.
 * v, out [C][H][W], 1 <= C <= 4; w [H][W] or NULL (all ones); guide [Cg][H][W], 0 <= Cg <= 4, or NULL / Cg = 0: no range term; k odd in
 * 1 .. 15; filtered [H][W] or NULL (DFE_E_ARG for each, and for v or out NULL).  The region R = rows y0 .. y0+Ho-1, columns
 * x0 .. x0+Wo-1 must be non-empty and lie inside the frame (DFE_E_SHAPE).  Neighbours are read: out and filtered must not overlap v, w,
 * guide or each other (DFE_E_ARG).  Asynchronous on the ctx's stream; allocates nothing.
 *   Validity (dfe_fill_holes_f32's rule): a(q) = min(w(q), 1) where w(q) is finite, w(q) >= 1e-6f (the fp32 constant) and every channel
 *     of v(q) is finite; else a(q) = 0.  With w == NULL, w(q) = 1.
 *   Range term, in fp32 without fused multiply-adds, no division and no exp on the device: with a guide and sigma > 0 the host forms
 *     inv_s2 = 1.0f / (sigma * sigma) in float; d2 = sum_c (g_c(p) - g_c(q))^2 in channel order starting from the first square;
 *     r = max(0, 1 - d2 * inv_s2); an r that is not finite counts as 0.  Without a guide, or with sigma <= 0 (or NaN): r = 1.
 *   Integer sample weight: wt(p, q) = (uint32)((a(q) * r) * 4096.0f + 0.5f), and wt(p, q) = 0 where a(q) = 0.  Everything behind this
 *     is integer arithmetic: the sums do not depend on their order and the result is exact whatever the kernel's schedule.
 *   Window: the k x k pixels centred on p, clipped to R -- samples outside R do not exist.
 *   Per pixel p of R: T = sum_q wt(p, q).  T == 0: out = 0 in every channel, filtered = 0.  Else filtered = 1 and, per channel
 *     separately, out_c(p) = the sample value v_c(q*) with the smallest key such that 2 S >= T, S = the sum of wt(p, q) over the samples
 *     whose key is at most that key: the LOWER weighted median.  Keys are the order-preserving integer image of the float's bits
 *     (u = bits; key = u with the sign bit set if it was clear, ~u if it was set), so -0 sorts below +0; the output's bits are those of
 *     an input sample.
 *   Outside R: out = 0, filtered = 0, written by the same launch.
 * Consequences: k = 1 copies v where wt > 0; unit weights and a full window give the plain median; a NaN or Inf under a = 0 never
 * leaks; a NaN in the guide at p gives T = 0.
 * One launch: a workgroup per 4 x 64 tile of the frame with its halo in LDS, a thread per pixel bisecting the key interval of its
 * window, all channels in one pass. */
int dfe_weighted_median_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *guide, int Cg, float sigma,
                            int k, int y0, int x0, int Ho, int Wo, float *out, float *filtered);
/* ---- guided upsampling: a field back at the camera's resolution, holes skipped, motion boundaries kept (NOT in the reference; DESIGN
 * section 4.28) -------------------------------------------------------------------------------------------------------------------- */
/* Joint bilateral upsampling (Kopf et al. 2007) with a confidence plane: each full-resolution pixel p takes the mean of the (2r)^2
 * low-resolution samples q around it, weighted by a tent in each axis, by the sample's confidence and by how much the full-resolution
 * frame at p looks like the low-resolution frame at q.
 * v [C][Hl][Wl], out [C][Hh][Wh], 1 <= C <= 4; w [Hl][Wl] or NULL (all ones); guide_hi [Cg][Hh][Wh] and guide_lo [Cg][Hl][Wl],
 * 0 <= Cg <= 4: both given when Cg > 0, both NULL when Cg = 0 (no range term); r in 1 .. 4; valid [Hh][Wh] or NULL; gain C finite HOST
 * floats or NULL (ones) -- DFE_E_ARG for each, and for v or out NULL.  Every size in 1 .. 32768 with Hl <= Hh and Wl <= Wh (it is an
 * upsampler; equal sizes are allowed), else DFE_E_SHAPE.  out and valid must not overlap an input or each other (DFE_E_ARG).
 * Asynchronous on the ctx's stream; allocates nothing.
 * Everything in fp32 without fused multiply-adds, the products rounded separately in the grouping written here, IEEE division.
 *   Validity (dfe_fill_holes_f32's rule): a(q) = min(w(q), 1) where w(q) is finite, w(q) >= 1e-6f (the fp32 constant) and every channel
 *     of v(q) is finite; else a(q) = 0, and v(q) is never read into arithmetic.
 *   Coordinates (dfe_image_scale_f32's mapping), per axis in exact int64 (x shown; y alike with Hl, Hh): num = (2 x + 1) Wl - Wh,
 *     den = 2 Wh; j0 = floor(num / den) (-1 for a negative num); the taps j = j0 - r + 1 .. j0 + r; n_j = r den - |num - j den|.  A tap
 *     with j outside [0, Wl) or with n_j = 0 does not exist: edge taps are dropped, not clamped, and the normalisation makes up for
 *     them.  tx_j = float32(double(n_j) / double(r den)): the tent 1 - |u - j| / r at u = num / den.
 *   Range term (dfe_weighted_median_f32's rule): with a guide and sigma > 0 the host forms inv_s2 = 1.0f / (sigma * sigma) in float;
 *     d2 = sum_c (guide_hi_c(p) - guide_lo_c(q))^2 in channel order starting from the first square; rr = max(0, 1 - d2 * inv_s2); an rr
 *     that is not finite counts as 0.  Without a guide, or with sigma <= 0 (or NaN): rr = 1.
 *   Sample weight: wt = (a(q) * rr) * (ty_i * tx_j).  A sample with a(q) = 0 or wt = 0 does not exist.
 *   Sums over the existing samples, rows ascending and columns ascending within a row, each started from its first term (not from 0:
 *     -0 survives): S = sum wt, N_c = sum wt * v_c(q).
 *   At least one sample: out_c(p) = gain_c * (N_c / S), valid(p) = 1.  None: out_c(p) = 0, valid(p) = 0.
 * Consequences: equal sizes, r = 1, no guide and w NULL give a bit copy times gain; r = 1 without guide or holes is
 * dfe_image_scale_f32's bilinear interpolation up to rounding (a dropped edge tap equals a clamped one); a NaN or Inf under a = 0 never
 * leaks; a NaN in guide_hi at p gives valid(p) = 0.  For a flow field gain = (Hh / Hl, Wh / Wl) keeps the vectors in pixels of the
 * grid they are on.
 * One launch: a workgroup per 8 x 64 tile of the output stages the tile's low-resolution footprint, at most (7 + 2r) x (63 + 2r)
 * samples, and the tents of its rows and columns in LDS; a thread per output pixel. */
int dfe_guided_upsample_f32(dfe_ctx *ctx, const float *v, int C, int Hl, int Wl, const float *w, const float *guide_hi,
                            const float *guide_lo, int Cg, float sigma, int r, const float *gain, int Hh, int Wh, float *out,
                            float *valid);
/* ---- temporal depth filter: a field carried along its own flow to the next frame's grid and fused with that frame's measurement (NOT
 * in the reference) ----------------------------------------------------------------------------------------- */
/* Forward warp with a z-buffer.  v, out [C][H][W], 1 <= C <= 4; w, wout [H][W]; flow [2][H][W], plane 0 = y, plane 1 = x (the layout of
 * every flow this library returns), from this grid to the next frame's; key [H][W] or NULL; gain, bias C finite HOST floats or NULL;
 * 0 < decay <= 1; src [H][W] or NULL; H W <= 2^31 - 1 (DFE_E_ARG for each, and for v, w, flow, out or wout NULL).  The region R = rows
 * y0 .. y0+Ho-1, columns x0 .. x0+Wo-1 must be non-empty and lie inside the frame (DFE_E_SHAPE).  The winners are gathered from v and w
 * while the outputs are written: out, wout and src must not overlap an input or each other (DFE_E_ARG).  Refused before any launch.
 * Asynchronous on the ctx's stream; the z-buffer (8 bytes per pixel of R) lives in the ctx's side buffer: nothing is allocated per call
 * once it has grown.  Everything in fp32 without fused multiply-adds.
 *   A sample exists (dfe_fill_holes_f32's rule) where w is finite, w >= 1e-6f (the fp32 constant) and every channel of v is finite.
 *     Unlike the other field operators the weight is NOT clipped at 1: here it counts observations.
 *   Sources: a pixel p = (y, x) of R whose sample exists, whose two flow components are finite and, with a key, whose key(p) is finite.
 *   Target of a source: q = (floorf((float(y) + f_y) + 0.5f), floorf((float(x) + f_x) + 0.5f)), each sum rounded to fp32 before the
 *     next (a fraction of .5 rounds up).  q is compared with R's bounds as floats, before any conversion to an integer; a source whose
 *     target lies outside R is dropped.
 *   Winner of a target: among its sources the one with the smallest key + 0.0f (-0 counts as +0); for equal keys, or key == NULL, the
 *     smallest source index s = y W + x.  The key is the occlusion rule: the caller passes depth, and the nearer surface covers the
 *     farther one.
 *   At a target q with winner s: out_c(q) = gain_c v_c(s) + bias_c, the product rounded, then the sum; a NULL gain or bias means no
 *     arithmetic for that term, and with both NULL the bits are copied.  wout(q) = w(s) if decay == 1, else w(s) decay: the raw weight,
 *     not clipped.  src(q) = s.
 *   At a target with no source, and everywhere outside R: out = 0, wout = 0, src = -1.
 * Launches: the z-buffer set to all-ones (a memset of the stream); the splat, a thread per pixel of R and one no-return 64-bit integer
 * minimum of (ordered key << 32 | s) on the target's word (the ordered key is the order-preserving integer image of the float's bits:
 * the sign bit flipped for non-negative values, every bit for negative ones) -- an integer minimum does not depend on the order of
 * arrival, so the result is reproducible bit for bit; the resolve, a thread per pixel of the frame. */
int dfe_forward_warp_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key, int y0,
                         int x0, int Ho, int Wo, const float *gain, const float *bias, float decay, float *out, float *wout,
                         int32_t *src);
/* Fusion of a propagated prior and a new measurement, pointwise.  prior, meas, out [C][H][W], 1 <= C <= 4; wp, wm, wout [H][W]; flag
 * [H][W] or NULL; tol >= 0 (not NaN); wmax finite and >= 1e-6 (DFE_E_ARG for each, and for another tensor NULL); the region as above
 * (DFE_E_SHAPE).  out may be prior or meas and wout may be wp or wm (a pixel is read before it is written; no other overlap).  One
 * launch, asynchronous on the ctx's stream; allocates nothing.  fp32 without fused multiply-adds, IEEE division.
 *   Per pixel of R: a = min(wp, wmax) where the prior's sample exists (the rule above), else 0; b alike from the measurement.  What lies
 *   under a zero weight is never read into arithmetic: a NaN in a hole does not leak.  With z the prior's values and m the measurement's:
 *     a = 0 and b = 0:  out = 0, wout = 0, flag = 0
 *     b = 0:            out = z (its bits), wout = a, flag = 1
 *     a = 0:            out = m (its bits), wout = b, flag = 2
 *     else d_c = z_c - m_c, d2 = sum_c d_c d_c in channel order starting from the first square, and
 *       d2 <= tol tol (the product formed in fp32 by the host), they agree:  s = a + b, r = a / s, out_c = m_c + r d_c (the mean of
 *                       the two weighted by the observations behind each), wout = min(s, wmax), flag = 3
 *       a > b:          the prior survives, weakened by the dissent: out = z (its bits), wout = a - b, flag = 4
 *       a <= b:         the measurement takes over: out = m (its bits), wout = b if a == b, else b - a, flag = 5
 *   Outside R: out = 0, wout = 0, flag = 0.
 * The squares are compared, so integer-valued fields with an integer tol give exact decisions.  A wout that falls below 1e-6 is a hole
 * to the next call by the sample rule: intended.  wmax is the forgetting: a prior never outweighs wmax observations.  The vote of the
 * last two rows removes isolated outliers without letting a wrong prior live forever. */
int dfe_temporal_fuse_f32(dfe_ctx *ctx, const float *prior, const float *wp, const float *meas, const float *wm, int C, int H, int W,
                          int y0, int x0, int Ho, int Wo, float tol, float wmax, float *out, float *wout, float *flag);
/* Both in one call: dfe_forward_warp_f32 of the state (v, w) along flow with key, gain, bias and decay, then dfe_temporal_fuse_f32 of
 * that prior with (meas, wm) -- the clear, the splat, and ONE resolve kernel that fuses in registers; the prior reaches memory only where
 * it is asked for (prior [C][H][W], wprior [H][W], src [H][W]: each may be NULL, as may flag).  Every output is bit-identical to the two
 * calls in a row.  Every bad argument is refused before any launch with the codes of the entries it joins; no output may overlap v, w,
 * flow, key or another output, and flag, prior, wprior, src may not overlap meas or wm (out may be meas, wout may be wm). */
int dfe_temporal_step_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key, int y0,
                          int x0, int Ho, int Wo, const float *gain, const float *bias, float decay, const float *meas, const float *wm,
                          float tol, float wmax, float *out, float *wout, float *flag, float *prior, float *wprior, int32_t *src);
/* Forward warp with a sub-pixel (four-tap, bilinear) splat on INTEGER accumulators: every source is spread over the
 * four pixels around where it lands, and a target is the weighted mean of what reached it.  The sums are integers, so they do not depend
 * on the order of arrival: reproducible bit for bit, like the nearest-pixel entry above.  v, w, flow, key, the region, gain, bias, decay,
 * out, wout, the sample rule, the sources, the overlap rule (out, wout, cover against the inputs and each other) and the error codes are
 * dfe_forward_warp_f32's; there is no src.  ztol finite and >= 0, quant finite and > 0, 0 <= min_cover <= 1 (DFE_E_ARG); cover [H][W] or
 * NULL.  fp32 without fused multiply-adds except for the integers.
 *   Position: py = float(y) + f_y, px = float(x) + f_x, each rounded to fp32; by = floorf(py), ay = py - by (exact); x alike.
 *   Tent weights on a grid of 1/128 per axis: uy1 = (int)floorf(ay * 128.0f + 0.5f), uy0 = 128 - uy1; x alike.  Tap (i, j), i, j in
 *     {0, 1}, targets (by + float(i), bx + float(j)) with the integer weight u = uy_i ux_j: the four sum to 16384 exactly (a partition of
 *     unity).  A tap with u == 0 does not exist.  A tap's target is compared with R's bounds as floats before any conversion; a tap
 *     outside R is dropped, the source's other taps stay.
 *   Fixed point: val_c = gain_c v_c + bias_c as above; V_c = (long long)rintf(val_c * quant); a source with any
 *     !(|val_c * quant| <= 16777216.0f) is dropped whole.  wd = w if decay == 1, else w * decay; Wf = (long long)rintf(fminf(wd, 256.0f)
 *     * 256.0f); a source with Wf == 0 is dropped whole.  A dropped source takes part in nothing below, the front included.
 *   Front (the occlusion rule): Z(q) = the minimum of key(s) + 0.0f over the taps that reach q, held as the order-preserving 32-bit
 *     integer image of the float (see above) and taken with an integer atomic minimum.  With key == NULL there is no front.
 *   Accumulate: a tap of source s contributes to q iff key == NULL or (key(s) + 0.0f) - Z(q) <= ztol (one rounded subtraction).  With
 *     omega = u Wf, three sums are kept in 64-bit integers by integer atomic adds: A_c(q) += omega V_c, B(q) += omega, U(q) += u.
 *     omega |V_c| <= 2^14 2^16 2^24 = 2^54: the result is defined while AT MOST 256 TAPS contribute to one target (|A_c| <= 2^62);
 *     beyond that the sums may wrap and the result is unspecified (never a fault).
 *   Resolve: a target exists iff B > 0 and U >= max(1, (int)ceilf(min_cover * 16384.0f)).  There out_c = ((float)A_c / (float)B) / quant
 *     (the conversions round to nearest even, the divisions are IEEE), wout = (float)B / (256.0f * (float)max(U, 16384)) and cover =
 *     (float)U / 16384.0f: an under-covered target carries proportionally fewer observations, an over-covered one the mean count, not
 *     the sum.  Everywhere else, and outside R: out = 0, wout = 0, cover = 0.
 * Consequences: an integer flow without collisions, values on the 1 / quant grid with |V_c| Wf < 2^24, weights on the 1 / 256 grid and
 * quant a power of two give dfe_forward_warp_f32's bits; a flow below half a pixel per frame moves the field (the nearest splat leaves
 * it where it is); the position is quantised to 1 / 128 px and the values to 1 / quant per step.
 * Launches: a clear of the accumulators ((C + 2) 64-bit words and one 32-bit front per pixel of R, in the ctx's side buffer: nothing is
 * allocated per call once it has grown); the front pass (skipped with key == NULL); the accumulate pass (option "splat_lds": the two
 * forms of both passes, the same bits); the resolve, a thread per pixel of the frame.  Asynchronous on the ctx's stream. */
int dfe_forward_splat_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key, int y0,
                          int x0, int Ho, int Wo, const float *gain, const float *bias, float decay, float ztol, float quant,
                          float min_cover, float *out, float *wout, float *cover);
/* dfe_temporal_step_f32 with dfe_forward_splat_f32 in place of the nearest warp: the clear, the front, the accumulate and ONE resolve
 * kernel that divides and fuses in registers (the fusion's own device function).  cover [H][W] in place of src; prior, wprior, cover and
 * flag may each be NULL.  Every output is bit-identical to dfe_forward_splat_f32 followed by dfe_temporal_fuse_f32; arguments, overlap
 * rules and error codes are those of the entries it joins. */
int dfe_temporal_step_splat_f32(dfe_ctx *ctx, const float *v, int C, int H, int W, const float *w, const float *flow, const float *key,
                                int y0, int x0, int Ho, int Wo, const float *gain, const float *bias, float decay, float ztol,
                                float quant, float min_cover, const float *meas, const float *wm, float tol, float wmax, float *out,
                                float *wout, float *flag, float *prior, float *wprior, float *cover);

/* replaces: image.rgb2y as prepareInput calls it (opticalflow_model.lua:136-138; un-vendored `image`, restated: parity unpinned).
 *   rgb [3][H][W] -> y [1][H][W] = 0.299 R + 0.587 G + 0.114 B, accumulated in that order with separately rounded products and sums. */
int dfe_rgb2y_f32(dfe_ctx *ctx, const float *rgb, int H, int W, float *y);
/* replaces: tensor:min(1) on an n x M view (tests/time_matching.lua:41-43: `output:min(1)` of the matcher's output behind
 *   nn.Reshape(wsize*wsize, ...)): val[m] = min_r in[r][m], idx[m] = the first r attaining it, 1-based; either may be NULL. */
int dfe_min_dim0_f32(dfe_ctx *ctx, const float *in, int n, int64_t M, float *val, int64_t *idx);
/* dfe_flow_depth_pair_f32 on uint8 frames [C][H][W]: float(frame) * scale is made on the device (one conversion pass into a per-ctx
 * buffer) and the fp32 pipeline runs on it -- results are bit-identical to the fp32 entry on the same values.  A quarter of the
 * host-to-device bytes. */
int dfe_flow_depth_pair_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int hWin, int wWin,
                           float foe_x, float foe_y, double extract_threshold, float scale, float *flow, float *scores, float *depth,
                           float *depth_conf);
/* dfe_multiscale_flow_pair_f32 (f16_scale == 0) or dfe_multiscale_flow_pair_f16 (f16_scale > 0: its `scale`) on uint8 frames: no
 * conversion pass -- the pyramid's preparation kernels, the only readers of the frames, take the bytes as they are (float(byte) * scale
 * at the load), so the results are bit-identical to the fp32 entries on the converted frames. */
int dfe_multiscale_flow_pair_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int maxh, int maxw,
                                const int *ratios, int nratios, float scale, float f16_scale, float *flow, int64_t *idx);
/* ---- sub-pixel flow for the raw-patch pyramid matcher (NOT in the reference: its flow is d * r for a whole cell d) --------------- */
/* For a pixel (y, x) with class id `id`: id decodes (x2yxMultiNumber, dfe_x2yx_multi) to a scale s with ratio r and a cell (a, b) of
 * that scale's maxh x maxw window; the integer displacement is ((a + 1 - chh) r, (b + 1 - chw) r), chh = (maxh + 1) / 2, chw alike.
 * cost(a', b') is the fp32 SSD of dfe_pyramid_scale_volume_f32 for scale s at the scale's pixel (y / r, x / r) and cell (a', b') --
 * the value that volume holds, inside the ring hole of a coarse scale too.  Per axis (x shown; y alike with a -+ 1), in fp32:
 *   c0 = cost(a, b), cm = cost(a, b-1), cp = cost(a, b+1);
 *   off = 0 if b-1 < 0 or b+1 >= maxw (a neighbour outside the window);
 *   else den = (cm - c0) + (cp - c0); off = den > 0 ? clamp((cm - cp) / (2 den), -0.5, 0.5) : 0   (the single-scale rule above);
 *   fx = (float)(dx r) + (float)r * off   (product and sum separately rounded).
 * The class id, and with it the integer flow, never changes; the refined flow is within r / 2 of it per axis.  The costs are fp32
 * sums over the prepared (down-sampled, zero-padded) scale frames, whatever form the matcher stored its volumes in: where every cost
 * of a frame pair is exactly representable in fp32 the result is defined bit for bit, else up to the rounding of the costs.
 * dfe_multiscale_flow_pair_subpixel_f32 / _u8: the arguments of dfe_multiscale_flow_pair_f32 / _u8; the matcher runs unchanged, then
 *   flow (required) is refined in place; idx (optional) is the matcher's.
 * dfe_multiscale_refine_subpixel_f32: the refinement alone, from any 1-based class map idx [H][W] (the staged path's
 *   dfe_cascade_flow_f32 / dfe_argbest_center, or another producer) into flow [2][H][W]; it prepares the padded scales itself.
 *   Pixels whose idx is not a class id keep what flow held. */
int dfe_multiscale_flow_pair_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int maxh, int maxw,
                                          const int *ratios, int nratios, float *flow, int64_t *idx);
int dfe_multiscale_flow_pair_subpixel_u8(dfe_ctx *ctx, const uint8_t *I0, const uint8_t *I1, int C, int H, int W, int k, int maxh,
                                         int maxw, const int *ratios, int nratios, float scale, float f16_scale, float *flow,
                                         int64_t *idx);
int dfe_multiscale_refine_subpixel_f32(dfe_ctx *ctx, const float *I0, const float *I1, int C, int H, int W, int k, int maxh, int maxw,
                                       const int *ratios, int nratios, const int64_t *idx, float *flow);
/* ---- pipelined ingest: the frame loop's host boundary --------------------------------------------------------------------------- */
/* replaces: the serial load -> filter -> match of depth_estimation_opticalflow.lua:66-150 (loader:getNextFrame, then the model) where
 *   frames arrive in HOST memory.  dfe_ingest_submit_u8 starts the upload of a uint8 frame pair (nbytes per frame; pinned host memory --
 *   dfe_host_alloc / dfe_host_register -- for a copy-engine transfer that runs beside the kernels) into one of the ctx's three device
 *   slots on the ctx's own copy stream and returns the slot; dfe_flow_depth_pair_u8_slot runs dfe_flow_depth_pair_u8's step on that
 *   slot's frames once they have landed (the compute stream waits for the slot's event; no host synchronisation).  Submit pair i+1, then
 *   compute pair i: the next pair travels while the kernels of this one run.  A slot comes round again with every third submit; the
 *   submit then waits ON THE HOST until the compute stream has consumed the slot's previous pair (two pairs back: in a loop that stays
 *   one pair ahead it never actually waits).  Outputs as dfe_flow_depth_pair_u8 (bit-identical), ready in ctx-stream order. */
int dfe_ingest_submit_u8(dfe_ctx *ctx, const uint8_t *hI0, const uint8_t *hI1, int64_t nbytes, int *slot);
int dfe_flow_depth_pair_u8_slot(dfe_ctx *ctx, int slot, int C, int H, int W, int k, int hWin, int wWin, float foe_x, float foe_y,
                                double extract_threshold, float scale, float *flow, float *scores, float *depth, float *depth_conf);


/* ---- version2/: the single-scale learned model as ONE call -------------------------------------------------------------------- */
/* replaces: version2/test.lua:40-53 on getNetwork(datap) of version2/network.lua:5-39 for one frame pair --
 *   network:forward({prev, cur}) = ParallelTable{ Sequential{SpatialContrastiveNormalization(C, gaussian1D(normalization_k)),
 *   SpatialPadding(-lWin, -tWin, -rWin, -bWin), conv stack}, Sequential{the same normalisation, the same conv stack (shared weights)} }
 *   -> SpatialMatching(hWin, wWin, false); then `output:min(3)`, idx - 1, yflow = floor(idx / wWin) - tWin, xflow = idx - yflow' * wWin - lWin
 *   with lWin = ceil(wWin/2) - 1, tWin = ceil(hWin/2) - 1 (test.lua:18-21).  The minimum is taken over the whole hWin x wWin window in
 *   index order (first minimum), which is what the decode that follows it assumes.
 *   prev, cur [C][H][W]; norm_kernel_host: the 1-D normalisation kernel (HOST, norm_k <= 33 taps); layers: HOST array of nlayers
 *   convolution layers (version2 puts no Tanh between them: tanh_after = 0; the struct's other fields as in getFilter).
 *   Outputs over the dense inference region H1 x W1 = (H - (hWin-1) - (hKernel-1)) x (W - (wWin-1) - (wKernel-1)):
 *   xflow, yflow [H1][W1] float (may be NULL), idx [H1][W1] int64 1-based as torch's min returns it (may be NULL),
 *   volume [H1][W1][hWin][wWin] (may be NULL: then it lives in the ctx scratch arena only). */
int dfe_version2_flow_pair_f32(dfe_ctx *ctx, const float *prev, const float *cur, int C, int H, int W, const float *norm_kernel_host,
                               int norm_k, float threshold, float thresval, const dfe_filter_layer *layers, int nlayers, int hWin,
                               int wWin, float *xflow, float *yflow, int64_t *idx, float *volume);
/* replaces: nn.SpatialMatching(maxh, maxw, false) followed by `output:min(3)` and the index -> displacement decode, as
 *   version2/test.lua:45-51 and tests/time_matching.lua:18,41-43 run them on feature maps (in1 [K][H1][W1], in2 [K][H1+maxh-1][W1+maxw-1]):
 *   idx [H1][W1] int64 1-based first minimum of the window (index order), yflow = floor((idx-1) / maxw) - (ceil(maxh/2) - 1),
 *   xflow = (idx-1) mod maxw - (ceil(maxw/2) - 1); any of the three may be NULL.  The volume is never written where the flat-tile
 *   matcher takes the shape (16- / 17-wide windows on maps at least 253 columns wide); the results are those of
 *   dfe_spatial_matching_f32 + the first minimum, bit for bit. */
int dfe_spatial_matching_argmin_f32(dfe_ctx *ctx, const float *in1, const float *in2, int K, int H1, int W1, int maxh, int maxw,
                                    int64_t *idx, float *xflow, float *yflow);
/* nn.SpatialConvolution [+ nn.Tanh] as an implicit GEMM on the matrix cores (v_mfma_f32_16x16x4_f32: f32 in, f32
 * accumulate, an fmaf chain in the reference's (input plane, ky, kx) order).  Same layouts as dfe_spatial_convolution_f32;
 * results differ from it by the fusing of each multiply-add only (<= 1e-5 relative to sum |terms|).  kH x kW up to what
 * fits one block's LDS (17 x 17 does); DFE_E_UNSUPPORTED beyond. */
int dfe_spatial_convolution_mfma_f32(dfe_ctx *ctx, const float *in, const float *weight, const float *bias, int nIn, int nOut,
                                     int H, int W, int kH, int kW, int tanh_after, float *out);

/* ---- next-row N2: gradients of the filter stack and of the soft-max / log layers, so that network:backward(input, df_do)
 *      reaches the convolution weights through the drop-in (radial/train_radial_opticalflow.lua:228-252,
 *      opticalflow.lua:296-338).  The modules are un-vendored nn; pinned by the finite-difference Jacobian of the
 *      forward (the method of tests/test_cascad.lua:21-25). ------------------------------------------------------ */
/* nn.SpatialConvolution:updateGradInput: gradIn[i][y][x] = sum_o sum_u sum_v w[o][i][u][v] gradOut[o][y-u][x-v];
 * gradOut [nOut][H-kH+1][W-kW+1], gradIn [nIn][H][W]. */
int dfe_spatial_convolution_grad_input_f32(dfe_ctx *ctx, const float *gradOut, const float *weight, int nIn, int nOut, int H,
                                           int W, int kH, int kW, float *gradIn);
/* nn.SpatialConvolution:accGradParameters(input, gradOutput, scale): gradWeight[o][i][u][v] += scale * sum_{y,x}
 * gradOut[o][y][x] in[i][y+u][x+v]; gradBias[o] += scale * sum gradOut[o] (gradBias may be NULL).  ACCUMULATES (zero the
 * buffers first, as zeroGradParameters does); shared between the two filter branches like the reference's clone(). */
int dfe_spatial_convolution_acc_grad_f32(dfe_ctx *ctx, const float *in, const float *gradOut, int nIn, int nOut, int H, int W,
                                         int kH, int kW, float scale, float *gradWeight, float *gradBias);
/* the same for nn.SpatialConvolutionMap (weight / gradWeight [nConn][kH][kW], conn [nConn][2] (from, to) 1-based, device int32) */
int dfe_spatial_convolution_map_grad_input_f32(dfe_ctx *ctx, const float *gradOut, const float *weight, const int32_t *conn,
                                               int nConn, int nIn, int nOut, int H, int W, int kH, int kW, float *gradIn);
int dfe_spatial_convolution_map_acc_grad_f32(dfe_ctx *ctx, const float *in, const float *gradOut, const int32_t *conn, int nConn,
                                             int nIn, int nOut, int H, int W, int kH, int kW, float scale, float *gradWeight,
                                             float *gradBias);
/* nn.Tanh:updateGradInput from the module's OUTPUT: gradIn = gradOut * (1 - out^2) */
int dfe_tanh_backward_f32(dfe_ctx *ctx, const float *out, const float *gradOut, int64_t n, float *gradIn);
/* nn.Log2 (Log.lua:13-28): forward clamps the INPUT in place to >= null_epsilon when clamp != 0 (:15-18), out = log(input);
 * backward gradIn = gradOut / input (the clamped one). */
int dfe_log2_forward_f32(dfe_ctx *ctx, float *input, int64_t n, float null_epsilon, int clamp, float *out);
int dfe_log2_backward_f32(dfe_ctx *ctx, const float *input, const float *gradOut, int64_t n, float *gradIn);
/* nn.LogSoftMax over rows [P][N] (radial/radial_opticalflow_network.lua:50) and its gradient gradIn = gradOut -
 * exp(out) * sum(gradOut); nn.SoftMax's gradient gradIn = out * (gradOut - sum(gradOut * out)) for the window soft-max
 * of getModel (opticalflow_model.lua:96-109; forward = dfe_softmin_f32 on the un-negated costs). */
int dfe_log_softmax_f32(dfe_ctx *ctx, const float *in, int64_t P, int N, float *out);
int dfe_log_softmax_backward_f32(dfe_ctx *ctx, const float *out, const float *gradOut, int64_t P, int N, float *gradIn);
int dfe_softmax_backward_f32(dfe_ctx *ctx, const float *out, const float *gradOut, int64_t P, int N, float *gradIn);

/* ---- A11 ('mean' extraction): marginal of the window over its columns --------------------------- */
/* replaces: input:reshape(H,W,maxh,maxw):sum(4) in getOutputConfidences2, opticalflow_model.lua:192.
 *   in [P][A][B] -> out [P][A], double accumulator as in TH. */
int dfe_marginal_sum_f32(dfe_ctx *ctx, const float *in, int64_t P, int A, int B, float *out);

/* ---- next-row N4: ego-motion rectification and the epipole / focus of expansion, the step in front of the polar warp
 *      (radial/radial_opticalflow_data.lua:211-231, depth_estimation_api.lua:139-147).  The reference calls the
 *      un-vendored, OpenCV-backed `sfm2`; restated from the calling convention -- parity unpinned. ---------------- */
/* e2 = K T / (K T)_3 * scale (data.lua:218-220: scale = networkp.wImg / calibrationp.wImg).  K row-major 3 x 3, T 3, host. */
int dfe_epipole(const double *K9, const double *T3, double scale, double *e2_xy);
/* sfm2.removeEgoMotion(img, K, R, 'bilinear') -> warped, mask: out(p) = bilinear(img, K R K^-1 p) (inverse != 0: R^T),
 * mask(p) = 1 where the source lies inside the frame, else 0 (and out = 0).  img / out [C][H][W], mask [H][W] or NULL;
 * K, R row-major host doubles.  The homography is formed in double; entries below the rounding error of their own sum of products
 * (16 eps x the sum of the absolute products) are set to 0 before it is rounded to float32, so that R = I gives the identity map. */
int dfe_remove_ego_motion_f32(dfe_ctx *ctx, const float *img, int C, int H, int W, const double *K9, const double *R9,
                              int inverse, float *out, float *mask);
/* sfm2.undistortImage(img, K, distP): inverse-map undistortion with the (k1, k2, p1, p2, k3) model of the .cal files (no skew:
 * fx, fy, cx, cy of K are used). */
int dfe_undistort_image_f32(dfe_ctx *ctx, const float *img, int C, int H, int W, const double *K9, const double *dist5,
                            float *out);
/* NOT IN THE REFERENCE: an estimator of this library for the pure-translation case (the reference obtains the focus of expansion
 * as the epipole K T of sfm2.getEgoMotion2's pose: dfe_ego_motion_from_*_f32 + dfe_epipole below are that route).
 * Focus of expansion of a dense flow field (flow_y, flow_x [H][W]; conf [H][W] or NULL: pixels with conf <= 0 or a NaN conf,
 * with |flow| < min_flow, and vectors of non-finite or zero length are skipped): least-squares intersection of the flow lines,
 * `iterations` Huber re-weightings (0..16).
 * foe_xy = (x, y) in pixels (host); n_used (may be NULL) = sum of the weights.  DFE_E_ARG when the lines are parallel. */
int dfe_foe_from_flow_f32(dfe_ctx *ctx, const float *flow_y, const float *flow_x, const float *conf, int H, int W,
                          float min_flow, int iterations, double *foe_xy, double *n_used);

/* ---- N4, the core: relative pose of the two frames from correspondences ------------------------------------------------------
 * replaces: sfm2.getEgoMotion2{im1, im2, K, maxPoints, pointsQuality, ransacMaxDist, pointsMinDistance} -> R, T, nFound, nInliers,
 *   fundmat (radial/radial_opticalflow_data.lua:211-217, radial/test_radial_opticalflow.lua:122-126; sfm2.getEgoMotion at
 *   depth_estimation_api.lua:141).  sfm2 (un-vendored, OpenCV) finds and tracks sparse corners itself; here the correspondences
 *   are an INPUT: pts1 / pts2 [N][2] = (x, y) pixel positions in the previous / current frame (device floats; weights [N] or NULL:
 *   entries <= 0 are skipped), or samples of the dense flow the matcher has produced (_from_flow: p2 = p1 + flow(p1) on a centred
 *   regular grid of at most max_points samples, conf <= 0 and non-finite flow skipped).  `iterations` 8-point RANSAC hypotheses are
 *   built -- each from 8 draws among the VALID correspondences only, so sparse weights cost no draws -- and scored
 *   in parallel on the device (Sampson distance <= ransac_max_dist pixels), the best is refitted over its inliers, projected onto
 *   the essential manifold and decomposed; cheirality picks among the four (R, T).  Restated from the calling convention: parity
 *   unpinned (3P).  Outputs (host doubles): R9 row-major, T3 (|T| = 1) with x2 ~ R x1 + T for camera coordinates of frame 1 in
 *   frame 2 -- so K T is the epipole in the current frame (data.lua:218) and dfe_remove_ego_motion_f32(prev, K, R, inverse = 1) undoes
 *   the rotation --, F9 = K^-T [T]x R K^-1 with unit Frobenius norm (may be NULL), n_found = usable samples, n_inliers.
 *   Deterministic for a given seed.  Synchronises.  DFE_E_ARG when no hypothesis reaches 8 inliers. */
int dfe_ego_motion_from_points_f32(dfe_ctx *ctx, const float *pts1, const float *pts2, const float *weights, int N, const double *K9,
                                   double ransac_max_dist, int iterations, unsigned seed, double *R9, double *T3, int *n_inliers,
                                   double *F9);
int dfe_ego_motion_from_flow_f32(dfe_ctx *ctx, const float *flow_y, const float *flow_x, const float *conf, int H, int W,
                                 const double *K9, int max_points, double ransac_max_dist, int iterations, unsigned seed, double *R9,
                                 double *T3, int *n_found, int *n_inliers, double *F9);

/* ---- N4, the step in front of the pose: corner detection and pyramidal Lucas-Kanade tracking, so that the pose can start from two
 *      IMAGES as sfm2.getEgoMotion{im1, im2, K, maxPoints, pointsQuality, pointsMinDistance} does (radial/radial_opticalflow_data.lua:
 *      211-217, depth_estimation_api.lua:141, test_opticalflow.lua:282, groundtruth_opticalflow.lua:283, version2/data.lua:96).  sfm2 is
 *      un-vendored (OpenCV behind it): parity is unpinned; this is the library's own tracker, every stage defined in DESIGN section 4
 *      and tested on its own against a float64 reference written from those definitions. -------------------------------------------- */
/* parameters of the corner selection and the tracker; the .cal files' sfm table carries max_points, points_quality, points_min_dist
 * and tracker_win_size */
typedef struct dfe_tracker_params {
    int max_points;        /* corners kept, 1..4096 */
    float quality;         /* a corner needs response >= quality * the frame's largest response, 0..1 */
    float min_dist;        /* kept corners are pairwise more than this many pixels apart, >= 1 */
    int win;               /* tracking window, odd, 3..31 */
    int levels;            /* pyramid levels, 1..8 (1: the frame only) */
    int max_iters;         /* Gauss-Newton steps per level, 1..64 */
    float eps;             /* a level stops after a step shorter than this, >= 0 */
    float min_eig;         /* a window whose structure tensor's smaller eigenvalue / win^2 is below this is not tracked */
    float max_err;         /* > 0: points whose mean absolute residual exceeds this are lost */
} dfe_tracker_params;
/* Corner response: gx(y, x) = (Y(y, x+1) - Y(y, x-1)) / 2 and gy likewise, indices clamped to the frame; a = sum gx^2, b = sum gx gy,
 * c = sum gy^2 over the 3 x 3 block around the pixel (clamped indices); resp = ((a + c) - sqrt((a - c)^2 + 4 b^2)) / 2, the smaller
 * eigenvalue.  Y, resp [H][W]. */
int dfe_corner_response_f32(dfe_ctx *ctx, const float *Y, int H, int W, float *resp);
/* Corner selection on a response map [H][W] (H, W <= 32768).  M = the largest response (NaNs ignored); none when M <= 0.  A pixel is
 * a candidate iff resp > 0 and resp >= quality * M (one float32 product); it is kept iff no other pixel within
 * dx^2 + dy^2 <= floor(min_dist^2) has a larger response, or an equal one at a smaller linear index y W + x (NaN never dominates).
 * The kept points, sorted by (response descending, linear index ascending) and cut to the first max_points, go to pts [n][2] = (x, y)
 * (device floats, capacity max_points) and resp_out [n] (or NULL); n_out (host) = n.  The result does not depend on scheduling.
 * 1 <= min_dist, 1 <= max_points <= 4096, 0 <= quality <= 1, else DFE_E_ARG.  Synchronises. */
int dfe_select_corners_f32(dfe_ctx *ctx, const float *resp, int H, int W, float quality, float min_dist, int max_points, float *pts,
                           float *resp_out, int *n_out);
/* One pyramid step: out [(H+1)/2][(W+1)/2], out(y, x) = sum_{i,j=-2..2} w_i w_j in(rho(2y+i, H), rho(2x+j, W)), w = (1,4,6,4,1)/16,
 * rho the reflection about the first and the last sample (-1 -> 1, n -> n-2; n = 1: always 0). */
int dfe_pyr_down_f32(dfe_ctx *ctx, const float *in, int H, int W, float *out);
/* Pyramidal Lucas-Kanade (DESIGN section 4 has the definition step by step).  Y0, Y1 [H][W]; pts0 / pts1 [N][2] = (x, y) device
 * floats; status [N] int32 (1 = tracked); err [N] (or NULL) = mean |residual| of the last evaluation at level 0.  Uses win, levels,
 * max_iters, eps, min_eig, max_err of params.  A point is lost when its level-0 window is weaker than min_eig, when pts1 leaves
 * [0, W-1] x [0, H-1], when the point or its displacement is not finite, or when max_err > 0 and err > max_err; lost points keep
 * pts1 = pts0 and err = 0.  The same call gives the same bits.  N = 0 does nothing. */
int dfe_track_points_lk_f32(dfe_ctx *ctx, const float *Y0, const float *Y1, int H, int W, const float *pts0, int N,
                            const dfe_tracker_params *params, float *pts1, int *status, float *err);
/* sfm2.getEgoMotion{im1, im2, K, ...} in one call: im0 / im1 [C][H][W], C = 3 (dfe_rgb2y_f32 first) or 1; response and corners of
 * frame 0, tracked into frame 1, then dfe_ego_motion_from_points_f32 with the status as the weights (same outputs, same conventions).
 * n_found = tracked corners.  pts0_out / pts1_out [max_points][2], status_out [max_points] (device; each may be NULL) receive the
 * first n_corners (host int, may be NULL) entries.  DFE_E_ARG when fewer than 8 corners are found or tracked.  Synchronises. */
int dfe_ego_motion_from_images_f32(dfe_ctx *ctx, const float *im0, const float *im1, int C, int H, int W, const double *K9,
                                   const dfe_tracker_params *params, double ransac_max_dist, int iterations, unsigned seed, double *R9,
                                   double *T3, int *n_found, int *n_inliers, double *F9, float *pts0_out, float *pts1_out,
                                   int *status_out, int *n_corners);

/* ---- video to depth in one session: nextFrameDepth() of depth_estimation_api.lua:134-198 (the loop of test_opticalflow.lua:276-367) --- */
/* image.scale(src, width, height), bilinear: src [C][Hs][Ws] -> dst [C][Hd][Wd] (depth_estimation_api.lua:71,144,
 * test_opticalflow.lua:278,283).  `image` is un-vendored: this is the library's own definition, parity unpinned.
 * Per axis (x shown; y alike with Hs, Hd), in exact int64 arithmetic: num = (2 x + 1) Ws - Wd, den = 2 Wd.  num < 0: i0 = 0, w = 0.
 * Otherwise i0 = num / den (integer division), w = float32(double(num % den) / double(den)).  i1 = min(i0 + 1, Ws - 1); if
 * i0 >= Ws - 1 then i0 = Ws - 1 and w = 0.  (Pixel centres at half-integers, edge clamp, no anti-aliasing: the mapping of
 * torch.nn.functional.interpolate(mode = "bilinear", align_corners = False).)  Value, in fp32: top = a + wx (b - a), bot alike on the row
 * below, out = top + wy (bot - top); a weight of exactly 0 takes the first operand as it is (no arithmetic on it).
 * Consequences: equal sizes give a bit copy; a 2 x reduction of integer-valued frames is the exact 2 x 2 mean.
 * _u8: the source is first converted as dfe_u8_to_f32 does, float(src) * scale, then the same arithmetic.
 * Every size 1 .. 32768, else DFE_E_ARG. */
int dfe_image_scale_f32(dfe_ctx *ctx, const float *src, int C, int Hs, int Ws, int Hd, int Wd, float *dst);
int dfe_image_scale_u8(dfe_ctx *ctx, const uint8_t *src, float scale, int C, int Hs, int Ws, int Hd, int Wd, float *dst);
/* replaces: depth_estimation_api.lua:176-182 -- mask2 = zeros(H, W); mask2:narrow(..):narrow(..):copy(mask); mask2:cmul(conf).
 * out [H][W] = 0, and out(y + oy, x + ox) = mask(y, x) conf(y + oy, x + ox) for mask [Hm][Wm]; conf [H][W].  out may be conf itself,
 * not mask.  DFE_E_ARG when the pasted region leaves [0, H) x [0, W). */
int dfe_mask_paste_mul_f32(dfe_ctx *ctx, const float *mask, int Hm, int Wm, const float *conf, int H, int W, int oy, int ox, float *out);

/* The stream: one object that carries what nextFrameDepth() keeps from frame to frame -- the previous undistorted frame, the previous
 * scaled frame and the previous frame's features -- and runs the whole step per camera frame. */
typedef struct dfe_stream dfe_stream;
typedef struct dfe_stream_params {
    int C, Hsrc, Wsrc;     /* the camera frame [C][Hsrc][Wsrc], C = 1 or 3 */
    int hImg, wImg;        /* geometry.hImg / wImg: the size the model works at */
    double K[9];           /* row-major, of the camera frame */
    int has_dist;          /* 0: no undistortion (the gopro branch, test_opticalflow.lua:279) */
    double dist[5];        /* (k1, k2, p1, p2, k3) */
    const dfe_filter_layer *layers;   /* HOST array, copied by dfe_stream_create; the device weights stay the caller's */
    int nlayers;           /* 0: the scaled frames are the features */
    int maxh, maxw;        /* the search window */
    int extraction;        /* 0 'max', 1 'max' with extractOutput + threshold, 2 'mean' */
    double threshold;
    int rectify;           /* 0 FEATURES: the previous features are warped (depth_estimation_api.lua:147);
                              1 IMAGE: the previous scaled image is warped, then filtered (test_opticalflow.lua:284) */
    int fix_mask_offset;   /* 0: the mask is pasted where the reference pastes it, one pixel up and left of the centre; 1: at the centre */
    dfe_tracker_params tracker;
    double ransac_max_dist;
    int iterations;
    unsigned seed;
    double min_inlier_ratio;   /* bad image below it; 0.2 in the reference (depth_estimation_api.lua:159) */
} dfe_stream_params;
/* Host only, no ctx: checks the parameters and returns the shapes they imply (each pointer may be NULL) --
 *   Hf, Wf   the feature maps, hImg - hKernel + 1 etc. (hKernel = sum kH - (nlayers - 1))
 *   H1, W1   the matcher's output region, Hf - maxh + 1 etc.
 *   oy, ox   where the rectification mask is pasted into [hImg][wImg].  FEATURES: floor((hImg - Hf) / 2) - 1 -- the reference hands a
 *            0-based offset to the 1-based narrow (depth_estimation_api.lua:177-179) -- or floor((hImg - Hf) / 2) with fix_mask_offset;
 *            a negative offset (Hf == hImg without the fix: an error in Lua too) is DFE_E_ARG.  IMAGE: 0.
 *   ix, iy   enlargeMask's arguments, ceil((wImg - W1) / 2) and ceil((hImg - H1) / 2) (:172-174)
 * DFE_E_SHAPE when the window does not fit the feature map; dfe_last_error(NULL) has the text. */
int dfe_stream_shapes(const dfe_stream_params *p, int *Hf, int *Wf, int *H1, int *W1, int *oy, int *ox, int *ix, int *iy);
/* Allocates every buffer the stream needs (pushes allocate nothing of their own; the ctx's arena settles during the first pair). */
int dfe_stream_create(dfe_ctx *ctx, const dfe_stream_params *p, dfe_stream **out);
/* One camera frame (device [C][Hsrc][Wsrc]; _u8: converted as dfe_u8_to_f32 does).  In the reference's order: undistort (:139, if
 * has_dist); dfe_ego_motion_from_images_f32(previous, current, K) (:141); dfe_image_scale to wImg x hImg (:144); with
 * K_small = diag(wImg / Wsrc, hImg / Hsrc, 1) K (the reference's Khalf) dfe_remove_ego_motion_f32(previous features, K_small, R,
 * inverse = 1) -> features, mask [Hf][Wf] (:147) -- IMAGE: the previous scaled image instead, mask [hImg][wImg], then the filter stack --;
 * the filter stack on the scaled frame (:149); dfe_flow_pair_filtered_f32 / _mean_f32 with nlayers = 0 on the two feature maps (:164-168);
 * dfe_enlarge_mask_f32(mask, ix, iy) (:172-174); dfe_mask_paste_mul_f32 with full_confidences (:176-182); the current frame, scaled
 * frame and features become the previous ones (:187-189).  Each result equals that composition of the public entries bit for bit.
 * Device outputs (each may be NULL): im_scaled [C][hImg][wImg]; flow [2][hImg][wImg], plane 0 = y, plane 1 = x; mask [hImg][wImg];
 * depth, depth_conf [hImg][wImg] = dfe_flow_to_depth_ardrone(plane 1, mask, imu_tx), computed when either is given.
 * Host outputs (each may be NULL): R9, T3, n_found, n_inliers as dfe_ego_motion_from_images_f32; status --
 *   0  the first frame (after create or reset): the state is primed, only im_scaled is written
 *   1  a result
 *   2  bad image (:159-162): n_inliers / n_found < min_inlier_ratio, or the pose step found or tracked fewer than 8 corners.  flow, mask,
 *      depth and depth_conf are zero (at hImg x wImg; the reference sizes them by the camera frame), R9 / T3 are not written in the
 *      second case, the return code is 0 and the state advances as after a result.
 * Any other error leaves the state as it was.  Synchronises (the pose is needed on the host). */
int dfe_stream_push_f32(dfe_stream *s, const float *frame, float imu_tx, float *im_scaled, float *flow, float *mask, float *depth,
                        float *depth_conf, double *R9, double *T3, int *n_found, int *n_inliers, int *status);
int dfe_stream_push_u8(dfe_stream *s, const uint8_t *frame, float scale, float imu_tx, float *im_scaled, float *flow, float *mask,
                       float *depth, float *depth_conf, double *R9, double *T3, int *n_found, int *n_inliers, int *status);
/* forgets the previous frame: the next push returns status 0 (a post stream, below, also forgets its temporal state) */
int dfe_stream_reset(dfe_stream *s);
/* (before its ctx is destroyed) */
void dfe_stream_destroy(dfe_stream *s);

/* ---- the session's post-processing chain: consistency, fill, median and temporal fusion behind the pair step (NOT in the reference;
 * DESIGN section 4.39).  dfe_stream_params, dfe_stream_create and dfe_stream_push_* above stay as they are; a stream made by
 * dfe_stream_create_post also takes dfe_stream_push_post_*.  Both structs begin with their own size, so a later version can grow them:
 * a struct_size other than sizeof is DFE_E_ARG. */
typedef struct dfe_stream_post {
    int struct_size;           /* sizeof(dfe_stream_post) */
    float consistency_tol;     /* > 0: the forward-backward check with this tol; 0: off; negative or NaN: DFE_E_ARG */
    int fill;                  /* 0 / 1: dfe_fill_holes_f32 */
    int fill_levels;           /* its `levels` (>= 0) */
    int median_k;              /* 0: off; odd 1 .. 15: dfe_weighted_median_f32's k */
    float median_sigma;        /* its sigma; <= 0: unguided */
    int temporal;              /* 0 / 1: the temporal depth filter (temporal.py's TemporalFilter on the one depth channel, key_channel 0).
                                  The members below are read only with temporal == 1 */
    float t_tol, t_wmax, t_decay;   /* tol >= 0; wmax finite and >= 1e-6; decay in (0, 1] */
    int t_has_gain;            /* 0 / 1: depth' = t_gain depth + t_bias from one grid to the next, each term only where it is given */
    float t_gain;
    int t_has_bias;
    float t_bias;
    int t_splat;               /* 0 nearest (dfe_forward_warp_f32), 1 bilinear (dfe_forward_splat_f32, with the three members below) */
    float t_ztol, t_quant, t_min_cover;   /* t_splat == 1: ztol finite and >= 0, quant finite and > 0, 0 <= min_cover <= 1 */
} dfe_stream_post;
typedef struct dfe_stream_post_out {   /* device pointers, each may be NULL */
    int struct_size;           /* sizeof(dfe_stream_post_out) */
    float *flow_bw;            /* [2][hImg][wImg]  (consistency on, else not written) */
    float *consistent;         /* [hImg][wImg]     (consistency on, else not written) */
    float *flow_post;          /* [2][hImg][wImg] */
    float *weight_post;        /* [hImg][wImg] */
    float *depth_post;         /* [hImg][wImg] */
    float *depth_post_conf;    /* [hImg][wImg] */
    float *depth_fused;        /* [hImg][wImg]     (temporal on, else not written) */
    float *fused_weight;       /* [hImg][wImg]     (temporal on, else not written) */
    float *fused_flag;         /* [hImg][wImg]     (temporal on, else not written) */
} dfe_stream_post_out;
/* Host only, no ctx (as dfe_stream_shapes): checks p as dfe_stream_shapes does (its codes, DFE_E_SHAPE included), then every member of
 * post (DFE_E_ARG); dfe_last_error(NULL) has the text. */
int dfe_stream_post_check(const dfe_stream_params *p, const dfe_stream_post *post);
/* dfe_stream_create with the chain's options: every buffer the chain needs, the temporal state included, lies in the stream's own block
 * (pushes allocate nothing of their own). */
int dfe_stream_create_post(dfe_ctx *ctx, const dfe_stream_params *p, const dfe_stream_post *post, dfe_stream **out);
/* dfe_stream_push_f32 / _u8 with the chain behind it.  The plain outputs (im_scaled .. status) are bit-identical to the plain push
 * whatever the options.  The chain runs on a push with status 1, after the plain steps; each stage is the public entry named, so every
 * post output equals the composition of those entries bit for bit.  With
 *   R      the matcher's region (floor((hImg - H1) / 2), floor((wImg - W1) / 2), H1, W1) of dfe_stream_shapes,
 *   prevf  the rectified previous features the forward matcher read, cur the current features,
 *   guide  dfe_remove_ego_motion_f32(previous scaled frame, C, hImg, wImg, K_small, Rot, inverse = 1) -- IMAGE mode: the frame the session
 *          rectified anyway; FEATURES mode: one more warp (feature grid and image grid share K_small, as in the reference, so the two
 *          are aligned to within the filter's crop):
 * 1. consistency (consistency_tol > 0): flow_bw = the session's matcher entry on (cur, prevf), flow planes only (extraction 0, 1:
 *    dfe_flow_pair_filtered_f32 with the stream's threshold; 2: _mean_f32); consistent = dfe_flow_consistency_f32(flow, flow_bw, hImg,
 *    wImg, R, tol); kept = (mask > 0 ? 1 : 0) consistent.  Without the stage kept = (mask > 0 ? 1 : 0).  mask is the push's own output.
 * 2. fill: dense, filled = dfe_fill_holes_f32(flow, 2, .., kept, R, fill_levels); w = kept > 0 ? filled : 0.25f filled.
 * 3. median (median_k): med, valid = dfe_weighted_median_f32(src, 2, .., w, guide, C, median_sigma, median_k, R), with src, w = dense and
 *    the w of stage 2 when fill is on, else flow and kept.
 * 4. flow_post = med, else dense, else flow; weight_post = valid, else filled, else mask consistent (one rounded product; without the
 *    consistency stage no factor is applied: with nothing enabled weight_post has mask's bits).  depth_post, depth_post_conf =
 *    dfe_flow_to_depth_ardrone(flow_post plane 1, weight_post, imu_tx), computed when a depth output of the chain is asked for or temporal
 *    is on.
 * 5. temporal: TemporalFilter.push(depth_post[None], depth_post_conf, flow_post, rectify = (K_small, Rot)) of temporal.py with the state in
 *    the stream.  The first result after a create, a reset or a bad image: dfe_temporal_fuse_f32 against a zero prior.  After that:
 *    dfe_forward_warp_f32 (t_splat 1: dfe_forward_splat_f32) of the state and its weight along the STORED flow, keyed on the state, with
 *    gain, bias and decay; dfe_remove_ego_motion_f32 of the two planes (prior, weight), which lie next to each other; the weight times
 *    the warp's mask (one rounded product); dfe_temporal_fuse_f32 over the whole frame with (depth_post, depth_post_conf).  The result
 *    and flow_post become the state.  The stage runs on every status-1 push of dfe_stream_push_post_*, whatever outputs were asked for.
 * post_out may be NULL (the state still advances).  Status 0 writes no post output.  Status 2 zeroes every post output that was given
 * and resets the temporal state.  Any error leaves the stream and the temporal state as they were.
 * dfe_stream_push_f32 / _u8 on a post stream return the plain result and reset the temporal state: the pair's post-processed depth was
 * not computed, so there is nothing to carry.  dfe_stream_push_post_* on a stream of dfe_stream_create is DFE_E_ARG. */
int dfe_stream_push_post_f32(dfe_stream *s, const float *frame, float imu_tx, float *im_scaled, float *flow, float *mask, float *depth,
                             float *depth_conf, const dfe_stream_post_out *post_out, double *R9, double *T3, int *n_found,
                             int *n_inliers, int *status);
int dfe_stream_push_post_u8(dfe_stream *s, const uint8_t *frame, float scale, float imu_tx, float *im_scaled, float *flow, float *mask,
                            float *depth, float *depth_conf, const dfe_stream_post_out *post_out, double *R9, double *T3, int *n_found,
                            int *n_inliers, int *status);

#ifdef __cplusplus
}
#endif
#endif
