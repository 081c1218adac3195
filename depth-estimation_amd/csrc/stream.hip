// stream.hip -- video to depth in one session: nextFrameDepth() of depth_estimation_api.lua:134-198, the one entry point an outside
// program calls per camera frame (ardrone/ardrone_api.cpp:77-84), and the same loop of test_opticalflow.lua:276-367.  The stream object
// holds what the loop carries from frame to frame -- the previous undistorted frame (last_im), the previous scaled frame (last_im_scaled)
// and the previous frame's features (last_filtered) -- in two slots each that swap roles per push, and runs the public entries in the
// reference's order on them: every result equals the composition of those entries bit for bit.  All device memory is one block made by
// dfe_stream_create; a push allocates nothing of its own.
// A stream made by dfe_stream_create_post also carries the post-processing chain of stream_post.hip (consistency, fill, median, temporal
// fusion), run behind the pair step by dfe_stream_push_post_*.
// Also here: dfe_mask_paste_mul_f32, the mask2:narrow():copy(mask) + cmul(full_confidences) of :176-182 in one launch.
#include "stream_post.h"
#include <cmath>
#include <cstring>
#include <new>

namespace {

// out = 0 outside the pasted region, mask * conf inside it; one thread per pixel of out
__global__ __launch_bounds__(256) void mask_paste_mul_kernel(const float *__restrict__ mask, int Hm, int Wm, const float *conf, int H, int W, int oy, int ox,
                                                             float *out) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int my = y - oy, mx = x - ox;
    const long long e = (long long)y * W + x;
    out[e] = (my >= 0 && my < Hm && mx >= 0 && mx < Wm) ? mask[(long long)my * Wm + mx] * conf[e] : 0.f;
}

struct StreamShapes { int Hf, Wf, H1, W1, oy, ox, ix, iy, K, maxplanes; };

// the checks of dfe_stream_shapes; ctx may be NULL (the text then goes where dfe_last_error(NULL) reads it)
int stream_shapes(dfe_ctx *ctx, const char *fn, const dfe_stream_params *p, StreamShapes *o) {
    DFE_REQUIRE(ctx, p, DFE_E_ARG, "%s: params is NULL", fn);
    DFE_REQUIRE(ctx, (p->C == 1 || p->C == 3) && p->Hsrc >= 1 && p->Hsrc <= 32768 && p->Wsrc >= 1 && p->Wsrc <= 32768 && p->hImg >= 1 && p->hImg <= 32768 &&
                         p->wImg >= 1 && p->wImg <= 32768, DFE_E_ARG, "%s: C=%d (1 or 3), frame %dx%d, geometry %dx%d (every size 1..32768)", fn, p->C, p->Hsrc,
                p->Wsrc, p->hImg, p->wImg);
    DFE_REQUIRE(ctx, p->nlayers >= 0 && p->nlayers <= 8 && (p->nlayers == 0 || p->layers) && p->maxh > 0 && p->maxw > 0 && p->extraction >= 0 && p->extraction <= 2 &&
                         (p->rectify == 0 || p->rectify == 1), DFE_E_ARG, "%s: %d layers (0..8), window %dx%d, extraction %d (0..2), rectify %d (0, 1)", fn,
                p->nlayers, p->maxh, p->maxw, p->extraction, p->rectify);
    DFE_REQUIRE(ctx, p->min_inlier_ratio == p->min_inlier_ratio, DFE_E_ARG, "%s: min_inlier_ratio is NaN", fn);
    DfeStackGeom sg;
    int rc = dfe_filter_stack_geom(ctx, fn, p->layers, p->nlayers, p->C, &sg);
    if (rc) return rc;
    o->K = sg.K; o->maxplanes = sg.maxplanes;
    o->Hf = p->hImg - sg.hk + 1; o->Wf = p->wImg - sg.wk + 1;
    o->H1 = o->Hf - p->maxh + 1; o->W1 = o->Wf - p->maxw + 1;
    DFE_REQUIRE(ctx, o->H1 > 0 && o->W1 > 0, DFE_E_SHAPE, "%s: geometry %dx%d too small for window %dx%d behind a %dx%d filter", fn, p->hImg, p->wImg, p->maxh, p->maxw,
                sg.hk, sg.wk);
    o->ix = (p->wImg - o->W1 + 1) / 2; o->iy = (p->hImg - o->H1 + 1) / 2;           // math.ceil(( .. ) / 2)
    if (p->rectify == 1) o->oy = o->ox = 0;
    else {
        // mask2:narrow(1, floor((hImg - Hf) / 2), Hf): a 0-based offset handed to the 1-based narrow -- one pixel up and left of the centre
        o->oy = (p->hImg - o->Hf) / 2 - (p->fix_mask_offset ? 0 : 1);
        o->ox = (p->wImg - o->Wf) / 2 - (p->fix_mask_offset ? 0 : 1);
        DFE_REQUIRE(ctx, o->oy >= 0 && o->ox >= 0, DFE_E_ARG, "%s: the reference's mask offset is negative for features of the geometry's size (fix_mask_offset)", fn);
    }
    return DFE_OK;
}

}  // namespace

struct dfe_stream {
    dfe_ctx *ctx = nullptr;
    dfe_stream_params p;
    dfe_filter_layer layers[8];         // the host copy of p.layers (stream_shapes: at most 8)
    StreamShapes sh;
    int Hm = 0, Wm = 0;                 // the rectification mask: the features' size, or the geometry's in IMAGE mode
    double Ksmall[9];
    bool primed = false;
    int cur = 0;                        // the slot this push writes; 1 - cur holds the previous frame
    DfeBuf block;                       // the stream's own device memory (dfe_grow once, freed by dfe_stream_destroy)
    float *full[2], *scaled[2], *feat[2];   // (nlayers == 0: feat[i] IS scaled[i])
    float *raw = nullptr;               // has_dist: the converted uint8 frame in front of the undistortion
    float *pp[2];                       // the filter stack's intermediate layers
    float *warped_img = nullptr;        // IMAGE: the rectified previous scaled frame
    float *warped = nullptr;            // the rectified previous features
    float *rmask = nullptr, *conf = nullptr, *flow_i = nullptr, *mask_i = nullptr, *spare = nullptr;
    bool has_post = false;              // made by dfe_stream_create_post
    DfeStreamPost post;
};

namespace {

// the filter stack on one frame [C][hImg][wImg] -> dst [K][Hf][Wf], layer by layer through the launcher dfe_flow_pair_filtered_f32 uses
int stream_filter(dfe_stream *s, const float *in, float *dst) {
    dfe_ctx *ctx = s->ctx;
    DfeStageScope st(ctx, DFE_STAGE_FILTER);
    int h = s->p.hImg, w = s->p.wImg;
    for (int i = 0; i < s->p.nlayers; ++i) {
        const dfe_filter_layer *L = &s->layers[i];
        float *o = i == s->p.nlayers - 1 ? dst : s->pp[i & 1];
        int rc = dfe_filter_layer_forward_batch(ctx, 1, &in, &L, &h, &w, &o);
        if (rc) return rc;
        in = o;
        h -= L->kH - 1; w -= L->kW - 1;
    }
    return DFE_OK;
}

// post_call: one of dfe_stream_push_post_* (the stream has the chain); po: its outputs, may be NULL
int stream_push(dfe_stream *s, const float *frame, const uint8_t *frame8, float scale, float imu_tx, float *im_scaled, float *flow, float *mask, float *depth,
                float *depth_conf, double *R9, double *T3, int *n_found, int *n_inliers, int *status, bool post_call = false,
                const dfe_stream_post_out *po = nullptr) {
    dfe_ctx *ctx = s->ctx;
    const dfe_stream_params &p = s->p;
    const StreamShapes &sh = s->sh;
    const int c = s->cur, pv = 1 - c;
    const size_t nsrc = (size_t)p.C * p.Hsrc * p.Wsrc, nimg = (size_t)p.hImg * p.wImg;
    int rc;
    // the current frame at full resolution, undistorted (depth_estimation_api.lua:139)
    if (frame8) {
        float *f = p.has_dist ? s->raw : s->full[c];
        rc = dfe_u8_to_f32(ctx, frame8, (int64_t)nsrc, scale, f);
        if (rc) return rc;
        frame = f;
    }
    if (p.has_dist) {
        rc = dfe_undistort_image_f32(ctx, frame, p.C, p.Hsrc, p.Wsrc, p.K, p.dist, s->full[c]);
        if (rc) return rc;
    } else if (!frame8) {
        DFE_HIP(ctx, hipMemcpyAsync(s->full[c], frame, nsrc * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    // scale (:144) and filter (:149) are enqueued before the pose step (:141), whose host waits then overlap them; the results do not
    // depend on the order
    rc = dfe_image_scale_f32(ctx, s->full[c], p.C, p.Hsrc, p.Wsrc, p.hImg, p.wImg, s->scaled[c]);
    if (rc) return rc;
    if (p.nlayers) {
        rc = stream_filter(s, s->scaled[c], s->feat[c]);
        if (rc) return rc;
    }
    if (im_scaled) DFE_HIP(ctx, hipMemcpyAsync(im_scaled, s->scaled[c], (size_t)p.C * nimg * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (!s->primed) {
        s->primed = true;
        s->cur = pv;
        s->post.thave = false;
        if (n_found) *n_found = 0;
        if (n_inliers) *n_inliers = 0;
        if (status) *status = 0;
        return DFE_OK;
    }
    double R[9], T[3];
    int nc = -1, nf = 0, ni = 0;
    rc = dfe_ego_motion_from_images_f32(ctx, s->full[pv], s->full[c], p.C, p.Hsrc, p.Wsrc, p.K, &p.tracker, p.ransac_max_dist, p.iterations, p.seed, R, T, &nf, &ni,
                                        nullptr, nullptr, nullptr, nullptr, &nc);
    bool bad = false, pose = true;
    // its "fewer than 8 corners or tracks" error: the pose step writes *n_corners, then *n_found, before it refuses either count
    // (tracker.hip says so where it does), and nc stays -1 through its argument errors, which are errors here too
    if (rc == DFE_E_ARG && nc >= 0 && (nc < 8 || nf < 8)) { bad = true; pose = false; ni = 0; }
    else if (rc) return rc;
    else bad = (double)ni / (double)nf < p.min_inlier_ratio;                                    // (:159)
    float *flow_o = flow ? flow : s->flow_i, *mask_o = mask ? mask : s->mask_i;
    const bool want_depth = depth || depth_conf;
    if (bad) {
        if (flow) DFE_HIP(ctx, hipMemsetAsync(flow, 0, 2 * nimg * 4, ctx->stream));
        if (mask) DFE_HIP(ctx, hipMemsetAsync(mask, 0, nimg * 4, ctx->stream));
        if (depth) DFE_HIP(ctx, hipMemsetAsync(depth, 0, nimg * 4, ctx->stream));
        if (depth_conf) DFE_HIP(ctx, hipMemsetAsync(depth_conf, 0, nimg * 4, ctx->stream));
        if (post_call) {
            rc = dfe_stream_post_zero(ctx, s->post, po);
            if (rc) return rc;
        }
    } else {
        // the rotation taken out of the previous frame (:147; test_opticalflow.lua:284 warps the image and filters it)
        if (p.rectify == 0) {
            rc = dfe_remove_ego_motion_f32(ctx, s->feat[pv], sh.K, sh.Hf, sh.Wf, s->Ksmall, R, 1, s->warped, s->rmask);
            if (rc) return rc;
        } else {
            rc = dfe_remove_ego_motion_f32(ctx, s->scaled[pv], p.C, p.hImg, p.wImg, s->Ksmall, R, 1, s->warped_img, s->rmask);
            if (rc) return rc;
            if (p.nlayers) {
                rc = stream_filter(s, s->warped_img, s->warped);
                if (rc) return rc;
            }
        }
        const float *prevf = (p.rectify == 1 && !p.nlayers) ? s->warped_img : s->warped;
        // prepareInput + model:forward + processOutput on the two feature maps (:164-168)
        if (p.extraction == 2)
            rc = dfe_flow_pair_filtered_mean_f32(ctx, prevf, s->feat[c], sh.K, sh.Hf, sh.Wf, nullptr, 0, p.maxh, p.maxw, p.hImg, p.wImg, flow_o, s->conf, nullptr);
        else
            rc = dfe_flow_pair_filtered_f32(ctx, prevf, s->feat[c], sh.K, sh.Hf, sh.Wf, nullptr, 0, p.maxh, p.maxw, p.extraction == 1, p.threshold, p.hImg, p.wImg,
                                            flow_o, s->conf, nullptr, nullptr);
        if (rc) return rc;
        if (mask || want_depth || post_call) {
            rc = dfe_enlarge_mask_f32(ctx, s->rmask, s->Hm, s->Wm, sh.ix, sh.iy);                  // (:172-174)
            if (rc) return rc;
            rc = dfe_mask_paste_mul_f32(ctx, s->rmask, s->Hm, s->Wm, s->conf, p.hImg, p.wImg, sh.oy, sh.ox, mask_o);   // (:176-182)
            if (rc) return rc;
        }
        if (want_depth) {
            // (the drone's C++ does this with the x-flow and the mask it gets back: ardrone/ardrone_api.cpp:99-140)
            float *d = depth ? depth : s->spare, *dc = depth_conf ? depth_conf : s->spare;
            rc = dfe_flow_to_depth_ardrone(ctx, flow_o + nimg, mask_o, p.hImg, p.wImg, imu_tx, d, dc);
            if (rc) return rc;
        }
        if (post_call) {
            const DfeStreamPostIn in{flow_o, mask_o, prevf, s->feat[c], s->scaled[pv], p.rectify == 1 ? s->warped_img : nullptr, sh.K, sh.Hf, sh.Wf, p.maxh, p.maxw,
                                     p.extraction, p.threshold, s->Ksmall, R, imu_tx};
            rc = dfe_stream_post_run(ctx, s->post, in, po);
            if (rc) return rc;
        }
    }
    // last_im = im; last_im_scaled = im_scaled; last_filtered = filtered (:187-189): the slots swap roles
    s->cur = pv;
    // the temporal state: advanced by the chain, forgotten behind a bad image and behind a plain push (nothing to carry it with)
    if (post_call && !bad && s->post.o.temporal) { s->post.tcur = 1 - s->post.tcur; s->post.thave = true; }
    else s->post.thave = false;
    if (pose) {
        if (R9) memcpy(R9, R, sizeof(R));
        if (T3) memcpy(T3, T, sizeof(T));
    }
    if (n_found) *n_found = nf;
    if (n_inliers) *n_inliers = ni;
    if (status) *status = bad ? 2 : 1;
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_mask_paste_mul_f32(dfe_ctx *ctx, const float *mask, int Hm, int Wm, const float *conf, int H, int W, int oy, int ox, float *out) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, mask && conf && out, DFE_E_ARG, "dfe_mask_paste_mul_f32: NULL tensor");
    DFE_REQUIRE(ctx, Hm >= 1 && Wm >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, DFE_E_ARG, "dfe_mask_paste_mul_f32: mask %dx%d in %dx%d (1..32768)", Hm, Wm, H, W);
    DFE_REQUIRE(ctx, oy >= 0 && ox >= 0 && Hm <= H - oy && Wm <= W - ox, DFE_E_ARG, "dfe_mask_paste_mul_f32: mask %dx%d at (%d, %d) leaves the %dx%d frame", Hm, Wm,
                oy, ox, H, W);
    hipLaunchKernelGGL(mask_paste_mul_kernel, dim3(dfe_cdiv(W, 64), dfe_cdiv(H, 4)), dim3(64, 4), 0, ctx->stream, mask, Hm, Wm, conf, H, W, oy, ox, out);
    DFE_LAUNCH_CHECK(ctx);
    return DFE_OK;
}

int dfe_stream_shapes(const dfe_stream_params *p, int *Hf, int *Wf, int *H1, int *W1, int *oy, int *ox, int *ix, int *iy) {
    StreamShapes s;
    int rc = stream_shapes(nullptr, "dfe_stream_shapes", p, &s);
    if (rc) return rc;
    if (Hf) *Hf = s.Hf;
    if (Wf) *Wf = s.Wf;
    if (H1) *H1 = s.H1;
    if (W1) *W1 = s.W1;
    if (oy) *oy = s.oy;
    if (ox) *ox = s.ox;
    if (ix) *ix = s.ix;
    if (iy) *iy = s.iy;
    return DFE_OK;
}

}  // extern "C"

namespace {

// dfe_stream_create (post == NULL) and dfe_stream_create_post behind their device guard
int stream_create(dfe_ctx *ctx, const char *fn, const dfe_stream_params *p, const dfe_stream_post *post, dfe_stream **out) {
    DFE_REQUIRE(ctx, out, DFE_E_ARG, "%s: out is NULL", fn);
    *out = nullptr;
    StreamShapes sh;
    int rc = stream_shapes(ctx, fn, p, &sh);
    if (rc) return rc;
    if (post && (rc = dfe_stream_post_validate(ctx, fn, post))) return rc;
    DFE_REQUIRE(ctx, (long long)p->Hsrc * p->Wsrc < (1ll << 31), DFE_E_SHAPE, "%s: frame %dx%d", fn, p->Hsrc, p->Wsrc);
    double Ki[9];
    DFE_REQUIRE(ctx, dfe_mat3_inv(p->K, Ki), DFE_E_ARG, "%s: K is singular", fn);
    DFE_REQUIRE(ctx, p->iterations >= 1 && p->iterations <= 65536 && p->ransac_max_dist > 0, DFE_E_ARG, "%s: iterations=%d (1..65536) ransac_max_dist=%g", fn,
                p->iterations, p->ransac_max_dist);
    dfe_stream *s = new (std::nothrow) dfe_stream;
    DFE_REQUIRE(ctx, s, DFE_E_ALLOC, "%s: out of host memory", fn);
    s->ctx = ctx;
    s->p = *p;
    if (p->nlayers) memcpy(s->layers, p->layers, (size_t)p->nlayers * sizeof(dfe_filter_layer));
    s->p.layers = s->layers;
    s->sh = sh;
    s->Hm = p->rectify == 1 ? p->hImg : sh.Hf;
    s->Wm = p->rectify == 1 ? p->wImg : sh.Wf;
    // K_small = diag(wImg / Wsrc, hImg / Hsrc, 1) K: the reference's Khalf (depth_estimation_api.lua:50-51) at one half
    const double sx = (double)p->wImg / (double)p->Wsrc, sy = (double)p->hImg / (double)p->Hsrc;
    for (int j = 0; j < 3; ++j) { s->Ksmall[j] = sx * p->K[j]; s->Ksmall[3 + j] = sy * p->K[3 + j]; s->Ksmall[6 + j] = p->K[6 + j]; }
    const size_t nimg = (size_t)p->hImg * p->wImg, n_full = (size_t)p->C * p->Hsrc * p->Wsrc, n_feat = (size_t)sh.K * sh.Hf * sh.Wf;
    auto lay = [&](DfeCarve c) {
        for (float *&f : s->full) f = c.take<float>(n_full);
        for (float *&f : s->scaled) f = c.take<float>(p->C * nimg);
        for (int i = 0; i < 2; ++i) s->feat[i] = p->nlayers ? c.take<float>(n_feat) : s->scaled[i];
        for (float *&f : s->pp) f = c.take<float>(p->nlayers > 1 ? sh.maxplanes * nimg : 0);
        s->raw = c.take<float>(p->has_dist ? n_full : 0);
        s->warped_img = c.take<float>(p->rectify == 1 ? p->C * nimg : 0);
        s->warped = c.take<float>((p->rectify == 0 || p->nlayers) ? n_feat : 0);
        s->rmask = c.take<float>(nimg);            // (at most hImg x wImg)
        s->conf = c.take<float>(nimg);
        s->flow_i = c.take<float>(nimg);           // [2][hImg][wImg], contiguous, in the space of two rounded planes: the second
        c.take<float>(nimg);                       // take keeps what follows where the stream's first layout put it
        s->mask_i = c.take<float>(nimg);
        s->spare = c.take<float>(nimg);
        if (s->has_post) s->post.take(c, p->rectify == 1);
        return c.off;
    };
    if (post) {
        s->has_post = true;
        s->post.o = *post;
        s->post.C = p->C; s->post.H = p->hImg; s->post.W = p->wImg;
        s->post.y0 = (p->hImg - sh.H1) / 2; s->post.x0 = (p->wImg - sh.W1) / 2; s->post.Ho = sh.H1; s->post.Wo = sh.W1;
    }
    rc = dfe_grow(ctx, s->block, lay(DfeCarve()), fn);
    if (rc) { delete s; return rc; }
    lay(DfeCarve(s->block.p));
    *out = s;
    return DFE_OK;
}

// a push of the post form: the stream must have the chain, and post_out the size this library knows
int stream_post_args(dfe_stream *s, const char *fn, const void *frame, const dfe_stream_post_out *po) {
    DFE_REQUIRE(s->ctx, s->has_post, DFE_E_ARG, "%s: the stream was made by dfe_stream_create, not dfe_stream_create_post", fn);
    DFE_REQUIRE(s->ctx, frame, DFE_E_ARG, "%s: frame is NULL", fn);
    DFE_REQUIRE(s->ctx, !po || po->struct_size == (int)sizeof(dfe_stream_post_out), DFE_E_ARG, "%s: post_out.struct_size = %d, this library's dfe_stream_post_out has %d bytes",
                fn, po ? po->struct_size : 0, (int)sizeof(dfe_stream_post_out));
    return DFE_OK;
}

}  // namespace

extern "C" {

int dfe_stream_create(dfe_ctx *ctx, const dfe_stream_params *p, dfe_stream **out) {
    DFE_ENTER(ctx);
    return stream_create(ctx, "dfe_stream_create", p, nullptr, out);
}

int dfe_stream_post_check(const dfe_stream_params *p, const dfe_stream_post *post) {
    StreamShapes s;
    int rc = stream_shapes(nullptr, "dfe_stream_post_check", p, &s);
    if (rc) return rc;
    return dfe_stream_post_validate(nullptr, "dfe_stream_post_check", post);
}

int dfe_stream_create_post(dfe_ctx *ctx, const dfe_stream_params *p, const dfe_stream_post *post, dfe_stream **out) {
    DFE_ENTER(ctx);
    DFE_REQUIRE(ctx, post, DFE_E_ARG, "dfe_stream_create_post: post is NULL");
    return stream_create(ctx, "dfe_stream_create_post", p, post, out);
}

int dfe_stream_push_post_f32(dfe_stream *s, const float *frame, float imu_tx, float *im_scaled, float *flow, float *mask, float *depth, float *depth_conf,
                             const dfe_stream_post_out *post_out, double *R9, double *T3, int *n_found, int *n_inliers, int *status) {
    if (!s) return dfe_fail(nullptr, DFE_E_ARG, "dfe_stream_push_post_f32: stream is NULL");
    DFE_ENTER(s->ctx);
    if (int rc = stream_post_args(s, "dfe_stream_push_post_f32", frame, post_out)) return rc;
    return stream_push(s, frame, nullptr, 1.f, imu_tx, im_scaled, flow, mask, depth, depth_conf, R9, T3, n_found, n_inliers, status, true, post_out);
}

int dfe_stream_push_post_u8(dfe_stream *s, const uint8_t *frame, float scale, float imu_tx, float *im_scaled, float *flow, float *mask, float *depth,
                            float *depth_conf, const dfe_stream_post_out *post_out, double *R9, double *T3, int *n_found, int *n_inliers, int *status) {
    if (!s) return dfe_fail(nullptr, DFE_E_ARG, "dfe_stream_push_post_u8: stream is NULL");
    DFE_ENTER(s->ctx);
    if (int rc = stream_post_args(s, "dfe_stream_push_post_u8", frame, post_out)) return rc;
    return stream_push(s, nullptr, frame, scale, imu_tx, im_scaled, flow, mask, depth, depth_conf, R9, T3, n_found, n_inliers, status, true, post_out);
}

int dfe_stream_push_f32(dfe_stream *s, const float *frame, float imu_tx, float *im_scaled, float *flow, float *mask, float *depth, float *depth_conf, double *R9,
                        double *T3, int *n_found, int *n_inliers, int *status) {
    if (!s) return dfe_fail(nullptr, DFE_E_ARG, "dfe_stream_push_f32: stream is NULL");
    DFE_ENTER(s->ctx);
    DFE_REQUIRE(s->ctx, frame, DFE_E_ARG, "dfe_stream_push_f32: frame is NULL");
    return stream_push(s, frame, nullptr, 1.f, imu_tx, im_scaled, flow, mask, depth, depth_conf, R9, T3, n_found, n_inliers, status);
}

int dfe_stream_push_u8(dfe_stream *s, const uint8_t *frame, float scale, float imu_tx, float *im_scaled, float *flow, float *mask, float *depth, float *depth_conf,
                       double *R9, double *T3, int *n_found, int *n_inliers, int *status) {
    if (!s) return dfe_fail(nullptr, DFE_E_ARG, "dfe_stream_push_u8: stream is NULL");
    DFE_ENTER(s->ctx);
    DFE_REQUIRE(s->ctx, frame, DFE_E_ARG, "dfe_stream_push_u8: frame is NULL");
    return stream_push(s, nullptr, frame, scale, imu_tx, im_scaled, flow, mask, depth, depth_conf, R9, T3, n_found, n_inliers, status);
}

int dfe_stream_reset(dfe_stream *s) {
    if (!s) return dfe_fail(nullptr, DFE_E_ARG, "dfe_stream_reset: stream is NULL");
    s->primed = false;
    s->post.thave = false;
    return DFE_OK;
}

void dfe_stream_destroy(dfe_stream *s) {
    if (!s) return;
    {
        DfeDeviceGuard guard(s->ctx);
        (void)hipStreamSynchronize(s->ctx->stream);   // nothing of this ctx may still be writing there
        if (s->block.p) (void)hipFree(s->block.p);
    }
    delete s;
}

}  // extern "C"
