// stream_post.hip -- the video session's post-processing chain (include/dfe.h: dfe_stream_push_post_*): behind the
// pair step of stream.hip the forward-backward check, the hole filling, the guided weighted median, the depth of the drone API on the
// result and the temporal depth filter, each the public entry a caller had to stitch in Python, on buffers of the stream's own block and
// with the filter's state kept on the device.  The kernels here are what that stitching did with elementwise tensor expressions: one
// thread per pixel, plain fp32, every product rounded on its own, so that each plane has the bits of the expression it replaces.
#include "stream_post.h"
#include <cmath>

namespace {

// kept = (mask > 0 ? 1 : 0) * consistent; consistent == NULL: no factor
__global__ __launch_bounds__(256) void post_kept_kernel(const float *__restrict__ mask, const float *__restrict__ consistent, long long n, float *__restrict__ kept) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float m = mask[i] > 0.f ? 1.f : 0.f;
    kept[i] = consistent ? m * consistent[i] : m;
}

// w = kept > 0 ? filled : 0.25f * filled: a filled hole counts a quarter of a measured pixel (_with_fill of subpixel.py)
__global__ __launch_bounds__(256) void post_reweight_kernel(const float *__restrict__ kept, const float *__restrict__ filled, long long n, float *__restrict__ w) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float f = filled[i];
    w[i] = kept[i] > 0.f ? f : 0.25f * f;
}

// out = a * b; out may be a or b
__global__ __launch_bounds__(256) void post_mul_kernel(const float *a, const float *b, long long n, float *out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = a[i] * b[i];
}

inline dim3 post_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

int post_copy(dfe_ctx *ctx, float *dst, const float *src, size_t n) {
    if (dst) DFE_HIP(ctx, hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return DFE_OK;
}

int post_clear(dfe_ctx *ctx, float *dst, size_t n) {
    if (dst) DFE_HIP(ctx, hipMemsetAsync(dst, 0, n * 4, ctx->stream));
    return DFE_OK;
}

}  // namespace

void DfeStreamPost::take(DfeCarve &c, bool image_mode) {
    const size_t n = (size_t)H * W;
    const bool cons = o.consistency_tol > 0.f, fill = o.fill != 0, med = o.median_k != 0;
    guide = c.take<float>(med && !image_mode ? C * n : 0);
    flow_bw = c.take<float>(cons ? 2 * n : 0);
    consistent = c.take<float>(cons ? n : 0);
    kept = c.take<float>(fill || med ? n : 0);
    mc = c.take<float>(cons && !fill && !med ? n : 0);
    dense = c.take<float>(fill ? 2 * n : 0);
    filled = c.take<float>(fill ? n : 0);
    w = c.take<float>(fill ? n : 0);
    this->med = c.take<float>(med ? 2 * n : 0);
    valid = c.take<float>(med ? n : 0);
    depth = c.take<float>(n);
    dconf = c.take<float>(n);
    const size_t t = o.temporal ? n : 0;
    for (float *&f : state) f = c.take<float>(2 * t);
    for (float *&f : sflow) f = c.take<float>(2 * t);
    prior = c.take<float>(2 * t);
    rot = c.take<float>(2 * t);
    rotmask = c.take<float>(t);
    flag = c.take<float>(t);
}

int dfe_stream_post_validate(dfe_ctx *ctx, const char *fn, const dfe_stream_post *o) {
    DFE_REQUIRE(ctx, o, DFE_E_ARG, "%s: post is NULL", fn);
    DFE_REQUIRE(ctx, o->struct_size == (int)sizeof(dfe_stream_post), DFE_E_ARG, "%s: post.struct_size = %d, this library's dfe_stream_post has %d bytes", fn,
                o->struct_size, (int)sizeof(dfe_stream_post));
    DFE_REQUIRE(ctx, o->consistency_tol >= 0.f, DFE_E_ARG, "%s: consistency_tol = %g (0: off, > 0: the tolerance)", fn, (double)o->consistency_tol);
    DFE_REQUIRE(ctx, (o->fill == 0 || o->fill == 1) && o->fill_levels >= 0, DFE_E_ARG, "%s: fill = %d (0, 1), fill_levels = %d (>= 0)", fn, o->fill, o->fill_levels);
    DFE_REQUIRE(ctx, o->median_k == 0 || (o->median_k >= 1 && o->median_k <= 15 && (o->median_k & 1)), DFE_E_ARG, "%s: median_k = %d (0: off, or odd 1 .. 15)", fn,
                o->median_k);
    DFE_REQUIRE(ctx, o->temporal == 0 || o->temporal == 1, DFE_E_ARG, "%s: temporal = %d (0, 1)", fn, o->temporal);
    if (!o->temporal) return DFE_OK;
    DFE_REQUIRE(ctx, o->t_tol >= 0.f, DFE_E_ARG, "%s: t_tol = %g must be >= 0", fn, (double)o->t_tol);
    DFE_REQUIRE(ctx, std::isfinite(o->t_wmax) && o->t_wmax >= 1e-6f, DFE_E_ARG, "%s: t_wmax = %g must be finite and >= 1e-6", fn, (double)o->t_wmax);
    DFE_REQUIRE(ctx, o->t_decay > 0.f && o->t_decay <= 1.f, DFE_E_ARG, "%s: t_decay = %g must lie in (0, 1]", fn, (double)o->t_decay);
    DFE_REQUIRE(ctx, (o->t_has_gain == 0 || (o->t_has_gain == 1 && std::isfinite(o->t_gain))) && (o->t_has_bias == 0 || (o->t_has_bias == 1 && std::isfinite(o->t_bias))),
                DFE_E_ARG, "%s: t_has_gain = %d, t_gain = %g, t_has_bias = %d, t_bias = %g (flags 0 / 1, a given number finite)", fn, o->t_has_gain, (double)o->t_gain,
                o->t_has_bias, (double)o->t_bias);
    DFE_REQUIRE(ctx, o->t_splat == 0 || o->t_splat == 1, DFE_E_ARG, "%s: t_splat = %d (0 nearest, 1 bilinear)", fn, o->t_splat);
    if (o->t_splat == 1) {
        DFE_REQUIRE(ctx, std::isfinite(o->t_ztol) && o->t_ztol >= 0.f, DFE_E_ARG, "%s: t_ztol = %g must be finite and >= 0", fn, (double)o->t_ztol);
        DFE_REQUIRE(ctx, std::isfinite(o->t_quant) && o->t_quant > 0.f, DFE_E_ARG, "%s: t_quant = %g must be finite and > 0", fn, (double)o->t_quant);
        DFE_REQUIRE(ctx, o->t_min_cover >= 0.f && o->t_min_cover <= 1.f, DFE_E_ARG, "%s: t_min_cover = %g must lie in [0, 1]", fn, (double)o->t_min_cover);
    }
    return DFE_OK;
}

int dfe_stream_post_zero(dfe_ctx *ctx, const DfeStreamPost &s, const dfe_stream_post_out *po) {
    if (!po) return DFE_OK;
    const size_t n = (size_t)s.H * s.W;
    float *const one[] = {po->consistent, po->weight_post, po->depth_post, po->depth_post_conf, po->depth_fused, po->fused_weight, po->fused_flag};
    for (float *f : one)
        if (int rc = post_clear(ctx, f, n)) return rc;
    if (int rc = post_clear(ctx, po->flow_bw, 2 * n)) return rc;
    return post_clear(ctx, po->flow_post, 2 * n);
}

int dfe_stream_post_run(dfe_ctx *ctx, DfeStreamPost &s, const DfeStreamPostIn &in, const dfe_stream_post_out *po) {
    const dfe_stream_post &o = s.o;
    const int H = s.H, W = s.W;
    const long long n = (long long)H * W;
    const bool fill = o.fill != 0, med = o.median_k != 0;
    int rc;
    // 1. consistency: the session's matcher with the two maps swapped, flow planes only, and the forward-backward check over R
    const float *cons = nullptr;
    if (o.consistency_tol > 0.f) {
        if (in.extraction == 2)
            rc = dfe_flow_pair_filtered_mean_f32(ctx, in.curf, in.prevf, in.K, in.Hf, in.Wf, nullptr, 0, in.maxh, in.maxw, H, W, s.flow_bw, nullptr, nullptr);
        else
            rc = dfe_flow_pair_filtered_f32(ctx, in.curf, in.prevf, in.K, in.Hf, in.Wf, nullptr, 0, in.maxh, in.maxw, in.extraction == 1, in.threshold, H, W, s.flow_bw,
                                            nullptr, nullptr, nullptr);
        if (rc) return rc;
        rc = dfe_flow_consistency_f32(ctx, in.flow, s.flow_bw, H, W, s.y0, s.x0, s.Ho, s.Wo, o.consistency_tol, s.consistent, nullptr);
        if (rc) return rc;
        cons = s.consistent;
    }
    const float *flow_post = in.flow, *weight_post = in.mask, *src = in.flow, *wsrc = nullptr;
    if (fill || med) {
        hipLaunchKernelGGL(post_kept_kernel, post_grid(n), dim3(256), 0, ctx->stream, in.mask, cons, n, s.kept);
        DFE_LAUNCH_CHECK(ctx);
        wsrc = s.kept;
    }
    // 2. fill
    if (fill) {
        rc = dfe_fill_holes_f32(ctx, in.flow, 2, H, W, s.kept, s.y0, s.x0, s.Ho, s.Wo, o.fill_levels, s.dense, s.filled);
        if (rc) return rc;
        hipLaunchKernelGGL(post_reweight_kernel, post_grid(n), dim3(256), 0, ctx->stream, (const float *)s.kept, (const float *)s.filled, n, s.w);
        DFE_LAUNCH_CHECK(ctx);
        src = flow_post = s.dense;
        wsrc = s.w;
        weight_post = s.filled;
    }
    // 3. median, guided by the rectified previous scaled frame
    if (med) {
        const float *guide = in.warped_img;
        if (!guide) {
            rc = dfe_remove_ego_motion_f32(ctx, in.prev_scaled, s.C, H, W, in.Ksmall, in.R, 1, s.guide, nullptr);
            if (rc) return rc;
            guide = s.guide;
        }
        rc = dfe_weighted_median_f32(ctx, src, 2, H, W, wsrc, guide, s.C, o.median_sigma, o.median_k, s.y0, s.x0, s.Ho, s.Wo, s.med, s.valid);
        if (rc) return rc;
        flow_post = s.med;
        weight_post = s.valid;
    }
    // 4. the result
    if (cons && !fill && !med) {
        hipLaunchKernelGGL(post_mul_kernel, post_grid(n), dim3(256), 0, ctx->stream, in.mask, cons, n, s.mc);
        DFE_LAUNCH_CHECK(ctx);
        weight_post = s.mc;
    }
    if (o.temporal || (po && (po->depth_post || po->depth_post_conf))) {
        rc = dfe_flow_to_depth_ardrone(ctx, flow_post + n, weight_post, H, W, in.imu_tx, s.depth, s.dconf);
        if (rc) return rc;
    }
    // 5. temporal: TemporalFilter.push with the state in the stream; the new state goes to the slot that does not hold the old one
    float *nv = nullptr;
    if (o.temporal) {
        nv = s.state[1 - s.tcur];
        if (!s.thave) {
            DFE_HIP(ctx, hipMemsetAsync(s.rot, 0, (size_t)(2 * n) * 4, ctx->stream));                 // a zero prior of zero weight
        } else {
            const float *sv = s.state[s.tcur], *sw = sv + n, *gain = o.t_has_gain ? &o.t_gain : nullptr, *bias = o.t_has_bias ? &o.t_bias : nullptr;
            if (o.t_splat == 1)
                rc = dfe_forward_splat_f32(ctx, sv, 1, H, W, sw, s.sflow[s.tcur], sv, 0, 0, H, W, gain, bias, o.t_decay, o.t_ztol, o.t_quant, o.t_min_cover, s.prior,
                                           s.prior + n, nullptr);
            else
                rc = dfe_forward_warp_f32(ctx, sv, 1, H, W, sw, s.sflow[s.tcur], sv, 0, 0, H, W, gain, bias, o.t_decay, s.prior, s.prior + n, nullptr);
            if (rc) return rc;
            // prior and weight are adjacent planes: the rotation takes both in one call, no concatenation
            rc = dfe_remove_ego_motion_f32(ctx, s.prior, 2, H, W, in.Ksmall, in.R, 1, s.rot, s.rotmask);
            if (rc) return rc;
            hipLaunchKernelGGL(post_mul_kernel, post_grid(n), dim3(256), 0, ctx->stream, (const float *)(s.rot + n), (const float *)s.rotmask, n, s.rot + n);
            DFE_LAUNCH_CHECK(ctx);
        }
        rc = dfe_temporal_fuse_f32(ctx, s.rot, s.rot + n, s.depth, s.dconf, 1, H, W, 0, 0, H, W, o.t_tol, o.t_wmax, nv, nv + n, s.flag);
        if (rc) return rc;
        DFE_HIP(ctx, hipMemcpyAsync(s.sflow[1 - s.tcur], flow_post, (size_t)(2 * n) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (!po) return DFE_OK;
    if (cons) {
        if ((rc = post_copy(ctx, po->flow_bw, s.flow_bw, 2 * n))) return rc;
        if ((rc = post_copy(ctx, po->consistent, s.consistent, n))) return rc;
    }
    if ((rc = post_copy(ctx, po->flow_post, flow_post, 2 * n))) return rc;
    if ((rc = post_copy(ctx, po->weight_post, weight_post, n))) return rc;
    if ((rc = post_copy(ctx, po->depth_post, s.depth, n))) return rc;
    if ((rc = post_copy(ctx, po->depth_post_conf, s.dconf, n))) return rc;
    if (o.temporal) {
        if ((rc = post_copy(ctx, po->depth_fused, nv, n))) return rc;
        if ((rc = post_copy(ctx, po->fused_weight, nv + n, n))) return rc;
        if ((rc = post_copy(ctx, po->fused_flag, s.flag, n))) return rc;
    }
    return DFE_OK;
}
