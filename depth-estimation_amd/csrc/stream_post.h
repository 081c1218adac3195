// stream_post.h -- the session's post-processing chain (include/dfe.h: dfe_stream_push_post_*), shared by stream.hip, which owns the
// stream object and calls the chain behind its own pair step, and stream_post.hip, which holds the chain and its kernels.
#pragma once
#include "dfe_internal.h"

// the chain's options, its buffers inside the stream's block and the temporal state
struct DfeStreamPost {
    dfe_stream_post o;
    int C = 0, H = 0, W = 0;              // the scaled frame [C][H][W]
    int y0 = 0, x0 = 0, Ho = 0, Wo = 0;   // the matcher's region R
    float *guide = nullptr;               // FEATURES mode with the median on: the rectified previous scaled frame [C][H][W]
    float *flow_bw = nullptr, *consistent = nullptr, *kept = nullptr, *mc = nullptr;
    float *dense = nullptr, *filled = nullptr, *w = nullptr, *med = nullptr, *valid = nullptr;
    float *depth = nullptr, *dconf = nullptr;
    // temporal: the state (value, weight: adjacent planes) and the flow it was measured with, in two slots; a push writes the slot that
    // does not hold the state, and the two swap when the push commits
    float *state[2] = {nullptr, nullptr}, *sflow[2] = {nullptr, nullptr};
    float *prior = nullptr, *rot = nullptr;   // [2][H][W] each: (prior, weight) carried along the flow, then through the rotation
    float *rotmask = nullptr, *flag = nullptr;
    int tcur = 0;                         // the slot that holds the state
    bool thave = false;                   // there is a state
    void take(DfeCarve &c, bool image_mode);
};
// every member of post (DFE_E_ARG); ctx may be NULL
DFE_HIDDEN int dfe_stream_post_validate(dfe_ctx *ctx, const char *fn, const dfe_stream_post *post);
// what the chain reads of a status-1 push: the push's flow and mask, the two feature maps [K][Hf][Wf] the forward matcher read, the
// previous scaled frame, its rectified copy where the session has made one (IMAGE mode, else NULL), the pose
struct DfeStreamPostIn {
    const float *flow, *mask, *prevf, *curf, *prev_scaled, *warped_img;
    int K, Hf, Wf, maxh, maxw, extraction;
    double threshold;
    const double *Ksmall, *R;
    float imu_tx;
};
// the chain on a status-1 push; po may be NULL.  With temporal on the new state lies in slot 1 - tcur afterwards: the caller swaps when
// the push commits
DFE_HIDDEN int dfe_stream_post_run(dfe_ctx *ctx, DfeStreamPost &s, const DfeStreamPostIn &in, const dfe_stream_post_out *po);
DFE_HIDDEN int dfe_stream_post_zero(dfe_ctx *ctx, const DfeStreamPost &s, const dfe_stream_post_out *po);   // status 2: every given output zeroed
