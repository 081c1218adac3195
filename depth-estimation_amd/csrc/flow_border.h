// flow_border.h -- the frame border of a pair step (frame mode of TailOut, cv_records.h), which no sweep writes: flow and scores 0, depth of
// a pixel at rest.  Device code shared by the kernels that write it beside their own work: the gated float sweep behind the int8 kernel
// (ssd_cost_volume.hip) and the pack kernel of the byte entries (ssd_flow_i8.hip).
#pragma once
#include "cv_records.h"

// where a step's results go, with the frame-mode fields of a pair call (as dfe_flow_finalize, postops.hip, sets them)
inline TailOut dfe_tailout_frame(const TailOut &out, const DfePairDepth *pd) {
    TailOut o = out;
    if (pd) {
        o.frame_H = pd->H; o.frame_W = pd->W; o.depth = pd->depth; o.conf = pd->conf;
        o.mw = pd->cx; o.mh = pd->cy; o.infty = (float)((double)pd->W / 2);   // test_opticalflow.lua:148 geometry.wImg/2
    }
    return o;
}

// The border of the frame o.frame_H x o.frame_W around the Ho x o.Wo interior at (o.pad_t, o.pad_l), enumerated directly -- top rows, bottom
// rows, then the two side bands of the rows between -- and dealt to `nthr` threads of which this one is `tid` (a grid-stride loop)
__device__ __forceinline__ void dfe_flow_border(const TailOut &o, int Ho, int tid, int nthr) {
    const int W = o.frame_W, nbot = o.frame_H - o.pad_t - Ho, side = W - o.Wo;
    const int nfull = (o.pad_t + nbot) * W, nborder = nfull + Ho * side;   // (H W < 2^31)
    for (int q = tid; q < nborder; q += nthr) {
        int fi, fj;
        if (q < nfull) {
            fi = (int)((unsigned)q / (unsigned)W);
            fj = q - fi * W;
            if (fi >= o.pad_t) fi += Ho;
        } else {
            const int e = q - nfull, iy = (int)((unsigned)e / (unsigned)side), c = e - iy * side;
            fi = o.pad_t + iy;
            fj = c < o.pad_l ? c : c + o.Wo;
        }
        const long long f = (long long)fi * W + fj;
        o.fy[f] = 0.f;
        o.fx[f] = 0.f;
        if (o.scores) o.scores[f] = 0.f;
        if (o.depth) pair_depth_px(fi, fj, 0.f, 0.f, o.mw, o.mh, o.infty, &o.depth[f], &o.conf[f]);
    }
}
