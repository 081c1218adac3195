// feat_matching_dispatch.hip -- nn.SpatialMatching on K-plane feature maps: the one place a matcher kernel is launched from.
// fm_select (fm_select.h) chooses; the launchers (dfe_fm_launch_*) take the job and the pick and do not decline.  No kernel of its own.
#include "dfe_internal.h"

int dfe_fm_run(dfe_ctx *ctx, const FmJob &job, FmPick *picked) {
    const FmPick pk = fm_select(dfe_fm_env(ctx), job);
    if (picked) *picked = pk;
    int rc = DFE_OK;
    switch (pk.kernel) {
    case FM_K_NONE:
        DFE_REQUIRE(ctx, picked, DFE_E_UNSUPPORTED, "dfe_fm_run: no kernel for form %d, K=%d %dx%d window %dx%d", (int)job.form, job.K, job.H1, job.W1, job.maxh, job.maxw);
        return DFE_OK;
    case FM_K_MFMA: {
        FmJob j = job;
        if (!j.norms) {   // the ctx's side buffer: NOT the arena, whose carved pointers this call must not invalidate
            void *nrm = nullptr;
            rc = dfe_aux_scratch(ctx, fm_mfma_scratch(j) * sizeof(float), &nrm);
            if (rc) return rc;
            j.norms = (float *)nrm;
            j.norms_ready = false;
        }
        rc = dfe_fm_launch_mfma(ctx, j, pk);
        break;
    }
    case FM_K_WIN64: rc = dfe_fm_launch_win64(ctx, job, pk); break;
    case FM_K_FLAT: rc = dfe_fm_launch_flat(ctx, job, pk); break;
    case FM_K_ROWS: rc = dfe_fm_launch_rows(ctx, job, pk); break;
    case FM_K_CHUNK: rc = dfe_fm_launch_chunk(ctx, job, pk); break;
    case FM_K_REF: rc = dfe_fm_launch_ref(ctx, job); break;
    }
    if (rc == DFE_OK) ctx->last_kernel = fm_kernel_name(pk.kernel, job.form);
    return rc;
}

int dfe_spatial_matching_dispatch(dfe_ctx *ctx, const float *in1, const float *in2, int K, int H1, int W1, int maxh, int maxw, float *out) {
    DFE_REQUIRE(ctx, in1 && in2 && out, DFE_E_ARG, "dfe_spatial_matching_f32: NULL tensor");
    DFE_REQUIRE(ctx, K > 0 && H1 > 0 && W1 > 0 && maxh > 0 && maxw > 0, DFE_E_SHAPE,
                "dfe_spatial_matching_f32: K=%d H1=%d W1=%d maxh=%d maxw=%d must be positive", K, H1, W1, maxh, maxw);
    FmJob j = fm_job(FM_VOLUME, in1, in2, K, H1, W1, maxh, maxw);
    j.out = out;
    return dfe_fm_run(ctx, j);
}
