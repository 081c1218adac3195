// subpixel_offset.h -- the per-axis parabolic sub-pixel rule (include/dfe.h; DESIGN sections 4.19 and 4.21), shared by the
// single-scale refinement (subpixel.hip) and the radial matcher's epilogue and stand-alone refinement (radial_pipeline.hip).
#pragma once
#include <hip/hip_runtime.h>

// the parabola's vertex on one axis through the costs before, at and after the minimum: every operation fp32 and separately
// rounded, in this order, IEEE division; 0 where a neighbour lies outside the searched window or the curvature is not positive
__device__ __forceinline__ float subpixel_offset(bool inside, float cm, float c0, float cp) {
#pragma clang fp contract(off)
    float off = 0.f;
    if (inside) {
        const float den = (cm - c0) + (cp - c0);
        if (den > 0.f) {
            off = (cm - cp) / (2.f * den);
            off = fminf(fmaxf(off, -0.5f), 0.5f);
        }
    }
    return off;
}
