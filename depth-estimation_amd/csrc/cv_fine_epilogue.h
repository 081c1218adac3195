// cv_fine_epilogue.h -- the finest scales of the multiscale matcher inside the kernel that makes their costs: the arguments (CvFineArgs)
// and the epilogue that reads them, shared by the tiled SSD kernel (ssd_cost_volume.hip) and the one-chunk feature matcher
// (feat_matching.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "dfe_wave.h"

// The finest scale of the multiscale matcher WITHOUT its volume (multiscale.hip -> ssd_cost_volume.hip): the tiled kernel's task rows
// (8 pixels x the 64 cells of an 8 x 8 window, lane <-> cell) go through soft-min, cascade add, arg-max and decode in registers
struct CvFineArgs {
    const float *pcasc;        // cascaded windows of the next coarser scale [H/2][W/2][64], or NULL (one ratio only)
    const float2 *pbest;       // its running best (value, 0-based class as int bits)
    long long *idx;            // out [H][W]: 1-based class ids, or NULL
    float *fy, *fx;            // out [H][W]: decoded displacement planes, or NULL
    int middle;                // centre class (yx2xMulti(0, 0)), 1-based
    float f16_scale, f16_inv;  // != 0: the costs are rounded to half precision (cost * scale) first, as a stored fp16 volume would be
    int dec[5 * 64];           // class id - 1 -> (oy << 16) | (ox & 0xffff)
    // a scale > 1 (the same epilogue up to the cascade add, then what cascade_px_kernel<false> leaves for the next finer scale):
    float *casc;               // != NULL: out [H][W][64] cascaded windows of THIS scale; idx / fy / fx unused
    float2 *best;              //          out [H][W] running best (value, 0-based class as int bits)
    int cls_base;              //          0-based class id of this scale's first ring cell
};

// The finest scale of the multiscale matcher, consumed where it is produced: a task row is 8 pixels x the 64 cells of their 8 x 8
// windows, lane <-> cell.  Per pixel: soft-min over the wave (wave minimum of the costs, exponential, wave sum in the association
// order of every other soft-min on the device, e * (1 / sum)), cascade add of the parent pixel's window (cell (a, b) reads the
// parent's cell (2 + a/2, 2 + b/2): one ds_bpermute of the parent value every lane holds for its own cell), arg-max over the 64
// classes of this scale (wave maximum, lowest lane attaining it) against the coarser chain's running best (this scale wins ties:
// its class ids are smaller), centre override, decode -- the operations of cascade_px_kernel<FINEST> in the lane <-> cell form, on
// the same values in the same order: bit-identical results, and the scale-1 volume (84 % of the pyramid's bytes) is never written
// or read.  The three reductions run for the 8 pixels together (wave_reduce8_transposed); lane 8 g finishes pixel g and stores it.
//   (-c) - max(-c) == min(c) - c bit for bit; costs are sums of squares (>= +0) and the cascaded values sums of probabilities, so the
//   integer order of the bit patterns is the float order (frames with NaN / Inf give garbage on either path, not the same garbage).
//   Centre override (bv == centre value): the centre is one of the 64 cells, so centre <= fv; if the coarser chain's best wins
//   (pbv > fv) it is larger than the centre, otherwise bv = fv and the test is "the centre cell attains the maximum" = its bit in
//   the ballot the arg-max needs anyway.
//   MID (a scale > 1 with a coarser one above it, cascade_px_kernel<false>): the cascaded window is stored for the next finer scale, and
//   the arg-max runs over the 48 ring cells in CLASS order (top two rows, left 4 x 2, right 4 x 2, bottom two rows): cells outside
//   the ring take the most negative integer before the maximum; among the cells that attain it the class order is "first non-empty
//   group, lowest cell in it" -- scalar arithmetic on the ballot.
template <int TX, bool F16, bool MID>
__device__ __forceinline__ void fine_epilogue(const float (&vrow)[TX], int lane, int y, int xt, int Wo, const CvFineArgs &fa) {
#pragma clang fp contract(off)
    static_assert(TX == 8, "8 fine pixels = 4 parent pixels");
    const int a = lane >> 3, b = lane & 7;
    const int gsrc = (((2 + (a >> 1)) << 3) + 2 + (b >> 1)) << 2;          // byte address for ds_bpermute: the parent cell this cell adds
    const bool has_parent = fa.pcasc != nullptr;                            // (launch-uniform)
    float par[4];
    float2 pb = make_float2(0.f, 0.f);
    if (has_parent) {
        const long long pp = (long long)(y >> 1) * (Wo >> 1) + (xt >> 1);
        const float *pc = fa.pcasc + pp * 64 + lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) par[j] = pc[j * 64];
        pb = fa.pbest[pp + (lane >> 4)];                                    // lane 8 g: the running best of pixel g's parent
    }
    float v[TX];
#pragma unroll
    for (int x = 0; x < TX; ++x) v[x] = F16 ? (float)(_Float16)(vrow[x] * fa.f16_scale) * fa.f16_inv : vrow[x];   // what a stored fp16 volume would hold
    const int mn = wave_reduce8_transposed<1>(v, lane);
    int bc[TX];
#define DFE_BCAST8(src)                                                                                                          \
    _Pragma("unroll") for (int x = 0; x < TX; ++x) bc[x] = __builtin_amdgcn_readlane(src, 8 * x);                                \
    asm volatile("" : "+s"(bc[0]), "+s"(bc[1]), "+s"(bc[2]), "+s"(bc[3]), "+s"(bc[4]), "+s"(bc[5]), "+s"(bc[6]), "+s"(bc[7]))   // (all eight read before the first use: no wait states between a v_readlane and its consumer)
    DFE_BCAST8(mn);
#pragma unroll
    for (int x = 0; x < TX; ++x) v[x] = dfe_exp_nonpos(__int_as_float(bc[x]) - v[x]);
    const int rs = __float_as_int(1.0f / __int_as_float(wave_reduce8_transposed<0>(v, lane)));
    DFE_BCAST8(rs);
#undef DFE_BCAST8
#pragma unroll
    for (int x = 0; x < TX; ++x) v[x] = v[x] * __int_as_float(bc[x]);
    if (has_parent) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = __int_as_float(__builtin_amdgcn_ds_bpermute(gsrc, __float_as_int(par[j])));
            v[2 * j] = v[2 * j] + g;
            v[2 * j + 1] = v[2 * j + 1] + g;
        }
    }
    if constexpr (MID) {
        float *cq = fa.casc + ((long long)y * Wo + xt) * 64 + lane;
        const bool ring = !(a >= 2 && a <= 5 && b >= 2 && b <= 5);
#pragma unroll
        for (int x = 0; x < TX; ++x) {
            cq[x * 64] = v[x];
            v[x] = ring ? v[x] : __int_as_float(0x80000000);
        }
    }
    const int fvp = wave_reduce8_transposed<2>(v, lane);
    const int mbit = (fa.middle - 1) & 63;
    unsigned long long codes = 0;                                           // byte x: pixel x's first maximal cell | centre-is-maximal << 6
#pragma unroll
    for (int x = 0; x < TX; ++x) {
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(__float_as_int(v[x]) == __builtin_amdgcn_readlane(fvp, 8 * x));
        unsigned long long code;
        if constexpr (MID) {                                                // (byte x: the class rank 0..47 of pixel x's first maximal ring cell)
            const unsigned long long top = hit & 0xffffull, left = hit & 0x0000030303030000ull, right = hit & 0x0000c0c0c0c00000ull;
            const int cell = __builtin_ctzll(top ? top : left ? left : right ? right : hit);
            const int side = 16 + ((cell >> 3) - 2) * 2 + (cell & 7);      // left columns 0, 1 -> ranks 16..23; right columns 6, 7 -> 24..31
            code = (unsigned long long)(cell < 16 ? cell : cell >= 48 ? cell - 16 : (cell & 7) < 2 ? side : side + 2);
        } else {
            code = (unsigned long long)__builtin_ctzll(hit) | (((hit >> mbit) & 1ull) << 6);
        }
        codes |= code << (8 * x);
    }
    if constexpr (MID) {
        if ((lane & 7) == 0) {
            const int g = lane >> 3;
            float bv = __int_as_float(fvp);
            int bi = ((int)(codes >> (8 * g)) & 0xff) + fa.cls_base;
            if (has_parent && !(bv >= pb.x)) { bv = pb.x; bi = __float_as_int(pb.y); }      // the scale wins ties against the coarser chain
            fa.best[(long long)y * Wo + xt + g] = make_float2(bv, __int_as_float(bi));
        }
        return;
    }
    if ((lane & 7) == 0) {
        const int g = lane >> 3;
        const int code = (int)(codes >> (8 * g)) & 0xff;
        int bi = code & 63;
        bool centre = (code & 64) != 0;
        if (has_parent && !(__int_as_float(fvp) >= pb.x)) { bi = __float_as_int(pb.y); centre = false; }   // the scale wins ties against the coarser chain
        int id = bi + 1;
        if (fa.middle > 0 && centre) id = fa.middle;
        const long long p = (long long)y * Wo + xt + g;
        if (fa.idx) fa.idx[p] = id;
        if (fa.fy) {
            const int d = fa.dec[id - 1];
            fa.fy[p] = (float)(d >> 16);
            fa.fx[p] = (float)(short)(d & 0xffff);
        }
    }
}
