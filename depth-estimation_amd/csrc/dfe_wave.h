// dfe_wave.h -- device primitives over a wave or a DPP row of it: the reductions of the soft-min and of the cost-volume epilogues, and the
// one exponential every soft-min goes through.  gfx950 (DPP, v_permlane16_swap / v_permlane32_swap); everything stays on the VALU.
#pragma once
#include <hip/hip_runtime.h>

// All-lanes MINIMUM of EIGHT ints per lane (one per column) in ~40 VALU ops instead of 8 x 6 steps: a halving
// butterfly -- after exchanging with lane^1, lane^2, lane^4 each lane is left with the single column (lane & 7), then
// the row rotate by 8 and gfx950's v_permlane16_swap / v_permlane32_swap finish it.  Everything stays on the VALU (DPP
// quad permutes / row rotates fold into v_min_i32_dpp; no LDS crossbar).  On return every lane holds the wave minimum
// of column (lane & 7).
template <int TX> __device__ __forceinline__ int wave_min8(const int (&k)[TX], int lane) {
    static_assert(TX == 8, "butterfly is written for 8 columns");
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
    int a[4], b[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int mine = b0 ? k[2 * i + 1] : k[2 * i], other = b0 ? k[2 * i] : k[2 * i + 1];
        a[i] = min(mine, __builtin_amdgcn_update_dpp(0, other, 0xB1, 0xf, 0xf, false));     // quad_perm [1,0,3,2]
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int mine = b1 ? a[2 * i + 1] : a[2 * i], other = b1 ? a[2 * i] : a[2 * i + 1];
        b[i] = min(mine, __builtin_amdgcn_update_dpp(0, other, 0x4E, 0xf, 0xf, false));     // quad_perm [2,3,0,1]
    }
    int c;
    {
        // row_ror:4 -- quad q takes from quad q+1 (mod 4): even quads (bit2 = 0) read an odd quad and vice versa, and
        // the following ror:8 completes the row whichever neighbour was used.
        const int mine = b2 ? b[1] : b[0], other = b2 ? b[0] : b[1];
        c = min(mine, __builtin_amdgcn_update_dpp(0, other, 0x124, 0xf, 0xf, false));
    }
    c = min(c, __builtin_amdgcn_update_dpp(0, c, 0x128, 0xf, 0xf, false));                  // row_ror:8
    {   // gfx950 lane-swap instructions keep the cross-row steps on the VALU (no LDS-pipe swizzle/bpermute)
        const auto r = __builtin_amdgcn_permlane16_swap(c, c, false, false);                // rows {0,1} and {2,3} pair up
        c = min((int)r[0], (int)r[1]);
        const auto q = __builtin_amdgcn_permlane32_swap(c, c, false, false);                // halves pair up
        c = min((int)q[0], (int)q[1]);
    }
    return c;
}

// exp(x) for x <= 0 -- the soft-min's arguments, -c - max(-c): v_exp_f32 on x * log2(e), two instructions.  The product's rounding
// moves the result by |x| * 2^-24 relative at most, i.e. by less than 4e-8 ABSOLUTE for every x <= 0 (|x| e^x <= 1/e), against the
// 1e-6 the soft-min is held to (the reference's own nn.SoftMax of that era used a polynomial exp: its numerics are
// unpinned anyway).  Round 2 had the library expf without its overflow branch (Cody-Waite reduction + ldexp: 7 instructions, 13 in
// the library form) -- the 64 calls per pixel were 60 % of the finest cascade kernel's arithmetic.  EVERY soft-min on the device goes
// through this function, so the staged and the one-call paths stay bit-identical to each other.
__device__ __forceinline__ float dfe_exp_nonpos(float x) {
    return __builtin_amdgcn_exp2f(x * 0x1.715476p+0f);
}

// wave reductions of the soft-min (multiscale.hip and the volume kernel's soft-min epilogue): everything on the VALU
__device__ __forceinline__ float wave_max_f32(float v) {
#define DFE_STEP(ctrl) v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false)))
    DFE_STEP(0xB1); DFE_STEP(0x4E); DFE_STEP(0x124); DFE_STEP(0x128);   // quad_perm [1,0,3,2], [2,3,0,1], row_ror:4, row_ror:8
#undef DFE_STEP
    const int b = __float_as_int(v);
    const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    v = fmaxf(__int_as_float((int)r[0]), __int_as_float((int)r[1]));
    const int c = __float_as_int(v);
    const auto q = __builtin_amdgcn_permlane32_swap(c, c, false, false);
    return fmaxf(__int_as_float((int)q[0]), __int_as_float((int)q[1]));
}
// wave sum in the association order of `for (off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off)` -- partners at
// distance 32, 16, 8, 4, 2, 1 -- on the VALU only (lane swaps + DPP), bit-identical to the shuffle version: after the
// distance-8 step lanes L and L^8 hold equal values, so row_ror:4 (partner (L+4) mod 16) reads the same number as L^4
__device__ __forceinline__ float wave_sum_f32_ordered(float v) {
    int b = __float_as_int(v);
    const auto q = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    v = __int_as_float((int)q[0]) + __int_as_float((int)q[1]);
    b = __float_as_int(v);
    const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    v = __int_as_float((int)r[0]) + __int_as_float((int)r[1]);
#define DFE_STEP(ctrl) v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false))
    DFE_STEP(0x128); DFE_STEP(0x124); DFE_STEP(0x4E); DFE_STEP(0xB1);   // row_ror:8, row_ror:4, quad_perm [2,3,0,1], [1,0,3,2]
#undef DFE_STEP
    return v;
}

// Reductions over the 16 lanes of a DPP row (lanes 16 r .. 16 r + 15), partners at distance 8, 4, 2, 1: the soft-max of windows of more
// than 64 cells gives a pixel to 16 lanes (softmin_body in multiscale.hip and the feature matcher's soft-max epilogue share this order,
// so the one-call single-scale model equals the staged modules bit for bit)
__device__ __forceinline__ float row16_max_f32(float v) {
#define DFE_STEP(ctrl) v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false)))
    DFE_STEP(0x128); DFE_STEP(0x124); DFE_STEP(0x4E); DFE_STEP(0xB1);   // row_ror:8, row_ror:4, quad_perm [2,3,0,1], [1,0,3,2]
#undef DFE_STEP
    return v;
}
__device__ __forceinline__ float row16_sum_f32_ordered(float v) {
#pragma clang fp contract(off)
#define DFE_STEP(ctrl) v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false))
    DFE_STEP(0x128); DFE_STEP(0x124); DFE_STEP(0x4E); DFE_STEP(0xB1);
#undef DFE_STEP
    return v;
}
// (value, index) -> the row's largest value and, among equal values, the smallest index
__device__ __forceinline__ void row16_argmax_first(float &b, int &bi) {
#define DFE_STEP(ctrl)                                                                                        \
    {                                                                                                         \
        const float ob = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(b), ctrl, 0xf, 0xf, false)); \
        const int oi = __builtin_amdgcn_update_dpp(0, bi, ctrl, 0xf, 0xf, false);                             \
        if (ob > b || (ob == b && oi < bi)) { b = ob; bi = oi; }                                              \
    }
    DFE_STEP(0x128); DFE_STEP(0x124); DFE_STEP(0x4E); DFE_STEP(0xB1);
#undef DFE_STEP
}

// Eight wave reductions at once, "transposed": v[x] is pixel x's value in this lane's cell; the butterfly's first three steps pair
// up REGISTERS as well as lanes (v_permlane32_swap / v_permlane16_swap exchange half-waves / rows between two registers, so one swap
// + one op serves two pixels), halving the live registers at every step, and the last three run on one register.  The result for
// pixel g ends up in lane 8 g.  Partners at distance 32, 16, 8, 4, 2, 1 and the lower lane's value on the left of every +: the sum
// has the association of wave_sum_f32_ordered / px_softmin64 bit for bit.  18 VALU operations instead of 8 x 12.
// OP 0: fp32 sum; 1 / 2: minimum / maximum of NON-NEGATIVE floats, taken on their bit patterns as integers (the same order, and no
// canonicalising v_max x, x, x in front of every operand the way fminf / fmaxf compile).
template <int OP>
__device__ __forceinline__ int wave_reduce8_op(int a, int b) {
#pragma clang fp contract(off)
    return OP == 0 ? __float_as_int(__int_as_float(a) + __int_as_float(b)) : OP == 1 ? min(a, b) : max(a, b);
}
template <int OP>
__device__ __forceinline__ int wave_reduce8_transposed(const float (&v)[8], int lane) {
    int r1[4], r2[2];
#pragma unroll
    for (int x = 0; x < 4; ++x) {        // lanes < 32: pixel x, lanes >= 32: pixel x + 4
        const auto q = __builtin_amdgcn_permlane32_swap(__float_as_int(v[x]), __float_as_int(v[x + 4]), false, false);
        r1[x] = wave_reduce8_op<OP>((int)q[0], (int)q[1]);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {        // rows 0..3: pixels x, x + 2, x + 4, x + 6
        const auto q = __builtin_amdgcn_permlane16_swap(r1[x], r1[x + 2], false, false);
        r2[x] = wave_reduce8_op<OP>((int)q[0], (int)q[1]);
    }
    const bool up = (lane & 8) != 0;     // from here on lane L works for pixel L >> 3
    const int keep = up ? r2[1] : r2[0], send = up ? r2[0] : r2[1];
    int r = wave_reduce8_op<OP>(keep, __builtin_amdgcn_update_dpp(0, send, 0x128, 0xf, 0xf, true));                  // row_ror:8
    r = wave_reduce8_op<OP>(r, __builtin_amdgcn_update_dpp(0, r, 0x104, 0xf, 0xf, true));                           // row_shl:4 (lane j reads lane j + 4)
    r = wave_reduce8_op<OP>(r, __builtin_amdgcn_update_dpp(0, r, 0x4E, 0xf, 0xf, true));                            // quad_perm [2,3,0,1]
    r = wave_reduce8_op<OP>(r, __builtin_amdgcn_update_dpp(0, r, 0xB1, 0xf, 0xf, true));                            // quad_perm [1,0,3,2]
    return r;                             // lane 8 g: pixel g (other lanes: partial results)
}
