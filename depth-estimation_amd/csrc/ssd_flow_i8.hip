// ssd_flow_i8.hip -- the single-scale flow step's sweep on the int8 matrix cores, for byte-valued frames (C = 3, k = 7, 33 x 33).
//
// For frames whose values are integers in 0..255 every partial sum of the SSD is an integer below 2^24: the float sweep
// (ssd_cv_rowimg_flow_kernel) is exact on them and any exact integer evaluation gives the same bits.  With a' = a - 128, b' = b - 128
//     cost(x, d) = S0(x) + S1(x + d) - 2 a'.b'
// where a'.b' is a dot product over the 147 taps of the patch: v_mfma_i32_16x16x64_i8.
//
// Layout.  A frame is packed to 4 bytes per pixel (three channels - 128, one zero byte), row pitch Wp pixels, zero (a' = 0) beyond the
// frame's width; the patch sums S0 / S1 are planes of the same pitch (the pack kernel makes both).  One wave owns a strip of 16 pixels (MFMA N side) of R
// consecutive output rows; the 48 candidate columns q = n + dx of a displacement row are three tiles of 16 on the M side.  A lane (n, g)
// of a result tile holds candidates q = 16 T + 4 g + i, i = 0..3, of ONE pixel n, so the running arg-min is lane-local.
// K = 256 = 4 MFMAs: lane groups 0, 1 hold patch rows 0..3 (one per MFMA; left / right four pixels of the row), groups 2, 3 hold rows 3..6;
// the frame-0 operand, which stays in registers for the whole strip, is zero in the duplicate row 3 and in the eighth pixel.  A frame-1
// fragment of image rows (r .. r+3) at displacement row dy is the fragment of rows (r-1 .. r+2) at dy + 1: the four fragments of a tile
// rotate through registers (the sweep runs in rounds of four steps) and every step loads ONE new 16-byte piece per lane and tile, into the
// registers of the oldest fragment, right after the step's MFMAs that read it: after a round every fragment is back where it started and
// nothing is copied.  The row addresses are scalar; a lane adds one 64-bit base per frame-1 row, made once per item.
//
// The plane ring.  A step wants 48 cells (192 B) of ONE S1-plane row, the same for all sixteen lanes of a lane group: read from memory as
// three 16-byte loads per lane that is three wave-loads of 1 KiB for 64 distinct bytes each.  So each wave keeps four plane rows in LDS
// (I8Ring: 4 slots x 64 cells, 1 KiB per wave; the block's LDS goes from 26112 to 30208 B, still more than three blocks per CU need): slot
// s & 3 holds plane row y0 + s, cells x0 .. x0 + 63 (x0 + 63 < Wp).  A step loads, per wave, ONE 256-byte row (buffer_load_dword: cell
// x0 + lane of row y0 + s + 4, the plane as a buffer of (H + 1) Wp cells, the row a scalar offset) and the three fragment pieces, and reads
// its three quads with broadcast ds_read_b128 at 16 g + 64 T + 256 (s & 3), immediates on one address register: 3.25 KiB through the vector
// memory path per step where 6 KiB went.  The row rides one step in a register (stg) and is written to its slot, (s + 3) & 3, at the top
// of the next step: the compiler counts that wait per register (s_waitcnt vmcnt(3): the three fragment loads issued behind it stay in
// flight), which it does not do for an LDS-DMA load, whose every ring read it fences with vmcnt(0) (1 us gained at VGA where this form gains 6.7; EXPERIMENTS.md,
// round 15).  Rows 0..3 are staged with the item's operands; no row beyond the last one a step consumes, y0 + 32 + R - 1, is loaded; the
// fall-back sweep, rare, keeps its loads from memory.  What orders the slots' reads and refills: the comment at the ring, in `step`.
//
// Two rows per item (R = 2).  At step s the fragments F_t = frame-1 rows (y0 + s + t | y0 + s + t + 3) serve row y0 at dy = s and row
// y0 + 1 at dy = s - 1, which also share the S1-plane row y0 + s.  Both compare frame-0 image rows y0 + 17 .. y0 + 22 with the same six
// frame-1 rows, one step apart: the product of frame-0 row Z with frame-1 row Z - 16 + dy is patch row Z - y0 - 16 of row y0 and patch
// row Z - y0 - 17 of row y0 + 1.  So a step forms, per tile,
//     C(s) = F_1.B[1] + F_2.B[2] + F_3.B[3]     (3 MFMAs)    B[t] = frame-0 rows (y0 + 16 + t | y0 + 19 + t), row y0's operands
//     D0   = C(s) + F_0.B[0]                    (1 MFMA)     row y0, dy = s: its patch row 0 (the duplicate row 3 of B[0] is zero)
//     D1   = C(s - 1) + F_3.Bbot                (1 MFMA)     row y0 + 1, dy = s - 1: its patch row 6, Bbot = (zero | frame-0 row y0 + 23)
// 15 MFMAs per step against the 12 of a one-row item (two independent chains of four would be 24).  C(s - 1) is carried in 12 registers;
// the round of four steps makes that a renaming, like the fragments.  Step 0 has no D1, step 33 nothing else.  D0's MFMA is the last to
// read F_0, so the step's load goes into F_0's registers behind it: issuing F_0's product first into an accumulator of its own and
// adding it to C with vector instructions keeps the load early but costs 4 v_add per tile, 24 v_mov_b64 on the back edge and 163 VGPRs
// (288 vector instructions per four steps against 216; not shipped).
//
// Arg-min.  A lane keeps four running keys, one per i: key = ((2 a'.b' - S1) << 7) + order, maximised; the plane cell of frame-1 row y1,
// column q holds Z - (S1 << 7) - 3 y1 - (q >> 4), so a key is ONE v_lshl_add of the MFMA result, (D << 8) + P, and nothing else is kept
// per tile: for the item's row y0 + r the candidate j = 3 dy + T (sweep order) lies in row y1 = y0 + r + dy and column block x0 / 16 + T,
// where the plane's term is -j - base, base = 3 (y0 + r) + x0 / 16 the same for all of the row's candidates.  An earlier candidate has
// the larger term and wins a tie; the terms of two candidates of one pixel differ by at most 98 < 128, so the term never outweighs a
// difference of the costs and need not be reduced.  The decode adds base back; which of a pixel's candidates i (and lane groups g) comes
// first is decided there, on (cost, index).
// The window.  Candidates outside 0 <= q - n <= 32 (first and third tile) are never selected out: their dot product STARTS from a penalty.
// The accumulator of the first / third tile starts from a per-lane quad (pen0 / pen2, made once per item) that holds kKeyPen = Q / 2 for a
// masked (g, i, n) and 0 otherwise -- the MFMA's C operand, so no instruction -- and a masked key is the key of E + Q.  E = 2 a'.b' - S1
// lies in [-7187712, 2408448] (147 taps of 2 * 127 * -128 - 128^2 .. 2 * 128 * 128 - 128^2) for masked candidates too (they read packed
// bytes, or zero beyond the frame), a span of 9596160: with Q = -10485760 every masked key of a pixel lies below every valid one, and as
// every running key sees tile 1, which is never masked, none ends on a masked candidate.  In a two-row item the penalty rides in C(s) and
// so reaches D0 and the next step's D1, whose masks are the same.  Range, with Z = 2^30: valid keys lie in [Z - 0.920e9 - order,
// Z + 0.308e9], masked ones from Z - 2.262e9 - order; dfe_flow_i8_plan admits (H + 1) Wp < 2^29 with Wp >= 80, so order = 3 y1 + (q >> 4)
// + 98 < 3 * 2^29 / 80 + 2^29 / (40 * 16) < 2.2e7: every key, and the decode's base + 127 - Z added to a valid one, stays inside 32 bits
// (tests/test_flow_i8_key7_cpu.py).  Per tile that is 4 v_lshl_add_u32 and 2 v_max3_i32 (the twelve keys of a row's step fold in six,
// a tile's keys paired with the same i of the neighbouring tile); with the fragment row's address a two-row step issues 37 vector instructions
// beside its 15 MFMAs, a one-row step 19 beside 12.
//
// Items.  flow_i8_items.h splits the rows into two-row and one-row wave items from the number of waves the device holds at once.
//
// Finalize.  At the end of an item the wave holds all that the finalize of its 16 x R pixels wants -- the minimum and its first index in
// registers, the centre cost and the lead cells in its LDS image -- so it writes their results itself (i8_finalize: the rules of
// dfe_finalize_rec_pixel, cv_records.h), lane group r the pixels of row r; no record goes to memory and comes back.  For a pixel with
// fewer than M lead cells above the threshold the first M hits in index order come from a second sweep of that strip row, which ranks
// the hits of a tile with ballots, leaves them in LDS and stops when every flagged pixel has M.
//
// The gate.  A block of the pack kernel that meets a value that is not an integer in 0..255 raises the step's verdict word; this kernel
// returns at entry when it is set.  A ctx has three such words, taken in turn: the pack kernel of step i clears the word of step i + 1, so
// nothing has to be reset between calls.  ONE launch follows (ssd_cv_rowimg_flow_gated_kernel, ssd_cost_volume.hip): it writes the
// frame's border, which no sweep writes, and reads the same word -- clear: nothing more; set: the float sweep and the finalize of its records.
#include "dfe_internal.h"
#include "cv_records.h"
#include "flow_i8_items.h"
#include "flow_border.h"
#include <algorithm>
#include <climits>

typedef int i8x16_t __attribute__((ext_vector_type(4)));   // 16 bytes of an MFMA operand / four i32 results

struct I8Args {
    const unsigned *pk0, *pk1;   // packed frames [H][Wp]
    const int *s0, *s1k;         // patch sums of frame 0 (plain) and frame 1 (as the key's addend: kKeyZ - (S1 << 7) - 3 y - (x >> 4)) [H][Wp]
    const unsigned *verdict;     // != 0: the frames are not byte-valued
    TailOut o;                   // where the wave's pixels go (cv_records.h)
    float thr;
    int M, middle;
    int Ho, Wo, Wp, nstrips, nrp;
    int n2, row0, nitems;        // flow_i8_items.h
};

constexpr int kI8Waves = 4;
// the key (header: Arg-min): the plane's offset Z, and the start value of a masked candidate's accumulator, Q / 2 in units of a'.b'
constexpr int kKeyZ = 1 << 30;
constexpr int kKeyPen = -10485760 / 2;

// max(a, b, c) as ONE instruction, whatever the compiler would make of max(max(a, b), c)
__device__ __forceinline__ int i8_max3(int a, int b, int c) {
    int r;
    asm("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// ------------------------------------------------------------------------------------------
// pack: planes of floats or of bytes -> (c0 - 128, c1 - 128, c2 - 128, 0) per pixel and the 7 x 7 x 3 sums of squares, one 32 x 32 tile per
// block (read with its 6-pixel halo).  Float planes: a block that meets a value that is not an integer in 0..255 raises the call's
// verdict word.  Byte planes (the byte entries at scale 1: any address, any W) raise nothing; with BORDER the z = 0 blocks also write the
// frame's border (flow_border.h), so that the int8 sweep is the only launch behind this one.  Both forms clear the NEXT call's word.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool i8_byte(float v, unsigned *b) {
    const bool ok = v >= 0.f && v <= 255.f && v == truncf(v);   // (NaN fails every comparison; -0.0 is 0)
    *b = ok ? (unsigned)((int)v - 128) & 255u : 0u;
    return ok;
}
__device__ __forceinline__ bool i8_byte(unsigned char v, unsigned *b) {
    *b = (unsigned)((int)v - 128) & 255u;
    return true;
}
__device__ __forceinline__ int i8_sq(unsigned p) {
    const int a = (int)(p << 24) >> 24, b = (int)(p << 16) >> 24, c = (int)(p << 8) >> 24;
    return a * a + b * b + c * c;
}
template <bool BORDER> struct I8PackBorder {};
template <> struct I8PackBorder<true> { TailOut o; int Ho; };
constexpr int kPackW = 32, kPackH = 32, kPackLW = kPackW + 6, kPackLH = kPackH + 6;
template <typename T, bool BORDER>
__global__ __launch_bounds__(256) void flow_i8_pack_kernel(const T *__restrict__ I0, const T *__restrict__ I1, int H, int W, long long plane, int Wp,
                                                           unsigned *__restrict__ pk0, unsigned *__restrict__ pk1, int *__restrict__ s0, int *__restrict__ s1k,
                                                           unsigned *__restrict__ verdict, unsigned *__restrict__ verdict_next, I8PackBorder<BORDER> bd) {
    constexpr bool BYTES = sizeof(T) == 1;
    static_assert(BYTES || !BORDER, "the border rides on the byte form");
    __shared__ int sq[kPackLH][kPackLW + 1];
    __shared__ int hs[kPackLH][kPackW];
    if constexpr (BORDER) {   // (at most 2^21 blocks of a frame with H W < 2^31: the thread index stays inside 31 bits)
        if (blockIdx.z == 0)
            dfe_flow_border(bd.o, bd.Ho, (int)((blockIdx.y * gridDim.x + blockIdx.x) * 256u + threadIdx.x), (int)(gridDim.x * gridDim.y * 256u));
    }
    const T *I = blockIdx.z ? I1 : I0;
    unsigned *pk = blockIdx.z ? pk1 : pk0;
    const int tx0 = blockIdx.x * kPackW, ty0 = blockIdx.y * kPackH;
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *verdict_next = 0u;   // (the NEXT call's word: no reset launch)
    bool bad = false;
    // every load of the thread is issued before the first is used: one memory latency, not one per trip.  The addresses are clamped into the
    // frame, so no load hangs on a branch; what lies outside the tile's image or outside the frame is dropped afterwards
    constexpr int NT = (kPackLH * kPackLW + 255) / 256;
    T v[NT][3];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int e = threadIdx.x + 256 * j;
        const int ly = e / kPackLW, lx = e - ly * kPackLW;
        const T *s = I + (long long)min(ty0 + ly, H - 1) * W + min(tx0 + lx, W - 1);
        v[j][0] = s[0];
        v[j][1] = s[plane];
        v[j][2] = s[2 * plane];
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int e = threadIdx.x + 256 * j;
        const int ly = e / kPackLW, lx = e - ly * kPackLW;
        const int gy = ty0 + ly, gx = tx0 + lx;
        unsigned b0, b1, b2;
        const bool ok0 = i8_byte(v[j][0], &b0), ok1 = i8_byte(v[j][1], &b1), ok2 = i8_byte(v[j][2], &b2);
        const bool in = gy < H && gx < W;   // (beyond the halo image, e >= kPackLH * kPackLW, nothing is written either)
        bad |= in && !(ok0 && ok1 && ok2);
        const unsigned p = in ? b0 | (b1 << 8) | (b2 << 16) : 0u;
        if (ly < kPackH && lx < kPackW && gy < H && gx < Wp) pk[(long long)gy * Wp + gx] = p;
        if (ly < kPackLH) sq[ly][lx] = i8_sq(p);
    }
    if constexpr (BYTES) {
        __syncthreads();
    } else {
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (any && threadIdx.x == 0) atomicOr(verdict, 1u);
    }
    for (int e = threadIdx.x; e < kPackLH * kPackW; e += 256) {
        const int ly = e / kPackW, lx = e - ly * kPackW;
        hs[ly][lx] = sq[ly][lx] + sq[ly][lx + 1] + sq[ly][lx + 2] + sq[ly][lx + 3] + sq[ly][lx + 4] + sq[ly][lx + 5] + sq[ly][lx + 6];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kPackH * kPackW; e += 256) {
        const int ly = e / kPackW, lx = e - ly * kPackW;
        const int gy = ty0 + ly, X = tx0 + lx;
        if (gy >= H || X >= Wp) continue;
        const int v = hs[ly][lx] + hs[ly + 1][lx] + hs[ly + 2][lx] + hs[ly + 3][lx] + hs[ly + 4][lx] + hs[ly + 5][lx] + hs[ly + 6][lx];
        const long long o = (long long)gy * Wp + X;
        if (blockIdx.z) s1k[o] = kKeyZ - (v << 7) - 3 * gy - (X >> 4);
        else s0[o] = v;
    }
}

// ------------------------------------------------------------------------------------------
// the sweep of one strip (16 pixels) over R output rows
// ------------------------------------------------------------------------------------------
constexpr int kCostPitch = 33;   // floats per pixel of the wave's lead-cell image in LDS (32 candidates, odd pitch)
template <int R> struct I8Lds {
    float cost[R][16][kCostPitch];   // displacement row 0, tiles 0 and 1: cost[n][q]
    float cen[R][16];                // the centre cell's cost of pixel n
    int sa[R][16];                   // S0 of pixel n: wanted in the peeled steps and at the end only, so not held in a register
    float fbh[R][16][DFE_FB];        // a flagged pixel's hits of the fall-back sweep: M (value, 1-based index) pairs, zero-padded
};

constexpr int kRingRow = 64;   // cells of a ring slot: the 48 a step reads and 16 that ride along in the 256-byte staging load
struct I8Ring { int row[4][kRingRow]; } __attribute__((aligned(16)));

template <int R, bool FB> struct I8Sweep {
    static constexpr int NS = 33 + R - 1;
    const I8Args &a;
    const int lane, n, g, x0, y0;
    i8x16_t A[3][4], B[4];
    i8x16_t Bbot, C[3];    // R == 2: frame-0 row y0 + 23 (row y0 + 1's own patch row) and the shared rows' products of the step before
    i8x16_t pen0, pen2;    // the first / third tile's accumulators start here: kKeyPen where candidate 4 g + i lies outside 0 <= q - n <= 32, else 0
    int best[R][4];        // the running key of candidates i, i = 0..3
    int held[R][4];        // a tile's keys that wait for the next tile's, their partners in one v_max3
    unsigned lo1, lop;     // the lane's byte offsets inside a row of the packed frame 1 and of the S1 plane (FB) / of a ring slot
    int *ring;             // !FB: the wave's four plane rows in LDS (the ring, below)
    __amdgpu_buffer_rsrc_t prs;   // !FB: the S1 plane as a buffer, (H + 1) Wp cells: a staging load is row (scalar offset) + 4 lane, no address arithmetic
    int stg;               // !FB: the plane row on its way into the ring: cell x0 + lane of row y0 + s + 3 at the top of step s
    // FB
    int sa[R];             // S0 of the lane's pixel (the sweep proper reads it from its LDS image)
    int cnt;
    bool flagged;
    float *fbp;
    I8Lds<(FB ? 1 : R)> *lds;

    __device__ __forceinline__ I8Sweep(const I8Args &a_, int lane_, int x0_, int y0_)
        : a(a_), lane(lane_), n(lane_ & 15), g(lane_ >> 4), x0(x0_), y0(y0_) {}

    __device__ __forceinline__ void load_operands() {
        const int h = g & 1, up = g >> 1;
        if constexpr (!FB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pen0[i] = 4 * g + i >= n ? 0 : kKeyPen;
                pen2[i] = 4 * g + i <= n ? 0 : kKeyPen;
            }
        }
        // frame 0: patch rows (0..3 | 3..6) of row y0's pixel n, zero in the duplicate row 3 and in the eighth pixel.  R == 2: image rows
        // y0 + 17 .. y0 + 22 of these are row y0 + 1's patch rows 0..5 as well; its patch row 6, image row y0 + 23, is Bbot's upper half
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned *p = a.pk0 + (y0 + 16 + t + 3 * up) * a.Wp + x0 + n + 16 + 4 * h;
            i8x16_t v = *reinterpret_cast<const i8x16_t *>(p);
            if (h) v[3] = 0;
            if (up && t == 0) v = i8x16_t{0, 0, 0, 0};
            B[t] = v;
        }
        if constexpr (R == 2) {
            Bbot = *reinterpret_cast<const i8x16_t *>(a.pk0 + (y0 + 23) * a.Wp + x0 + n + 16 + 4 * h);
            if (h) Bbot[3] = 0;
            if (!up) Bbot = i8x16_t{0, 0, 0, 0};
        }
        // frame 1: the fragments of displacement row 0.  A lane's byte offset from (row, x0) is the same for the whole item: fragment rows
        // (+ 0 | + 3 rows, pixel n + 4 h) and plane cells (4 g); at most 4 (3 Wp + 19) < 2^32 as (H + 1) Wp < 2^29, the tile's 64 T an immediate
        lo1 = 4u * (unsigned)(3 * up * a.Wp + n + 4 * h);
        lop = 16u * (unsigned)g;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const char *frow = reinterpret_cast<const char *>(a.pk1 + (y0 + t) * a.Wp + x0);
#pragma unroll
            for (int T = 0; T < 3; ++T) A[T][t] = *reinterpret_cast<const i8x16_t *>(frow + lo1 + 64 * T);
        }
        // the ring's first four rows: slot t = plane row y0 + t, cells x0 .. x0 + 63 (x0 + 63 < Wp: dfe_flow_i8_plan)
        if constexpr (!FB) {
            prs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int *>(a.s1k), 0, 4 * (a.Ho + DFE_FLOW_MARGIN + 1) * a.Wp, 0x00020000);
#pragma unroll
            for (int t = 0; t < 4; ++t) ring[kRingRow * t + lane] = __builtin_amdgcn_raw_buffer_load_b32(prs, 4 * lane, 4 * ((y0 + t) * a.Wp + x0), 0);
            __builtin_amdgcn_wave_barrier();
        }
    }

    // the keys of one result tile D of row y0 + r, and the row's lead cells (sr == 0) and centre cell (sr == 16) where the step is the peeled
    // one that holds them: sr is the row's displacement row there, anything else in the steady state.  A masked candidate's D carries
    // kKeyPen, so its key lies below every valid key of the pixel and nothing selects.  The row's running keys take the tiles in pairs, one
    // v_max3 per i and pair: tiles (0, 1) of an even displacement row (`odd` false), whose tile 2 waits in `held` for tile 0 of the odd row
    // behind it, which pairs its own tiles (1, 2).  Displacement row 32 (sr == 32, even) has no row behind it: its tile 2 takes a v_max.
    __device__ __forceinline__ void take(int T, int r, int sr, bool odd, const i8x16_t &D, const i8x16_t &P, int pb) {
        const bool hold = odd ? T == 1 : T != 1, alone = sr == 32 && T == 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = (int)((unsigned)D[i] << 8) + P[i];
            if (alone) best[r][i] = max(best[r][i], k);
            else if (hold) held[r][i] = k;
            else best[r][i] = i8_max3(best[r][i], held[r][i], k);
        }
        // S1 back from the plane cell: P - Z + pb + T = -(S1 << 7) exactly.  In tile 0 the cells q < n hold the penalty: i8_item reads
        // cost[n][q] at q = n + k, k = 0..7, only
        if (T < 2 && sr == 0) {   // the lead cells' row
#pragma unroll
            for (int i = 0; i < 4; ++i) lds->cost[r][n][16 * T + 4 * g + i] = (float)(lds->sa[r][n] - ((P[i] + (pb - kKeyZ + T)) >> 7) - 2 * D[i]);
        }
        if (T == 1 && sr == 16) {   // the centre cell: dx = 16, q = 16 + n (tile 1: no penalty)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * g + i == n) lds->cen[r][n] = (float)(lds->sa[r][n] - ((P[i] + (pb - kKeyZ + T)) >> 7) - 2 * D[i]);
        }
    }

    // one step: frame-1 rows y0 + s ..; PH = s mod 4, the rotation of the fragment registers.  S is the step's number where the step is one of
    // the peeled ones (the lead cells' rows, the centre cells' rows, the two edge steps of a two-row item, the last step), -1 in the steady state,
    // which tests nothing.  The fallback sweep (R = 1: every step is a displacement row) takes all of it at run time.
    template <int PH, int S> __device__ __forceinline__ void step(int s) {
        const bool more = FB ? s + 1 < NS : S != NS - 1;
        const int pb = 3 * (y0 + s) + (x0 >> 4);   // the plane's order term of tile 0 of this row, taken off where S1 itself is wanted
        // the rows' addresses live in scalar registers; a lane adds its offset (load_operands; the compiler keeps it as a 64-bit base and adds
        // the scalar row with one v_lshl_add_u64) and the tile's 64 T bytes
        const char *frow = reinterpret_cast<const char *>(a.pk1 + (y0 + s + 4) * a.Wp + x0);   // the one new row of the next step's fragments (rows s + 4 | s + 7)
        const unsigned lo1 = this->lo1, lop = this->lop;
        i8x16_t P[3];
        if constexpr (FB) {
            const char *prow = reinterpret_cast<const char *>(a.s1k + (y0 + s) * a.Wp + x0);
#pragma unroll
            for (int T = 0; T < 3; ++T) P[T] = *reinterpret_cast<const i8x16_t *>(prow + lop + 64 * T);
        } else {
            // The ring.  Slot PH holds plane row y0 + s: the step's three quads are broadcast reads at 16 g + 64 T, immediates on one address
            // register.  The row on its way in (stg, loaded at the step before: row y0 + s + 3) goes to slot (PH + 3) & 3, which step s - 1
            // read and whose next reader is step s + 3; then row y0 + s + 4 is loaded into stg.  The last rows a sweep consumes are
            // y0 + NS - 1: the peeled steps past it load and write nothing, the steady ones (s <= 31) clamp the row, so the two or three
            // loads past the end fetch row y0 + NS - 1 again, into a slot that no later step reads.
            // Order.  (1) A slot's read stands behind the write that filled it: both are LDS instructions of ONE wave, which the LDS
            // executes in issue order, and the compiler keeps the ds_write_b32 above the wave barrier and the ds_read_b128 below it; the
            // write itself waits for its row with the s_waitcnt vmcnt(3) in front of it (counted: the three fragment loads issued behind
            // stg's stay in flight; tools/i8_loop_hist.py prints the loops' waits).  (2) A slot's refill, that ds_write_b32, stands behind the
            // slot's reads for the same reason, three steps later in issue order, and the reads' data is in registers (the s_waitcnt
            // lgkmcnt in front of `take`'s v_lshl_add_u32) long before that.  No other wave touches the ring.
            constexpr bool wr = S < 0 || (S >= 1 && S + 3 <= NS - 1), ld = S < 0 || S + 4 <= NS - 1;
            if constexpr (wr) ring[kRingRow * ((PH + 3) & 3) + lane] = stg;
            __builtin_amdgcn_wave_barrier();
            if constexpr (ld) stg = __builtin_amdgcn_raw_buffer_load_b32(prs, 4 * lane, 4 * ((y0 + min(s + 4, NS - 1)) * a.Wp + x0), 0);
            const char *slot = reinterpret_cast<const char *>(ring + kRingRow * (PH & 3));
#pragma unroll
            for (int T = 0; T < 3; ++T) P[T] = *reinterpret_cast<const i8x16_t *>(slot + lop + 64 * T);
        }
#pragma unroll
        for (int T = 0; T < 3; ++T) {
            // the tile's accumulator starts from the window's penalty quad (the MFMA's C operand: no instruction); the fall-back sweep
            // forms costs from D and tests `valid` itself: it starts from zero
            const i8x16_t c0 = FB || T == 1 ? i8x16_t{0, 0, 0, 0} : T == 0 ? pen0 : pen2;
            if constexpr (R == 2) {
                // Row y0 at dy = s and row y0 + 1 at dy = s - 1 compare frame-0 rows y0 + 17 .. y0 + 22 with the same six frame-1 rows, a
                // step apart: C, the three MFMAs of fragments 1..3, is row y0's patch rows 1..6 now and row y0 + 1's patch rows 0..5 at the
                // next step.  Each row adds the one patch row of its own: 5 MFMAs where two chains of four stood.  Step 0 has no row y0 + 1
                // yet, step 33 nothing but its last patch row; C passes from step to step through the round's renaming, like the fragments
                constexpr bool first = S == 0, last = S == NS - 1;
                i8x16_t D0, D1;
                if (!first) D1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[T][(3 + PH) & 3], Bbot, C[T], 0, 0, 0);
                if (!last) {
                    i8x16_t c = c0;   // in C(s), so in D0 and in the next step's D1: the two rows' masks are the same
#pragma unroll
                    for (int t = 1; t < 4; ++t) c = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[T][(t + PH) & 3], B[t], c, 0, 0, 0);
                    C[T] = c;
                    D0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[T][PH & 3], B[0], c, 0, 0, 0);
                    // D0's MFMA was the last reader of the oldest fragment: the new row is loaded into its registers, as in the one-row step
                    __builtin_amdgcn_sched_barrier(0);
                    A[T][PH & 3] = *reinterpret_cast<const i8x16_t *>(frow + lo1 + 64 * T);
                    take(T, 0, S, PH & 1, D0, P[T], pb);
                }
                if (!first) take(T, 1, S - 1, (PH + 1) & 1, D1, P[T], pb);
            } else {
                i8x16_t D = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[T][PH & 3], B[0], c0, 0, 0, 0);
                // the fragment of the oldest row has been read by the step's last MFMA that needs it: the new row is loaded into its registers, a
                // renaming and no copy.  The barrier keeps the scheduler from hoisting the load above those MFMAs, which costs spare fragments
                // (18 VGPRs more with R = 2, 28 with R = 1) and measured slower
                if (more) {
                    __builtin_amdgcn_sched_barrier(0);
                    A[T][PH & 3] = *reinterpret_cast<const i8x16_t *>(frow + lo1 + 64 * T);
                }
#pragma unroll
                for (int t = 1; t < 4; ++t) D = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[T][(t + PH) & 3], B[t], D, 0, 0, 0);
                if constexpr (!FB) {
                    take(T, 0, S, PH & 1, D, P[T], pb);
                } else {
                    // rank this tile's hits of every flagged pixel in candidate order: lane groups below mine, then my own earlier ones
                    bool hit[4];
                    float cv[4];
                    unsigned long long bal[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = 4 * g + i;
                        cv[i] = (float)(sa[0] - ((P[T][i] + (pb - kKeyZ + T)) >> 7) - 2 * D[i]);
                        bool valid = flagged;
                        if (T == 0) valid = valid && m >= n;
                        if (T == 2) valid = valid && m <= n;
                        hit[i] = valid && cv[i] > a.thr;
                        bal[i] = __builtin_amdgcn_ballot_w64(hit[i]);
                    }
                    const unsigned long long mine = 0x0001000100010001ull << n;
                    const unsigned long long below = mine & ((1ull << (16 * g)) - 1ull);
                    int k = cnt, tot = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        k += __builtin_popcountll(bal[i] & below);
                        tot += __builtin_popcountll(bal[i] & mine);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (hit[i]) {
                            if (k < a.M) {
                                fbp[2 * k] = cv[i];
                                fbp[2 * k + 1] = (float)(s * 33 + 16 * T + 4 * g + i - n + 1);
                            }
                            ++k;
                        }
                    }
                    cnt += tot;
                }
            }
        }
    }

    // four steps from step s on: S0 is the first one's number where the round holds peeled steps, -1 in the steady state
    template <int S0> __device__ __forceinline__ void round(int s) {
        step<0, S0 < 0 ? -1 : S0>(s);
        step<1, S0 < 0 ? -1 : S0 + 1>(s + 1);
        step<2, S0 < 0 ? -1 : S0 + 2>(s + 2);
        step<3, S0 < 0 ? -1 : S0 + 3>(s + 3);
    }

    __device__ __forceinline__ bool fb_done() const { return FB && __builtin_amdgcn_ballot_w64(flagged && cnt < a.M) == 0ull; }

    // The sweep proper runs whole rounds of four steps, after which every fragment is back in the registers it started in, and has no exit
    // inside a round; the lead cells' rows (steps 0 .. R - 1) lie in round 0, the centre cells' rows (16 .. 16 + R - 1) in round 4, and the
    // one or two steps past the eighth round stand alone.  The fallback sweep leaves as soon as every flagged pixel has its M hits.
    __device__ __forceinline__ void run() {
        if constexpr (FB) {
            for (int s = 0; s < NS; s += 4) {
                if (fb_done()) break;
                step<0, -1>(s);
                if (s + 1 >= NS) break;
                step<1, -1>(s + 1);
                if (s + 2 >= NS) break;
                step<2, -1>(s + 2);
                if (s + 3 >= NS) break;
                step<3, -1>(s + 3);
            }
        } else {
            round<0>(0);
#pragma nounroll
            for (int s = 4; s < 16; s += 4) round<-1>(s);
            round<16>(16);
#pragma nounroll
            for (int s = 20; s < 32; s += 4) round<-1>(s);
            step<0, 32>(32);
            if constexpr (R == 2) step<1, 33>(33);
        }
    }
};

__device__ __forceinline__ void i8_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The finalize of the lane's pixel (x, y) from what the wave holds: dfe_finalize_rec_pixel's rules (cv_records.h) for the 33 x 33 window,
// without the record in between.  d: 0-based first index of the minimum `best`; cen: the centre cell's cost; lead: the pixel's eight lead
// cells, hm: bit k set = lead cell k lies above the threshold; fbh: the hits of the fall-back sweep, read where `flag` is set.
template <int M>
__device__ __forceinline__ void i8_finalize(const TailOut &o, int middle, int y, int x, float best, float cen, int d, const float *lead, unsigned hm,
                                            bool flag, const float *fbh) {
    const long long pg = o.p_off + (y * o.Wo + x);                       // (Ho Wo < 2^31 and H W < 2^31: flow_pipeline_novol)
    const int fo = (y + o.row_off + o.pad_t) * o.pitch + x + o.pad_l;
    int id0 = d;
    if (middle > 0 && best == cen) id0 = middle - 1;
    if (o.idx) o.idx[pg] = (long long)id0 + 1;
    if (o.best) o.best[pg] = best;
    const int fl = id0 / 33;
    const float dyf = (float)(fl - 16), dxf = (float)(id0 - fl * 33 - 16);
    if (o.fy) o.fy[fo] = dyf;
    if (o.fx) o.fx[fo] = dxf;
    if (o.frame_H && o.depth) pair_depth_px(y + o.pad_t, x + o.pad_l, dyf, dxf, o.mw, o.mh, o.infty, &o.depth[fo], &o.conf[fo]);
    if (o.scores) {
        float hv[M], hi[M];
        if (flag) {   // rare: fewer than M lead cells pass; the fall-back sweep left the first M hits of the whole window, zero-padded
#pragma unroll
            for (int j = 0; j < M; ++j) { hv[j] = fbh[2 * j]; hi[j] = fbh[2 * j + 1]; }
        } else {      // the first M set bits of hm (at least M are set)
            unsigned h = hm;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const int k = __builtin_ctz(h | 0x100u);
                h &= h - 1u;
                hv[j] = lead[k];
                hi[j] = (float)(k + 1);
            }
        }
        if (hv[0] > 0) {
            if (M == 4) dfe_sort4(hv, hi); else dfe_sort8(hv, hi);
            if (o.imaxs) o.imaxs[pg] = (long long)hi[0];
#pragma unroll
            for (int j = 1; j < M; ++j) hv[j] += hv[j - 1];
            double acc = 0;
#pragma unroll
            for (int j = 0; j < M; ++j) acc += hv[j];
            if (o.padded) o.scores[fo] = (float)acc; else o.scores[pg] = (float)acc;
        } else if (o.padded) {
            o.scores[fo] = 0.f;
        }
    }
}

// one wave item: strip `strip`, rows y0 .. y0 + R - 1, of which it writes those from ylo on
template <int R> __device__ __forceinline__ void i8_item(const I8Args &a, I8Lds<R> *lds, I8Ring *ring, int lane, int strip, int y0, int ylo) {
    const int x0 = strip * 16;
    const int n = lane & 15, g = lane >> 4;

    I8Sweep<R, false> sw(a, lane, x0, y0);
    sw.lds = lds;
    sw.ring = &ring->row[0][0];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        for (int i = 0; i < 4; ++i) sw.best[r][i] = INT_MIN;
        lds->sa[r][n] = a.s0[(y0 + r + 16) * a.Wp + x0 + n + 16];
    }
    sw.load_operands();
    sw.run();
    i8_lds_fence();

    const int x = x0 + n;
    const bool xin = x < a.Wo;
    // lane group r finishes the pixels of row r: what it needs of that row
    int fE = 0, fd = 0, fsa = 0;
    unsigned fhm = 0;
    bool fflag = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        // (cost, index) of the lane's four running keys, then of the pixel's four lane groups.  Every running key has seen tile 1, which
        // is never masked: each holds a valid candidate
        long long kb = LLONG_MIN;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int bt = sw.best[r][i] + (3 * (y0 + r) + (x0 >> 4) + 127 - kKeyZ);   // (E << 7) + 127 - j
            const int j = 127 - (bt & 127);
            const int dy = j / 3, T = j - 3 * dy;
            const int d = dy * 33 + 16 * T + 4 * g + i - n;
            const long long k64 = ((long long)(bt >> 7) << 12) | (long long)(4095 - d);
            kb = k64 > kb ? k64 : kb;
        }
        {
            long long o = __shfl_xor(kb, 16);
            kb = o > kb ? o : kb;
            o = __shfl_xor(kb, 32);
            kb = o > kb ? o : kb;
        }
        const int E = (int)(kb >> 12), d = 4095 - (int)(kb & 4095);
        // lead cells: lane l takes cells (l & 3), + 4 of pixel l >> 2, so a pixel's eight verdicts are two nibbles of the ballots
        const int pn = lane >> 2, pk = lane & 3;
        const float l0 = lds->cost[r][pn][pn + pk], l1 = lds->cost[r][pn][pn + pk + 4];
        const unsigned long long m0 = __builtin_amdgcn_ballot_w64(l0 > a.thr), m1 = __builtin_amdgcn_ballot_w64(l1 > a.thr);
        const unsigned hm = ((unsigned)(m0 >> (4 * n)) & 15u) | (((unsigned)(m1 >> (4 * n)) & 15u) << 4);
        const bool flag = xin && __builtin_popcount(hm) < a.M;
        if (g == r) { fE = E; fd = d; fsa = lds->sa[r][n]; fhm = hm; fflag = flag; }
        const int y = y0 + r;
        if (y >= ylo && __builtin_amdgcn_ballot_w64(flag)) {   // rare: rank the hits of the flagged pixels over the whole window
            I8Sweep<1, true> fs(a, lane, x0, y);
            fs.sa[0] = lds->sa[r][n];
            fs.cnt = 0;
            fs.flagged = flag;
            fs.fbp = &lds->fbh[r][n][0];
            fs.lds = nullptr;
            fs.ring = nullptr;
            fs.load_operands();
            fs.run();
            if (flag && g == 0)
                for (int j = 2 * min(fs.cnt, a.M); j < 2 * a.M; ++j) fs.fbp[j] = 0.f;
        }
    }
    i8_lds_fence();   // (the hits of the fall-back sweep came from all four lane groups)
    const int fr = R == 2 ? g & 1 : 0, y = y0 + fr;
    if (g < R && xin && y >= ylo) {
        const float best = (float)(fsa - fE), cen = lds->cen[fr][n];
        const float *lead = &lds->cost[fr][n][n], *fbh = &lds->fbh[fr][n][0];
        if (a.M == 4) i8_finalize<4>(a.o, a.middle, y, x, best, cen, fd, lead, fhm, fflag, fbh);
        else i8_finalize<8>(a.o, a.middle, y, x, best, cen, fd, lead, fhm, fflag, fbh);
    }
}

// Three waves per SIMD: 168 registers, the MFMA results in VGPRs (left to itself the compiler takes 188 with the accumulators in AGPRs,
// two waves per SIMD, and reads every result back with v_accvgpr_read).
template <int R>
__global__ __launch_bounds__(kI8Waves * 64) __attribute__((amdgpu_waves_per_eu(3, 3))) void ssd_flow_i8_kernel(I8Args a) {
    if (*a.verdict) return;   // not byte-valued: the gated float sweep behind this launch does the step
    __shared__ I8Lds<R> lds_all[kI8Waves];
    __shared__ I8Ring ring_all[kI8Waves];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int item = blockIdx.x * kI8Waves + wave;
    if (item >= a.nitems) return;   // (no block-wide barrier below: a wave works alone)
    if constexpr (R == 2) {
        if (item < a.n2) {
            const int strip = item / a.nrp, rp = item - strip * a.nrp;
            i8_item<2>(a, &lds_all[wave], &ring_all[wave], lane, strip, min(2 * rp, a.Ho - 2), 2 * rp);   // (the last pair of an odd Ho is shifted upwards)
            return;
        }
    }
    const int row = a.row0 + (item - a.n2), strip = row / a.Ho, y = row - strip * a.Ho;
    i8_item<1>(a, reinterpret_cast<I8Lds<1> *>(&lds_all[wave]), &ring_all[wave], lane, strip, y, y);
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
size_t dfe_flow_i8_plan(int H, int W, DfeFlowI8Bufs *b) {
    const int Ho = H - DFE_FLOW_MARGIN, Wo = W - DFE_FLOW_MARGIN;
    DfeFlowI8Bufs p{};
    if (Ho < 1 || Wo < 8) return 0;
    p.nstrips = dfe_cdiv(Wo, 16);
    p.Wp = 16 * p.nstrips + 64;   // candidate columns reach x0 + 54, frame-0 columns x0 + 38
    if ((long long)(H + 1) * p.Wp >= (1ll << 29)) return 0;   // (32-bit offsets in the sweep)
    p.px = (size_t)(H + 1) * p.Wp;
    if (b) *b = p;
    return p.px;
}

// the verdict ring: step i8_seq takes word i8_seq % 3 and has its pack kernel clear word (i8_seq + 1) % 3 for the step after it
int dfe_flow_i8_turn(dfe_ctx *ctx, DfeFlowI8Bufs *b) {
    if (!ctx->i8_verdict.p) {
        int rc = dfe_grow(ctx, ctx->i8_verdict, 256, "i8 verdict");
        if (rc) return rc;
        DFE_HIP(ctx, hipMemsetAsync(ctx->i8_verdict.p, 0, 256, ctx->stream));
    }
    ++ctx->i8_seq;
    b->verdict = (unsigned *)ctx->i8_verdict.p + ctx->i8_seq % 3;
    b->verdict_next = (unsigned *)ctx->i8_verdict.p + (ctx->i8_seq + 1) % 3;
    return DFE_OK;
}

// pack (T = float: the gate; T = unsigned char: no gate, and the frame's border) + the int8 sweep
template <typename T>
static int i8_launch(dfe_ctx *ctx, const T *I0, const T *I1, int H, int W, const DfeFlowI8Bufs &b, const CvNovolArgs &nv, const TailOut &out,
                     const DfePairDepth *pd) {
    constexpr bool BYTES = sizeof(T) == 1;
    const int Ho = H - DFE_FLOW_MARGIN, Wo = W - DFE_FLOW_MARGIN;
    DFE_REQUIRE(ctx, out.Wo == Wo && out.row_off == 0 && out.p_off == 0, DFE_E_ARG, "int8 flow sweep: one band of the whole pair");
    const dim3 pgrid(dfe_cdiv(b.Wp, kPackW), dfe_cdiv(H, kPackH), 2);
    if constexpr (BYTES) {
        DFE_REQUIRE(ctx, pd != nullptr, DFE_E_ARG, "int8 flow sweep on bytes: a pair step");
        I8PackBorder<true> bd;
        bd.o = dfe_tailout_frame(out, pd);
        bd.Ho = Ho;
        hipLaunchKernelGGL((flow_i8_pack_kernel<T, true>), pgrid, dim3(256), 0, ctx->stream, I0, I1, H, W, (long long)H * W, b.Wp, b.pk0, b.pk1, b.s0, b.s1k,
                           b.verdict, b.verdict_next, bd);
    } else {
        hipLaunchKernelGGL((flow_i8_pack_kernel<T, false>), pgrid, dim3(256), 0, ctx->stream, I0, I1, H, W, (long long)H * W, b.Wp, b.pk0, b.pk1, b.s0, b.s1k,
                           b.verdict, b.verdict_next, I8PackBorder<false>{});
    }
    DFE_LAUNCH_CHECK(ctx);
    I8Args a;
    a.pk0 = b.pk0; a.pk1 = b.pk1; a.s0 = b.s0; a.s1k = b.s1k; a.verdict = b.verdict;
    a.o = dfe_tailout_frame(out, pd); a.thr = nv.thr; a.M = nv.M; a.middle = dfe_window_middle(33, 33);
    a.Ho = Ho; a.Wo = Wo; a.Wp = b.Wp; a.nstrips = b.nstrips;
    const int R = Ho >= 2 ? 2 : 1;
    if (!ctx->i8_slots) {   // waves resident at once: CUs x blocks of the kernel that a CU holds x waves of a block
        int nb = 0;
        DFE_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, ssd_flow_i8_kernel<2>, kI8Waves * 64, 0));
        ctx->i8_slots = ctx->ncu * (nb > 0 ? nb : 1) * kI8Waves;
    }
    const I8ItemPlan ip = flow_i8_item_plan(Ho, a.nstrips, ctx->opt[DFE_OPT_I8_SLOTS] > 0 ? ctx->opt[DFE_OPT_I8_SLOTS] : ctx->i8_slots);
    a.nrp = ip.nrp; a.n2 = (int)ip.n2; a.row0 = (int)ip.row0; a.nitems = (int)(ip.n2 + ip.n1);
    const int nblk = dfe_cdiv(a.nitems, kI8Waves);
    {
        DfeProfScope prof(ctx, true);
        if (R == 2) hipExtLaunchKernelGGL(ssd_flow_i8_kernel<2>, dim3(nblk), dim3(kI8Waves * 64), 0, ctx->stream, prof.a, prof.b, 0, a);
        else hipExtLaunchKernelGGL(ssd_flow_i8_kernel<1>, dim3(nblk), dim3(kI8Waves * 64), 0, ctx->stream, prof.a, prof.b, 0, a);
    }
    DFE_LAUNCH_CHECK(ctx);
    ctx->last_kernel = "ssd_flow_i8_kernel";
    ctx->i8_last = true;
    return DFE_OK;
}

int dfe_flow_i8_launch(dfe_ctx *ctx, const float *I0, const float *I1, int H, int W, const DfeFlowI8Bufs &b, const CvNovolArgs &nv, const TailOut &out,
                       const DfePairDepth *pd) {
    return i8_launch<float>(ctx, I0, I1, H, W, b, nv, out, pd);
}
int dfe_flow_i8_launch_bytes(dfe_ctx *ctx, const unsigned char *I0, const unsigned char *I1, int H, int W, const DfeFlowI8Bufs &b, const CvNovolArgs &nv,
                             const TailOut &out, const DfePairDepth *pd) {
    return i8_launch<unsigned char>(ctx, I0, I1, H, W, b, nv, out, pd);
}
