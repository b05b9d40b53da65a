// x3mlp.hip -- fp32-accurate GEMMs of the actor MLP on gfx950's bf16 MFMA,
// operands pre-split into bf16 planes and stored in MFMA fragment order.
//
// Arithmetic (as gemm_x3.hip): every fp32 x is split exactly into three bf16
// parts x = hi + mid + lo (hi = RN(x), mid = RN(x - hi), lo = RN(x - hi -
// mid)); a product keeps the six partial products >= 2^-16 |ab| (hh, hm, mh,
// mm, hl, lh), each exact in the fp32 MFMA accumulator.  6 bf16 MFMAs per
// fp32 product: 2,500 / 6 = 417 TFLOP/s of fp32-class peak vs 157 for the
// f32 MFMA.
//
// What is new here: the split happens ONCE, in the producer (the previous
// GEMM's epilogue, or mm_x3_tp_pack for weights and the front-end output),
// into the "TP" layout below.  The GEMM main loop then has no VALU work at
// all: operand tiles go HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4,
// one 1-KiB wave-instruction per fragment tile), double-buffered, and the
// waves only issue ds_read_b128 + MFMA.
//
// TP layout of a logical [R, C] fp32 matrix (R padded to 256, C to 32):
//   block (rt, ks) = rows 16 rt .. +15, cols 32 ks .. +31, 3 KiB contiguous:
//   [plane 3][chunk c 4][row r 16][8 bf16], element j of chunk c = column
//   32 ks + kcol(c, j), kcol(c, j) = 4 c + j (j < 4) or 16 + 4 c + (j - 4):
//   the MFMA takes any order of k inside a step as long as both operands use
//   it, and this one lets a 16-lane group read a row's 64 contiguous bytes
//   (the fp32 A source below) instead of 16-byte pieces 32 bytes apart.
// so lane l of a 16x16x32 MFMA operand fragment (row l & 15, k 8 (l >> 4) ..
// +7) reads the 16 bytes at l * 16 of a plane block: lane-linear, conflict
// free, and exactly the image one global_load_lds_dwordx4 writes.
// Padding rows / columns hold zeros (the packers and epilogues write them).
//
// Precision template P (MM_PREC_*): P_X3 is the above; P_F16 keeps ONE fp16
// plane per operand (round-to-nearest), one f16 MFMA per product: the fp16
// actor/critic of BASELINE configs[4].  Storage stays fp32 (activations,
// gradients, master weights); an A-operand scale (a power of two, exact)
// keeps small gradients out of the fp16 subnormal range and the epilogue
// multiplies by its inverse (cscale).  The TP layout of P_F16 is the same
// with one plane (1 KiB blocks).
//
// k_wgrad: the weight gradient dW [N, K] = sum_m dY[m, n] X[m, k] of every
// nn.Linear in the update (networks.py:35-41, 87-106 under autograd).  The
// reduction runs over the M rows, which both operands store row-major, so each
// workgroup stages a 32-row step of dY and X into LDS already transposed into
// fragment order (one thread: one column x 8 rows -> split -> 16-byte LDS
// writes), waves own contiguous runs of output tiles (A fragments reused
// along a run), and the row slices' partials are summed in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "marlmaze.h"
#include "policy_device.h"

namespace mm {
namespace x3 {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

enum { P_X3 = MM_PREC_X3, P_F16 = MM_PREC_F16, P_X2 = MM_PREC_X2 };
template <int P>
struct Prec {
    static constexpr int kPlanes = P == P_X3 ? 3 : P == P_X2 ? 2 : 1;
    static constexpr int kBlk = 512 * kPlanes;  // uint16 per (rt, ks) block
    static constexpr bool kScaled = P != P_X3;  // operand scales / the output's cscale apply
};
constexpr float kX2Lo = 2048.f;         // P_X2: lo = RN16(2^11 (x - hi))
constexpr float kX2LoInv = 1.f / 2048.f;

// Range guard of the fp16-plane precisions.  P_X2 (x s = hi + 2^-11 lo) and P_F16 (x s rounded) hold every
// operand value as fp16 planes: |x s| >= 65520 rounds hi to inf (lo then to -inf), and every output that
// value reaches becomes inf or NaN, where the fp32 reference stays finite.  The kernels therefore check
// their OUTPUT accumulators, not their inputs (cheaper -- an output tile is a few values per lane -- and
// exact: an out-of-range operand always reaches a non-finite accumulator, an in-range one never does):
// a lane whose accumulators hold an inf / NaN (exponent field all ones) ORs bit 0 into g_range_flag.  mm_gemm_range_flag reads and clears the flag, stream-ordered,
// and the caller redoes the work at x3 (bf16x3: fp32's range).  (A non-finite INPUT also raises it: the
// redo then reproduces fp32's inf / NaN.)  The flag is written by vector atomics only.
__device__ unsigned int g_range_flag;

template <int P>
__device__ __forceinline__ void range_acc(uint32_t& rm, const f32x4& a) {  // rm: the largest |bits| (no compares)
    if constexpr (P != P_X3) {
#pragma unroll
        for (int g = 0; g < 4; g++) rm = max(rm, __float_as_uint(a[g]) & 0x7FFFFFFFu);
    }
    (void)rm;
    (void)a;
}
// the epilogues' form: a wave-wide mask in SGPRs (v_cmp_class + s_or), no VGPR held over the columns
template <int P>
__device__ __forceinline__ void range_val(uint64_t& rb, float x) {
    if constexpr (P != P_X3) rb |= __builtin_amdgcn_ballot_w64(!__builtin_isfinite(x));
    (void)rb;
    (void)x;
}
template <int P>
__device__ __forceinline__ void range_note_wave(uint64_t rb) {
    if constexpr (P != P_X3) {
        if (rb != 0 && (threadIdx.x & 63) == 0)
            __hip_atomic_fetch_or(&g_range_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    (void)rb;
}
template <int P>
__device__ __forceinline__ void range_note(uint32_t rm) {
    if constexpr (P != P_X3) {  // an exponent field of all ones: inf or NaN
        if (rm >= 0x7F800000u) __hip_atomic_fetch_or(&g_range_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    (void)rm;
}

constexpr int kBlk = 1536;  // uint16 per (rt, ks) block of P_X3: 3 planes x 512
constexpr int kRowPad = 256;

__host__ __device__ inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// column (inside a 32-wide k-step) of element j of fragment chunk c
__host__ __device__ inline int kcol(int c, int j) { return j < 4 ? 4 * c + j : 12 + 4 * c + j; }

__device__ __forceinline__ uint32_t bf16_rn(float x) {  // round-to-nearest-even (finite x)
    const uint32_t u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ void split3(float x, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
    hi = bf16_rn(x);
    const float r1 = x - __uint_as_float(hi << 16);
    mid = bf16_rn(r1);
    const float r2 = r1 - __uint_as_float(mid << 16);
    lo = bf16_rn(r2);
}

// 8 consecutive fp32 -> three 16-byte plane pieces
__device__ __forceinline__ void split8(const float* v, uint4& h, uint4& m, uint4& l) {
    uint32_t hh[8], mm_[8], ll[8];
#pragma unroll
    for (int j = 0; j < 8; j++) split3(v[j], hh[j], mm_[j], ll[j]);
    h = make_uint4(hh[0] | (hh[1] << 16), hh[2] | (hh[3] << 16), hh[4] | (hh[5] << 16), hh[6] | (hh[7] << 16));
    m = make_uint4(mm_[0] | (mm_[1] << 16), mm_[2] | (mm_[3] << 16), mm_[4] | (mm_[5] << 16),
                   mm_[6] | (mm_[7] << 16));
    l = make_uint4(ll[0] | (ll[1] << 16), ll[2] | (ll[3] << 16), ll[4] | (ll[5] << 16), ll[6] | (ll[7] << 16));
}

// x * s -> fp16 (round to nearest even), two values packed
__device__ __forceinline__ uint32_t f16x2_rn(float x0, float x1) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    const h2 h = __builtin_convertvector((__attribute__((ext_vector_type(2))) float){x0, x1}, h2);
    return __builtin_bit_cast(uint32_t, h);
}

__device__ __forceinline__ uint4 f16x8_rn(const float* v, float s) {
    return make_uint4(f16x2_rn(v[0] * s, v[1] * s), f16x2_rn(v[2] * s, v[3] * s), f16x2_rn(v[4] * s, v[5] * s),
                      f16x2_rn(v[6] * s, v[7] * s));
}

// P_X2: two values x s -> (hi, lo) fp16 pairs, hi = RN16(x s), lo = RN16(2^11 (x s - hi)).  x s - hi is exact
// (hi is the nearest fp16 to x s: Sterbenz), the 2^11 is exact, so lo carries the next 11 significand bits
// and x s = hi + 2^-11 lo to 2^-22 relative while hi is normal (|x s| >= 2^-14).
__device__ __forceinline__ void pair2(float x0, float x1, float s, uint32_t& h, uint32_t& l) {
    typedef __attribute__((ext_vector_type(2))) float f2;
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    const f2 v = f2{x0, x1} * s;
    const h2 hv = __builtin_convertvector(v, h2);
    const f2 r = (v - __builtin_convertvector(hv, f2)) * kX2Lo;
    h = __builtin_bit_cast(uint32_t, hv);
    l = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, h2));
}

// x2 plane storage ("x2p") of an [M, n] activation or input gradient (n % 4 == 0): fp16 [M][n / 4][2][4] --
// per row and group of four columns the four hi halves, then the four lo halves, of pair2(x, s) of the fp32
// values that would have been stored (s = 1 for activations, the gradient scale for input gradients, whose
// consumers then read at scale 1 and apply cscale = 1 / s).  A row is n plane pairs = 4 n bytes, as fp32, and a
// 16-byte piece (one column group, both planes) sits where the four fp32 values would: every kernel addresses
// the tensor exactly as the fp32 matrix [M, ld] (ld: the row pitch in 4-byte units, ld % 4 == 0, rows 16-byte
// aligned for the LDS-DMA and the 16-byte loads).  A GEMM lane's 16-byte A load is its hi and its lo fragment
// halves; an epilogue lane quad (four adjacent columns of a row) exchanges its (hi, lo) pairs and stores one
// dword per lane, the addresses of the fp32 store; in LDS the hi piece of a group is 16-byte, the lo piece
// 8-byte aligned (ds_read_b64_tr_b16 takes 8-byte-aligned pieces of one row).
__device__ __forceinline__ void pair1(float x, _Float16& h, _Float16& l) {  // pair2 of one value at s = 1
    h = (_Float16)x;
    l = (_Float16)((x - (float)h) * kX2Lo);
}
// the dword lane (lane & 3) of a column quad stores: [hi0 hi1], [hi2 hi3], [lo0 lo1], [lo2 lo3] of the quad's
// four (hi, lo) pairs.  Every lane of the quad must be active (DPP quad permutes).
__device__ __forceinline__ uint32_t x2p_quad_word(_Float16 h, _Float16 l, int lane) {
    const int p = (int)((uint32_t)__builtin_bit_cast(unsigned short, h) |
                        ((uint32_t)__builtin_bit_cast(unsigned short, l) << 16));
    const uint32_t pa = (uint32_t)__builtin_amdgcn_mov_dpp(p, 0x88, 0xF, 0xF, true);  // quad_perm [0, 2, 0, 2]
    const uint32_t pb = (uint32_t)__builtin_amdgcn_mov_dpp(p, 0xDD, 0xF, 0xF, true);  // quad_perm [1, 3, 1, 3]
    return __builtin_amdgcn_perm(pb, pa, (lane & 2) ? 0x07060302u : 0x05040100u);  // the lo / the hi halves
}

// 8 values -> the two 16-byte P_X2 plane pieces
__device__ __forceinline__ void pair8(const float* v, float s, uint4& h, uint4& l) {
    uint32_t hh[4], ll[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pair2(v[2 * k], v[2 * k + 1], s, hh[k], ll[k]);
    h = make_uint4(hh[0], hh[1], hh[2], hh[3]);
    l = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}

// the 8 values of one fragment piece -> the P planes (16 bytes each) at dst, dst + 64, ... (uint4 units)
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l);

template <int P>
__device__ __forceinline__ void store_piece(const float* v, float s, uint4* dst) {
    if constexpr (P == P_X3) {  // the hardware bf16 conversions (split2): ~4 VALU per value, not ~20
        uint32_t h[4], m[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; k++) split2(v[2 * k], v[2 * k + 1], h[k], m[k], l[k]);
        dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
        dst[64] = make_uint4(m[0], m[1], m[2], m[3]);
        dst[128] = make_uint4(l[0], l[1], l[2], l[3]);
    } else if constexpr (P == P_X2) {
        uint4 h, l;
        pair8(v, s, h, l);
        dst[0] = h;
        dst[64] = l;
    } else {
        dst[0] = f16x8_rn(v, s);
    }
}

// one fragment product, the precision's MFMAs (P_X3: the six partial products, small terms first; P_X2:
// hi hi into acc, the cross terms hi lo + lo hi into accx -- combined by x2_combine before the epilogue)
template <int P>
__device__ __forceinline__ f32x4 mma(const bf16x8* a, const bf16x8* b, f32x4 acc, f32x4& accx) {
    if constexpr (P == P_X2) {
#define MM_H8(x) __builtin_bit_cast(f16x8, x)
        accx = __builtin_amdgcn_mfma_f32_16x16x32_f16(MM_H8(a[1]), MM_H8(b[0]), accx, 0, 0, 0);
        accx = __builtin_amdgcn_mfma_f32_16x16x32_f16(MM_H8(a[0]), MM_H8(b[1]), accx, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(MM_H8(a[0]), MM_H8(b[0]), acc, 0, 0, 0);
#undef MM_H8
        return acc;
    }
    (void)accx;
    if constexpr (P == P_X3) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[0]),
                                                     acc, 0, 0, 0);
    }
    return acc;
}

// P_X2: the product = hi hi + 2^-11 (hi lo + lo hi), one rounding (the scaling by 2^-11 is exact)
template <int P>
__device__ __forceinline__ f32x4 x2_combine(f32x4 acc, f32x4 accx) {
    if constexpr (P == P_X2) {
#pragma unroll
        for (int g = 0; g < 4; g++) acc[g] = fmaf(accx[g], kX2LoInv, acc[g]);
    }
    (void)accx;
    return acc;
}

// fp32 [R, C] (row-major, leading dimension ld; trans: element (i, j) at
// X[j * ld + i]) -> TP.  One thread per (rt, ks, c, r) 8-element piece.
template <int P>
__global__ __launch_bounds__(256) void k_tp_pack(const float* __restrict__ X, int R, int C, int ld, int trans,
                                                 int nks, long total, uint16_t* __restrict__ tp) {
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int l = (int)(e & 63);  // lane-linear position inside a plane block
        const long blk = e >> 6;      // (rt, ks)
        const int ks = (int)(blk % nks);
        const int rt = (int)(blk / nks);
        const int row = 16 * rt + (l & 15), c = l >> 4;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int col = 32 * ks + kcol(c, j);
            v[j] = (row < R && col < C) ? (trans ? X[(size_t)col * ld + row] : X[(size_t)row * ld + col]) : 0.f;
        }
        store_piece<P>(v, 1.f, reinterpret_cast<uint4*>(tp + blk * Prec<P>::kBlk) + l);
    }
}

// several packs in one launch (the update packs every weight of a network before its backward):
// the pieces of all segments laid end to end, each piece packed as by k_tp_pack
constexpr int kMaxPackSegs = 16;
struct PackSegs {
    mm_pack_seg_t s[kMaxPackSegs];
    long pre[kMaxPackSegs + 1];  // piece prefix
    int nks[kMaxPackSegs];
    int nseg;
};

template <int P>
__global__ __launch_bounds__(256) void k_tp_pack_multi(PackSegs ps) {
    const long total = ps.pre[ps.nseg];
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        int k = 0;
        while (k + 1 < ps.nseg && t >= ps.pre[k + 1]) k++;
        const mm_pack_seg_t& g = ps.s[k];
        const long e = t - ps.pre[k];
        const int l = (int)(e & 63);
        const long blk = e >> 6;
        const int nks = ps.nks[k], ks = (int)(blk % nks), rt = (int)(blk / nks);
        const int row = 16 * rt + (l & 15), c = l >> 4;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int col = 32 * ks + kcol(c, j);
            v[j] = (row < g.R && col < g.C) ? (g.trans ? g.X[(size_t)col * g.ld + row] : g.X[(size_t)row * g.ld + col])
                                            : 0.f;
        }
        store_piece<P>(v, 1.f, reinterpret_cast<uint4*>(g.tp + blk * Prec<P>::kBlk) + l);
    }
}

#ifndef X3_WAVES
#define X3_WAVES 16
#endif
constexpr int kWaves = X3_WAVES;  // the streaming kernel's waves per workgroup (one row tile each)
constexpr int kThreads = 64 * kWaves;
constexpr int kBM = 16 * kWaves;  // rows per workgroup: one row tile per wave
static_assert(kBM <= kRowPad, "A row blocks must stay inside the TP row padding");
// per precision: P_X2 holds two accumulator sets (17 column tiles: 136 registers), so its workgroups are
// 8 waves (two per SIMD, 256 registers each) instead of 16
template <int P>
struct SW {
    static constexpr int kWaves = P == P_X2 ? 8 : ::mm::x3::kWaves;
    static constexpr int kThreads = 64 * kWaves;
    static constexpr int kBM = 16 * kWaves;
};

template <int NT, int P = P_X3>
struct Cfg {
    static constexpr int kPiecesB = Prec<P>::kPlanes * NT;      // 1-KiB B pieces per k-step
    static constexpr int kPerWaveB = (kPiecesB + SW<P>::kWaves - 1) / SW<P>::kWaves;
    static constexpr int kStageB = NT * Prec<P>::kBlk;          // uint16 per B stage
    static constexpr int kEpiLen = kWaves * 16 * 36 * 2;         // uint16: the waves' TP epilogue slices
    static constexpr int kLen0 = kStageB > kEpiLen ? kStageB : kEpiLen;  // stage buffer 0 doubles as epilogue
    static_assert((kLen0 + kStageB) * 2 <= 160 * 1024, "LDS");
};

// ReLU bit masks in accumulator order: for row tile rt, lane l, 3 words; bit
// 4 c + g = (value at row 16 rt + 4 (l >> 4) + g, column 16 c + (l & 15)) > 0.
// A forward GEMM with relu writes them (mbits_out); the input-gradient GEMM of
// the next layer, whose output has the same [M, N] tiling, reads them
// (mbits_in) to apply the ReLU backward without touching the fp32 activations.
constexpr int kMaskWords = 3;  // 96 bits >= 4 * NT for NT <= 24

struct Epi {
    const float* bias;       // [N] or null
    const float* mask;       // fp32 [M, ldm] or null: out *= (mask > 0) (the ReLU-backward of the layer below)
    const uint32_t* mbits_in;  // or null: out *= bit (one column block, N <= 272)
    uint32_t* mbits_out;       // or null: bit = (out > 0) after bias / ReLU
    float* c;                // fp32 [M, ldc] or null
    uint16_t* ctp;           // TP of the output or null (needs one column block)
    float* colsum;           // EM_BWD, or null: per row tile column sums of the output [rows / 16][N]
    int ldc, ldm, relu, cnks;  // cnks = TP column blocks of the output (ceil(N / 32))
    float cscale;              // P_F16: out = acc * cscale before bias (the inverse of the A scale)
    int bufok;                 // fp32 c (and colsum) addressable through buffer resources (< 2^31 bytes)
    int c16;                   // c holds fp16 [M, ldc] (EM_FWD16 / EM_BWD16: P_F16's stored activations / gradients;
                               // P_X2: x2 planes, ldc the row pitch in 4-byte units as for fp32)
    float oscale;              // EM_BWD16: c = fp16(out * oscale) (the input gradient pre-scaled for its consumers)
};

// B piece i (column tile i / planes, plane i % planes) of k-step ks -> LDS (one 1-KiB LDS-DMA)
template <int P>
__device__ __forceinline__ void dma_b(const uint16_t* Bg, int nks, int ks, int i, uint16_t* dst, int lane) {
    constexpr int np = Prec<P>::kPlanes;
    const int ct = i / np, p = i - np * ct;
    const uint4* src = reinterpret_cast<const uint4*>(Bg + ((size_t)ct * nks + ks) * Prec<P>::kBlk + p * 512);
    __builtin_amdgcn_global_load_lds(src + lane, dst, 16, 0, 0);
}

// x -> (hi, mid, lo) with the hardware round-to-nearest-even conversion
// (v_cvt_pk_bf16_f32), two values at a time; same values as split3
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
    const bf2 hb = __builtin_convertvector((__attribute__((ext_vector_type(2))) float){x0, x1}, bf2);
    h = __builtin_bit_cast(uint32_t, hb);
    const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xFFFF0000u);
    const bf2 mb = __builtin_convertvector((__attribute__((ext_vector_type(2))) float){r0, r1}, bf2);
    m = __builtin_bit_cast(uint32_t, mb);
    const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xFFFF0000u);
    const bf2 lb = __builtin_convertvector((__attribute__((ext_vector_type(2))) float){s0, s1}, bf2);
    l = __builtin_bit_cast(uint32_t, lb);
}

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2v;
constexpr uint32_t kBufOOB = 0x80000000u;  // an offset past every buffer (num_records < 2^31)


// A operand sources.  A wave owns one row tile; per k-step each lane needs the
// 8 values (row 16 rt + (l & 15), k 32 ks + 8 (l >> 4) .. +7) as three bf16x8.
struct ASrcTP {  // pre-split TP planes: three lane-linear 1-KiB loads
    typedef bf16x8 Raw[3];
    const uint16_t* A;  // the wave's row tile
    int nks;
    __device__ void init(const uint16_t* base, int rt, int nks_, int, int, int, float) {
        nks = nks_;
        A = base + (size_t)rt * nks * kBlk;
    }
    __device__ __forceinline__ void load(int ks, Raw& r, int lane) const {
        const uint4* p = reinterpret_cast<const uint4*>(A + (size_t)ks * kBlk);
#pragma unroll
        for (int q = 0; q < 3; q++) r[q] = __builtin_bit_cast(bf16x8, p[64 * q + lane]);
    }
    template <int P>
    __device__ __forceinline__ void frag(const Raw& r, bf16x8 (&a)[3]) const {
        static_assert(P == P_X3, "pre-split TP A operands are bf16x3");
#pragma unroll
        for (int q = 0; q < 3; q++) a[q] = r[q];
    }
};

// a lane's 8 fp32 A values of one k-step (r[0]: k 4c..4c+3, r[1]: k 16+4c..: kcol order) -> its fragment
// planes: split (P_X3), hi / lo pairs of x s (P_X2), or rounded after scaling (P_F16)
template <int P>
__device__ __forceinline__ void frag_f32(const float4 (&r)[2], float scale, bf16x8 (&a)[3]) {
    if constexpr (P == P_X3) {
        uint32_t h[4], m[4], l[4];
        split2(r[0].x, r[0].y, h[0], m[0], l[0]);
        split2(r[0].z, r[0].w, h[1], m[1], l[1]);
        split2(r[1].x, r[1].y, h[2], m[2], l[2]);
        split2(r[1].z, r[1].w, h[3], m[3], l[3]);
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
        a[1] = __builtin_bit_cast(bf16x8, make_uint4(m[0], m[1], m[2], m[3]));
        a[2] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
    } else if constexpr (P == P_X2) {
        uint32_t h[4], l[4];
        pair2(r[0].x, r[0].y, scale, h[0], l[0]);
        pair2(r[0].z, r[0].w, scale, h[1], l[1]);
        pair2(r[1].x, r[1].y, scale, h[2], l[2]);
        pair2(r[1].z, r[1].w, scale, h[3], l[3]);
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
        a[1] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
    } else {
        const float s = scale;
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(f16x2_rn(r[0].x * s, r[0].y * s), f16x2_rn(r[0].z * s, r[0].w * s),
                                                     f16x2_rn(r[1].x * s, r[1].y * s), f16x2_rn(r[1].z * s, r[1].w * s)));
    }
}

// fp32 row-major [M, lda]: VW = 4 (16-byte loads; lda % 4 == 0) or 2 (8-byte
// loads: lda, K even, e.g. the critic's [M, 130] observations), split (P_X3)
// or rounded after scaling (P_F16) in registers
template <int VW>
struct ASrcF32V {
    typedef float4 Raw[2];
    __amdgpu_buffer_rsrc_t rs;  // A [M, lda] (the host keeps M lda 4 < 2^31: row chunks)
    uint32_t roff;              // this lane's row (clamped inside the matrix), column 4 (l >> 4), bytes
    int K, kq;
    float scale;
    __device__ void init(const float* base, int rt, int, int M, int lda, int K_, float scale_) {
        const int lane = threadIdx.x & 63;
        const int r = min(16 * rt + (lane & 15), M - 1);  // rows past M: computed, never stored
        K = K_;
        scale = scale_;
        kq = 4 * (lane >> 4);
        rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)((size_t)M * lda * 4), 0x00020000);
        roff = 4u * ((uint32_t)r * (uint32_t)lda + (uint32_t)kq);
    }
    // columns past K: an out-of-range offset reads zeros (no exec-masked conditional loads)
    __device__ __forceinline__ void load(int ks, Raw& r, int) const {
        const int k = 32 * ks + kq;  // kcol(c, 0..3) = 4c.., kcol(c, 4..7) = 16 + 4c..
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t o = roff + 4u * (32 * ks + 16 * h);
            if constexpr (VW == 4) {
                const u32x4v v = __builtin_amdgcn_raw_buffer_load_b128(rs, k + 16 * h < K ? o : kBufOOB, 0, 0);
                r[h] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                                   __uint_as_float(v.w));
            } else {
                const u32x2v x = __builtin_amdgcn_raw_buffer_load_b64(rs, k + 16 * h < K ? o : kBufOOB, 0, 0);
                const u32x2v y = __builtin_amdgcn_raw_buffer_load_b64(rs, k + 16 * h + 2 < K ? o + 8 : kBufOOB, 0, 0);
                r[h] = make_float4(__uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(y.x),
                                   __uint_as_float(y.y));
            }
        }
    }
    template <int P>
    __device__ __forceinline__ void frag(const Raw& r, bf16x8 (&a)[3]) const {
        frag_f32<P>(r, scale, a);
    }
};
typedef ASrcF32V<4> ASrcF32;
typedef ASrcF32V<2> ASrcF32U;

// fp16 row-major [M, lda] (P_F16 at scale 1: the f16 networks' stored front-end output h, K = 460, which the
// B-resident kernel does not take): the lane's two 8-byte runs of 4 halves ARE its fragment, no conversion
struct ASrcF16V {
    typedef u32x2v Raw[2];
    __amdgpu_buffer_rsrc_t rs;
    uint32_t roff;  // this lane's row (clamped inside the matrix), column 4 (l >> 4), bytes
    int K, kq;
    __device__ void init(const unsigned short* base, int rt, int, int M, int lda, int K_, float) {
        const int lane = threadIdx.x & 63;
        const int r = min(16 * rt + (lane & 15), M - 1);  // rows past M: computed, never stored
        K = K_;
        kq = 4 * (lane >> 4);
        rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)((size_t)M * lda * 2), 0x00020000);
        roff = 2u * ((uint32_t)r * (uint32_t)lda + (uint32_t)kq);
    }
    __device__ __forceinline__ void load(int ks, Raw& r, int) const {  // columns past K: zeros (out of range)
        const int k = 32 * ks + kq;
#pragma unroll
        for (int h = 0; h < 2; h++)
            r[h] = __builtin_amdgcn_raw_buffer_load_b64(rs, k + 16 * h < K ? roff + 2u * (32 * ks + 16 * h) : kBufOOB, 0, 0);
    }
    template <int P>
    __device__ __forceinline__ void frag(const Raw& r, bf16x8 (&a)[3]) const {
        static_assert(P == P_F16, "fp16 A: P_F16");
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(r[0].x, r[0].y, r[1].x, r[1].y));
    }
};

// x2 planes (P_X2 at scale 1; lda: the row pitch in 4-byte units): ASrcF32's loads -- a lane's 16 bytes are
// the hi halves k .. k + 3, then the lo halves -- and no conversion
struct ASrcX2PV : ASrcF32V<4> {
    template <int P>
    __device__ __forceinline__ void frag(const Raw& r, bf16x8 (&a)[3]) const {
        static_assert(P == P_X2, "x2 planes: P_X2");
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(r[0].x), __float_as_uint(r[0].y),
                                                     __float_as_uint(r[1].x), __float_as_uint(r[1].y)));
        a[1] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(r[0].z), __float_as_uint(r[0].w),
                                                     __float_as_uint(r[1].z), __float_as_uint(r[1].w)));
    }
};

// One k-step on stage buffer `cur`: split this step's A (raw -> fragments),
// prefetch the next step's raw A (registers) and B pieces (the other buffer;
// the DMA issues spread over the column loop), the 6 x NT MFMAs, one barrier.
template <int NT, int P, class AS>
__device__ __forceinline__ void k_step(f32x4 (&acc)[NT], f32x4 (&accx)[NT], const AS& as, const typename AS::Raw& raw,
                                       typename AS::Raw& rawn, const uint16_t* Bg, int nks, int ks,
                                       const uint16_t* cur, uint16_t* nxt, int wave, int lane) {
    using C = Cfg<NT, P>;
    constexpr int np = Prec<P>::kPlanes;
    const bool more = ks + 1 < nks;
    bf16x8 a[3];
    as.template frag<P>(raw, a);
#ifndef X3_NO_ALOAD  // diagnostic builds (tools/x3_variants.sh) only
    as.load(more ? ks + 1 : ks, rawn, lane);
#endif
    const bf16x8* b8 = reinterpret_cast<const bf16x8*>(cur) + lane;
#pragma unroll
    for (int c = 0; c < NT; c++) {
#ifndef X3_NO_DMA
        if (more && c < C::kPerWaveB) {
#else
        if (false) {
#endif
            const int i = wave + SW<P>::kWaves * c;
            if (i < C::kPiecesB) dma_b<P>(Bg, nks, ks + 1, i, nxt + i * 512, lane);
        }
        bf16x8 b[3];
#pragma unroll
        for (int q = 0; q < np; q++) b[q] = b8[(c * np + q) * 64];
        acc[c] = mma<P>(a, b, acc[c], accx[c]);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // vmcnt(0): this wave's next-stage pieces and A loads landed; the barrier: every
                      // wave's, and stage `cur` is no longer read
    __builtin_amdgcn_sched_barrier(0);
}

// Epilogue modes (template parameter EM, so each kernel carries only its own
// epilogue and the main loop keeps its registers):
//   EM_F32:  fp32 out (+ bias)(ReLU)(* (fp32 mask > 0))
//   EM_FWD:  fp32 out (+ bias)(ReLU) and the ReLU bit mask (mbits_out)
//   EM_BWD:  fp32 out * bits (mbits_in): the input gradient through the ReLU below
//   EM_TP:   TP out (+ bias)(ReLU)(* (fp32 mask > 0))
// Accumulators acc[c]: lane l holds rows 4 (l >> 4) + g, column 16 c + (l & 15).
// fp32 rows are stored straight from the accumulators (16 lanes = 64 contiguous
// bytes of a row); no workgroup barrier.
//   EM_FWD16: EM_FWD with fp16 out (P_F16: the update's activations stored at the operand precision --
//             the next GEMM rounds them to fp16 anyway -- half the bytes of every activation read / write)
//   EM_BWD16: EM_BWD with fp16 out * oscale (P_F16: the input gradient stored pre-scaled, as its consumers'
//             operands; the column sums stay those of the fp32 values)
enum { EM_F32 = 0, EM_FWD = 1, EM_BWD = 2, EM_TP = 3, EM_FWD16 = 4, EM_BWD16 = 5 };
constexpr bool em_fwd(int em) { return em == EM_FWD || em == EM_FWD16; }
constexpr bool em_bwd(int em) { return em == EM_BWD || em == EM_BWD16; }
constexpr bool em_16(int em) { return em == EM_FWD16 || em == EM_BWD16; }

template <int NT, int EM, int P>
__device__ __forceinline__ void epilogue_f32(const f32x4 (&acc)[NT], int rt, int M, int N, int col0, const Epi& ep,
                                             const float* sbias, int lane) {
    uint64_t rb = 0;  // the range guard (range_val), noted at the end
    const int rq = 4 * (lane >> 4);  // first of this lane's four rows (within the tile)
    const float* sb = sbias + (lane & 15);  // one base register, column c at immediate offset 64 c
    uint32_t bits[kMaskWords] = {0u, 0u, 0u};
    if (EM == EM_BWD) {
        const uint32_t* mb = ep.mbits_in + ((size_t)rt * 64 + lane) * kMaskWords;
#pragma unroll
        for (int w = 0; w < kMaskWords; w++) bits[w] = mb[w];
    }
#pragma unroll
    for (int c = 0; c < NT; c++) {
        const int col = col0 + 16 * c + (lane & 15);
        // the unit's bias sits in LDS: a global load here would make every column
        // wait (vmcnt) for the previous columns' stores
        const float bv = (EM != EM_BWD && ep.bias) ? sb[16 * c] : 0.f;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = 16 * rt + rq + g, bit = 4 * c + g;
            float x = acc[c][g];
            range_val<P>(rb, x);
            if (Prec<P>::kScaled) x *= ep.cscale;
            if (EM == EM_BWD) {
                if (!((bits[bit >> 5] >> (bit & 31)) & 1u)) x = 0.f;
            } else {
                x += bv;
                if (ep.relu) x = fmaxf(x, 0.f);
            }
            if (EM == EM_FWD && x > 0.f && col < N && row < M) bits[bit >> 5] |= 1u << (bit & 31);
            if (row >= M || col >= N) continue;
            if (EM == EM_F32 && ep.mask && !(ep.mask[(size_t)row * ep.ldm + col] > 0.f)) x = 0.f;
            ep.c[(size_t)row * ep.ldc + col] = x;
        }
        if (EM == EM_BWD && ep.colsum) {  // the bias gradient's partial: this tile's 16-row column sums
            float cs = 0.f;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int row = 16 * rt + rq + g;
                if (row < M && ((bits[(4 * c + g) >> 5] >> ((4 * c + g) & 31)) & 1u))
                    cs += Prec<P>::kScaled ? acc[c][g] * ep.cscale : acc[c][g];
            }
            cs += __shfl_xor(cs, 16);
            cs += __shfl_xor(cs, 32);
            if (lane < 16 && col < N && 16 * rt < M) ep.colsum[(size_t)rt * N + col] = cs;
        }
        __builtin_amdgcn_sched_barrier(0);  // one column at a time: bounded live values
    }
    if (EM == EM_FWD) {
        uint32_t* mb = ep.mbits_out + ((size_t)rt * 64 + lane) * kMaskWords;
#pragma unroll
        for (int w = 0; w < kMaskWords; w++) mb[w] = bits[w];
    }
    range_note_wave<P>(rb);
}

// TP output through a 2-KiB wave-private LDS slice, 32 columns at a time, where
// each lane picks up the 8 consecutive values of its fragment-order piece.
template <int NT>
__device__ __forceinline__ void epilogue_tp(const f32x4 (&acc)[NT], float* slice, int rt, int M, int N,
                                            const Epi& ep, int lane) {
    const int rq = 4 * (lane >> 4);
    const int rr = lane & 15, row = 16 * rt + rr, ch = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < (16 * NT + 31) / 32; ks++) {
        if (ks >= ep.cnks) break;  // the output is narrower than the tile block
        // tiles 2 ks, 2 ks + 1 -> slice [16 rows][32 cols] (stride 36 floats: conflict-free writes)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int c = 2 * ks + h;
#pragma unroll
            for (int g = 0; g < 4; g++)
                slice[(rq + g) * 36 + 16 * h + (lane & 15)] = c < NT ? acc[c < NT ? c : 0][g] : 0.f;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float4 v0 = *reinterpret_cast<const float4*>(slice + rr * 36 + kcol(ch, 0));
        const float4 v1 = *reinterpret_cast<const float4*>(slice + rr * 36 + kcol(ch, 4));
        float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int col = 32 * ks + kcol(ch, j);
            float x = 0.f;
            if (col < N && row < M) {
                x = v[j] + (ep.bias ? ep.bias[col] : 0.f);
                if (ep.relu) x = fmaxf(x, 0.f);
                if (ep.mask && !(ep.mask[(size_t)row * ep.ldm + col] > 0.f)) x = 0.f;
            }
            v[j] = x;
        }
        uint4 h, m, l;
        split8(v, h, m, l);
        uint4* dst = reinterpret_cast<uint4*>(ep.ctp + ((size_t)rt * ep.cnks + ks) * kBlk) + lane;
        dst[0] = h;
        dst[64] = m;
        dst[128] = l;
        __builtin_amdgcn_wave_barrier();  // the slice is rewritten next round
        __builtin_amdgcn_sched_barrier(0);
    }
    for (int ks = (16 * NT + 31) / 32; ks < ep.cnks; ks++) {  // columns beyond the block: zeros
        uint4* dst = reinterpret_cast<uint4*>(ep.ctp + ((size_t)rt * ep.cnks + ks) * kBlk) + lane;
        dst[0] = dst[64] = dst[128] = make_uint4(0, 0, 0, 0);
    }
}

// C[M, N] = A[M, K] . B[N, K]^T, B in TP, A from source AS.  Workgroup: 16
// waves, 256 rows x 16 NT columns; wave w owns row tile w and all NT column
// tiles.  A is private to a wave: straight from HBM to registers, one k-step
// ahead.  B (the weights) is shared: LDS-DMA into a double-buffered stage, the
// DMA issues spread over the MFMA stream.  One barrier per k-step; four waves
// per SIMD hide the LDS latency of the B fragment reads.  Persistent over
// 256-row units.
// Epilogue of one row tile x ctn column tiles (global tiles tg0 .. tg0 + ctn - 1; tg0 even), all stores
// through buffer resources: rows past M fall past num_records and are dropped by the hardware, so there is
// one code path with no per-element branches or 64-bit address arithmetic (lane offsets per row, the
// column tile at an immediate offset); only a tile crossing N selects an out-of-range offset for its
// lanes past N.  ReLU bits: bit 4 c + g of the tile-local words = bit 4 (tg0 + c) + g of the row tile's
// mask, i.e. local byte m is global byte tg0 / 2 + m -- each block writes (EM_FWD) and reads (EM_BWD)
// whole bytes of its own tiles.  Bits of rows past M are left unspecified (every reader masks by row);
// columns past N compute to exact zeros (zero B rows and bias) and record 0.
template <int P, int CT, int EM>
__device__ __forceinline__ void bres_epilogue(const f32x4 (&acc)[CT], int rt, int tg0, int ctn, int M, int N,
                                              const Epi& ep, __amdgpu_buffer_rsrc_t crs,
                                              __amdgpu_buffer_rsrc_t srs, const float* sb, int lane) {
    constexpr int NW = (4 * CT + 31) / 32;  // local mask words
    uint64_t rb = 0;  // the range guard (range_val), noted at the end
    int rq = 4 * (lane >> 4);
    asm volatile("" : "+v"(rq));  // offsets formed here, not hoisted over the main loop and held
    const int row0 = 16 * rt + rq, cl = lane & 15;
    constexpr uint32_t esz = (em_16(EM) && P != P_X2) ? 2u : 4u;  // bytes per output element (x2 planes: a pair)
    uint32_t voff[4];
#pragma unroll
    for (int g = 0; g < 4; g++) voff[g] = esz * ((uint32_t)(row0 + g) * (uint32_t)ep.ldc + (uint32_t)cl);
    const int soff = 16 * (int)esz * tg0;  // bytes: the block's first column tile
    uint32_t lbits[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) lbits[w] = 0u;
    if (em_bwd(EM)) {
        const uint8_t* mi =
            reinterpret_cast<const uint8_t*>(ep.mbits_in + ((size_t)rt * 64 + lane) * kMaskWords) + tg0 / 2;
#pragma unroll
        for (int m = 0; m < (CT + 1) / 2; m++)
            if (2 * m < ctn) lbits[m >> 2] |= (uint32_t)mi[m] << (8 * (m & 3));
        if (16 * rt + 16 > M) {  // the last row tile: rows past M masked out (their bits are unspecified)
            uint32_t rmask = 0u;
#pragma unroll
            for (int g = 0; g < 4; g++) rmask |= (row0 + g < M ? 1u : 0u) << g;
#pragma unroll
            for (int w = 0; w < NW; w++) lbits[w] &= rmask * 0x11111111u;
        }
    }
    const float* sbl = sb + cl;
#pragma unroll
    for (int c = 0; c < CT; c++) {
        if (c >= ctn || 16 * (tg0 + c) >= N) continue;  // wave-uniform (continue: the loop stays unrolled)
        const int col = 16 * (tg0 + c) + cl;
        const bool part = 16 * (tg0 + c) + 16 > N;  // wave-uniform: a tile crossing N
        const float bv = (!em_bwd(EM) && ep.bias) ? sbl[16 * c] : 0.f;
        float cs = 0.f;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int bit = 4 * c + g;
            float x = acc[c][g];
            range_val<P>(rb, x);
            if (Prec<P>::kScaled) x *= ep.cscale;
            if (em_bwd(EM)) {
                const bool on = (lbits[bit >> 5] >> (bit & 31)) & 1u;
                if (!on) x = 0.f;
                cs += x;
            } else {
                x += bv;
                if (ep.relu) x = fmaxf(x, 0.f);
                if (em_fwd(EM)) lbits[bit >> 5] |= (x > 0.f ? 1u : 0u) << (bit & 31);
            }
            uint32_t o = voff[g] + 16u * esz * c;
            if (part && col >= N) o = kBufOOB;
#ifdef BRES_NO_STORE  // diagnostic builds only
            if (x == 1234.5f)
#endif
            if constexpr (em_16(EM) && P == P_X2) {
                // x2 planes: pair2 of the value (hi past 65504 is inf: the range guard sees it); the column
                // quad's pairs regrouped, one dword per lane at the fp32 store's address (N % 4 == 0: a quad is
                // inside N or past it; every lane is active here)
                _Float16 h, l;
                pair1(EM == EM_BWD16 ? x * ep.oscale : x, h, l);
                range_val<P>(rb, (float)h);
                __builtin_amdgcn_raw_buffer_store_b32(x2p_quad_word(h, l, lane), crs, o, soff, 0);
            } else if constexpr (em_16(EM)) {
                // round to nearest; past 65504 it is inf: the range guard sees it
                const _Float16 h = (_Float16)(EM == EM_BWD16 ? x * ep.oscale : x);
                range_val<P>(rb, (float)h);
                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, h), crs, o, soff, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), crs, o, soff, 0);
            }
        }
        if (em_bwd(EM) && ep.colsum) {  // the bias gradient's partial: this tile's 16-row column sums
            cs += __shfl_xor(cs, 16);
            cs += __shfl_xor(cs, 32);
            const uint32_t so = (lane < 16 && col < N) ? 4u * ((uint32_t)rt * (uint32_t)N + (uint32_t)col) : kBufOOB;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(cs), srs, so, 0, 0);
        }
    }
    if (em_fwd(EM)) {
        uint8_t* mb = reinterpret_cast<uint8_t*>(ep.mbits_out + ((size_t)rt * 64 + lane) * kMaskWords) + tg0 / 2;
#pragma unroll
        for (int m = 0; m < (CT + 1) / 2; m++)
            if (2 * m < ctn) mb[m] = (uint8_t)(lbits[m >> 2] >> (8 * (m & 3)));
    }
    range_note_wave<P>(rb);
}

#ifdef X3_STAMPS  // diagnostic builds only (tools/x3_stamps.sh): per-wave phase clocks of k_x3nt
__device__ unsigned long long g_x3_stamps[256 * 16 * kWaves * 8];
#define X3_STAMP(it, slot, val)                                                                       \
    do {                                                                                              \
        if (lane == 0 && blockIdx.x < 256 && (it) < 16)                                               \
            g_x3_stamps[((blockIdx.x * 16 + (it)) * kWaves + wave) * 8 + (slot)] = (val);             \
    } while (0)
#else
#define X3_STAMP(it, slot, val) \
    do {                        \
    } while (0)
#endif

template <int NT, int P, class AS, class AT, int EM>
__global__ __launch_bounds__(SW<P>::kThreads) void k_x3nt(const AT* __restrict__ A, int lda, float ascale,
                                                   const uint16_t* __restrict__ B, int M, int N, int K, int nks,
                                                   int nrb, int ncb, Epi ep) {
    using C = Cfg<NT, P>;
    static_assert(EM != EM_TP || P == P_X3, "TP outputs are bf16x3");
    // two distinct LDS objects: the compiler's alias scopes then let a B read of
    // one stage run while the DMA into the other is in flight
    __shared__ float sbias[16 * NT];  // the unit's bias columns (EM_F32 / EM_FWD); first: small LDS offsets
    __shared__ __attribute__((aligned(16))) uint16_t sB0[C::kLen0];
    __shared__ __attribute__((aligned(16))) uint16_t sB1[C::kStageB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (unused when !ep.bufok: then the ranges below are not consulted)
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)ep.c, (short)0, (int)((size_t)M * ep.ldc * (em_16(EM) && P != P_X2 ? 2 : 4)), 0x00020000);
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)ep.colsum, (short)0, (int)((size_t)((M + 15) / 16) * N * 4), 0x00020000);
    // workgroup g takes units g, g + G, ...  XCD-aware unit order: units u and
    // u + 8 (one XCD) are the column blocks of one row block, so its A is shared
    // through that XCD's L2
    const int nunits = ((nrb + 7) / 8) * 8 * ncb;
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
        const int xcd = u & 7, slot = u >> 3;
        const int rb = (slot / ncb) * 8 + xcd, cb = slot % ncb;
        if (rb >= nrb) continue;  // workgroup-uniform
        const int rt = rb * SW<P>::kWaves + wave;  // this wave's row tile
        const int it = (u - (int)blockIdx.x) / (int)gridDim.x;
        (void)it;
        X3_STAMP(it, 0, __builtin_amdgcn_s_memtime());
        X3_STAMP(it, 4, __builtin_amdgcn_s_memrealtime());
        AS as;
        as.init(A, rt, nks, M, lda, K, ascale);
        const uint16_t* Bg = B + (size_t)cb * NT * nks * Prec<P>::kBlk;
        if (!em_bwd(EM) && EM != EM_TP && ep.bias && threadIdx.x < 16 * NT) {  // visible after the prologue barrier
            int t = threadIdx.x;
            asm volatile("" : "+v"(t));  // recomputed per unit, not a loop-invariant address held (spilled) across it
            const int col = cb * 16 * NT + t;
            sbias[t] = col < N ? ep.bias[col] : 0.f;
        }

        f32x4 acc[NT], accx[NT];
#pragma unroll
        for (int c = 0; c < NT; c++) acc[c] = accx[c] = f32x4{0.f, 0.f, 0.f, 0.f};

        typename AS::Raw r0, r1;
        for (int i = wave; i < C::kPiecesB; i += SW<P>::kWaves) dma_b<P>(Bg, nks, 0, i, sB0 + i * 512, lane);
        as.load(0, r0, lane);
        __syncthreads();
        X3_STAMP(it, 1, __builtin_amdgcn_s_memtime());
        // k-steps in pairs so the two stage buffers are compile-time distinct
        // (no wait of a B fragment read on the other buffer's DMA)
        int ks = 0;
        for (; ks + 1 < nks; ks += 2) {
            k_step<NT, P>(acc, accx, as, r0, r1, Bg, nks, ks, sB0, sB1, wave, lane);
            k_step<NT, P>(acc, accx, as, r1, r0, Bg, nks, ks + 1, sB1, sB0, wave, lane);
        }
        if (ks < nks) k_step<NT, P>(acc, accx, as, r0, r1, Bg, nks, ks, sB0, sB1, wave, lane);
#pragma unroll
        for (int c = 0; c < NT; c++) acc[c] = x2_combine<P>(acc[c], accx[c]);
        X3_STAMP(it, 2, __builtin_amdgcn_s_memtime());

        // ---- epilogue (after the last k-step's barrier both stage buffers are free) ----
        if constexpr (EM == EM_TP) {
            epilogue_tp<NT>(acc, reinterpret_cast<float*>(sB0) + wave * 16 * 36, rt, M, N, ep, lane);
        } else if constexpr (em_16(EM)) {  // (the host requires bufok)
            bres_epilogue<P, NT, EM>(acc, rt, cb * NT, NT, M, N, ep, crs, srs, sbias, lane);
        } else {
            if (ep.bufok && !ep.mask)  // buffer stores, one code path (bres_epilogue; tiles cb NT .. : even when bits)
                bres_epilogue<P, NT, EM>(acc, rt, cb * NT, NT, M, N, ep, crs, srs, sbias, lane);
            else
                epilogue_f32<NT, EM, P>(acc, rt, M, N, cb * 16 * NT, ep, sbias, lane);
        }
        // the next unit's DMA overwrites the epilogue slices: LDS reads done everywhere
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt((15 << 0) | (7 << 4) | (0 << 8) | (3 << 14));  // lgkmcnt(0) only
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        X3_STAMP(it, 3, __builtin_amdgcn_s_memtime());
        X3_STAMP(it, 5, __builtin_amdgcn_s_memrealtime());
    }
}

// ---------------------------------------------------------------------------
// The actor trunk's three ReLU layers in ONE launch for small M (the rollout's per-step forward at BASELINE
// configs[1]: 4,096 mazes = 8,192 rows; networks.py:35-36 under torch.no_grad, PPO.py:170-186):
//   h3 = relu(relu(relu(h0 W0^T + b0) W1^T + b1) W2^T + b2)
// At that size each layer on k_x3nt is a chain of k-steps at its launch floor (~13.6 us each, 160
// workgroups).  Here one workgroup owns 16 RT rows through all three layers.  The unit's h0 rows and each
// hidden layer's output stay in LDS, already in the precision's fragment planes (TP order, converted ONCE:
// h0 at staging, each hidden layer in its producer's epilogue), so a wave's A fragment is one lane-linear
// ds_read_b128 per plane and no wave repeats another's conversion.  Wave w owns the column-tile pair
// (2w, 2w + 1) -- one 32-column TP block of the output -- and tile 16 (N <= 272) is split by row tiles
// over waves 0, 5, 2 (SIMDs 0, 1, 2: no SIMD carries a whole third tile); the weight
// fragments come straight from the TP planes in L2 into registers, D k-steps ahead.  Only h0 is read from
// HBM and only h3 written.  Bit-identical to three k_x3nt launches (EM_F32, ReLU): the same conversion of
// the same fp32 values (store_piece = frag_f32 per value), the same MFMA sequence per output tile in k
// order (mma), the same epilogue arithmetic.  The weight-fragment loads follow the k_wgrad_rect rule
// (DESIGN.md section 4): their VGPR offsets are advanced in place and held live until consumed.
// ---------------------------------------------------------------------------
constexpr int kTrWaves = 8;
constexpr int kTrMaxN = 272;   // 17 column tiles: pairs 0..7 to waves 0..7, tile 16's row tiles to waves 0, 5, 2
constexpr int kTrMaxK0 = 512;  // padded width of the staged h0
constexpr int kTrSlice = 16 * 36;  // floats: a wave's [16 rows][32 columns] epilogue slice (stride 36)
struct TrunkArgs {
    const float* h0;
    const uint16_t* w[3];  // TP [N_l, K_l] in the precision P (K_1 = N_0, K_2 = N_1)
    const float* b[3];     // [N_l] or null
    float* out;            // fp32 [M, ldc]
    int lda, ldc, M, K0;
    int N[3];
    int bx;  // uint16 offset of the second activation buffer (bufH) from the first (bufX)
    // the fused heads + sampler (k_trunk3<.., HS = true>: k_head_act's arithmetic on the LDS-resident h3)
    const float* hw;  // [6, N2] = [move_head.weight; mark_head.weight]
    const float* hb;  // [6]
    const uint8_t* masks;
    uint64_t seed, offset;
    const uint64_t* offset_dev;
    int8_t* act;
    float* logp;
    float* joint;
    float* logits;
    int hoff;  // float offset (from the LDS base) of the h3 rows, stride N2 + 4
};

#ifdef X3_STAMPS  // diagnostic builds only (tools/trunk_stamps.py): per-wave phase clocks of k_trunk3
__device__ unsigned long long g_tr_stamps[1024 * kTrWaves * 10];
#define TR_STAMP(slot, val)                                                                      \
    do {                                                                                         \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 1024)                                        \
            g_tr_stamps[(blockIdx.x * kTrWaves + (threadIdx.x >> 6)) * 10 + (slot)] = (val);     \
    } while (0)
#else
#define TR_STAMP(slot, val) \
    do {                    \
    } while (0)
#endif

// the column tile of a wave's accumulator slot c: 2 w, 2 w + 1, then 16 (one row tile of it, on waves 0, 5, 2)
__device__ __forceinline__ int trunk_tile(int wave, int c) { return c < 2 ? 2 * wave + c : 16; }
// the row tile of tile 16 on wave w (-1: none)
__device__ __forceinline__ int trunk_r16(int w) { return w == 0 ? 0 : w == 5 ? 1 : w == 2 ? 2 : -1; }

// one layer: dst = relu(src W^T + b) for the unit's 16 RT rows.  src: TP blocks (rt, ks) of the layer
// input in LDS (nks = ceil(K / 32) per row tile); dst: the same for the output (dstL), or the global output
// rows (dstL null).  NC: the wave's tiles; D: the weight prefetch depth in k-steps, nks % D == 0 -- both
// compile-time, and the k-loop is branch-free (groups of D steps, the last one peeled): branches in it made
// the compiler's wait counting fall back to waiting for every load in flight at each step.
template <int P, int RT, int D, int NC>
__device__ __forceinline__ void trunk_layer_n(const uint16_t* src, int K, const uint16_t* W, int N, const float* sb,
                                              uint16_t* dstL, float* slice, float* h3s, const TrunkArgs& ta, int m0,
                                              int wave, int lane, uint32_t& rm, int stamp) {
    constexpr int np = Prec<P>::kPlanes;
    constexpr uint32_t kBS = 2u * Prec<P>::kBlk;  // bytes per TP block (16 rows x 32 k, all planes)
    const int nks = rup(K, 32) / 32, tiles = (N + 15) / 16;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)W, (short)0, (int)((uint32_t)tiles * nks * kBS), 0x00020000);
    // slot s holds the fragments of the k-steps s, s + D, ...; ob[s][c]: the lane's byte offset of its
    // fragment piece in block (tile, next k-step of the slot), advanced in place after each use
    uint32_t ob[D][NC];
#pragma unroll
    for (int s = 0; s < D; s++)
#pragma unroll
        for (int c = 0; c < NC; c++) ob[s][c] = ((uint32_t)trunk_tile(wave, c) * nks + s) * kBS + 16u * lane;
    bf16x8 bq[D][NC][3];
    auto issue = [&](int s) {
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int p = 0; p < np; p++)
                bq[s][c][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, ob[s][c] + 1024u * p, 0, 0));
    };
    auto advance = [&](int s) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NC; c++) asm volatile("v_add_u32 %0, %0, %1" : "+v"(ob[s][c]) : "s"((uint32_t)D * kBS));
    };
    const bf16x8* const a8 = reinterpret_cast<const bf16x8*>(src) + lane;
    f32x4 acc[NC][RT], accx[NC][RT];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int rt = 0; rt < RT; rt++) acc[c][rt] = accx[c][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // slot 2 (tile 16) covers one row tile r2 (trunk_r16); its A fragment picked by per-lane selects (from
    // threadIdx, not the wave-uniform value: a uniform select became a branch)
    static_assert(RT <= 3, "tile 16's row tiles: waves 0, 5, 2");
    const int r2 = trunk_r16(wave);
    const int r2v = trunk_r16((int)(threadIdx.x >> 6));
    // A fragments one k-step ahead (the last step re-reads its own block: no branch in the loop)
    bf16x8 an[RT][3];
    auto load_a = [&](int ks) {
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int q = 0; q < np; q++) an[rt][q] = a8[((rt * nks + ks) * np + q) * 64];
    };
    load_a(0);
    auto compute = [&](int ks, int s) {
        bf16x8 a[RT][3];
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int q = 0; q < np; q++) a[rt][q] = an[rt][q];
        load_a(min(ks + 1, nks - 1));
#pragma unroll
        for (int c = 0; c < (NC < 2 ? NC : 2); c++)
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[c][rt] = mma<P>(a[rt], bq[s][c], acc[c][rt], accx[c][rt]);
        if constexpr (NC == 3) {
            bf16x8 a2[3];
#pragma unroll
            for (int q = 0; q < np; q++) {
                a2[q] = a[0][q];
#pragma unroll
                for (int rt = 1; rt < RT; rt++) a2[q] = r2v == rt ? a[rt][q] : a2[q];
            }
            acc[2][0] = mma<P>(a2, bq[s][2], acc[2][0], accx[2][0]);
        }
    };
#pragma unroll
    for (int s = 0; s < D; s++) issue(s);
    const int G = nks / D;
    for (int g = 0; g + 1 < G; g++) {
#pragma unroll
        for (int s = 0; s < D; s++) {
            compute(g * D + s, s);
            advance(s);
            issue(s);
        }
    }
#pragma unroll
    for (int s = 0; s < D; s++) compute((G - 1) * D + s, s);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < D; s++)
#pragma unroll
        for (int c = 0; c < NC; c++) asm volatile("" ::"v"(ob[s][c]));  // held to here (all loads consumed)
    TR_STAMP(stamp, __builtin_amdgcn_s_memtime());
    (void)stamp;
    // epilogue: the k_x3nt arithmetic (x2_combine; cscale 1; + bias; ReLU)
    const int rq = 4 * (lane >> 4);
    float x[NC][RT][4];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const float bv = sb[16 * trunk_tile(wave, c) + (lane & 15)];
#pragma unroll
        for (int rt = 0; rt < (c < 2 ? RT : 1); rt++) {
            const f32x4 v = x2_combine<P>(acc[c][rt], accx[c][rt]);
            range_acc<P>(rm, v);
#pragma unroll
            for (int g = 0; g < 4; g++) x[c][rt][g] = fmaxf(v[g] + bv, 0.f);
        }
    }
    if (!dstL) {  // the last layer: fp32 rows of the output (16 lanes: 64 contiguous bytes of a row), and / or
                  // the unit's rows in LDS for the fused heads (h3s, rows of N + 4 floats)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int col = 16 * trunk_tile(wave, c) + (lane & 15);
#pragma unroll
            for (int rt = 0; rt < (c < 2 ? RT : 1); rt++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int rl = 16 * (c < 2 ? rt : r2) + rq + g, row = m0 + rl;
                    if (h3s && col < N) h3s[rl * (N + 4) + col] = x[c][rt][g];
                    if (ta.out && row < ta.M && col < N) ta.out[(size_t)row * ta.ldc + col] = x[c][rt][g];
                }
        }
        return;
    }
    // a hidden layer: each owned 32-column block (tile pair) through an fp32 slice into fragment order,
    // converted once (store_piece), into the next layer's input blocks; a missing tile of a pair is zeros.
    // x2 / x3: the slice is the destination block itself (2 KiB of fp32 fit its np KiB; the block is this
    // wave's until the layer's barrier), 32 floats a row with the float4 groups XOR-swizzled by row / 2 (a
    // 16-row column read then touches distinct banks); f16: the wave's own slice (rows of 36 floats).
    const int nksD = rup(N, 32) / 32, rr = lane & 15, ch = lane >> 4;
    auto sidx = [&](int row, int col) {
        return np >= 2 ? row * 32 + ((((col >> 2) ^ ((row >> 1) & 7))) << 2) + (col & 3) : row * 36 + col;
    };
    // slots c0, c1 (-1: no tile) of the wave's row tile rs -> block (rt, ks)
    auto put_block = [&](int ks, int rt, int rs, int c0, int c1) {
        uint16_t* const blk = dstL + (size_t)(rt * nksD + ks) * np * 512;
        float* const sl = np >= 2 ? reinterpret_cast<float*>(blk) : slice;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            sl[sidx(rq + g, lane & 15)] = c0 >= 0 ? x[c0 >= 0 ? c0 : 0][rs][g] : 0.f;
            sl[sidx(rq + g, 16 + (lane & 15))] = c1 >= 0 ? x[c1 >= 0 ? c1 : 0][rs][g] : 0.f;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float4 v0 = *reinterpret_cast<const float4*>(sl + sidx(rr, kcol(ch, 0)));
        const float4 v1 = *reinterpret_cast<const float4*>(sl + sidx(rr, kcol(ch, 4)));
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (in place: every lane has read the block before it is overwritten)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        store_piece<P>(v, 1.f, reinterpret_cast<uint4*>(blk) + lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the slice is rewritten next
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
        if (NC >= 1) put_block(wave, rt, rt, 0, NC >= 2 ? 1 : -1);
    if (NC >= 3) put_block(8, r2, 0, 2, -1);
    (void)nksD;
}

template <int P, int RT, int D>
__device__ __forceinline__ void trunk_layer(const uint16_t* src, int K, const uint16_t* W, int N, const float* sb,
                                            uint16_t* dstL, float* slice, float* h3s, const TrunkArgs& ta, int m0,
                                            int wave, int lane, uint32_t& rm, int stamp) {
    const int tiles = (N + 15) / 16, nks = rup(K, 32) / 32;
    // wave-uniform: slots 0, 1 = tiles 2 w, 2 w + 1; slot 2 = one row tile of tile 16 (N > 256)
    const int nc = 2 * wave >= tiles ? 0 : 2 * wave + 1 >= tiles ? 1 : (trunk_r16(wave) >= 0 && trunk_r16(wave) < RT && tiles > 16) ? 3 : 2;
    if (nks % D == 0) {
        if (nc == 3) trunk_layer_n<P, RT, D, 3>(src, K, W, N, sb, dstL, slice, h3s, ta, m0, wave, lane, rm, stamp);
        else if (nc == 2) trunk_layer_n<P, RT, D, 2>(src, K, W, N, sb, dstL, slice, h3s, ta, m0, wave, lane, rm, stamp);
        else if (nc == 1) trunk_layer_n<P, RT, D, 1>(src, K, W, N, sb, dstL, slice, h3s, ta, m0, wave, lane, rm, stamp);
    } else {  // (shapes other than the actor's: no prefetch beyond the next k-step)
        if (nc == 3) trunk_layer_n<P, RT, 1, 3>(src, K, W, N, sb, dstL, slice, h3s, ta, m0, wave, lane, rm, stamp);
        else if (nc == 2) trunk_layer_n<P, RT, 1, 2>(src, K, W, N, sb, dstL, slice, h3s, ta, m0, wave, lane, rm, stamp);
        else if (nc == 1) trunk_layer_n<P, RT, 1, 1>(src, K, W, N, sb, dstL, slice, h3s, ta, m0, wave, lane, rm, stamp);
    }
}

// HS: the actor's heads + the action draw fused after the last layer (PPO.py:170-186 with networks.py:38-41):
// k_head_act's per-row code (heads_row_dot, heads_butterfly, heads_finish<MM_ACT_SAMPLE>: policy_device.h) on the unit's h3
// rows in LDS, so the draws, log-probs and logits equal the unfused trunk + k_head_act's bit for bit; h3 is
// then written to HBM only when asked (ta.out)
template <int P, int RT, int D, bool HS>
__global__ __launch_bounds__(64 * kTrWaves) void k_trunk3(TrunkArgs ta) {
    constexpr int np = Prec<P>::kPlanes;
    constexpr int kIt = (RT * (kTrMaxK0 / 32) * 64 + 64 * kTrWaves - 1) / (64 * kTrWaves);  // h0 pieces per thread (max)
    constexpr int kHw = (6 * kTrMaxN + 64 * kTrWaves - 1) / (64 * kTrWaves);              // head weights per thread
    extern __shared__ __attribute__((aligned(16))) float tls[];
    float* const sbias = tls;                       // [3][kTrMaxN], zero past N
    float* const shw = tls + 3 * kTrMaxN;           // [6][N2]: the head weights (HS)
    float* const slices = shw + 6 * kTrMaxN;        // f16: [waves][kTrSlice] (x2 / x3 convert in place)
    uint16_t* const bufX = reinterpret_cast<uint16_t*>(slices + (np == 1 ? kTrWaves * kTrSlice : 0));  // h0, then layer 1's output
    uint16_t* const bufH = bufX + ta.bx;                                                 // layer 0's output
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = blockIdx.x * 16 * RT;
    TR_STAMP(0, __builtin_amdgcn_s_memtime());
    TR_STAMP(8, __builtin_amdgcn_s_memrealtime());
    {  // the unit's h0 rows as TP blocks (zero past M and past K0 up to the 32-column padding): every load
       // issued first, branch-free (out-of-range pieces read zeros through the buffer range check), their
       // offsets held until the data is consumed (the k_wgrad_rect rule)
        const int nks0 = rup(ta.K0, 32) / 32, npc = RT * nks0 * 64;
        const int nrows = min(16 * RT, ta.M - m0);
        const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(ta.h0 + (size_t)m0 * ta.lda), (short)0, (int)((uint32_t)nrows * ta.lda * 4u), 0x00020000);
        uint32_t off[kIt][2];
        float4 v[kIt][2];
#pragma unroll
        for (int j = 0; j < kIt; j++) {
            const int i = threadIdx.x + 64 * kTrWaves * j, l = i & 63, blk = i >> 6;  // blk = rt nks0 + ks
            const int rt = blk / nks0, ks = blk - nks0 * rt;
            const int row = 16 * rt + (l & 15), k0 = 32 * ks + 4 * (l >> 4);
#pragma unroll
            for (int h = 0; h < 2; h++)
                off[j][h] = (i < npc && row < nrows && k0 + 16 * h < ta.K0) ? 4u * ((uint32_t)row * ta.lda + k0 + 16 * h)
                                                                           : kBufOOB;
        }
#pragma unroll
        for (int j = 0; j < kIt; j++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const u32x4v d = __builtin_amdgcn_raw_buffer_load_b128(hrs, off[j][h], 0, 0);
                v[j][h] = make_float4(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z),
                                      __uint_as_float(d.w));
            }
        // the biases: thread t < 272 loads column t of each layer's (zero past N_l, or for a null bias), in
        // flight together with h0
        const uint32_t boff = 4u * threadIdx.x;
        float bv[3];
#pragma unroll
        for (int l = 0; l < 3; l++) {
            const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)ta.b[l], (short)0, ta.b[l] ? 4 * ta.N[l] : 0, 0x00020000);
            bv[l] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brs, boff, 0, 0));
        }
        if (threadIdx.x < kTrMaxN) {
#pragma unroll
            for (int l = 0; l < 3; l++) sbias[kTrMaxN * l + threadIdx.x] = bv[l];
        }
        asm volatile("" ::"v"(boff));
        if constexpr (HS) {  // the head weights [6, N2], flat (row pitch N2, as k_head_act's)
            const __amdgpu_buffer_rsrc_t wrs =
                __builtin_amdgcn_make_buffer_rsrc((void*)ta.hw, (short)0, 4 * 6 * ta.N[2], 0x00020000);
            uint32_t woff[kHw];
            float wv[kHw];
#pragma unroll
            for (int u = 0; u < kHw; u++) woff[u] = 4u * (threadIdx.x + 64 * kTrWaves * u);
#pragma unroll
            for (int u = 0; u < kHw; u++) wv[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, woff[u], 0, 0));
#pragma unroll
            for (int u = 0; u < kHw; u++) {
                const int e = threadIdx.x + 64 * kTrWaves * u;
                if (e < 6 * kTrMaxN) shw[e] = wv[u];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < kHw; u++) asm volatile("" ::"v"(woff[u]));
        }
#pragma unroll
        for (int j = 0; j < kIt; j++) {
            const int i = threadIdx.x + 64 * kTrWaves * j;
            if (i < npc) {
                const float e[8] = {v[j][0].x, v[j][0].y, v[j][0].z, v[j][0].w, v[j][1].x, v[j][1].y, v[j][1].z, v[j][1].w};
                store_piece<P>(e, 1.f, reinterpret_cast<uint4*>(bufX + (size_t)(i >> 6) * np * 512) + (i & 63));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kIt; j++)
#pragma unroll
            for (int h = 0; h < 2; h++) asm volatile("" ::"v"(off[j][h]));
    }
    __syncthreads();
    TR_STAMP(1, __builtin_amdgcn_s_memtime());
    float* const slice = slices + wave * kTrSlice;
    uint32_t rm = 0;  // the range guard (range_acc)
    trunk_layer<P, RT, D>(bufX, ta.K0, ta.w[0], ta.N[0], sbias, bufH, slice, nullptr, ta, m0, wave, lane, rm, 2);
    __syncthreads();
    TR_STAMP(3, __builtin_amdgcn_s_memtime());
    trunk_layer<P, RT, D>(bufH, ta.N[0], ta.w[1], ta.N[1], sbias + kTrMaxN, bufX, slice, nullptr, ta, m0, wave, lane,
                          rm, 4);
    __syncthreads();
    TR_STAMP(5, __builtin_amdgcn_s_memtime());
    float* const h3s = HS ? tls + ta.hoff : nullptr;  // (bufH, free in the last layer, or a region of its own)
    trunk_layer<P, RT, D>(bufX, ta.N[1], ta.w[2], ta.N[2], sbias + 2 * kTrMaxN, nullptr, slice, h3s, ta, m0, wave,
                          lane, rm, 6);
    range_note<P>(rm);
    if constexpr (HS) {  // the heads' row code on the LDS rows: 8 lanes a row, 16 RT rows (waves 0 .. 2 RT - 1)
        __syncthreads();
        const int K = ta.N[2];
        if (threadIdx.x < kHeadLanes * 16 * RT) {  // wave-uniform
            const int j = threadIdx.x % kHeadLanes, rl = threadIdx.x / kHeadLanes, row = m0 + rl;  // (m0 is even)
            const bool valid = row < ta.M;
            float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (valid) heads_row_dot(h3s + rl * (K + 4), K, shw, K, j, acc);
            heads_butterfly(acc);
            heads_finish<MM_ACT_SAMPLE>(acc, ta.hb, ta.masks, row, ta.M, valid && j == 0, ta.seed, ta.offset,
                                        ta.offset_dev, ta.act, ta.logp, ta.joint, ta.logits);
        }
    }
    TR_STAMP(7, __builtin_amdgcn_s_memtime());
    TR_STAMP(9, __builtin_amdgcn_s_memrealtime());
}

// Backward of the actor heads into the last hidden layer (networks.py:38-41 +
// the ReLU of :36): dY[m, n] = (sum_j dz[m, j] W[j, n]) * bit(m, n), W [J, N]
// the concatenated head weights, bits the last forward GEMM's ReLU mask.  Same
// tile map as the GEMM epilogue (one wave per 16-row tile, lane l: rows
// 4 (l >> 4) + g, columns 16 c + (l & 15)), so the mask bits line up; also the
// per-tile column sums (the last layer's bias gradient, before the final sum).
// D16: dY stored fp16 as fp16(dY * oscale) (P_F16's pre-scaled input gradients; the sums stay fp32)
constexpr int kHeadsMaxJ = 8;
template <int NT, int D16 = 0>  // D16: 0 fp32 dy, 1 fp16(dy oscale), 2 the x2 planes of dy oscale (row pitch N)
__global__ __launch_bounds__(256) void k_heads_bwd(const float* __restrict__ dz, int J, const float* __restrict__ W,
                                                   const uint32_t* __restrict__ bits, int M, int N,
                                                   float* __restrict__ dy, float* __restrict__ colsum,
                                                   float oscale = 1.f) {
    __shared__ float sw[kHeadsMaxJ][16 * NT];
    {  // loads batched ahead of the LDS writes (one L2 round trip per workgroup); 256 threads
        constexpr int kN = kHeadsMaxJ * 16 * NT, kPer = (kN + 255) / 256;
        float t[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int e = threadIdx.x + 256 * u, j = e / (16 * NT), n = e % (16 * NT);
            t[u] = (e < kN && j < J && n < N) ? W[(size_t)j * N + n] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int e = threadIdx.x + 256 * u;
            if (e < kN) sw[e / (16 * NT)][e % (16 * NT)] = t[u];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int rt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (16 * rt >= M) return;
    const int rq = 4 * (lane >> 4);
    uint64_t rb = 0;  // D16: the range guard of the fp16 stores
    float z[4][kHeadsMaxJ];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int row = 16 * rt + rq + g;
#pragma unroll
        for (int j = 0; j < kHeadsMaxJ; j++) z[g][j] = (row < M && j < J) ? dz[(size_t)row * J + j] : 0.f;
    }
    uint32_t b[kMaskWords];
#pragma unroll
    for (int w = 0; w < kMaskWords; w++) b[w] = bits[((size_t)rt * 64 + lane) * kMaskWords + w];
#pragma unroll
    for (int c = 0; c < NT; c++) {
        const int col = 16 * c + (lane & 15);
        float cs = 0.f;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = 16 * rt + rq + g, bit = 4 * c + g;
            float x = 0.f;
#pragma unroll
            for (int j = 0; j < kHeadsMaxJ; j++) x = fmaf(z[g][j], sw[j][col], x);
            if (!((b[bit >> 5] >> (bit & 31)) & 1u)) x = 0.f;
            uint32_t qw = 0u;  // D16 == 2: this lane's dword of its column quad's planes (every lane takes part)
            if constexpr (D16 == 2) {
                _Float16 h, l;
                pair1(x * oscale, h, l);
                range_val<P_X2>(rb, (float)h);
                qw = x2p_quad_word(h, l, lane);
            }
            if (row < M && col < N) {
                if constexpr (D16 == 2) {  // (N % 4 == 0: a quad is inside N or past it)
                    reinterpret_cast<uint32_t*>(dy)[(size_t)row * N + col] = qw;
                } else if constexpr (D16) {
                    const _Float16 h = (_Float16)(x * oscale);
                    range_val<P_F16>(rb, (float)h);
                    reinterpret_cast<_Float16*>(dy)[(size_t)row * N + col] = h;
                } else {
                    dy[(size_t)row * N + col] = x;
                }
                cs += x;
            }
        }
        cs += __shfl_xor(cs, 16);
        cs += __shfl_xor(cs, 32);
        if (lane < 16 && col < N) colsum[(size_t)rt * N + col] = cs;
    }
    if constexpr (D16 == 2) range_note_wave<P_X2>(rb);
    else if constexpr (D16) range_note_wave<P_F16>(rb);
}

// The weight-gradient kernels (k_wgrad, k_wgrad_rect, k_wgrad_dma, k_wgrad_tr, k_wgrad_mix, k_wg_reduce) and
// the parts they share; their plan and launches are below (WgPlan, launch_wgrad*).
#include "wgrad_kernels.h"

// ---------------------------------------------------------------------------
// k_bres: C[M, N] = A[M, K] . B[N, K]^T with a column block of B RESIDENT in
// LDS for the whole launch (the forward and input-gradient GEMMs of the actor
// and critic, K <= 288 for x3).  Why (tools/x3_stamps.py on k_x3nt, 264 x 264,
// M = 419,430): k_x3nt streams B through LDS one k-step at a time, so its 16
// waves meet at a barrier every k-step and split A, read B and issue MFMAs in
// lock-step: 12.2k cycles per k-step against 6.5k of MFMA work, plus 15k of
// prologue and 21k of epilogue per 256-row unit that no other wave overlaps.
// Here each workgroup loads its block of B once (LDS-DMA), and after one
// barrier its waves run independently: a wave owns 32 rows (two row tiles)
// x <= CT column tiles at a time, loads and splits its own A (fp32, one
// k-step ahead), reads B fragments from LDS (each feeds both row tiles) and
// writes its outputs -- one wave's loads and stores overlap the others'
// MFMAs, and nothing waits for the slowest wave.
//
// Column blocks: B of a tile over the whole K is planes x (32-wide steps x 1
// KiB + a final 16-wide step x 512 B when K % 32 is 1..16, on the 16x16x16
// MFMA); the block is as many tiles as fit 160 KiB (x3, K = 264: 6 tiles ->
// 17 = 6 + 6 + 5; f16: all 17).  Workgroups of one XCD split over the blocks
// in proportion to their tiles, and the XCD takes every 8th 32-row unit, so
// the blocks re-reading a unit's A rows do it through the same L2.  Waves
// whose block is wider than CT take the sub-blocks of a unit in turn (A again
// from L1 / L2).
#ifndef BRES_WAVES
#define BRES_WAVES 12
#endif
#ifndef BRES_BPREF
#define BRES_BPREF 0
#endif
// waves per workgroup (one workgroup per CU: the B block fills LDS).  12 (168 registers per wave: no spills,
// the epilogue's row offsets and both A buffers held) measured 5-8% faster than 16 (128 registers, spilling)
// and than 8 (tools/bres_variants.sh + tools/bench_gemm_ab.py)
constexpr int kBresWaves = BRES_WAVES;

struct BresPlan {
    int xcds;   // XCDs the grid spreads over (8, or 1)
    int nblk;   // column blocks
    int ctb;    // column tiles of the widest block (the LDS the launch reserves)
    int tiles;  // column tiles of the output
    int tstart[9];  // block b: column tiles tstart[b] .. tstart[b + 1] - 1 (starts even when ReLU bits are involved)
    int nfull;  // 32-wide k-steps
    int half;   // 1: a final 16-wide k-step
    int first[9];  // per XCD: block b's workgroups are first[b] .. first[b + 1] - 1
};
constexpr int kBresMaxBlk = 8;

// A through a buffer resource: a load whose offset is past the buffer's end returns zeros, so the
// columns past K cost one select of the offset -- no branch, and no wait on the loaded value (a select
// on the value, or two load forms merged at a branch, made the compiler wait for each k-step's loads
// at the end of the step that issued them: no prefetch at all)

struct BresA {
    __amdgpu_buffer_rsrc_t rsrc;  // A: base, num_records = M lda 4 bytes
    uint32_t roff[2];             // this lane's row of row tile r (r < RT), + 4 kq bytes
};

// A for one 32-wide k-step: row tile r's lane row, columns k = 32 ks + 4 (l >> 4) .. +3 and +16 .. +19;
// zeros at columns >= K
template <int RT, int VW>
__device__ __forceinline__ void bres_load(const BresA& as, int ks, int K, int kq, float4 (&raw)[RT][2]) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int kk = 32 * ks + kq + 16 * h;
#pragma unroll
        for (int r = 0; r < RT; r++) {
            if constexpr (VW == 16) {  // fp16 A: the 4 halves k .. k + 3 as 8 bytes; r[.][0] packs both halves'
                const uint32_t o = as.roff[r] + 2u * (32 * ks + 16 * h);
                const u32x2v v = __builtin_amdgcn_raw_buffer_load_b64(as.rsrc, kk < K ? o : kBufOOB, 0, 0);
                if (h == 0) raw[r][0].x = __uint_as_float(v.x), raw[r][0].y = __uint_as_float(v.y);
                else raw[r][0].z = __uint_as_float(v.x), raw[r][0].w = __uint_as_float(v.y);
                raw[r][1] = make_float4(0.f, 0.f, 0.f, 0.f);
                continue;
            }
            const uint32_t o = as.roff[r] + 4u * (32 * ks + 16 * h);
            // (VW 32, x2 planes: fp32 A's 16-byte load -- raw[.][h] = [hi k .. k + 3][lo k .. k + 3]; bres_frag
            // regroups the two pieces into the hi and the lo fragment in place)
            if constexpr (VW == 4 || VW == 32) {
                const u32x4v v = __builtin_amdgcn_raw_buffer_load_b128(as.rsrc, kk < K ? o : kBufOOB, 0, 0);
                raw[r][h] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                                        __uint_as_float(v.w));
            } else {
                const u32x2v a = __builtin_amdgcn_raw_buffer_load_b64(as.rsrc, kk < K ? o : kBufOOB, 0, 0);
                const u32x2v b = __builtin_amdgcn_raw_buffer_load_b64(as.rsrc, kk + 2 < K ? o + 8 : kBufOOB, 0, 0);
                raw[r][h] = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(b.x),
                                        __uint_as_float(b.y));
            }
        }
    }
}

// 8 fp32 -> the precision's A fragment planes (P_X3: exact three-way split; P_F16: x * s rounded)
template <int P, int VW>
__device__ __forceinline__ void bres_frag(const float4 (&r)[2], float s, bf16x8 (&a)[3]) {
    if constexpr (VW == 16) {  // fp16 A (P_F16, scale 1): the loaded halves are the fragment
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(r[0].x), __float_as_uint(r[0].y),
                                                     __float_as_uint(r[0].z), __float_as_uint(r[0].w)));
        return;
    }
    if constexpr (VW == 32) {
        // x2 planes (scale 1): r[0] = [hi k ..][lo k ..], r[1] = [hi k + 16 ..][lo k + 16 ..] -> the hi fragment
        // (r[0].xy, r[1].xy) and the lo fragment (r[0].zw, r[1].zw).  Two register swaps in the raw registers
        // themselves (dead after this step until reloaded: the callers' raw sets are their own locals), so an
        // MFMA operand is a loaded register quadruple and no copy of the eight is held
        static_assert(P == P_X2, "x2 planes: P_X2");
        float4(&m)[2] = const_cast<float4(&)[2]>(r);
        // (the two wait states between a VALU write and an MFMA reading it as an operand: inside the string)
        asm("v_swap_b32 %0, %2\n\tv_swap_b32 %1, %3\n\ts_nop 1"
            : "+v"(m[0].z), "+v"(m[0].w), "+v"(m[1].x), "+v"(m[1].y));
#pragma unroll
        for (int q = 0; q < 2; q++)
            a[q] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(m[q].x), __float_as_uint(m[q].y),
                                                         __float_as_uint(m[q].z), __float_as_uint(m[q].w)));
        return;
    }
#ifdef BRES_NO_SPLIT  // diagnostic builds only: the raw bits as fragments (no split VALU; outputs wrong)
    a[0] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(r[0].x), __float_as_uint(r[0].y),
                                                 __float_as_uint(r[1].x), __float_as_uint(r[1].y)));
    a[1] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(r[0].z), __float_as_uint(r[0].w),
                                                 __float_as_uint(r[1].z), __float_as_uint(r[1].w)));
    a[2] = a[0];
    return;
#endif
    if constexpr (P == P_X3) {
        uint32_t h[4], m[4], l[4];
        split2(r[0].x, r[0].y, h[0], m[0], l[0]);
        split2(r[0].z, r[0].w, h[1], m[1], l[1]);
        split2(r[1].x, r[1].y, h[2], m[2], l[2]);
        split2(r[1].z, r[1].w, h[3], m[3], l[3]);
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
        a[1] = __builtin_bit_cast(bf16x8, make_uint4(m[0], m[1], m[2], m[3]));
        a[2] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
    } else if constexpr (P == P_X2) {
        uint32_t h[4], l[4];
        pair2(r[0].x, r[0].y, s, h[0], l[0]);
        pair2(r[0].z, r[0].w, s, h[1], l[1]);
        pair2(r[1].x, r[1].y, s, h[2], l[2]);
        pair2(r[1].z, r[1].w, s, h[3], l[3]);
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
        a[1] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
    } else {
        a[0] = __builtin_bit_cast(bf16x8, make_uint4(f16x2_rn(r[0].x * s, r[0].y * s), f16x2_rn(r[0].z * s, r[0].w * s),
                                                     f16x2_rn(r[1].x * s, r[1].y * s), f16x2_rn(r[1].z * s, r[1].w * s)));
    }
}

// the final 16-wide step: the 4 values k = 4 (l >> 4) .. +3 (the j < 4 half of a TP piece)
template <int P, int VW>
__device__ __forceinline__ void bres_frag16(const float4 (&rr)[2], float s, uint2 (&a)[3]) {
    const float4& r = rr[0];  // (fp32 / fp16 A: the 16-byte piece of the j < 4 half)
    if constexpr (VW == 16) {  // fp16 A: the j < 4 half is the first 8 bytes
        a[0] = make_uint2(__float_as_uint(r.x), __float_as_uint(r.y));
        return;
    }
    if constexpr (VW == 32) {  // x2 planes: the piece is [hi k .. k + 3][lo k .. k + 3]
        a[0] = make_uint2(__float_as_uint(r.x), __float_as_uint(r.y));
        a[1] = make_uint2(__float_as_uint(r.z), __float_as_uint(r.w));
        return;
    }
    if constexpr (P == P_X3) {
        uint32_t h[2], m[2], l[2];
        split2(r.x, r.y, h[0], m[0], l[0]);
        split2(r.z, r.w, h[1], m[1], l[1]);
        a[0] = make_uint2(h[0], h[1]);
        a[1] = make_uint2(m[0], m[1]);
        a[2] = make_uint2(l[0], l[1]);
    } else if constexpr (P == P_X2) {
        uint32_t h[2], l[2];
        pair2(r.x, r.y, s, h[0], l[0]);
        pair2(r.z, r.w, s, h[1], l[1]);
        a[0] = make_uint2(h[0], h[1]);
        a[1] = make_uint2(l[0], l[1]);
    } else {
        a[0] = make_uint2(f16x2_rn(r.x * s, r.y * s), f16x2_rn(r.z * s, r.w * s));
    }
}

template <int P>
__device__ __forceinline__ f32x4 mma16(const uint2 (&a)[3], const uint2* b, f32x4 acc, f32x4& accx) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
    if constexpr (P == P_X2) {
#define MM_H4(x) __builtin_bit_cast(h4, x)
        accx = __builtin_amdgcn_mfma_f32_16x16x16f16(MM_H4(a[1]), MM_H4(b[0]), accx, 0, 0, 0);
        accx = __builtin_amdgcn_mfma_f32_16x16x16f16(MM_H4(a[0]), MM_H4(b[1]), accx, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(MM_H4(a[0]), MM_H4(b[0]), acc, 0, 0, 0);
#undef MM_H4
        return acc;
    }
    (void)accx;
    if constexpr (P == P_X3) {
#define MM_B16(x) __builtin_bit_cast(s4, x)
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(MM_B16(a[2]), MM_B16(b[0]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(MM_B16(a[0]), MM_B16(b[2]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(MM_B16(a[1]), MM_B16(b[1]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(MM_B16(a[1]), MM_B16(b[0]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(MM_B16(a[0]), MM_B16(b[1]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(MM_B16(a[0]), MM_B16(b[0]), acc, 0, 0, 0);
#undef MM_B16
    } else {
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h4, a[0]), __builtin_bit_cast(h4, b[0]), acc, 0,
                                                     0, 0);
    }
    return acc;
}

// Epilogue of one row tile x ctn column tiles (global tiles tg0 .. tg0 + ctn - 1; tg0 even).  ReLU bits:
// bit 4 c + g of the tile-local word = bit 4 (tg0 + c) + g of the row tile's mask, i.e. local byte m is
// global byte tg0 / 2 + m -- each block writes (EM_FWD) and reads (EM_BWD) whole bytes of its own tiles.
// one 32-wide k-step: cur -> fragments, step ks + 1 -> nxt (past the last step: offsets past K, zeros),
// the CT column tiles' MFMAs for both row tiles (each B fragment read feeds both)
template <int P, int CT, int RT, int VW, int D = 1>
__device__ __forceinline__ void bres_step(f32x4 (&acc)[RT][CT], f32x4 (&accx)[RT][CT], const float4 (&cur)[RT][2],
                                          float4 (&nxt)[RT][2],
                                          const BresA& as, int ks, int K, int kq, int ctb, int c0, int ctn,
                                          float ascale, const uint16_t* sF, int lane) {
    constexpr int np = Prec<P>::kPlanes;
    bf16x8 a[RT][3];
#pragma unroll
    for (int r = 0; r < RT; r++) bres_frag<P, VW>(cur[r], ascale, a[r]);
    bres_load<RT, VW>(as, ks + D, K, kq, nxt);  // D steps ahead (past the last step: zeros)
    int boff = ((ks * ctb + c0) * np) * 64 + lane;  // bf16x8 units
    asm volatile("" : "+v"(boff));                  // one base per step (not 18 hoisted addresses)
    const bf16x8* bp = reinterpret_cast<const bf16x8*>(sF) + boff;
#if BRES_BPREF
    // column c + 1's B fragments read while column c's MFMAs run
    bf16x8 bb[2][3];
#pragma unroll
    for (int q = 0; q < np; q++) bb[0][q] = bp[q * 64];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        if (c < ctn) {  // wave-uniform (a guard, not a break: the loop stays fully unrolled, acc in registers)
            if (c + 1 < CT && c + 1 < ctn) {
#pragma unroll
                for (int q = 0; q < np; q++) bb[(c + 1) & 1][q] = bp[((c + 1) * np + q) * 64];
            }
#pragma unroll
            for (int r = 0; r < RT; r++) acc[r][c] = mma<P>(a[r], bb[c & 1], acc[r][c], accx[r][c]);
        }
    }
#else
#pragma unroll
    for (int c = 0; c < CT; c++) {
        if (c < ctn) {  // wave-uniform (a guard, not a break: the loop stays fully unrolled, acc in registers)
            bf16x8 bb[3];
#ifdef BRES_NO_BREAD  // diagnostic builds only: B fragments from the A registers (no LDS reads; outputs wrong)
#pragma unroll
            for (int q = 0; q < np; q++) bb[q] = a[0][(q + c) % 3];
#else
#pragma unroll
            for (int q = 0; q < np; q++) bb[q] = bp[(c * np + q) * 64];
#endif
#pragma unroll
            for (int r = 0; r < RT; r++) acc[r][c] = mma<P>(a[r], bb, acc[r][c], accx[r][c]);
        }
    }
#endif
}

template <int P, int CT, int RT, int EM, int VW>
__global__ __launch_bounds__(64 * kBresWaves) void k_bres(const float* __restrict__ A, int lda, float ascale,
                                                   const uint16_t* __restrict__ B, int M, int N, int K, int nks,
                                                   BresPlan pl, Epi ep) {
    static_assert(EM == EM_F32 || em_fwd(EM) || em_bwd(EM), "row-major outputs");
    static_assert(VW != 16 || P == P_F16, "fp16 A: P_F16");
    static_assert(VW != 32 || P == P_X2, "x2 planes A: P_X2");
    constexpr int np = Prec<P>::kPlanes;
    extern __shared__ __attribute__((aligned(16))) uint16_t smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int X = pl.xcds, x = (int)blockIdx.x % X, wi = (int)blockIdx.x / X;
    X3_STAMP(0, 0, __builtin_amdgcn_s_memtime());
    X3_STAMP(0, 4, __builtin_amdgcn_s_memrealtime());
    if (wi >= pl.first[pl.nblk]) return;  // a surplus workgroup: uniform, before any barrier
    int b = 0;
    while (b + 1 < pl.nblk && wi >= pl.first[b + 1]) b++;
    const int t0 = pl.tstart[b], ctb = pl.tstart[b + 1] - t0;
    const int nfull = pl.nfull, half = pl.half;
    uint16_t* sF = smem;                               // [nfull][ctb][np][512]: a step's pieces at immediate offsets
    uint16_t* sT = smem + (size_t)ctb * nfull * np * 512;  // [ctb][np][256]: the 16-wide step
    float* sbias = reinterpret_cast<float*>(sT + ctb * np * 256 * half);

    // ---- the block of B -> LDS, once ----
    const int nF = ctb * nfull * np;
    for (int p = wave; p < nF; p += kBresWaves) {
        const int q = p % np, cks = p / np, c = cks % ctb, ks = cks / ctb;
        const uint4* src =
            reinterpret_cast<const uint4*>(B + ((size_t)(t0 + c) * nks + ks) * Prec<P>::kBlk + q * 512);
        __builtin_amdgcn_global_load_lds(src + lane, sF + (size_t)p * 512, 16, 0, 0);
    }
    if (half) {
        for (int p = wave; p < ctb * np; p += kBresWaves) {
            const int q = p % np, c = p / np;
            const uint2* src =
                reinterpret_cast<const uint2*>(B + ((size_t)(t0 + c) * nks + nfull) * Prec<P>::kBlk + q * 512);
            reinterpret_cast<uint2*>(sT + p * 256)[lane] = src[2 * lane];
        }
    }
    if (!em_bwd(EM) && ep.bias)
        for (int t = threadIdx.x; t < ctb * 16; t += 64 * kBresWaves) {
            const int col = 16 * t0 + t;
            sbias[t] = col < N ? ep.bias[col] : 0.f;
        }
    __syncthreads();  // vmcnt(0) + barrier: every wave's DMA pieces and writes landed
    X3_STAMP(0, 1, __builtin_amdgcn_s_memtime());

    // ---- independent waves ----
    // the workgroup takes groups of 16 consecutive 32-row units (512 rows, one per wave): groups
    // x + X (wb + nW t) for t = 0, 1, ...  -- each CU's loads and stores stay inside one ~0.5 MB stretch
    // of A and C at a time (scattering a workgroup's waves over the matrix measured ~2x slower)
    const int nu = (M + 16 * RT - 1) / (16 * RT);
    const int nW = pl.first[b + 1] - pl.first[b], wb = wi - pl.first[b];
    const int nsb = (ctb + CT - 1) / CT;
    const int kq = 4 * (lane >> 4);
    // gfx9 buffer resource word 3 0x00020000: 32-bit data format, raw (stride 0) addressing
    constexpr uint32_t aesz = VW == 16 ? 2u : 4u;  // VW 16: A is fp16 [M, lda] (32: x2 planes, a pair per element)
    const __amdgpu_buffer_rsrc_t arsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)A, (short)0, (int)((size_t)M * lda * aesz), 0x00020000);
    const __amdgpu_buffer_rsrc_t crs =  // C [M, ldc]: rows past M past num_records
        __builtin_amdgcn_make_buffer_rsrc((void*)ep.c, (short)0, (int)((size_t)M * ep.ldc * (em_16(EM) && P != P_X2 ? 2 : 4)),
                                          0x00020000);
    const __amdgpu_buffer_rsrc_t srs =  // colsum [ceil(M / 16), N]
        __builtin_amdgcn_make_buffer_rsrc((void*)ep.colsum, (short)0, (int)((size_t)((M + 15) / 16) * N * 4),
                                          0x00020000);
    for (int t = 0;; t++) {
        const int u = (x + X * (wb + nW * t)) * kBresWaves + wave;
        if (u >= nu) break;
        BresA as;
        as.rsrc = arsrc;
#pragma unroll
        for (int r = 0; r < RT; r++) {
#ifdef BRES_ROW0  // diagnostic builds only: every unit reads the first 32 rows (A L2-resident; outputs wrong)
            const int row = min(16 * r + (lane & 15), M - 1);
#else
            const int row = min(16 * (RT * u + r) + (lane & 15), M - 1);  // rows past M: computed, not stored
#endif
            as.roff[r] = aesz * ((uint32_t)row * (uint32_t)lda + (uint32_t)kq);
        }
        for (int s = 0; s < nsb; s++) {
            const int c0 = s * CT, ctn = min(CT, ctb - c0);
            f32x4 acc[RT][CT], accx[RT][CT];  // accx: P_X2's cross terms (unused otherwise)
#pragma unroll
            for (int r = 0; r < RT; r++)
#pragma unroll
                for (int c = 0; c < CT; c++) acc[r][c] = accx[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            // A register buffers: step ks splits cur and loads a later step into another buffer, so the
            // loads stay in flight over whole steps (one buffer made the compiler copy at the loop end,
            // waiting for the loads it had just issued).  RT = 2 (x3): two buffers, one step ahead; RT = 1
            // (f16, bound by its A loads): three buffers, two steps ahead.
            uint2 a4[RT][3];
            if constexpr (RT == 1) {
                float4 rA[RT][2], rB[RT][2], rC[RT][2];
                bres_load<RT, VW>(as, 0, K, kq, rA);
                bres_load<RT, VW>(as, 1, K, kq, rB);
                int ks = 0;
                for (; ks + 3 <= nfull; ks += 3) {
                    bres_step<P, CT, RT, VW, 2>(acc, accx, rA, rC, as, ks, K, kq, ctb, c0, ctn, ascale, sF, lane);
                    bres_step<P, CT, RT, VW, 2>(acc, accx, rB, rA, as, ks + 1, K, kq, ctb, c0, ctn, ascale, sF, lane);
                    bres_step<P, CT, RT, VW, 2>(acc, accx, rC, rB, as, ks + 2, K, kq, ctb, c0, ctn, ascale, sF, lane);
                }
                const int rem = nfull - ks;  // A holds step ks, B step ks + 1
                if (rem >= 1) bres_step<P, CT, RT, VW, 2>(acc, accx, rA, rC, as, ks, K, kq, ctb, c0, ctn, ascale, sF, lane);
                if (rem >= 2) bres_step<P, CT, RT, VW, 2>(acc, accx, rB, rA, as, ks + 1, K, kq, ctb, c0, ctn, ascale, sF, lane);
                if (half) {  // step nfull is in A (rem 0), B (rem 1) or C (rem 2)
#pragma unroll
                    for (int r = 0; r < RT; r++)
                        bres_frag16<P, VW>(rem == 0 ? rA[r] : rem == 1 ? rB[r] : rC[r], ascale, a4[r]);
                }
            } else {
                float4 rawA[RT][2], rawB[RT][2];
                bres_load<RT, VW>(as, 0, K, kq, rawA);
                int ks = 0;
                for (; ks + 2 <= nfull; ks += 2) {
                    bres_step<P, CT, RT, VW>(acc, accx, rawA, rawB, as, ks, K, kq, ctb, c0, ctn, ascale, sF, lane);
                    bres_step<P, CT, RT, VW>(acc, accx, rawB, rawA, as, ks + 1, K, kq, ctb, c0, ctn, ascale, sF, lane);
                }
                const bool odd = ks < nfull;
                if (odd) bres_step<P, CT, RT, VW>(acc, accx, rawA, rawB, as, ks, K, kq, ctb, c0, ctn, ascale, sF, lane);
                if (half) {
#pragma unroll
                    for (int r = 0; r < RT; r++) bres_frag16<P, VW>(odd ? rawB[r] : rawA[r], ascale, a4[r]);
                }
            }
            if (half) {
                const uint2* bp = reinterpret_cast<const uint2*>(sT) + (size_t)(c0 * np) * 64 + lane;
#pragma unroll
                for (int c = 0; c < CT; c++) {
                    if (c < ctn) {
                        uint2 bb[3];
#pragma unroll
                        for (int q = 0; q < np; q++) bb[q] = bp[(c * np + q) * 64];
#pragma unroll
                        for (int r = 0; r < RT; r++) acc[r][c] = mma16<P>(a4[r], bb, acc[r][c], accx[r][c]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RT; r++)
#pragma unroll
                for (int c = 0; c < CT; c++) acc[r][c] = x2_combine<P>(acc[r][c], accx[r][c]);
#pragma unroll
            for (int r = 0; r < RT; r++)
                bres_epilogue<P, CT, EM>(acc[r], RT * u + r, t0 + c0, ctn, M, N, ep, crs, srs, sbias + 16 * c0, lane);
        }
        X3_STAMP(1 + t, 2, __builtin_amdgcn_s_memtime());  // end of unit t
    }
    X3_STAMP(0, 3, __builtin_amdgcn_s_memtime());
    X3_STAMP(0, 5, __builtin_amdgcn_s_memrealtime());
}

// ---------------------------------------------------------------------------
// k_critic_update: the per-row part of the update's critic (K0 -> 64 -> 64 -> 1, P_X2) in one persistent
// launch: the three forward layers, dV of the value loss, dY1 = dV w2 (h1 > 0) and dY0 = (dY1 W1) (h0 > 0),
// replacing three k_bres forwards, k_mse_loss's dV, k_heads_bwd and the k_bres input gradient -- with their
// fragments, k order, MFMA sequence and epilogue arithmetic, so every output equals theirs bit for bit
// (k_critic_value's update-side sibling).  One workgroup per CU holds the packed planes of W0, W1, W1^T and w2
// in LDS (k_bres's images); each wave walks 16-row tiles on its own (no barrier after the weights are in):
// x from HBM once, h0 / h1 / dY1 from accumulator layout to the next layer's A layout through a wave-private
// fp32 tile in LDS instead of through HBM.  It writes what the weight-gradient launches read: V, dV, h0, h1,
// dY1, dY0 (fp32 [M, 64]) and the 16-row column sums of dY1 and dY0 (the bias gradients' partials).
// ---------------------------------------------------------------------------
constexpr int kCuWaves = 8;
constexpr int kCuScr = 68;           // floats per row of the wave-private fp32 tile
// LDS (bytes)
constexpr int kCuW0 = 0;                        // [4 k-steps][4 tiles][2 planes][1 KiB]
constexpr int kCuT0 = kCuW0 + 32768;            // [4][2][512 B]: the 16-wide tail step
constexpr int kCuW1 = kCuT0 + 4096;             // [2][4][2][1 KiB]
constexpr int kCuW1T = kCuW1 + 16384;
constexpr int kCuW2 = kCuW1T + 16384;           // [2][1][2][1 KiB]
constexpr int kCuScrOff = kCuW2 + 4096;         // [waves][16][kCuScr] fp32
constexpr int kCuLds = kCuScrOff + kCuWaves * 16 * kCuScr * 4;
static_assert(kCuLds <= 160 * 1024, "k_critic_update's LDS");

struct CuArgs {
    const float* x;  // [M, ldx] observations
    int ldx, K0, M;
    const float* rtg;                    // [M]
    const uint16_t *w0, *w1, *w1t, *w2;  // P_X2 TP packs: W0 [64, K0], W1 [64, 64], W1^T, w2 [1, 64]
    const float *b0, *b1, *w2f, *b2;
    float gscale, norm;                  // 2^floor(log2 M); 2 / M
    float *v, *dv;                       // [M]
    float *h0, *h1, *dy1, *dy0;          // [M, 64]
    float *cs1, *cs0;                    // [ceil(M / 16), 64]: column sums of dY1 / dY0 per 16-row tile
};

__device__ __forceinline__ void cu_wave_sync() {  // the wave's LDS writes before its reads (and back)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// an accumulator-layout tile block -> the wave's fp32 tile [16][kCuScr]
__device__ __forceinline__ void cu_put(float* scr, const f32x4 (&t)[4], int lane) {
    float* p = scr + 4 * (lane >> 4) * kCuScr + (lane & 15);
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int g = 0; g < 4; g++) p[g * kCuScr + 16 * c] = t[c][g];
}

// NT column tiles' products of one k-step: mma<P_X2>'s three MFMAs per tile (lo hi and hi lo into accx, hi hi
// into acc -- each accumulator sees that sequence), issued tile-interleaved so that one wave per SIMD does not
// wait on back-to-back dependent MFMAs
template <int NT>
__device__ __forceinline__ void cu_mma(const bf16x8 (&a)[3], const bf16x8 (&b)[NT][2], f32x4 (&acc)[NT],
                                       f32x4 (&accx)[NT]) {
#define MM_H8(x) __builtin_bit_cast(f16x8, x)
#pragma unroll
    for (int c = 0; c < NT; c++) accx[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(MM_H8(a[1]), MM_H8(b[c][0]), accx[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NT; c++) accx[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(MM_H8(a[0]), MM_H8(b[c][1]), accx[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NT; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(MM_H8(a[0]), MM_H8(b[c][0]), acc[c], 0, 0, 0);
#undef MM_H8
}
// the same on the 16-deep MFMA (mma16<P_X2>'s sequence): a, b[c] = (hi, lo) pieces of four halves
template <int NT>
__device__ __forceinline__ void cu_mma16(const uint2 (&a)[2], const uint2 (&b)[NT][2], f32x4 (&acc)[NT],
                                         f32x4 (&accx)[NT]) {
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
#define MM_H4(x) __builtin_bit_cast(h4, x)
#pragma unroll
    for (int c = 0; c < NT; c++) accx[c] = __builtin_amdgcn_mfma_f32_16x16x16f16(MM_H4(a[1]), MM_H4(b[c][0]), accx[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NT; c++) accx[c] = __builtin_amdgcn_mfma_f32_16x16x16f16(MM_H4(a[0]), MM_H4(b[c][1]), accx[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NT; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x16f16(MM_H4(a[0]), MM_H4(b[c][0]), acc[c], 0, 0, 0);
#undef MM_H4
}

// one 64-wide layer of the wave's tile: A rows from its fp32 tile (k_bres's fp32-A fragments at scale s),
// B the NT column tiles of a resident pack [2 k-steps][NT][2 planes][1 KiB]
template <int NT>
__device__ __forceinline__ void cu_layer64(const float* scr, float s, const unsigned char* sB, int lane,
                                           f32x4 (&acc)[NT]) {
    f32x4 accx[NT];
#pragma unroll
    for (int c = 0; c < NT; c++) acc[c] = accx[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ar = scr + (lane & 15) * kCuScr + 4 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
        float4 raw[2];
        raw[0] = *reinterpret_cast<const float4*>(ar + 32 * ks);
        raw[1] = *reinterpret_cast<const float4*>(ar + 32 * ks + 16);
        bf16x8 a[3];
        a[2] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        bres_frag<P_X2, 4>(raw, s, a);
        const bf16x8* bp = reinterpret_cast<const bf16x8*>(sB) + (ks * NT * 2) * 64 + lane;
        bf16x8 bb[NT][2];
#pragma unroll
        for (int c = 0; c < NT; c++) bb[c][0] = bp[(c * 2) * 64], bb[c][1] = bp[(c * 2 + 1) * 64];
        cu_mma<NT>(a, bb, acc, accx);
    }
#pragma unroll
    for (int c = 0; c < NT; c++) acc[c] = x2_combine<P_X2>(acc[c], accx[c]);
}

__global__ __launch_bounds__(64 * kCuWaves) void k_critic_update(CuArgs ca) {
    extern __shared__ __attribute__((aligned(16))) uint16_t smem[];
    unsigned char* sm = reinterpret_cast<unsigned char*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K0 = ca.K0, M = ca.M, ldx = ca.ldx;
    // k_bres's steps of K0 = 130 or 132 (the critic of two agents): four 32-wide, the 16-wide tail
    constexpr int nks0 = 5, nfull = 4;

    // ---- the packed weights -> LDS, once (k_bres's images of the four packs) ----
    for (int i = threadIdx.x; i < nfull * 8 * 64; i += 64 * kCuWaves) {
        const int p = i >> 6, q = p & 1, c = (p >> 1) & 3, ks = p >> 3;
        reinterpret_cast<uint4*>(sm + kCuW0)[i] =
            reinterpret_cast<const uint4*>(ca.w0 + ((size_t)c * nks0 + ks) * 1024 + q * 512)[i & 63];
    }
    for (int i = threadIdx.x; i < 8 * 64; i += 64 * kCuWaves) {
        const int p = i >> 6, q = p & 1, c = p >> 1;
        reinterpret_cast<uint2*>(sm + kCuT0)[i] =
            reinterpret_cast<const uint2*>(ca.w0 + ((size_t)c * nks0 + nfull) * 1024 + q * 512)[2 * (i & 63)];
    }
    for (int i = threadIdx.x; i < 16 * 64; i += 64 * kCuWaves) {
        const int p = i >> 6, q = p & 1, c = (p >> 1) & 3, ks = p >> 3;
        const size_t o = ((size_t)c * 2 + ks) * 1024 + q * 512;
        reinterpret_cast<uint4*>(sm + kCuW1)[i] = reinterpret_cast<const uint4*>(ca.w1 + o)[i & 63];
        reinterpret_cast<uint4*>(sm + kCuW1T)[i] = reinterpret_cast<const uint4*>(ca.w1t + o)[i & 63];
    }
    for (int i = threadIdx.x; i < 4 * 64; i += 64 * kCuWaves) {
        const int p = i >> 6, q = p & 1, ks = p >> 1;
        reinterpret_cast<uint4*>(sm + kCuW2)[i] =
            reinterpret_cast<const uint4*>(ca.w2 + (size_t)ks * 1024 + q * 512)[i & 63];
    }
    __syncthreads();

    const int cl = lane & 15, rq = 4 * (lane >> 4), kq = 4 * (lane >> 4);
    float b0r[4], b1r[4], w2r[4];
#pragma unroll
    for (int c = 0; c < 4; c++) b0r[c] = ca.b0[16 * c + cl], b1r[c] = ca.b1[16 * c + cl], w2r[c] = ca.w2f[16 * c + cl];
    const float b2 = ca.b2[0], gs = ca.gscale, gsi = 1.f / ca.gscale, norm = ca.norm;
    float* scr = reinterpret_cast<float*>(sm + kCuScrOff) + wave * 16 * kCuScr;
    // x through a buffer resource, as k_bres reads it: offsets past the end (the columns >= K0) return zeros;
    // the [M, 64] outputs too: rows past M fall past num_records and are dropped
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)ca.x, (short)0, (int)((size_t)M * ldx * 4), 0x00020000);
    const int obytes = (int)((size_t)M * 64 * 4);
    const __amdgpu_buffer_rsrc_t rh0 = __builtin_amdgcn_make_buffer_rsrc((void*)ca.h0, (short)0, obytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rh1 = __builtin_amdgcn_make_buffer_rsrc((void*)ca.h1, (short)0, obytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry1 = __builtin_amdgcn_make_buffer_rsrc((void*)ca.dy1, (short)0, obytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry0 = __builtin_amdgcn_make_buffer_rsrc((void*)ca.dy0, (short)0, obytes, 0x00020000);
    uint32_t rm = 0u;  // the range guard: the largest |bits| of the x2 accumulators

    const int ntiles = (M + 15) / 16, stride = kCuWaves * (int)gridDim.x;
    float4 raw[5][1][2];  // a tile's x as k_bres's fp32-A loads (8-byte rows), one tile ahead
    {
        BresA as;
        as.rsrc = xrs;
        as.roff[0] = as.roff[1] =
            4u * ((uint32_t)min(16 * (kCuWaves * (int)blockIdx.x + wave) + cl, M - 1) * (uint32_t)ldx + (uint32_t)kq);
#pragma unroll
        for (int ks = 0; ks < 5; ks++) bres_load<1, 2>(as, ks, K0, kq, raw[ks]);
    }
    for (int rt = kCuWaves * (int)blockIdx.x + wave; rt < ntiles; rt += stride) {
        // ---- this tile's A fragments of layer 0; then the next tile's loads ----
        bf16x8 af[4][3];
        uint2 at[3];
        at[2] = make_uint2(0u, 0u);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            af[ks][2] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            bres_frag<P_X2, 2>(raw[ks][0], 1.f, af[ks]);
        }
        bres_frag16<P_X2, 2>(raw[nfull][0], 1.f, at);
        float rtgv[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = 16 * rt + rq + g;
            rtgv[g] = (cl == 0 && row < M) ? ca.rtg[row] : 0.f;
        }
        {
            BresA as;
            as.rsrc = xrs;
            as.roff[0] = as.roff[1] = 4u * ((uint32_t)min(16 * (rt + stride) + cl, M - 1) * (uint32_t)ldx + (uint32_t)kq);
#pragma unroll
            for (int ks = 0; ks < 5; ks++) bres_load<1, 2>(as, ks, K0, kq, raw[ks]);
        }
        uint32_t voff[4];  // this lane's four rows of an [M, 64] output, column cl (tile c at immediate 64 c)
#pragma unroll
        for (int g = 0; g < 4; g++) voff[g] = 4u * ((uint32_t)(16 * rt + rq + g) * 64u + (uint32_t)cl);

        // ---- layer 0 (k_bres: the 32-wide steps, the 16-wide tail, combine, bias, ReLU) ----
        f32x4 h0[4];
        {
            f32x4 accx[4];
#pragma unroll
            for (int c = 0; c < 4; c++) h0[c] = accx[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < nfull; ks++) {
                const bf16x8* bp = reinterpret_cast<const bf16x8*>(sm + kCuW0) + (ks * 8) * 64 + lane;
                bf16x8 bb[4][2];
#pragma unroll
                for (int c = 0; c < 4; c++) bb[c][0] = bp[(c * 2) * 64], bb[c][1] = bp[(c * 2 + 1) * 64];
                cu_mma<4>(af[ks], bb, h0, accx);
            }
            {
                const uint2* bp = reinterpret_cast<const uint2*>(sm + kCuT0) + lane;
                uint2 bb[4][2];
#pragma unroll
                for (int c = 0; c < 4; c++) bb[c][0] = bp[(c * 2) * 64], bb[c][1] = bp[(c * 2 + 1) * 64];
                const uint2 a2[2] = {at[0], at[1]};
                cu_mma16<4>(a2, bb, h0, accx);
            }
#pragma unroll
            for (int c = 0; c < 4; c++) {
                h0[c] = x2_combine<P_X2>(h0[c], accx[c]);
                range_acc<P_X2>(rm, h0[c]);
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    h0[c][g] = fmaxf(h0[c][g] + b0r[c], 0.f);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(h0[c][g]), rh0, voff[g], 64 * c, 0);
                }
            }
        }
        cu_put(scr, h0, lane);
        cu_wave_sync();

        // ---- layer 1, the value head, dV ----
        f32x4 h1[4];
        cu_layer64<4>(scr, 1.f, sm + kCuW1, lane, h1);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            range_acc<P_X2>(rm, h1[c]);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                h1[c][g] = fmaxf(h1[c][g] + b1r[c], 0.f);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(h1[c][g]), rh1, voff[g], 64 * c, 0);
            }
        }
        cu_wave_sync();
        cu_put(scr, h1, lane);
        cu_wave_sync();
        f32x4 vv[1];
        cu_layer64<1>(scr, 1.f, sm + kCuW2, lane, vv);
        range_acc<P_X2>(rm, vv[0]);
        float dvb[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = 16 * rt + rq + g;
            float dv = 0.f;
            if (cl == 0 && row < M) {  // column 0 of the head's tile; k_mse_loss's dV
                const float v = vv[0][g] + b2;
                ca.v[row] = v;
                dv = (v - rtgv[g]) * norm;
                ca.dv[row] = dv;
            }
            dvb[g] = __shfl(dv, lane & 48);  // rows past M: 0, and with it every gradient term of the row
        }

        // ---- dY1 = dV w2 (h1 > 0) (k_heads_bwd); dY0 = (dY1 W1) (h0 > 0) at the gradient scale (k_bres) ----
        const bool tile_ok = lane < 16;  // (16 rt < M: the loop's bound)
        f32x4 dy[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float cs = 0.f;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                dy[c][g] = h1[c][g] > 0.f ? fmaf(dvb[g], w2r[c], 0.f) : 0.f;
                if (16 * rt + rq + g < M) cs += dy[c][g];
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dy[c][g]), ry1, voff[g], 64 * c, 0);
            }
            cs += __shfl_xor(cs, 16);
            cs += __shfl_xor(cs, 32);
            if (tile_ok) ca.cs1[(size_t)rt * 64 + 16 * c + cl] = cs;
        }
        cu_wave_sync();
        cu_put(scr, dy, lane);
        cu_wave_sync();
        cu_layer64<4>(scr, gs, sm + kCuW1T, lane, dy);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            range_acc<P_X2>(rm, dy[c]);
            float cs = 0.f;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                dy[c][g] = (h0[c][g] > 0.f && 16 * rt + rq + g < M) ? dy[c][g] * gsi : 0.f;
                cs += dy[c][g];
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dy[c][g]), ry0, voff[g], 64 * c, 0);
            }
            cs += __shfl_xor(cs, 16);
            cs += __shfl_xor(cs, 32);
            if (tile_ok) ca.cs0[(size_t)rt * 64 + 16 * c + cl] = cs;
        }
        cu_wave_sync();  // the fp32 tile is read: the next tile writes it
    }
    range_note_wave<P_X2>(__builtin_amdgcn_ballot_w64(rm >= 0x7F800000u));
}

}  // namespace x3
}  // namespace mm

using namespace mm::x3;

#ifdef X3_STAMPS
extern "C" int mm_x3_stamps_read(unsigned long long* out, long n) {
    const long cap = (long)(sizeof(g_x3_stamps) / sizeof(g_x3_stamps[0]));
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_x3_stamps), (n < cap ? n : cap) * sizeof(unsigned long long), 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int mm_trunk_stamps_read(unsigned long long* out, long n) {
    const long cap = (long)(sizeof(g_tr_stamps) / sizeof(g_tr_stamps[0]));
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tr_stamps), (n < cap ? n : cap) * sizeof(unsigned long long), 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int mm_x3_stamps_clear() {
    static unsigned long long zero[256 * 16 * kWaves * 8];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_x3_stamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice) == hipSuccess
               ? 0 : -1;
}
#endif

extern "C" long mm_x3_tp_len(int R, int C) { return (long)(rup(R, kRowPad) / 16) * (rup(C, 32) / 32) * kBlk; }

extern "C" long mm_gemm_tp_len(int prec, int R, int C) {
    if (prec != MM_PREC_X3 && prec != MM_PREC_F16 && prec != MM_PREC_X2) return MM_E_ARG;
    return mm_x3_tp_len(R, C) / 3 * (prec == MM_PREC_X3 ? 3 : prec == MM_PREC_X2 ? 2 : 1);
}

extern "C" long mm_x3_mbits_len(int M) { return (long)(rup(M, kRowPad) / 16) * 64 * kMaskWords; }

extern "C" int mm_gemm_tp_pack(int prec, const float* X, int R, int C, int ld, int trans, uint16_t* tp,
                               void* stream) {
    if (!X || !tp || R <= 0 || C <= 0 || ld < (trans ? R : C)) return MM_E_ARG;
    if ((uintptr_t)tp & 15) return MM_E_ARG;
    const int nks = rup(C, 32) / 32;
    const long total = (long)(rup(R, kRowPad) / 16) * nks * 64;
    const int grid = (int)std::min<long>((total + 255) / 256, 256L * 64);
    if (prec == MM_PREC_X3)
        hipLaunchKernelGGL(k_tp_pack<P_X3>, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, R, C, ld, trans, nks,
                           total, tp);
    else if (prec == MM_PREC_F16)
        hipLaunchKernelGGL(k_tp_pack<P_F16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, R, C, ld, trans, nks,
                           total, tp);
    else if (prec == MM_PREC_X2)
        hipLaunchKernelGGL(k_tp_pack<P_X2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, R, C, ld, trans, nks,
                           total, tp);
    else
        return MM_E_ARG;
    return (int)hipGetLastError();
}

extern "C" int mm_gemm_tp_pack_multi(int prec, const mm_pack_seg_t* segs, int nseg, void* stream) {
    if (!segs || nseg <= 0 || nseg > kMaxPackSegs) return MM_E_ARG;
    PackSegs ps;
    ps.nseg = nseg;
    ps.pre[0] = 0;
    for (int k = 0; k < nseg; k++) {
        const mm_pack_seg_t& g = segs[k];
        if (!g.X || !g.tp || g.R <= 0 || g.C <= 0 || g.ld < (g.trans ? g.R : g.C) || ((uintptr_t)g.tp & 15))
            return MM_E_ARG;
        ps.s[k] = g;
        ps.nks[k] = rup(g.C, 32) / 32;
        ps.pre[k + 1] = ps.pre[k] + (long)(rup(g.R, kRowPad) / 16) * ps.nks[k] * 64;
    }
    const int grid = (int)std::min<long>((ps.pre[nseg] + 255) / 256, 256L * 64);
    if (prec == MM_PREC_X3)
        hipLaunchKernelGGL(k_tp_pack_multi<P_X3>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ps);
    else if (prec == MM_PREC_F16)
        hipLaunchKernelGGL(k_tp_pack_multi<P_F16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ps);
    else if (prec == MM_PREC_X2)
        hipLaunchKernelGGL(k_tp_pack_multi<P_X2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ps);
    else
        return MM_E_ARG;
    return (int)hipGetLastError();
}

extern "C" int mm_x3_tp_pack(const float* X, int R, int C, int ld, int trans, uint16_t* tp, void* stream) {
    return mm_gemm_tp_pack(MM_PREC_X3, X, R, C, ld, trans, tp, stream);
}

static int persistent_grid() {  // one 16-wave workgroup per CU
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    }
    return cus;
}

template <int NT, int P, class AS, class AT>
static int launch_nt(const AT* a, int lda, float ascale, const uint16_t* b, int M, int N, int K, int ncb,
                     const Epi& ep, hipStream_t s) {
    constexpr int kT = SW<P>::kThreads;
    const int nks = rup(K, 32) / 32;
    const int nrb = rup(M, SW<P>::kBM) / SW<P>::kBM;
    const int grid = std::min(rup(nrb, 8) * ncb, persistent_grid() * (P == P_X2 ? 2 : 1));
    if (ep.ctp && ep.c) return MM_E_ARG;  // one output form per launch
    if constexpr (P == P_X3) {
        if (ep.ctp) {
            hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, EM_TP>), dim3(grid), dim3(kT), 0, s, a, lda, ascale, b, M,
                               N, K, nks, nrb, ncb, ep);
            return (int)hipGetLastError();
        }
    } else if (ep.ctp) {
        return MM_E_ARG;
    }
    if (ep.c16) {  // fp16 activations out: P_F16's forward with bits, through the buffer-store epilogue
        if constexpr (P == P_F16) {
            if (!ep.mbits_out || !ep.bufok) return MM_E_ARG;
            hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, EM_FWD16>), dim3(grid), dim3(kT), 0, s, a, lda, ascale, b, M, N,
                               K, nks, nrb, ncb, ep);
            return (int)hipGetLastError();
        }
        if constexpr (P == P_X2 && !std::is_same<AS, ASrcF32U>::value) {  // x2 planes out: forward or input gradient
            if ((!ep.mbits_out && !ep.mbits_in) || !ep.bufok) return MM_E_ARG;
            if (ep.mbits_out)
                hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, EM_FWD16>), dim3(grid), dim3(kT), 0, s, a, lda, ascale, b,
                                   M, N, K, nks, nrb, ncb, ep);
            else
                hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, EM_BWD16>), dim3(grid), dim3(kT), 0, s, a, lda, ascale, b,
                                   M, N, K, nks, nrb, ncb, ep);
            return (int)hipGetLastError();
        }
        return MM_E_ARG;
    }
    if (ep.mbits_out)
        hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, EM_FWD>), dim3(grid), dim3(kT), 0, s, a, lda, ascale, b, M, N,
                           K, nks, nrb, ncb, ep);
    else if (ep.mbits_in)
        hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, EM_BWD>), dim3(grid), dim3(kT), 0, s, a, lda, ascale, b, M, N,
                           K, nks, nrb, ncb, ep);
    else if constexpr (std::is_same<AS, ASrcX2PV>::value)
        return MM_E_ARG;  // x2 planes A: the hidden layers' forms only (with bits)
    else
        hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, EM_F32>), dim3(grid), dim3(kT), 0, s, a, lda, ascale, b, M, N,
                           K, nks, nrb, ncb, ep);
    return (int)hipGetLastError();
}

template <int P, class AS, class AT>
static int dispatch_nt(const AT* a, int lda, float ascale, const uint16_t* b_tp, int M, int N, int K, const Epi& ep,
                       hipStream_t s) {
    // column tiling: one block of <= 17 tiles, or several blocks of 15 (B rows are padded to 256)
    const int tiles = (N + 15) / 16;
    int NT, ncb;
    if (tiles <= 1) { NT = 1; ncb = 1; }
    else if (tiles <= 4) { NT = 4; ncb = 1; }
    else if (tiles <= 8) { NT = 8; ncb = 1; }
    else if (tiles <= 17) { NT = 17; ncb = 1; }
    else { NT = 15; ncb = (tiles + 14) / 15; }
    // few rows (the rollout's 4,096-8,192-row calls, the reference's 3,000-sample minibatches): too few
    // 256-row units to fill the chip, so the columns are split into 4-tile blocks (x5 workgroups at N =
    // 264).  Needs the buffer-store epilogue when bits are involved (it writes whole mask bytes per block).
    const int nrb = rup(M, SW<P>::kBM) / SW<P>::kBM;
    if (tiles > 4 && !ep.ctp && (ep.bufok || (!ep.mbits_in && !ep.mbits_out)) && 2L * nrb * ncb <= persistent_grid()) {
        NT = 4;
        ncb = (tiles + 3) / 4;
    }
    if (ncb * NT * 16 > rup(N, kRowPad)) return MM_E_ARG;  // B TP row padding would be overrun
    if (ep.ctp && ncb != 1) return MM_E_ARG;
    switch (NT) {
        case 1: return launch_nt<1, P, AS>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
        case 4: return launch_nt<4, P, AS>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
        case 8: return launch_nt<8, P, AS>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
        case 15:
            if constexpr (std::is_same<AS, ASrcX2PV>::value)
                return MM_E_ARG;  // (plane A comes with bits: N <= 272, one block)
            else
                return launch_nt<15, P, AS>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
        default: return launch_nt<17, P, AS>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
    }
}

// 8-byte-row A sources serve only narrow outputs (the critic's first layer)
template <int P>
static int dispatch_nt_u(const float* a, int lda, float ascale, const uint16_t* b_tp, int M, int N, int K,
                         const Epi& ep, hipStream_t s) {
    const int tiles = (N + 15) / 16;
    if (tiles <= 1) return launch_nt<1, P, ASrcF32U>(a, lda, ascale, b_tp, M, N, K, 1, ep, s);
    if (tiles <= 4) return launch_nt<4, P, ASrcF32U>(a, lda, ascale, b_tp, M, N, K, 1, ep, s);
    return MM_E_ARG;
}

// ---- k_bres dispatch ----
static int g_gemm_algo = -1;  // MM_GEMM_*; -1: not read from the environment yet
static bool bres_enabled() {
    if (g_gemm_algo < 0) {
        const char* e = getenv("MARLMAZE_GEMM_BRES");
        g_gemm_algo = (e && e[0] == '0') ? MM_GEMM_STREAM : MM_GEMM_AUTO;
    }
    return g_gemm_algo == MM_GEMM_AUTO;
}

extern "C" int mm_gemm_nt_algo(int algo) {
    bres_enabled();
    const int prev = g_gemm_algo;
    if (algo == MM_GEMM_AUTO || algo == MM_GEMM_STREAM) g_gemm_algo = algo;
    return prev;
}

constexpr int kBresMinRows = 16384;
// the B-resident kernel's row threshold: kBresMinRows, or MARLMAZE_BRES_MIN_ROWS (A/B runs of the small-M
// calls: the rollout's 4,096-8,192-row GEMMs)
static int bres_min_rows() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("MARLMAZE_BRES_MIN_ROWS");
        v = e ? atoi(e) : kBresMinRows;
        if (v < 1) v = 1;
    }
    return v;
}
// wave units: C_NARROW two row tiles x 6 column tiles (acc 48 registers; each B fragment read feeds two
// tiles) -- x3, and f16 up to 6 tiles; C_WIDE (f16) one row tile x up to 17 column tiles (acc 68: the
// whole 264-wide output per wave, A read once)
// C_PAIR (x2): one row tile x up to 9 column tiles (two accumulator sets: 72 registers), the widest block
// two B planes leave room for at K = 264
enum { C_NARROW = 0, C_WIDE = 1, C_PAIR = 2 };
template <int C>
struct BresCfg {
    static constexpr int CT = C == C_NARROW ? 6 : C == C_WIDE ? 17 : 9, RT = C == C_NARROW ? 2 : 1;
};

// The column blocks and the per-XCD workgroup split (see k_bres); false: the shape does not fit.
static bool bres_plan(int prec, int M, int N, int K, int lda, int ldc, bool bits, BresPlan& pl, int& cfg) {
    // A and C through buffer resources (num_records < 2^31, in-range offsets < 2^31 = kBufOOB)
    if (M < bres_min_rows() || (size_t)M * lda * 4 >= ((size_t)1 << 31) || (size_t)(M + 16) * ldc * 4 >= ((size_t)1 << 31))
        return false;
    const int np = prec == MM_PREC_X3 ? 3 : prec == MM_PREC_X2 ? 2 : 1;
    const int tiles = (N + 15) / 16;
    const int nks = rup(K, 32) / 32, rem = K % 32;
    pl.half = rem != 0 && rem <= 16;
    pl.nfull = nks - pl.half;
    const long tile_bytes = (long)np * (pl.nfull * 1024L + pl.half * 512L) + 64;  // + the bias columns
    int cmax = (int)((160L * 1024) / tile_bytes);
    if (prec == MM_PREC_X2) cmax = std::min(cmax, BresCfg<C_PAIR>::CT);  // one sub-block per wave
    if (cmax < 1 || pl.nfull < 1) return false;
    // blocks: as few as fit, then the narrowest widest block; every block but the last holds e tiles, and
    // with ReLU bits e is even (blocks start at even tiles: whole mask bytes per block) -- x3 at K = 264:
    // 6 + 6 + 5, x2: 8 + 9
    int nblk = 0, e_best = 0, ctb = 0;
    for (int nb = (tiles + cmax - 1) / cmax; nb <= kBresMaxBlk && !nblk; nb++) {
        if (nb == 1) {
            nblk = 1;
            ctb = e_best = tiles;
            break;
        }
        for (int e = cmax; e >= 1; e--) {
            if (bits && (e & 1)) continue;
            const int last = tiles - e * (nb - 1);
            if (last < 1 || last > cmax) continue;
            const int wmax = std::max(e, last);
            if (!nblk || wmax < ctb) {
                nblk = nb;
                ctb = wmax;
                e_best = e;
            }
        }
    }
    if (!nblk) return false;
    if (nblk > 1 && std::min(e_best, tiles - e_best * (nblk - 1)) < 4 && prec != MM_PREC_X2)
        return false;  // A re-read per block: x3 at K = 460 (3 tiles) measured slower
    // f16 / x2 at K = 460 (blocks re-reading A of 460 columns): the streaming kernel measured faster (f16
    // 0.81x; x2, four 4-5-tile blocks: 568 vs 462 us at 419,430 rows -- BRES_X2_WIDE_K=1 builds that form)
#ifndef BRES_X2_WIDE_K
#define BRES_X2_WIDE_K 0
#endif
    if (prec != MM_PREC_X3 && nblk > 1 && K > 288 && (prec != MM_PREC_X2 || !BRES_X2_WIDE_K)) return false;
    cfg = prec == MM_PREC_X2 ? C_PAIR : (prec == MM_PREC_F16 && ctb > BresCfg<C_NARROW>::CT) ? C_WIDE : C_NARROW;
    pl.nblk = nblk;
    pl.ctb = ctb;
    pl.tiles = tiles;
    for (int bk = 0; bk <= kBresMaxBlk; bk++) pl.tstart[bk] = std::min(tiles, bk * e_best);
    pl.tstart[nblk] = tiles;
    const int G = persistent_grid();
    pl.xcds = G % 8 == 0 ? 8 : 1;
    const int per = G / pl.xcds;
    if (per < nblk) return false;
    // workgroups per block in proportion to its tiles: greedy on the largest tiles-per-workgroup
    // (equal counts per block, so that the blocks sweep the row groups in step for L2 reuse of A, measured
    // 3% slower at x2 264 x 264, round 6)
    int w[kBresMaxBlk];
    for (int bk = 0; bk < nblk; bk++) w[bk] = 1;
    for (int left = per - nblk; left > 0; left--) {
        int best = 0;
        for (int bk = 1; bk < nblk; bk++) {
            const int tb = pl.tstart[bk + 1] - pl.tstart[bk], tbest = pl.tstart[best + 1] - pl.tstart[best];
            if ((long)tb * w[best] > (long)tbest * w[bk]) best = bk;
        }
        w[best]++;
    }
    pl.first[0] = 0;
    for (int bk = 0; bk < nblk; bk++) pl.first[bk + 1] = pl.first[bk] + w[bk];
    for (int bk = nblk + 1; bk <= kBresMaxBlk; bk++) pl.first[bk] = pl.first[nblk];
    return true;
}

template <int P, int C, int EM, int VW>
static int launch_bres(const float* a, int lda, float ascale, const uint16_t* b, int M, int N, int K,
                       const BresPlan& pl, const Epi& ep, hipStream_t s) {
    constexpr int CT = BresCfg<C>::CT, RT = BresCfg<C>::RT;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)k_bres<P, CT, RT, EM, VW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024) != hipSuccess)
            return MM_E_ARG;
        attr = true;
    }
    constexpr int np = Prec<P>::kPlanes;
    const size_t lds = (size_t)pl.ctb * np * (pl.nfull * 1024 + pl.half * 512) + (size_t)pl.ctb * 16 * 4;
    hipLaunchKernelGGL((k_bres<P, CT, RT, EM, VW>), dim3(persistent_grid()), dim3(64 * kBresWaves), lds, s, a, lda, ascale, b,
                       M, N, K, rup(K, 32) / 32, pl, ep);
    return (int)hipGetLastError();
}

template <int P, int C, int VW>
static int dispatch_bres_c(const float* a, int lda, float ascale, const uint16_t* b, int M, int N, int K,
                           const BresPlan& pl, const Epi& ep, hipStream_t s) {
    if (ep.c16) {
        if constexpr (P == P_F16 || (P == P_X2 && VW != 2)) {  // fp16 out (P_F16) / x2 planes out (P_X2)
            if (ep.mbits_out) return launch_bres<P, C, EM_FWD16, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
            if (ep.mbits_in) return launch_bres<P, C, EM_BWD16, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
        }
        return MM_E_ARG;
    }
    if (ep.mbits_out) return launch_bres<P, C, EM_FWD, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
    if (ep.mbits_in) return launch_bres<P, C, EM_BWD, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
    // (x2 planes A without bits: the input gradient into the fp32-stored h0, dY1 W1)
    return launch_bres<P, C, EM_F32, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
}

template <int P, int VW>
static int dispatch_bres(const float* a, int lda, float ascale, const uint16_t* b, int M, int N, int K,
                         const BresPlan& pl, int cfg, const Epi& ep, hipStream_t s) {
    if constexpr (P == P_X2) {
        (void)cfg;
        return dispatch_bres_c<P, C_PAIR, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
    } else {
        if constexpr (P == P_F16)
            if (cfg == C_WIDE) return dispatch_bres_c<P, C_WIDE, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
        return dispatch_bres_c<P, C_NARROW, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
    }
}

static int check_common(const uint16_t* b_tp, int M, int N, int K, const float* mask, int ldm, float* c, int ldc,
                        uint16_t* c_tp) {
    if (!b_tp || M < 0 || N <= 0 || K <= 0 || (!c && !c_tp)) return MM_E_ARG;
    if (c && (ldc < N || ((uintptr_t)c & 3))) return MM_E_ARG;
    if (mask && ldm < N) return MM_E_ARG;
    if (((uintptr_t)b_tp | (uintptr_t)c_tp) & 15) return MM_E_ARG;
    return 0;
}

// C = A . B^T (+bias)(ReLU)(* (mask > 0)): A TP of [M, K], B TP of [N, K];
// outputs fp32 c [M, ldc] and/or TP ctp of [M, N].
extern "C" int mm_x3_nt(const uint16_t* a_tp, const uint16_t* b_tp, int M, int N, int K, const float* bias, int relu,
                        const float* mask, int ldm, float* c, int ldc, uint16_t* c_tp, void* stream) {
    int e = check_common(b_tp, M, N, K, mask, ldm, c, ldc, c_tp);
    if (e) return e;
    if (!a_tp || ((uintptr_t)a_tp & 15)) return MM_E_ARG;
    if (M == 0) return 0;
    Epi ep{bias, mask, nullptr, nullptr, c, c_tp, nullptr, ldc, ldm, relu, rup(N, 32) / 32, 1.f,
           c && (size_t)(M + 16) * ldc * 4 < ((size_t)1 << 31), 0, 1.f};
    return dispatch_nt<P_X3, ASrcTP>(a_tp, 0, 1.f, b_tp, M, N, K, ep, (hipStream_t)stream);
}

static int gemm_nt_f32a(int prec, const float* a, int lda, float ascale, const uint16_t* b_tp, int M, int N, int K,
                        const float* bias, int relu, const float* mask, int ldm, const uint32_t* mbits_in,
                        uint32_t* mbits_out, float* colsum, float cscale, float* c, int ldc, uint16_t* c_tp,
                        void* stream, int flags = 0, float oscale = 1.f) {
    int e = check_common(b_tp, M, N, K, mask, ldm, c, ldc, c_tp);
    if (e) return e;
    if (prec != MM_PREC_X3 && prec != MM_PREC_F16 && prec != MM_PREC_X2) return MM_E_ARG;
    // x2 planes (P_X2): a / c addressed exactly as the fp32 matrices (lda / ldc in 4-byte units)
    const bool ap = flags & MM_GEMM_A_X2P, cp = flags & MM_GEMM_C_X2P;
    const bool a16 = flags & MM_GEMM_A_F16, c16 = flags & MM_GEMM_C_F16;
    if (flags & ~(MM_GEMM_A_F16 | MM_GEMM_C_F16 | MM_GEMM_A_X2P | MM_GEMM_C_X2P)) return MM_E_ARG;
    if (ap || cp) {
        if (prec != MM_PREC_X2 || mask || c_tp || a16 || c16) return MM_E_ARG;
        if (!a || (K & 3) || (lda & 3) || lda < K || ((uintptr_t)a & 15)) return MM_E_ARG;  // 16-byte rows
        // plane A: at scale 1; without ReLU bits (the input gradient into an fp32-stored layer input) on the
        // B-resident kernel only, in one row chunk (see below)
        const bool plain_a = ap && !mbits_in && !mbits_out;
        if (ap && ascale != 1.f) return MM_E_ARG;
        if (cp && ((!mbits_out && !mbits_in) || (N & 3) || (ldc & 3) || ((uintptr_t)c & 15))) return MM_E_ARG;
        if ((mbits_in || mbits_out) && (N > 16 * 17 || (mbits_in && mbits_out))) return MM_E_ARG;
        if (mbits_in && (bias || relu)) return MM_E_ARG;
        if (colsum && (!mbits_in || !c)) return MM_E_ARG;
        if (M == 0) return plain_a ? MM_E_ARG : 0;
        const size_t wmaxp = std::max(std::max((size_t)lda, (size_t)ldc), (size_t)N);
        const size_t capp = ((((size_t)1 << 31) - 1) / (4 * wmaxp) - 32) / kRowPad * kRowPad;
        if ((size_t)M > capp) {  // row chunks, as below
            if (capp < (size_t)kRowPad || plain_a) return MM_E_ARG;
            for (size_t m0 = 0; m0 < (size_t)M; m0 += capp) {
                const int mr = (int)std::min(capp, (size_t)M - m0);
                const size_t rt0 = m0 / 16;
                const int rc = gemm_nt_f32a(prec, a + m0 * lda, lda, ascale, b_tp, mr, N, K, bias, relu, nullptr, 0,
                                            mbits_in ? mbits_in + rt0 * 64 * kMaskWords : nullptr,
                                            mbits_out ? mbits_out + rt0 * 64 * kMaskWords : nullptr,
                                            colsum ? colsum + rt0 * N : nullptr, cscale, c + m0 * ldc, ldc, nullptr,
                                            stream, flags, oscale);
                if (rc) return rc;
            }
            return 0;
        }
        Epi epp{bias, nullptr, mbits_in, mbits_out, c, nullptr, colsum, ldc, 0, relu, rup(N, 32) / 32, cscale, 1,
                cp ? 1 : 0, oscale};
        hipStream_t sp = (hipStream_t)stream;
        BresPlan plp;
        int cfgp = C_PAIR;
        // the kernel choice of the fp32-storage call below (same plan, same row chunks)
        const bool bres = bres_enabled() && bres_plan(prec, M, N, K, lda, ldc, mbits_in || mbits_out, plp, cfgp);
        if (plain_a && !bres) return MM_E_ARG;  // (the streaming kernel takes a plane A through ReLU bits only)
        if (ap)
            return bres ? dispatch_bres<P_X2, 32>(a, lda, 1.f, b_tp, M, N, K, plp, cfgp, epp, sp)
                        : dispatch_nt<P_X2, ASrcX2PV>(a, lda, 1.f, b_tp, M, N, K, epp, sp);
        return bres ? dispatch_bres<P_X2, 4>(a, lda, ascale, b_tp, M, N, K, plp, cfgp, epp, sp)
                    : dispatch_nt<P_X2, ASrcF32>(a, lda, ascale, b_tp, M, N, K, epp, sp);
    }
    // fp16 activations (P_F16 only): A fp16 at scale 1 on the B-resident kernel; C fp16 for the forward with bits
    if ((a16 || c16) && (prec != MM_PREC_F16 || mask || c_tp)) return MM_E_ARG;
    if (a16 && (ascale != 1.f || (K & 3) || (lda & 3) || ((uintptr_t)a & 7))) return MM_E_ARG;
    if (c16 && ((!mbits_out && !mbits_in) || ((uintptr_t)c & 1))) return MM_E_ARG;
    if (prec == MM_PREC_X3 && (ascale != 1.f || cscale != 1.f)) return MM_E_ARG;  // the split is exact: no scaling
    const bool v4 = !a16 && !(K & 3) && !(lda & 3) && !((uintptr_t)a & 15);
    const bool v2 = !a16 && !(K & 1) && !(lda & 1) && !((uintptr_t)a & 7);
    if (!a || lda < K || !(v4 || v2 || a16) || (!v4 && !a16 && N > 64)) return MM_E_ARG;  // 8-byte rows: narrow outputs only
    if ((mbits_in || mbits_out) && (N > 16 * 17 || c_tp || mask || (mbits_in && mbits_out))) return MM_E_ARG;
    if (mbits_in && (bias || relu)) return MM_E_ARG;  // the input-gradient form: no bias, no ReLU of its own
    if (colsum && (!mbits_in || !c)) return MM_E_ARG;
    if (M == 0) return 0;
    // the kernels address A and C through buffer resources (num_records < 2^31 bytes): larger calls run
    // in row chunks of a multiple of 256 rows (whole row tiles of the bit masks and column sums)
    const size_t wmax = std::max(std::max((size_t)lda, (size_t)ldc), std::max((size_t)ldm, (size_t)N));
    const size_t cap = ((((size_t)1 << 31) - 1) / (4 * wmax) - 32) / kRowPad * kRowPad;
    if ((size_t)M > cap) {
        if (cap < (size_t)kRowPad || c_tp) return MM_E_ARG;
        for (size_t m0 = 0; m0 < (size_t)M; m0 += cap) {
            const int mr = (int)std::min(cap, (size_t)M - m0);
            const size_t rt0 = m0 / 16;
            const float* am = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a) + m0 * lda * (a16 ? 2 : 4));
            float* cm = reinterpret_cast<float*>(reinterpret_cast<char*>(c) + m0 * ldc * (c16 ? 2 : 4));
            const int rc = gemm_nt_f32a(prec, am, lda, ascale, b_tp, mr, N, K, bias, relu,
                                        mask ? mask + m0 * ldm : nullptr, ldm,
                                        mbits_in ? mbits_in + rt0 * 64 * kMaskWords : nullptr,
                                        mbits_out ? mbits_out + rt0 * 64 * kMaskWords : nullptr,
                                        colsum ? colsum + rt0 * N : nullptr, cscale, cm, ldc, nullptr, stream, flags,
                                        oscale);
            if (rc) return rc;
        }
        return 0;
    }
    Epi ep{bias, mask, mbits_in, mbits_out, c, c_tp, colsum, ldc, ldm, relu, rup(N, 32) / 32, cscale, c != nullptr,
           c16 ? 1 : 0, oscale};
    hipStream_t s = (hipStream_t)stream;
    BresPlan pl;
    int cfg = C_NARROW;
    if (a16 || (c16 && mbits_in)) {  // fp16 A, or fp16 input gradients: the B-resident kernel, or for fp16 A
                                      // where it does not fit (K = 460) the streaming kernel with ASrcF16V
        if (!bres_plan(prec, M, N, K, lda, ldc, mbits_in || mbits_out, pl, cfg)) {
            if (a16 && !(c16 && mbits_in))
                return dispatch_nt<P_F16, ASrcF16V>(reinterpret_cast<const unsigned short*>(a), lda, 1.f, b_tp, M, N,
                                                    K, ep, s);
            return MM_E_ARG;
        }
        return a16 ? dispatch_bres<P_F16, 16>(a, lda, 1.f, b_tp, M, N, K, pl, cfg, ep, s)
                   : (v4 ? dispatch_bres<P_F16, 4>(a, lda, ascale, b_tp, M, N, K, pl, cfg, ep, s)
                         : dispatch_bres<P_F16, 2>(a, lda, ascale, b_tp, M, N, K, pl, cfg, ep, s));
    }
    if (!mask && !c_tp && bres_enabled() && bres_plan(prec, M, N, K, lda, ldc, mbits_in || mbits_out, pl, cfg)) {
        if (prec == MM_PREC_X3)
            return v4 ? dispatch_bres<P_X3, 4>(a, lda, 1.f, b_tp, M, N, K, pl, cfg, ep, s)
                      : dispatch_bres<P_X3, 2>(a, lda, 1.f, b_tp, M, N, K, pl, cfg, ep, s);
        if (prec == MM_PREC_X2)
            return v4 ? dispatch_bres<P_X2, 4>(a, lda, ascale, b_tp, M, N, K, pl, cfg, ep, s)
                      : dispatch_bres<P_X2, 2>(a, lda, ascale, b_tp, M, N, K, pl, cfg, ep, s);
        return v4 ? dispatch_bres<P_F16, 4>(a, lda, ascale, b_tp, M, N, K, pl, cfg, ep, s)
                  : dispatch_bres<P_F16, 2>(a, lda, ascale, b_tp, M, N, K, pl, cfg, ep, s);
    }
    if (prec == MM_PREC_X3)
        return v4 ? dispatch_nt<P_X3, ASrcF32>(a, lda, 1.f, b_tp, M, N, K, ep, s)
                  : dispatch_nt_u<P_X3>(a, lda, 1.f, b_tp, M, N, K, ep, s);
    if (prec == MM_PREC_X2)
        return v4 ? dispatch_nt<P_X2, ASrcF32>(a, lda, ascale, b_tp, M, N, K, ep, s)
                  : dispatch_nt_u<P_X2>(a, lda, ascale, b_tp, M, N, K, ep, s);
    return v4 ? dispatch_nt<P_F16, ASrcF32>(a, lda, ascale, b_tp, M, N, K, ep, s)
              : dispatch_nt_u<P_F16>(a, lda, ascale, b_tp, M, N, K, ep, s);
}

// The same with A fp32 row-major [M, lda] (K % 4 == 0, lda % 4 == 0, 16-byte
// aligned), split into bf16 planes in registers inside the GEMM.
extern "C" int mm_x3_nt_f32a(const float* a, int lda, const uint16_t* b_tp, int M, int N, int K, const float* bias,
                             int relu, const float* mask, int ldm, const uint32_t* mbits_in, uint32_t* mbits_out,
                             float* colsum, float* c, int ldc, uint16_t* c_tp, void* stream) {
    if (!a || (K & 3) || (lda & 3) || ((uintptr_t)a & 15)) return MM_E_ARG;
    return gemm_nt_f32a(MM_PREC_X3, a, lda, 1.f, b_tp, M, N, K, bias, relu, mask, ldm, mbits_in, mbits_out, colsum,
                        1.f, c, ldc, c_tp, stream);
}

extern "C" int mm_gemm_nt(int prec, const float* a, int lda, float ascale, const uint16_t* b_tp, int M, int N, int K,
                          const float* bias, int relu, const uint32_t* mbits_in, uint32_t* mbits_out, float* colsum,
                          float cscale, float* c, int ldc, void* stream) {
    if (!c) return MM_E_ARG;
    return gemm_nt_f32a(prec, a, lda, ascale, b_tp, M, N, K, bias, relu, nullptr, 0, mbits_in, mbits_out, colsum,
                        cscale, c, ldc, nullptr, stream);
}

extern "C" int mm_gemm_nt_h(int prec, int flags, const void* a, int lda, float ascale, const uint16_t* b_tp, int M,
                            int N, int K, const float* bias, int relu, const uint32_t* mbits_in, uint32_t* mbits_out,
                            float* colsum, float cscale, float oscale, void* c, int ldc, void* stream) {
    if (!c) return MM_E_ARG;
    return gemm_nt_f32a(prec, static_cast<const float*>(a), lda, ascale, b_tp, M, N, K, bias, relu, nullptr, 0,
                        mbits_in, mbits_out, colsum, cscale, static_cast<float*>(c), ldc, nullptr, stream, flags,
                        oscale);
}

// ---- the fused small-M trunk (k_trunk3) ----
// row tiles per workgroup: 2 (MARLMAZE_TRUNK_RT=3: 3 where the LDS holds them -- fewer workgroups
// re-reading the weights from L2, but each one's k-loops 1.27x longer: 25.3 vs 22.3 us at 8,192 rows, x2).  Weight fragments D
// k-steps ahead: 1 for x2 / x3, 3 for f16 (its k-steps are 3x shorter); MARLMAZE_TRUNK_D=1 or 3 forces one.
static int trunk_env(const char* name) {
    const char* e = getenv(name);
    return e ? atoi(e) : 0;
}

// LDS: the biases, the f16 kernels' epilogue slices, then two activation buffers of TP blocks (uint16):
// bufX = h0 / layer 1's output, bufH = layer 0's output
static void trunk_bufs(int prec, int RT, int K0, int N0, int N1, int& bx, size_t& lds) {
    const int np = prec == MM_PREC_X3 ? 3 : prec == MM_PREC_X2 ? 2 : 1;
    const int nx = std::max(rup(K0, 32), rup(N1, 32)) / 32, nh = rup(N0, 32) / 32;
    bx = RT * nx * np * 512;
    lds = (size_t)(9 * kTrMaxN + (np == 1 ? kTrWaves * kTrSlice : 0)) * 4 + (size_t)RT * (nx + nh) * np * 1024;
}

// the fused heads' h3 rows (16 RT rows of N2 + 4 floats): in bufH when it holds them (free during the last
// layer), else in a region appended to the LDS; hoff in floats from the LDS base
static void trunk_h3(int prec, int RT, int K0, int N0, int N1, int N2, int& hoff, size_t& lds) {
    const int np = prec == MM_PREC_X3 ? 3 : prec == MM_PREC_X2 ? 2 : 1;
    int bx;
    trunk_bufs(prec, RT, K0, N0, N1, bx, lds);
    const size_t need = (size_t)16 * RT * (N2 + 4) * 4, hbytes = (size_t)RT * (rup(N0, 32) / 32) * np * 1024;
    const size_t bufx = (size_t)(9 * kTrMaxN + (np == 1 ? kTrWaves * kTrSlice : 0)) * 4;
    if (need <= hbytes) {
        hoff = (int)((bufx + (size_t)bx * 2) / 4);
    } else {
        hoff = (int)(lds / 4);
        lds += need;
    }
}

static int trunk_pick_rt(int prec, int K0, int N0, int N1) {
    int bx;
    size_t lds;
    if (trunk_env("MARLMAZE_TRUNK_RT") == 3) {
        trunk_bufs(prec, 3, K0, N0, N1, bx, lds);
        if (lds <= 160 * 1024) return 3;
    }
    trunk_bufs(prec, 2, K0, N0, N1, bx, lds);
    return lds <= 160 * 1024 ? 2 : 0;
}

extern "C" int mm_trunk3_ok(int prec, int M, int K0, int N0, int N1, int N2, int lda) {
    if (prec != MM_PREC_X3 && prec != MM_PREC_F16 && prec != MM_PREC_X2) return 0;
    if (M < 0 || K0 <= 0 || (K0 & 3) || (lda & 3) || lda < K0 || rup(K0, 32) > kTrMaxK0) return 0;
    if (N0 <= 0 || N1 <= 0 || N2 <= 0 || N0 > kTrMaxN || N1 > kTrMaxN || N2 > kTrMaxN) return 0;
    return trunk_pick_rt(prec, K0, N0, N1) ? 1 : 0;
}

template <int P, int RT, int D, bool HS = false>
static int launch_trunk(const TrunkArgs& ta, size_t lds, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)k_trunk3<P, RT, D, HS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024) != hipSuccess)
            return MM_E_ARG;
        attr = true;
    }
    hipLaunchKernelGGL((k_trunk3<P, RT, D, HS>), dim3((ta.M + 16 * RT - 1) / (16 * RT)), dim3(64 * kTrWaves), lds, s,
                       ta);
    return (int)hipGetLastError();
}

template <int P>
static int launch_trunk_p(TrunkArgs& ta, int RT, hipStream_t s) {
    const int de = trunk_env("MARLMAZE_TRUNK_D");
    const int d = de == 1 || de == 3 ? de : P == P_F16 ? 3 : 1;
    size_t lds;
    trunk_bufs(P, RT, ta.K0, ta.N[0], ta.N[1], ta.bx, lds);
    if (RT == 3) return d == 3 ? launch_trunk<P, 3, 3>(ta, lds, s) : launch_trunk<P, 3, 1>(ta, lds, s);
    return d == 3 ? launch_trunk<P, 2, 3>(ta, lds, s) : launch_trunk<P, 2, 1>(ta, lds, s);
}

extern "C" int mm_trunk3(int prec, const float* h0, int lda, int M, int K0, const uint16_t* w0, const float* b0,
                         int N0, const uint16_t* w1, const float* b1, int N1, const uint16_t* w2, const float* b2,
                         int N2, float* out, int ldc, void* stream) {
    if (!mm_trunk3_ok(prec, M, K0, N0, N1, N2, lda) || !h0 || !out || !w0 || !w1 || !w2 || ldc < N2) return MM_E_ARG;
    if (((uintptr_t)h0 & 15) || (((uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2) & 15) || ((uintptr_t)out & 3))
        return MM_E_ARG;
    if (M == 0) return 0;
    TrunkArgs ta{h0, {w0, w1, w2}, {b0, b1, b2}, out, lda, ldc, M, K0, {N0, N1, N2}, 0,
                 nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    const int RT = trunk_pick_rt(prec, K0, N0, N1);
    hipStream_t s = (hipStream_t)stream;
    if (prec == MM_PREC_X2) return launch_trunk_p<P_X2>(ta, RT, s);
    if (prec == MM_PREC_F16) return launch_trunk_p<P_F16>(ta, RT, s);
    return launch_trunk_p<P_X3>(ta, RT, s);
}

// the trunk + the actor heads + PPO.get_action in one launch (two row tiles a workgroup; D as mm_trunk3)
extern "C" int mm_trunk3_head_sample_ok(int prec, int M, int K0, int N0, int N1, int N2, int lda) {
    if (!mm_trunk3_ok(prec, M, K0, N0, N1, N2, lda) || (N2 & 3)) return 0;
    int hoff;
    size_t lds;
    trunk_h3(prec, 2, K0, N0, N1, N2, hoff, lds);
    return lds <= 160 * 1024 ? 1 : 0;
}

extern "C" int mm_trunk3_head_sample(int prec, const float* h0, int lda, int M, int K0, const uint16_t* w0,
                                     const float* b0, int N0, const uint16_t* w1, const float* b1, int N1,
                                     const uint16_t* w2, const float* b2, int N2, const float* head_w,
                                     const float* head_b, const uint8_t* masks, uint64_t seed, uint64_t offset,
                                     const uint64_t* offset_dev, int8_t* actions, float* logp, float* joint_logp,
                                     float* logits, float* h3, int ldh3, void* stream) {
    if (!mm_trunk3_head_sample_ok(prec, M, K0, N0, N1, N2, lda) || !h0 || !w0 || !w1 || !w2 || !head_w || !head_b ||
        !masks || !actions || (h3 && (ldh3 < N2 || ((uintptr_t)h3 & 3))))
        return MM_E_ARG;
    if (((uintptr_t)h0 & 15) || (((uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2) & 15)) return MM_E_ARG;
    if (M == 0) return 0;
    TrunkArgs ta{h0, {w0, w1, w2}, {b0, b1, b2}, h3, lda, ldh3, M, K0, {N0, N1, N2}, 0,
                 head_w, head_b, masks, seed, offset, offset_dev, actions, logp, joint_logp, logits, 0};
    size_t lds;
    trunk_bufs(prec, 2, K0, N0, N1, ta.bx, lds);
    trunk_h3(prec, 2, K0, N0, N1, N2, ta.hoff, lds);
    hipStream_t s = (hipStream_t)stream;
    if (prec == MM_PREC_X2) return launch_trunk<P_X2, 2, 1, true>(ta, lds, s);
    if (prec == MM_PREC_F16) return launch_trunk<P_F16, 2, 3, true>(ta, lds, s);
    return launch_trunk<P_X3, 2, 1, true>(ta, lds, s);
}

// dY = (dz W) * bits (the heads' backward through the last ReLU, bits from the
// last forward GEMM's mbits_out, N <= 272, J <= 8), and the per-16-row-tile
// column sums colsum [ceil(M / 16), N].
// the same with dY as x2 planes of dY * oscale (P_X2's pre-scaled input gradients, [M][N / 4][2][4] fp16)
extern "C" int mm_x3_heads_bwd_x2p(const float* dz, int J, const float* W, const uint32_t* bits, int M, int N,
                                   void* dy, float* colsum, float oscale, void* stream) {
    if (!dz || !W || !bits || !dy || !colsum || J <= 0 || J > kHeadsMaxJ || N <= 0 || N > 272 || (N & 3) || M < 0)
        return MM_E_ARG;
    if (M == 0) return 0;
    const int nrt = (M + 15) / 16;
    hipLaunchKernelGGL((k_heads_bwd<17, 2>), dim3((nrt + 3) / 4), dim3(256), 0, (hipStream_t)stream, dz, J, W, bits,
                       M, N, static_cast<float*>(dy), colsum, oscale);
    return (int)hipGetLastError();
}

// the same with dY fp16 = fp16(dY * oscale) (P_F16's pre-scaled input gradients)
extern "C" int mm_x3_heads_bwd_h16(const float* dz, int J, const float* W, const uint32_t* bits, int M, int N,
                                   void* dy, float* colsum, float oscale, void* stream) {
    if (!dz || !W || !bits || !dy || !colsum || J <= 0 || J > kHeadsMaxJ || N <= 0 || N > 272 || M < 0)
        return MM_E_ARG;
    if (M == 0) return 0;
    const int nrt = (M + 15) / 16;
    hipLaunchKernelGGL((k_heads_bwd<17, 1>), dim3((nrt + 3) / 4), dim3(256), 0, (hipStream_t)stream, dz, J, W, bits,
                       M, N, static_cast<float*>(dy), colsum, oscale);
    return (int)hipGetLastError();
}

extern "C" int mm_x3_heads_bwd(const float* dz, int J, const float* W, const uint32_t* bits, int M, int N, float* dy,
                               float* colsum, void* stream) {
    if (!dz || !W || !bits || !dy || !colsum || J <= 0 || J > kHeadsMaxJ || N <= 0 || N > 272 || M < 0)
        return MM_E_ARG;
    if (M == 0) return 0;
    const int nrt = (M + 15) / 16;
    hipLaunchKernelGGL(k_heads_bwd<17>, dim3((nrt + 3) / 4), dim3(256), 0, (hipStream_t)stream, dz, J, W, bits, M, N,
                       dy, colsum);
    return (int)hipGetLastError();
}

// ---- weight gradient ----
struct WgPlan {
    int TN, NTK, ncb, nslices, rows, TPW, tpw;  // TPW: the instantiation (>= tpw, the balanced run length)
};

static WgPlan wg_plan(int prec, int M, int N, int K) {
    WgPlan p;
    p.TN = (N + 15) / 16;
    const int tk_all = (K + 15) / 16;
    // column blocks: at most 20 tiles per wave (the register budget of 2 waves per SIMD) and two image sets
    // within 160 KiB of LDS; a slice's blocks share its dY rows through the XCD's L2
    p.ncb = (tk_all + kWgMaxT - 1) / kWgMaxT;
    const int kb = prec == MM_PREC_X3 ? 1536 : prec == MM_PREC_X2 ? 1024 : 512;
    auto fits = [&](int ncb) {
        const int ntk = (tk_all + ncb - 1) / ncb;
        return p.TN * ntk <= kWgWaves * 20 && 2 * (p.TN + ntk) * kb * 2 <= 160 * 1024;
    };
    while (!fits(p.ncb)) p.ncb++;
    p.NTK = (tk_all + p.ncb - 1) / p.ncb;
    p.tpw = (p.TN * p.NTK + kWgWaves - 1) / kWgWaves;
    static const int kTPW[] = {1, 2, 3, 5, 8, 12, 16, 20};
    p.TPW = 0;
    for (int t : kTPW)
        if (t >= p.tpw) {
            p.TPW = t;
            break;
        }
    // about one unit per CU: slices of whole 32-row steps (a floor of 512 rows per slice, to shrink the slices'
    // partials at BASELINE configs[1]'s 52,428-row minibatch, measured slower: 24.6 vs 23.5 ms per update)
    const int want = std::max(1, std::min((M + 31) / 32, persistent_grid() / p.ncb));
    p.rows = rup((M + want - 1) / want, 32);
    p.nslices = std::max(1, (M + p.rows - 1) / p.rows);
    return p;
}

__global__ void k_range_flag(uint32_t* out, int clear) {
    if (threadIdx.x == 0) {  // vector atomics on the flag (no scalar-cache writes)
        const uint32_t v = clear ? __hip_atomic_exchange(&g_range_flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                 : __hip_atomic_load(&g_range_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (out) out[0] = v;
    }
}

extern "C" int mm_gemm_range_flag(uint32_t* out, int clear, void* stream) {
    hipLaunchKernelGGL(k_range_flag, dim3(1), dim3(64), 0, (hipStream_t)stream, out, clear);
    return (int)hipGetLastError();
}

extern "C" long mm_gemm_wgrad_ws_len(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    long n = 0;  // the larger of the two precisions' plans
    for (int prec : {MM_PREC_X3, MM_PREC_F16, MM_PREC_X2}) {
        const WgPlan p = wg_plan(prec, M, N, K);
        n = std::max(n, (long)p.nslices * N * K);
    }
    return n;
}

template <int P>
static int launch_wgrad(const WgPlan& p, const float* dy, int lddy, float dscale, const float* x, int ldx, int M,
                        int N, int K, float cscale, float* ws, hipStream_t s) {
    const dim3 grid(rup(p.nslices, 8) * p.ncb), block(kWgThreads);
    const size_t lds = (size_t)2 * (p.TN + p.NTK) * Prec<P>::kBlk * sizeof(uint16_t);
#define MM_WG(T)                                                                                               \
    case T:                                                                                                    \
        {                                                                                                      \
            static bool attr = false;                                                                          \
            if (!attr) {                                                                                       \
                if (hipFuncSetAttribute((const void*)k_wgrad<P, T>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        160 * 1024) != hipSuccess)                                             \
                    return MM_E_ARG;                                                                           \
                attr = true;                                                                                   \
            }                                                                                                  \
        }                                                                                                      \
        hipLaunchKernelGGL((k_wgrad<P, T>), grid, block, lds, s, dy, lddy, dscale, x, ldx, M, N, K, p.TN, p.NTK, \
                           p.tpw, p.rows, p.nslices, p.ncb, cscale, ws);                                       \
        break;
    switch (p.TPW) {
        MM_WG(1) MM_WG(2) MM_WG(3) MM_WG(5) MM_WG(8) MM_WG(12) MM_WG(16) MM_WG(20)
        default: return MM_E_ARG;
    }
#undef MM_WG
    return (int)hipGetLastError();
}

// the structured kernel for the (TN, NTK) blocks the actor and critic produce; 1 = no instantiation
template <int P, int TN, int NTK, int XB = 4, int AB = 4>
static int launch_rect_t(const WgPlan& p, const float* dy, int lddy, float dscale, const float* x, int ldx, int M,
                         int N, int K, float cscale, float* ws, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)k_wgrad_rect<P, TN, NTK, XB, AB>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return MM_E_ARG;
        attr = true;
    }
    const size_t lds = (size_t)2 * (TN + NTK) * Prec<P>::kBlk * sizeof(uint16_t);
    hipLaunchKernelGGL((k_wgrad_rect<P, TN, NTK, XB, AB>), dim3(rup(p.nslices, 8) * p.ncb), dim3(kWgThreads), lds, s,
                       dy, lddy, dscale, x, ldx, M, N, K, p.rows, p.nslices, p.ncb, cscale, ws);
    return (int)hipGetLastError();
}

// the DMA-staged x2 kernel (k_wgrad_dma) for the actor trunk's two large shapes; MARLMAZE_WG_DMA=0 keeps
// k_wgrad_rect (A/B)
static int g_wgrad_algo = -1;
static bool wg_dma_enabled() {
    if (g_wgrad_algo < 0) {
        const char* e = getenv("MARLMAZE_WG_DMA");
        g_wgrad_algo = (e && e[0] == '0') ? MM_WGRAD_REG : MM_WGRAD_DMA;
    }
    return g_wgrad_algo == MM_WGRAD_DMA;
}

extern "C" int mm_gemm_wgrad_algo(int algo) {
    wg_dma_enabled();
    const int prev = g_wgrad_algo;
    if (algo == MM_WGRAD_DMA || algo == MM_WGRAD_REG) g_wgrad_algo = algo;
    return prev;
}

template <int TN, int NTK>
static int launch_dma_t(const WgPlan& p, const float* dy, int lddy, float dscale, const float* x, int ldx, int M,
                        int N, int K, float cscale, float* ws, hipStream_t s) {
    hipLaunchKernelGGL((k_wgrad_dma<P_X2, TN, NTK>), dim3(rup(p.nslices, 8) * p.ncb), dim3(kWgThreads), 0, s, dy,
                       lddy, dscale, x, ldx, M, N, K, p.rows, p.nslices, p.ncb, cscale, ws);
    return (int)hipGetLastError();
}

// the plane-operand kernel (k_wgrad_tr): dY and X as x2 planes, lddy / ldx their row pitches in 4-byte units
template <int TN, int NTK>
static int launch_tr_t(const WgPlan& p, const uint32_t* dy, int lddy, const uint32_t* x, int ldx, int M, int N, int K,
                       float cscale, float* ws, hipStream_t s) {
    hipLaunchKernelGGL((k_wgrad_tr<TN, NTK>), dim3(rup(p.nslices, 8) * p.ncb), dim3(kWgThreads), 0, s, dy, lddy, x,
                       ldx, M, N, K, p.rows, p.nslices, p.ncb, cscale, ws);
    return (int)hipGetLastError();
}

static bool wg_x2p_shape(const WgPlan& p) { return p.TN == 17 && p.NTK == 9; }  // the 264 x 264 layers' blocks

// the mixed kernel (k_wgrad_mix): dY as x2 planes (lddy its row pitch in 4-byte units), X fp32
template <int TN, int NTK>
static int launch_mix_t(const WgPlan& p, const uint32_t* dy, int lddy, const float* x, int ldx, int M, int N, int K,
                        float cscale, float* ws, hipStream_t s) {
    hipLaunchKernelGGL((k_wgrad_mix<TN, NTK>), dim3(rup(p.nslices, 8) * p.ncb), dim3(kWgThreads), 0, s, dy, lddy, x,
                       ldx, M, N, K, p.rows, p.nslices, p.ncb, cscale, ws);
    return (int)hipGetLastError();
}

static bool wg_mix_shape(const WgPlan& p) { return p.TN == 17 && p.NTK == 8; }  // the 264 x 460 layer's blocks

template <int P, int XB = 4, int AB = 4>
static int launch_rect_p(const WgPlan& p, const float* dy, int lddy, float dscale, const float* x, int ldx, int M,
                         int N, int K, float cscale, float* ws, hipStream_t s) {
    if constexpr (P == P_X2 && XB == 4 && AB == 4) {
        // 16-byte pieces: rows and bases 16-byte aligned (else the register-staged kernel)
        const bool al = (lddy % 4 == 0) && (ldx % 4 == 0) && ((reinterpret_cast<uintptr_t>(dy) & 15) == 0) &&
                        ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
        if (wg_dma_enabled() && al) {
            if (p.TN == 17 && p.NTK == 9) return launch_dma_t<17, 9>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
            if (p.TN == 17 && p.NTK == 8) return launch_dma_t<17, 8>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
        }
    }
#define MM_WR(a, b)                                                                                              \
    if (p.TN == a && p.NTK == b)                                                                                 \
        return launch_rect_t<P, a, b, XB, AB>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
    if constexpr (XB == 2 && P == P_X3) {  // fp16 X at x3: the actor heads' weight gradient over h3 only
        MM_WR(1, 17)
    } else {
        MM_WR(17, 9) MM_WR(17, 8) MM_WR(1, 17) MM_WR(4, 9) MM_WR(4, 4) MM_WR(1, 4)
    }
#undef MM_WR
    return (XB == 2 || AB == 2) ? MM_E_ARG : 1;  // fp16 operands: no generic-kernel fallback
}

static int launch_wgrad_rect(int prec, const WgPlan& p, const float* dy, int lddy, float dscale, const float* x,
                             int ldx, int M, int N, int K, float cscale, float* ws, hipStream_t s, bool x16 = false,
                             bool a16 = false) {
    if (x16 || a16) {  // fp16 operands (X: P_F16 / P_X3; dY: P_F16): the structured kernel only
        if ((size_t)M * lddy * 4 >= ((size_t)1 << 31) || (size_t)M * ldx * 4 >= ((size_t)1 << 31)) return MM_E_ARG;
        if ((x16 && (ldx & 1)) || (a16 && (lddy & 1))) return MM_E_ARG;  // fp16 rows: dword-aligned
        if (prec == MM_PREC_X3) return a16 ? MM_E_ARG : launch_rect_p<P_X3, 2>(p, dy, lddy, 1.f, x, ldx, M, N, K, 1.f, ws, s);
        if (prec != MM_PREC_F16) return MM_E_ARG;
        if (a16 && x16) return launch_rect_p<P_F16, 2, 2>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
        if (a16) return launch_rect_p<P_F16, 4, 2>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
        return launch_rect_p<P_F16, 2>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
    }
#ifdef WG_GENERIC  // diagnostic builds: the generic kernel for every shape
    return 1;
#endif
    if ((size_t)M * lddy * 4 >= ((size_t)1 << 31) || (size_t)M * ldx * 4 >= ((size_t)1 << 31))
        return 1;  // loads through buffer resources (num_records < 2^31): the generic kernel
    return prec == MM_PREC_X3   ? launch_rect_p<P_X3>(p, dy, lddy, 1.f, x, ldx, M, N, K, 1.f, ws, s)
           : prec == MM_PREC_X2 ? launch_rect_p<P_X2>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s)
                                : launch_rect_p<P_F16>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
}

static int gemm_wgrad(int prec, const float* dy, int lddy, float dscale, const float* x, int ldx, int M, int N, int K,
                      float cscale, float* ws, float* dw, void* stream, int flags = 0) {
    if (M < 0 || N <= 0 || K <= 0 || N > 16 * kWgMaxT || lddy < N || ldx < K) return MM_E_ARG;
    if (flags & ~(MM_GEMM_B_F16 | MM_GEMM_A_F16 | MM_GEMM_A_X2P | MM_GEMM_B_X2P)) return MM_E_ARG;
    const bool x16 = flags & MM_GEMM_B_F16, a16 = flags & MM_GEMM_A_F16;  // a16: dY fp16 (pre-scaled)
    // dY as x2 planes (pre-scaled: dscale 1) with X as planes too (k_wgrad_tr) or fp32 (A_X2P alone: k_wgrad_mix)
    if (flags & (MM_GEMM_A_X2P | MM_GEMM_B_X2P)) {
        const bool mix = flags == MM_GEMM_A_X2P;
        if ((!mix && flags != (MM_GEMM_A_X2P | MM_GEMM_B_X2P)) || prec != MM_PREC_X2 || dscale != 1.f)
            return MM_E_ARG;
        hipStream_t sp = (hipStream_t)stream;
        if (M == 0) return dw ? (int)hipMemsetAsync(dw, 0, sizeof(float) * (size_t)N * K, sp) : MM_E_ARG;
        if (!dy || !x || !ws || (N & 3) || (!mix && (K & 3)) || (lddy & 3) || (ldx & 3) ||
            (((uintptr_t)dy | (uintptr_t)x) & 15) || (size_t)M * lddy * 4 >= ((size_t)1 << 31) ||
            (size_t)M * ldx * 4 >= ((size_t)1 << 31))
            return MM_E_ARG;
        const WgPlan pp = wg_plan(prec, M, N, K);
        if (!(mix ? wg_mix_shape(pp) : wg_x2p_shape(pp))) return MM_E_ARG;
        const uint32_t* dyp = reinterpret_cast<const uint32_t*>(dy);
        const uint32_t* xp = reinterpret_cast<const uint32_t*>(x);
        const int ep = mix ? launch_mix_t<17, 8>(pp, dyp, lddy, x, ldx, M, N, K, cscale, ws, sp)
                           : launch_tr_t<17, 9>(pp, dyp, lddy, xp, ldx, M, N, K, cscale, ws, sp);
        if (ep || !dw) return ep;
        const long np = (long)N * K;
        hipLaunchKernelGGL(k_wg_reduce, dim3((unsigned)((np + 15) / 16)), dim3(256), 0, sp, ws, pp.nslices, np, dw);
        return (int)hipGetLastError();
    }
    if (prec != MM_PREC_X3 && prec != MM_PREC_F16 && prec != MM_PREC_X2) return MM_E_ARG;
    if (prec == MM_PREC_X3 && (dscale != 1.f || cscale != 1.f)) return MM_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) return dw ? (int)hipMemsetAsync(dw, 0, sizeof(float) * (size_t)N * K, s) : MM_E_ARG;
    if (!dy || !x || !ws) return MM_E_ARG;
    const WgPlan p = wg_plan(prec, M, N, K);
    if (!p.TPW) return MM_E_ARG;
    int e = launch_wgrad_rect(prec, p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s, x16, a16);
    if (e == 1 && !x16 && !a16)
        e = prec == MM_PREC_X3   ? launch_wgrad<P_X3>(p, dy, lddy, 1.f, x, ldx, M, N, K, 1.f, ws, s)
            : prec == MM_PREC_X2 ? launch_wgrad<P_X2>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s)
                                 : launch_wgrad<P_F16>(p, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, s);
    if (e) return e;
    const long n = (long)N * K;
    if (!dw) return 0;  // mm_gemm_wgrad_partials: the caller reduces (mm_wsum_multi)
    hipLaunchKernelGGL(k_wg_reduce, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, ws, p.nslices, n, dw);
    return (int)hipGetLastError();
}

extern "C" int mm_gemm_wgrad(int prec, const float* dy, int lddy, float dscale, const float* x, int ldx, int M, int N,
                             int K, float cscale, float* ws, float* dw, void* stream) {
    if (!dw) return MM_E_ARG;
    return gemm_wgrad(prec, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, dw, stream);
}

extern "C" int mm_gemm_wgrad_h(int prec, int flags, const float* dy, int lddy, float dscale, const void* x, int ldx,
                               int M, int N, int K, float cscale, float* ws, float* dw, void* stream) {
    if (!dw) return MM_E_ARG;
    return gemm_wgrad(prec, dy, lddy, dscale, static_cast<const float*>(x), ldx, M, N, K, cscale, ws, dw, stream,
                      flags);
}

extern "C" int mm_gemm_wgrad_partials_h(int prec, int flags, const float* dy, int lddy, float dscale, const void* x,
                                        int ldx, int M, int N, int K, float cscale, float* ws, void* stream) {
    if (M <= 0) return MM_E_ARG;
    return gemm_wgrad(prec, dy, lddy, dscale, static_cast<const float*>(x), ldx, M, N, K, cscale, ws, nullptr, stream,
                      flags);
}

extern "C" int mm_gemm_a16_ok(int M, int N, int K, int lda, int ldc) {
    BresPlan pl;
    int cfg = C_NARROW;
    return bres_enabled() && bres_plan(MM_PREC_F16, M, N, K, lda, ldc, true, pl, cfg) ? 1 : 0;
}

// whether the x2 trunk shape [M, K] -> [M, N] takes plane storage end to end: the weight gradient dW [N, K]
// has k_wgrad_tr's blocks and the plane rows fit the kernels' buffer resources (the GEMMs take planes at
// every shape of P_X2)
extern "C" int mm_gemm_x2p_ok(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0 || N > 16 * kWgMaxT || (N & 3) || (K & 3)) return 0;
    if ((size_t)(M + 16) * std::max(N, K) * 4 >= ((size_t)1 << 31)) return 0;
    return wg_x2p_shape(wg_plan(MM_PREC_X2, M, N, K)) ? 1 : 0;
}

// the x2 plane-A input gradient without ReLU bits ([M, N] planes -> fp32 [M, K]: the layer below stores its
// input fp32) runs on the B-resident kernel only, in one row chunk
static bool x2p_plain_a_ok(int M, int N, int K, int lda, int ldc) {
    if (M <= 0 || N <= 0 || K <= 0 || (N & 3) || (lda & 3) || lda < N || ldc < K) return false;
    const size_t wmax = std::max(std::max((size_t)lda, (size_t)ldc), (size_t)K);
    if ((size_t)M > ((((size_t)1 << 31) - 1) / (4 * wmax) - 32) / kRowPad * kRowPad) return false;
    BresPlan pl;
    int cfg = C_PAIR;
    return bres_enabled() && bres_plan(MM_PREC_X2, M, K, N, lda, ldc, false, pl, cfg);
}

// whether the input gradient dY [M, N] of the x2 layer [M, K] -> [M, N] can be stored as (pre-scaled) planes
// beside an fp32 layer input X [M, K]: the weight gradient dW [N, K] has k_wgrad_mix's blocks, and the plain
// plane-A input gradient dY W runs at M rows under the current GEMM algorithm
extern "C" int mm_gemm_x2p_dy_ok(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0 || N > 16 * kWgMaxT || (N & 3) || (K & 3)) return 0;
    if ((size_t)(M + 16) * std::max(N, K) * 4 >= ((size_t)1 << 31)) return 0;
    return wg_mix_shape(wg_plan(MM_PREC_X2, M, N, K)) && x2p_plain_a_ok(M, N, K, N, K) ? 1 : 0;
}

extern "C" int mm_gemm_wgrad_slices(int prec, int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0 || (prec != MM_PREC_X3 && prec != MM_PREC_F16 && prec != MM_PREC_X2))
        return MM_E_ARG;
    const WgPlan p = wg_plan(prec, M, N, K);
    return p.TPW ? p.nslices : MM_E_ARG;
}

extern "C" int mm_gemm_wgrad_partials(int prec, const float* dy, int lddy, float dscale, const float* x, int ldx, int M,
                                      int N, int K, float cscale, float* ws, void* stream) {
    if (M <= 0) return MM_E_ARG;
    return gemm_wgrad(prec, dy, lddy, dscale, x, ldx, M, N, K, cscale, ws, nullptr, stream);
}

// ---- the fused per-row part of the critic update (k_critic_update) ----
// The shapes k_critic_update serves: the reference critic's (K0 = 130 or 132, 8-byte rows) where every GEMM
// of the unfused x2 update runs on k_bres in one row chunk -- the kernel whose bits the fused launch gives.
extern "C" int mm_critic_update_ok(int M, int K0, int ldx) {
    if (M <= 0 || K0 <= 128 || K0 > 132 || (K0 & 1) || (ldx & 1) || ldx < K0) return 0;  // (130: two agents)
    const size_t wmax = std::max(ldx, 64);
    if ((size_t)(M + 320) * wmax * 4 >= ((size_t)1 << 31)) return 0;
    if (!bres_enabled()) return 0;
    BresPlan pl;
    int cfg = C_PAIR;
    return bres_plan(MM_PREC_X2, M, 64, K0, ldx, 64, true, pl, cfg) && bres_plan(MM_PREC_X2, M, 64, 64, 64, 64, true, pl, cfg) &&
                   bres_plan(MM_PREC_X2, M, 1, 64, 64, 1, false, pl, cfg)
               ? 1
               : 0;
}

extern "C" int mm_critic_update(const float* x, int ldx, int K0, int M, const float* rtg, const uint16_t* w0_tp,
                                const float* b0, const uint16_t* w1_tp, const uint16_t* w1t_tp, const float* b1,
                                const uint16_t* w2_tp, const float* w2, const float* b2, float* v, float* dv,
                                float* h0, float* h1, float* dy1, float* dy0, float* cs1, float* cs0,
                                void* stream) {
    if (!x || !rtg || !w0_tp || !b0 || !w1_tp || !w1t_tp || !b1 || !w2_tp || !w2 || !b2 || !v || !dv || !h0 ||
        !h1 || !dy1 || !dy0 || !cs1 || !cs0)
        return MM_E_ARG;
    if (((uintptr_t)x & 7) || (((uintptr_t)w0_tp | (uintptr_t)w1_tp | (uintptr_t)w1t_tp | (uintptr_t)w2_tp) & 15))
        return MM_E_ARG;
    if (mm_critic_update_ok(M, K0, ldx) != 1) return MM_E_ARG;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)k_critic_update, hipFuncAttributeMaxDynamicSharedMemorySize, kCuLds) !=
            hipSuccess)
            return MM_E_ARG;
        attr = true;
    }
    const int G = std::min(persistent_grid(), ((M + 15) / 16 + kCuWaves - 1) / kCuWaves);
    int e2 = 0;
    const float gscale = ldexpf(1.f, (frexpf((float)M, &e2), e2 - 1));  // 2^floor(log2 M)
    CuArgs ca{x, ldx, K0, M, rtg, w0_tp, w1_tp, w1t_tp, w2_tp, b0, b1, w2, b2, gscale, (float)(2.0 / (double)M),
              v, dv, h0, h1, dy1, dy0, cs1, cs0};
    hipLaunchKernelGGL(k_critic_update, dim3(G), dim3(64 * kCuWaves), kCuLds, (hipStream_t)stream, ca);
    return (int)hipGetLastError();
}
