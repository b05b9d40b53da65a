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
// actor/critic of BASELINE configs[4]; P_X2 two fp16 planes (hi, lo), three
// f16 MFMAs per product.  Storage stays fp32 unless a call says otherwise
// (fp16 rows, x2 planes); an A-operand scale (a power of two, exact) keeps
// small gradients out of the fp16 subnormal range and the epilogue multiplies
// by its inverse (cscale).  The TP layout of P_F16 / P_X2 is the same with one
// / two planes (1- / 2-KiB blocks).
//
// This translation unit, in include order (each kernel header is included once, inside namespace mm::x3):
//   gemm_parts.h             what the kernels share: conversions, MFMA sequences, epilogues, the A operand
//   (here)                   the TP pack kernels
//   gemm_stream.h            k_x3nt: B streamed through LDS by k-step
//   gemm_bres.h              k_bres: a column block of B resident in LDS
//   trunk_kernel.h           k_trunk3: the actor trunk's three layers (+ heads and sampler) for small M
//   critic_update_kernel.h   k_critic_update: the per-row part of the critic update
//   (here)                   k_heads_bwd
//   wgrad_kernels.h          the weight-gradient kernels
// and then all host code: the GEMM entry (gemm_nt_f32a: one validation, one row-chunk loop, one route to a
// kernel family and its template arguments), the B-resident plan, the trunk, heads, weight-gradient and
// critic-update launches, and the extern "C" entries of include/marlmaze.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "marlmaze.h"
#include "policy_device.h"

namespace mm {
namespace x3 {

#include "gemm_parts.h"

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

#include "gemm_stream.h"
#include "gemm_bres.h"
#include "trunk_kernel.h"
#include "critic_update_kernel.h"

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
    static unsigned long long zero[256 * 16 * kStampWaves * 8];
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

// ---- run-time (precision, A form, epilogue mode) -> template arguments, for both kernel families ----
// A forms (VW): gemm_parts.h's row-major forms 4, 2, 16, 32, and 0: pre-split TP planes (mm_x3_nt only)
template <int P, int VW>
struct PV {
    static constexpr int prec = P, vw = VW;
};
// the (precision, row-major A form) pairs that exist; f: a generic lambda taking a PV
template <class F>
static int with_pv(int prec, int vw, F&& f) {
    if (prec == MM_PREC_X3) return vw == 4 ? f(PV<P_X3, 4>{}) : vw == 2 ? f(PV<P_X3, 2>{}) : MM_E_ARG;
    if (prec == MM_PREC_X2)
        return vw == 4 ? f(PV<P_X2, 4>{}) : vw == 2 ? f(PV<P_X2, 2>{}) : vw == 32 ? f(PV<P_X2, 32>{}) : MM_E_ARG;
    if (prec == MM_PREC_F16)
        return vw == 4 ? f(PV<P_F16, 4>{}) : vw == 2 ? f(PV<P_F16, 2>{}) : vw == 16 ? f(PV<P_F16, 16>{}) : MM_E_ARG;
    return MM_E_ARG;
}

// The epilogue modes a family has for (P, VW) -- STREAM: k_x3nt, else k_bres -- which is also the set of its
// instantiations: TP outputs are bf16x3 on the streaming kernel; fp16 / plane outputs belong to P_F16 (the
// input-gradient form on k_bres only) and P_X2 (not from 8-byte rows); the streaming kernel takes a plane A
// through ReLU bits only.
template <int P, int VW, bool STREAM>
constexpr bool em_has(int em) {
    if (em == EM_TP) return STREAM && P == P_X3;
    if (em_16(em)) return P == P_F16 ? !(STREAM && em == EM_BWD16) : (P == P_X2 && VW != 2);
    if (em == EM_F32) return !(STREAM && VW == 32);
    return true;
}
// an Epi's epilogue mode in that family, or -1: refused.  (The last two rules were the streaming launch's alone:
// no call reaches k_bres with a TP output, or with an fp16 / plane output and a null c -- gemm_nt_f32a refuses
// both before it routes -- so for k_bres they never fire.)
template <int P, int VW, bool STREAM>
static int epi_mode(const Epi& ep) {
    const int em = ep.ctp      ? EM_TP
                   : ep.c16    ? (ep.mbits_out ? EM_FWD16 : ep.mbits_in ? EM_BWD16 : -1)
                   : ep.mbits_out ? EM_FWD
                   : ep.mbits_in  ? EM_BWD
                                  : EM_F32;
    if (em < 0 || !em_has<P, VW, STREAM>(em)) return -1;
    if (ep.ctp && ep.c) return -1;       // one output form per launch
    if (ep.c16 && !ep.bufok) return -1;  // fp16 / plane outputs: the buffer-store epilogue
    return em;
}
// f(integral_constant<EM>) for the family's mode em; MM_E_ARG for -1
template <int P, int VW, bool STREAM, int EM = 0, class F>
static int with_em(int em, F&& f) {
    if constexpr (EM > EM_BWD16) {
        return MM_E_ARG;
    } else {
        if constexpr (em_has<P, VW, STREAM>(EM))
            if (em == EM) return f(std::integral_constant<int, EM>{});
        return with_em<P, VW, STREAM, EM + 1>(em, f);
    }
}

// ---- k_x3nt dispatch ----
template <int VW>
struct StreamA;  // the streaming kernel's A source and element type of a form
template <>
struct StreamA<0> {
    typedef ASrcTP AS;
    typedef uint16_t AT;
};
template <>
struct StreamA<4> {
    typedef ASrcF32 AS;
    typedef float AT;
};
template <>
struct StreamA<2> {
    typedef ASrcF32U AS;
    typedef float AT;
};
template <>
struct StreamA<16> {
    typedef ASrcF16V AS;
    typedef unsigned short AT;
};
template <>
struct StreamA<32> {
    typedef ASrcX2PV AS;
    typedef float AT;
};

template <int NT, int P, int VW>
static int launch_nt(const void* a, int lda, float ascale, const uint16_t* b, int M, int N, int K, int ncb,
                     const Epi& ep, hipStream_t s) {
    using AS = typename StreamA<VW>::AS;
    using AT = typename StreamA<VW>::AT;
    constexpr int kT = SW<P>::kThreads;
    const int nks = rup(K, 32) / 32;
    const int nrb = rup(M, SW<P>::kBM) / SW<P>::kBM;
    const int grid = std::min(rup(nrb, 8) * ncb, persistent_grid() * (P == P_X2 ? 2 : 1));
    return with_em<P, VW, true>(epi_mode<P, VW, true>(ep), [&](auto em) {
        hipLaunchKernelGGL((k_x3nt<NT, P, AS, AT, decltype(em)::value>), dim3(grid), dim3(kT), 0, s,
                           static_cast<const AT*>(a), lda, ascale, b, M, N, K, nks, nrb, ncb, ep);
        return (int)hipGetLastError();
    });
}

template <int P, int VW>
static int dispatch_stream(const void* a, int lda, float ascale, const uint16_t* b_tp, int M, int N, int K,
                           const Epi& ep, hipStream_t s) {
    // column tiling: one block of <= 17 tiles, or several blocks of 15 (B rows are padded to 256)
    const int tiles = (N + 15) / 16;
    if (VW == 2 && tiles > 4) return MM_E_ARG;  // 8-byte rows serve only narrow outputs (the critic's first layer)
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
    if (NT == 1) return launch_nt<1, P, VW>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
    if (NT == 4) return launch_nt<4, P, VW>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
    if constexpr (VW != 2) {
        if (NT == 8) return launch_nt<8, P, VW>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
        if (NT == 17) return launch_nt<17, P, VW>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
        if constexpr (VW != 32)  // (plane A comes with bits: N <= 272, one block)
            return launch_nt<15, P, VW>(a, lda, ascale, b_tp, M, N, K, ncb, ep, s);
    }
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
    // 0.81x; x2, four 4-5-tile blocks: 568 vs 462 us at 419,430 rows)
    if (prec != MM_PREC_X3 && nblk > 1 && K > 288) return false;
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

template <int P, int VW>
static int dispatch_bres(const float* a, int lda, float ascale, const uint16_t* b, int M, int N, int K,
                         const BresPlan& pl, int cfg, const Epi& ep, hipStream_t s) {
    return with_em<P, VW, false>(epi_mode<P, VW, false>(ep), [&](auto em) {
        constexpr int EM = decltype(em)::value;
        if constexpr (P == P_X2) {
            return launch_bres<P, C_PAIR, EM, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
        } else {
            if constexpr (P == P_F16)
                if (cfg == C_WIDE) return launch_bres<P, C_WIDE, EM, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
            return launch_bres<P, C_NARROW, EM, VW>(a, lda, ascale, b, M, N, K, pl, ep, s);
        }
    });
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
    return dispatch_stream<P_X3, 0>(a_tp, 0, 1.f, b_tp, M, N, K, ep, (hipStream_t)stream);
}

// One row chunk of a row-major-A call (validated by gemm_nt_f32a; vw: the A form) -> its kernel: the B-resident
// kernel where the algorithm switch allows it and its plan fits, else the streaming one.  fp16 A and fp16 input
// gradients take the B-resident kernel whatever the switch says; fp16 input gradients and a plane A without
// ReLU bits exist there only.
static int gemm_route(int prec, int vw, const void* a, int lda, float ascale, const uint16_t* b_tp, int M, int N,
                      int K, const Epi& ep, hipStream_t s) {
    const bool bits = ep.mbits_in || ep.mbits_out;
    const bool h16_bwd = prec == MM_PREC_F16 && ep.c16 && ep.mbits_in, plain_planes = vw == 32 && !bits;
    BresPlan pl;
    int cfg = C_NARROW;
    const bool bres = (vw == 16 || h16_bwd || (!ep.mask && !ep.ctp && bres_enabled())) &&
                      bres_plan(prec, M, N, K, lda, ep.ldc, bits, pl, cfg);
    if (!bres && (h16_bwd || plain_planes)) return MM_E_ARG;
    return with_pv(prec, vw, [&](auto pv) {
        constexpr int P = decltype(pv)::prec, VW = decltype(pv)::vw;
        return bres ? dispatch_bres<P, VW>(static_cast<const float*>(a), lda, ascale, b_tp, M, N, K, pl, cfg, ep, s)
                    : dispatch_stream<P, VW>(a, lda, ascale, b_tp, M, N, K, ep, s);
    });
}

// C = A . B^T with a row-major A [M, lda]: fp32 (16- or 8-byte rows), fp16 rows (MM_GEMM_A_F16) or x2 planes
// (MM_GEMM_A_X2P); C fp32, fp16 (MM_GEMM_C_F16), x2 planes (MM_GEMM_C_X2P) or TP.  Planes are addressed exactly as
// the fp32 matrices (lda / ldc in 4-byte units).
static int gemm_nt_f32a(int prec, const float* a, int lda, float ascale, const uint16_t* b_tp, int M, int N, int K,
                        const float* bias, int relu, const float* mask, int ldm, const uint32_t* mbits_in,
                        uint32_t* mbits_out, float* colsum, float cscale, float* c, int ldc, uint16_t* c_tp,
                        void* stream, int flags = 0, float oscale = 1.f) {
    int e = check_common(b_tp, M, N, K, mask, ldm, c, ldc, c_tp);
    if (e) return e;
    if (prec != MM_PREC_X3 && prec != MM_PREC_F16 && prec != MM_PREC_X2) return MM_E_ARG;
    if (flags & ~(MM_GEMM_A_F16 | MM_GEMM_C_F16 | MM_GEMM_A_X2P | MM_GEMM_C_X2P)) return MM_E_ARG;
    const bool ap = flags & MM_GEMM_A_X2P, cp = flags & MM_GEMM_C_X2P;
    const bool a16 = flags & MM_GEMM_A_F16, c16 = flags & MM_GEMM_C_F16;
    const bool planes = ap || cp, halves = a16 || c16, bits = mbits_in || mbits_out;
    // the storage forms belong to one precision each, and go with neither the fp32 mask nor a TP output
    if ((planes && (prec != MM_PREC_X2 || halves)) || (halves && prec != MM_PREC_F16)) return MM_E_ARG;
    if ((planes || halves) && (mask || c_tp)) return MM_E_ARG;
    // scales: the x3 split is exact (no scaling); stored planes and fp16 rows are operands at scale 1
    if (prec == MM_PREC_X3 && (ascale != 1.f || cscale != 1.f)) return MM_E_ARG;
    if ((ap || a16) && ascale != 1.f) return MM_E_ARG;
    // A rows -> the operand form: 16-byte rows (fp32: 4, planes: 32; a call with plane C takes no others), fp16
    // rows of whole 8-byte pieces (16), or fp32 8-byte rows (2: narrow outputs only, the critic's first layer)
    if (!a || lda < K) return MM_E_ARG;
    const bool q4 = !(K & 3) && !(lda & 3), q2 = !(K & 1) && !(lda & 1);
    const int vw = a16                              ? (q4 && !((uintptr_t)a & 7) ? 16 : 0)
                   : q4 && !((uintptr_t)a & 15)     ? (ap ? 32 : 4)
                   : !planes && q2 && !((uintptr_t)a & 7) ? 2
                                                          : 0;
    if (!vw || (vw == 2 && N > 64)) return MM_E_ARG;
    // C forms: planes and fp16 come with ReLU bits (the hidden layers' forward and input gradient)
    if (cp && ((N & 3) || (ldc & 3) || ((uintptr_t)c & 15))) return MM_E_ARG;
    if (c16 && ((uintptr_t)c & 1)) return MM_E_ARG;
    if ((cp || c16) && !bits) return MM_E_ARG;
    if (bits && (N > 16 * 17 || c_tp || mask || (mbits_in && mbits_out))) return MM_E_ARG;
    if (mbits_in && (bias || relu)) return MM_E_ARG;  // the input-gradient form: no bias, no ReLU of its own
    if (colsum && (!mbits_in || !c)) return MM_E_ARG;
    // a plane A without ReLU bits (the input gradient into an fp32-stored layer input): the B-resident kernel
    // only, in one row chunk
    const bool plain_planes = ap && !bits;
    if (M == 0) return plain_planes ? MM_E_ARG : 0;
    // the kernels address A and C through buffer resources (num_records < 2^31 bytes): larger calls run
    // in row chunks of a multiple of 256 rows (whole row tiles of the bit masks and column sums)
    const size_t wmax = std::max(std::max((size_t)lda, (size_t)ldc), std::max((size_t)ldm, (size_t)N));
    const size_t cap = ((((size_t)1 << 31) - 1) / (4 * wmax) - 32) / kRowPad * kRowPad;
    const bool chunks = (size_t)M > cap;
    if (chunks && (cap < (size_t)kRowPad || c_tp || plain_planes)) return MM_E_ARG;
    const size_t step = chunks ? cap : (size_t)M, aesz = a16 ? 2 : 4, cesz = c16 ? 2 : 4;  // (planes: 4, a pair)
    for (size_t m0 = 0; m0 < (size_t)M; m0 += step) {
        const int mr = (int)std::min(step, (size_t)M - m0);
        const size_t rt0 = m0 / 16;
        Epi ep{bias,
               mask ? mask + m0 * ldm : nullptr,
               mbits_in ? mbits_in + rt0 * 64 * kMaskWords : nullptr,
               mbits_out ? mbits_out + rt0 * 64 * kMaskWords : nullptr,
               c ? reinterpret_cast<float*>(reinterpret_cast<char*>(c) + m0 * ldc * cesz) : nullptr,
               c_tp,
               colsum ? colsum + rt0 * N : nullptr,
               ldc, ldm, relu, rup(N, 32) / 32, cscale, c != nullptr, (cp || c16) ? 1 : 0, oscale};
        const int rc = gemm_route(prec, vw, reinterpret_cast<const char*>(a) + m0 * lda * aesz, lda, ascale, b_tp, mr,
                                  N, K, ep, (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
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
