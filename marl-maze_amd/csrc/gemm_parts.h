// ---------------------------------------------------------------------------
// What the GEMM kernels share (see x3mlp.hip's header for the arithmetic and the TP layout).  Included once by
// x3mlp.hip, inside namespace mm::x3, before every kernel header:
//   Prec, the range guard, the fp32 -> plane conversions (split2 / pair2 / pair1, cvt2, store_piece,
//   x2p_quad_word), the MFMA sequences (mma, x2_term, x2_mma_tiles, x2_combine), Epi and the epilogues
//   (EM_*, epilogue_f32, epilogue_tp, bres_epilogue), and the row-major A operand (a_load_half, a_frag,
//   a_frag16).
// Users: k_x3nt (gemm_stream.h), k_bres (gemm_bres.h), k_trunk3 (trunk_kernel.h), k_critic_update
// (critic_update_kernel.h), the weight-gradient kernels (wgrad_kernels.h) and the pack kernels and k_heads_bwd
// in x3mlp.hip.  k_critic_update and k_trunk3 give k_bres's / k_x3nt's bits BECAUSE they call these functions.
// ---------------------------------------------------------------------------
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

// two fp32 values -> one dword of each of the precision's planes (w[0 .. kPlanes - 1]): the exact three-way
// bf16 split (P_X3; the hardware conversions: ~4 VALU per value, not ~20), the (hi, lo) fp16 pairs of x s
// (P_X2), or x s rounded to fp16 (P_F16).  Every fp32 -> fragment conversion below goes through this one, but
// store_piece<P_F16>, which states the same f16x2_rn(x0 s, x1 s) itself (see there): for f16, store_piece and
// a_frag -- and with them k_trunk3's bits and k_x3nt's -- agree through these two equal expressions.
template <int P>
__device__ __forceinline__ void cvt2(float x0, float x1, float s, uint32_t (&w)[3]) {
    if constexpr (P == P_X3) split2(x0, x1, w[0], w[1], w[2]);
    else if constexpr (P == P_X2) pair2(x0, x1, s, w[0], w[1]);
    else w[0] = f16x2_rn(x0 * s, x1 * s);
}

// the 8 values of one fragment piece -> the P planes (16 bytes each) at dst, dst + 64, ... (uint4 units)
template <int P>
__device__ __forceinline__ void store_piece(const float* v, float s, uint4* dst) {
    if constexpr (P == P_F16) {  // (one expression: through w[][] eight k_wgrad_rect instantiations re-ordered)
        dst[0] = make_uint4(f16x2_rn(v[0] * s, v[1] * s), f16x2_rn(v[2] * s, v[3] * s), f16x2_rn(v[4] * s, v[5] * s),
                            f16x2_rn(v[6] * s, v[7] * s));
    } else {
        uint32_t w[4][3];
#pragma unroll
        for (int k = 0; k < 4; k++) cvt2<P>(v[2 * k], v[2 * k + 1], s, w[k]);
#pragma unroll
        for (int q = 0; q < Prec<P>::kPlanes; q++) dst[64 * q] = make_uint4(w[0][q], w[1][q], w[2][q], w[3][q]);
    }
}

// ---- MFMA ------------------------------------------------------------------
// One 16x16 MFMA on plane fragments: a 32-deep operand is a bf16x8 (16 bytes a lane), a 16-deep one (the final
// half k-step of the B-resident kernels) a uint2
__device__ __forceinline__ f32x4 mfma_f16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_f16(uint2 a, uint2 b, f32x4 c) {
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h4, a), __builtin_bit_cast(h4, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_bf16(uint2 a, uint2 b, f32x4 c) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4, a), __builtin_bit_cast(s4, b), c, 0, 0, 0);
}

// The x2 order, stated once: a product is three MFMAs -- term 0 lo hi and term 1 hi lo into accx, term 2 hi hi
// into acc (combined by x2_combine before the epilogue).  a, b: the (hi, lo) fragments.
template <int T, class V>
__device__ __forceinline__ void x2_term(const V* a, const V* b, f32x4& acc, f32x4& accx) {
    if constexpr (T == 2) acc = mfma_f16(a[0], b[0], acc);
    else accx = mfma_f16(a[1 - T], b[T], accx);
}

// one fragment product, the precision's MFMAs (P_X3: the six partial products, small terms first; P_X2: the
// x2 order, one tile's terms back to back), 32- or 16-deep by the operand type
template <int P, class V>
__device__ __forceinline__ f32x4 mma(const V* a, const V* b, f32x4 acc, f32x4& accx) {
    if constexpr (P == P_X2) {
        x2_term<0>(a, b, acc, accx);
        x2_term<1>(a, b, acc, accx);
        x2_term<2>(a, b, acc, accx);
    } else if constexpr (P == P_X3) {
        acc = mfma_bf16(a[2], b[0], acc);
        acc = mfma_bf16(a[0], b[2], acc);
        acc = mfma_bf16(a[1], b[1], acc);
        acc = mfma_bf16(a[1], b[0], acc);
        acc = mfma_bf16(a[0], b[1], acc);
        acc = mfma_bf16(a[0], b[0], acc);
    } else {
        acc = mfma_f16(a[0], b[0], acc);
    }
    (void)accx;
    return acc;
}

// NT column tiles' x2 products of one k-step, issued tile-interleaved (term by term over the tiles: each
// accumulator sees the x2 order, and a kernel with one wave per SIMD -- k_critic_update -- does not wait on
// back-to-back dependent MFMAs)
template <int NT, class V>
__device__ __forceinline__ void x2_mma_tiles(const V* a, const V (&b)[NT][2], f32x4 (&acc)[NT], f32x4 (&accx)[NT]) {
#pragma unroll
    for (int c = 0; c < NT; c++) x2_term<0>(a, b[c], acc[c], accx[c]);
#pragma unroll
    for (int c = 0; c < NT; c++) x2_term<1>(a, b[c], acc[c], accx[c]);
#pragma unroll
    for (int c = 0; c < NT; c++) x2_term<2>(a, b[c], acc[c], accx[c]);
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

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2v;
constexpr uint32_t kBufOOB = 0x80000000u;  // an offset past every buffer (num_records < 2^31)

// diagnostic builds only (tools/x3_stamps.sh): per-wave phase clocks of k_x3nt and k_bres (lane, wave: the
// kernels' locals)
constexpr int kStampWaves = 16;  // wave slots per workgroup (k_x3nt's 16 waves; k_bres uses 12)
#ifdef X3_STAMPS
__device__ unsigned long long g_x3_stamps[256 * 16 * kStampWaves * 8];
#define X3_STAMP(it, slot, val)                                                                       \
    do {                                                                                              \
        if (lane == 0 && blockIdx.x < 256 && (it) < 16)                                               \
            g_x3_stamps[((blockIdx.x * 16 + (it)) * kStampWaves + wave) * 8 + (slot)] = (val);        \
    } while (0)
#else
#define X3_STAMP(it, slot, val) \
    do {                        \
    } while (0)
#endif

// ---- the row-major A operand -------------------------------------------------
// A lane's share of one 32-wide k-step of its row (row 16 rt + (l & 15)): the 8 values at k = 32 ks + kq + {0 ..
// 3, 16 .. 19}, kq = 4 (l >> 4) -- kcol order -- as raw[0] (k ..) and raw[1] (k + 16 ..), then as the precision's
// fragment planes.  Written once per operand form VW, for the streaming kernel's sources (ASrcF32V: the
// fragments; its loads are a_load_half's written out in place, see there), the B-resident kernel (bres_load,
// bres_step) and k_critic_update, which gives k_bres's bits by calling these:
//   4   fp32, 16-byte rows (K, lda % 4 == 0): one 16-byte load per half
//   2   fp32, 8-byte rows (K, lda even: the critic's [M, 130] observations): two 8-byte loads per half
//   16  fp16 rows (P_F16 at scale 1): a half is the 4 halves k .. k + 3, 8 bytes, which ARE the fragment;
//       raw[0] packs both halves', raw[1] is unused
//   32  x2 planes (P_X2 at scale 1; addressed as the fp32 matrix, lda in 4-byte units): fp32's 16-byte load is
//       [hi k .. k + 3][lo k .. k + 3]
// Loads go through a buffer resource: an offset past the buffer's end returns zeros, so the columns past K cost
// one select of the offset -- no branch, and no wait on the loaded value (a select on the value, or two load
// forms merged at a branch, made the compiler wait for each k-step's loads at the end of the step that issued
// them: no prefetch at all).
template <int VW>
constexpr uint32_t kAEsz = VW == 16 ? 2u : 4u;  // bytes per A element

// half h of k-step ks -> raw; roff: the lane's row (clamped inside the matrix), column kq, in bytes
template <int VW>
__device__ __forceinline__ void a_load_half(__amdgpu_buffer_rsrc_t rs, uint32_t roff, int ks, int h, int K, int kq,
                                            float4 (&raw)[2]) {
    const int kk = 32 * ks + kq + 16 * h;
    const uint32_t o = roff + kAEsz<VW> * (32 * ks + 16 * h);
    if constexpr (VW == 16) {
        const u32x2v v = __builtin_amdgcn_raw_buffer_load_b64(rs, kk < K ? o : kBufOOB, 0, 0);
        if (h == 0) raw[0].x = __uint_as_float(v.x), raw[0].y = __uint_as_float(v.y);
        else raw[0].z = __uint_as_float(v.x), raw[0].w = __uint_as_float(v.y);
        raw[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else if constexpr (VW == 4 || VW == 32) {
        const u32x4v v = __builtin_amdgcn_raw_buffer_load_b128(rs, kk < K ? o : kBufOOB, 0, 0);
        raw[h] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    } else {
        const u32x2v a = __builtin_amdgcn_raw_buffer_load_b64(rs, kk < K ? o : kBufOOB, 0, 0);
        const u32x2v b = __builtin_amdgcn_raw_buffer_load_b64(rs, kk + 2 < K ? o + 8 : kBufOOB, 0, 0);
        raw[h] = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(b.x), __uint_as_float(b.y));
    }
}

__device__ __forceinline__ bf16x8 a_bits(float x, float y, float z, float w) {
    return __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z),
                                                 __float_as_uint(w)));
}

// raw -> the fragment planes a[0 .. kPlanes - 1]: fp32 converted at scale s (cvt2), fp16 as loaded, x2 planes
// regrouped.  The x2-plane fragment -- hi = (r[0].xy, r[1].xy), lo = (r[0].zw, r[1].zw) -- has two forms, chosen
// per kernel for its registers: a_frag<P_X2, 32> swaps two register pairs in the raw registers themselves
// (dead after this step until reloaded: the callers' raw sets are their own locals), so an MFMA operand is a
// loaded register quadruple and no copy of the eight is held (k_bres); a_frag_x2p_copy copies (k_x3nt).
__device__ __forceinline__ void a_frag_x2p_copy(const float4 (&r)[2], bf16x8 (&a)[3]) {
    a[0] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(r[0].x), __float_as_uint(r[0].y),
                                                 __float_as_uint(r[1].x), __float_as_uint(r[1].y)));
    a[1] = __builtin_bit_cast(bf16x8, make_uint4(__float_as_uint(r[0].z), __float_as_uint(r[0].w),
                                                 __float_as_uint(r[1].z), __float_as_uint(r[1].w)));
}
template <int P, int VW>
__device__ __forceinline__ void a_frag(const float4 (&r)[2], float s, bf16x8 (&a)[3]) {
    static_assert(VW != 16 || P == P_F16, "fp16 A: P_F16");
    static_assert(VW != 32 || P == P_X2, "x2 planes A: P_X2");
    if constexpr (VW == 16) {
        a[0] = a_bits(r[0].x, r[0].y, r[0].z, r[0].w);
    } else if constexpr (VW == 32) {
        float4(&m)[2] = const_cast<float4(&)[2]>(r);
        // (the two wait states between a VALU write and an MFMA reading it as an operand: inside the string)
        asm("v_swap_b32 %0, %2\n\tv_swap_b32 %1, %3\n\ts_nop 1"
            : "+v"(m[0].z), "+v"(m[0].w), "+v"(m[1].x), "+v"(m[1].y));
#pragma unroll
        for (int q = 0; q < 2; q++) a[q] = a_bits(m[q].x, m[q].y, m[q].z, m[q].w);
    } else {
        uint32_t w[4][3];
        cvt2<P>(r[0].x, r[0].y, s, w[0]);
        cvt2<P>(r[0].z, r[0].w, s, w[1]);
        cvt2<P>(r[1].x, r[1].y, s, w[2]);
        cvt2<P>(r[1].z, r[1].w, s, w[3]);
#pragma unroll
        for (int q = 0; q < Prec<P>::kPlanes; q++)
            a[q] = __builtin_bit_cast(bf16x8, make_uint4(w[0][q], w[1][q], w[2][q], w[3][q]));
    }
}

// the final 16-wide step: the 4 values k = 4 (l >> 4) .. +3 (the j < 4 half of a TP piece: raw[0]; fp16 A: its
// first 8 bytes; x2 planes: [hi k .. k + 3][lo k .. k + 3])
template <int P, int VW>
__device__ __forceinline__ void a_frag16(const float4 (&rr)[2], float s, uint2 (&a)[3]) {
    const float4& r = rr[0];
    if constexpr (VW == 16 || VW == 32) {
        a[0] = make_uint2(__float_as_uint(r.x), __float_as_uint(r.y));
        if constexpr (VW == 32) a[1] = make_uint2(__float_as_uint(r.z), __float_as_uint(r.w));
    } else {
        uint32_t w[2][3];
        cvt2<P>(r.x, r.y, s, w[0]);
        cvt2<P>(r.z, r.w, s, w[1]);
#pragma unroll
        for (int q = 0; q < Prec<P>::kPlanes; q++) a[q] = make_uint2(w[0][q], w[1][q]);
    }
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
