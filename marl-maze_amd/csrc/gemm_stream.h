// ---------------------------------------------------------------------------
// k_x3nt, the streaming GEMM: C[M, N] = A[M, K] . B[N, K]^T with B (TP planes) streamed through LDS one k-step
// at a time by LDS-DMA, A from one of the sources below.  Included once by x3mlp.hip, inside namespace mm::x3,
// after gemm_parts.h; its dispatch and launches (dispatch_stream, launch_nt) are in x3mlp.hip.
// ---------------------------------------------------------------------------
// the streaming kernel's waves per workgroup (one row tile each); 8 measured equal
constexpr int kWaves = 16;
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

// B piece i (column tile i / planes, plane i % planes) of k-step ks -> LDS (one 1-KiB LDS-DMA)
template <int P>
__device__ __forceinline__ void dma_b(const uint16_t* Bg, int nks, int ks, int i, uint16_t* dst, int lane) {
    constexpr int np = Prec<P>::kPlanes;
    const int ct = i / np, p = i - np * ct;
    const uint4* src = reinterpret_cast<const uint4*>(Bg + ((size_t)ct * nks + ks) * Prec<P>::kBlk + p * 512);
    __builtin_amdgcn_global_load_lds(src + lane, dst, 16, 0, 0);
}

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

// row-major A [M, lda] in the operand form VW (gemm_parts.h, "the row-major A operand"): 4 / 2 fp32 with 16- /
// 8-byte rows, converted in registers at `scale`; 16 fp16 rows (P_F16 at scale 1: the f16 networks' stored
// front-end output h, K = 460, which the B-resident kernel does not take); 32 x2 planes (P_X2 at scale 1).  The
// host keeps M lda 4 < 2^31 (row chunks).  One struct for the four forms; the kernels are instantiated on the
// names ASrcF32V<4>, ASrcF32V<2>, ASrcF16V and ASrcX2PV.
template <int VW>
struct ASrcF32V {
    typedef float4 Raw[2];
    __amdgpu_buffer_rsrc_t rs;
    uint32_t roff;  // this lane's row (clamped inside the matrix), column 4 (l >> 4), bytes
    int K, kq;
    float scale;
    template <class AT>
    __device__ void init(const AT* base, int rt, int, int M, int lda, int K_, float scale_) {
        const int lane = threadIdx.x & 63;
        const int r = min(16 * rt + (lane & 15), M - 1);  // rows past M: computed, never stored
        K = K_;
        scale = scale_;
        kq = 4 * (lane >> 4);
        rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)((size_t)M * lda * kAEsz<VW>), 0x00020000);
        roff = kAEsz<VW> * ((uint32_t)r * (uint32_t)lda + (uint32_t)kq);
    }
    // a_load_half's loads and selects, written out: through the shared function every k_x3nt instantiation on
    // these sources gained one or two VGPRs
    __device__ __forceinline__ void load(int ks, Raw& r, int) const {
        const int k = 32 * ks + kq;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t o = roff + kAEsz<VW> * (32 * ks + 16 * h);
            if constexpr (VW == 16) {
                const u32x2v v = __builtin_amdgcn_raw_buffer_load_b64(rs, k + 16 * h < K ? o : kBufOOB, 0, 0);
                if (h == 0) r[0].x = __uint_as_float(v.x), r[0].y = __uint_as_float(v.y);
                else r[0].z = __uint_as_float(v.x), r[0].w = __uint_as_float(v.y);
            } else if constexpr (VW == 4 || VW == 32) {
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
        if constexpr (VW == 32) a_frag_x2p_copy(r, a);
        else a_frag<P, VW>(r, scale, a);
    }
};
typedef ASrcF32V<4> ASrcF32;
typedef ASrcF32V<2> ASrcF32U;
struct ASrcF16V : ASrcF32V<16> {};
struct ASrcX2PV : ASrcF32V<32> {};

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
    as.load(more ? ks + 1 : ks, rawn, lane);
    const bf16x8* b8 = reinterpret_cast<const bf16x8*>(cur) + lane;
#pragma unroll
    for (int c = 0; c < NT; c++) {
        if (more && c < C::kPerWaveB) {
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

static_assert(kWaves == kStampWaves, "the phase clocks' wave slots (gemm_parts.h)");

// C[M, N] = A[M, K] . B[N, K]^T, B in TP, A from source AS.  Workgroup: 16
// waves, 256 rows x 16 NT columns; wave w owns row tile w and all NT column
// tiles.  A is private to a wave: straight from HBM to registers, one k-step
// ahead.  B (the weights) is shared: LDS-DMA into a double-buffered stage, the
// DMA issues spread over the MFMA stream.  One barrier per k-step; four waves
// per SIMD hide the LDS latency of the B fragment reads.  Persistent over
// 256-row units.
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
