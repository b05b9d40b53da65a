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
//
// Included once by x3mlp.hip, inside namespace mm::x3, after gemm_parts.h; the plan (bres_plan) and the launches
// are in x3mlp.hip.
// ---------------------------------------------------------------------------

// waves per workgroup (one workgroup per CU: the B block fills LDS).  12 (168 registers per wave: no spills,
// the epilogue's row offsets and both A buffers held) measured 5-8% faster than 16 (128 registers, spilling)
// and than 8
constexpr int kBresWaves = 12;

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

// A through a buffer resource (gemm_parts.h, "the row-major A operand")
struct BresA {
    __amdgpu_buffer_rsrc_t rsrc;  // A: base, num_records = M lda 4 bytes
    uint32_t roff[2];             // this lane's row of row tile r (r < RT), + 4 kq bytes
};

// A for one 32-wide k-step, RT row tiles: zeros at columns >= K
template <int RT, int VW>
__device__ __forceinline__ void bres_load(const BresA& as, int ks, int K, int kq, float4 (&raw)[RT][2]) {
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int r = 0; r < RT; r++) a_load_half<VW>(as.rsrc, as.roff[r], ks, h, K, kq, raw[r]);
}

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
    for (int r = 0; r < RT; r++) a_frag<P, VW>(cur[r], ascale, a[r]);
    bres_load<RT, VW>(as, ks + D, K, kq, nxt);  // D steps ahead (past the last step: zeros)
    int boff = ((ks * ctb + c0) * np) * 64 + lane;  // bf16x8 units
    asm volatile("" : "+v"(boff));                  // one base per step (not 18 hoisted addresses)
    const bf16x8* bp = reinterpret_cast<const bf16x8*>(sF) + boff;
    // (column c + 1's B fragments read while column c's MFMAs run measured no faster: DESIGN.md section 3)
#pragma unroll
    for (int c = 0; c < CT; c++) {
        if (c < ctn) {  // wave-uniform (a guard, not a break: the loop stays fully unrolled, acc in registers)
            bf16x8 bb[3];
#pragma unroll
            for (int q = 0; q < np; q++) bb[q] = bp[(c * np + q) * 64];
#pragma unroll
            for (int r = 0; r < RT; r++) acc[r][c] = mma<P>(a[r], bb, acc[r][c], accx[r][c]);
        }
    }
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
    constexpr uint32_t aesz = kAEsz<VW>;  // VW 16: A is fp16 [M, lda] (32: x2 planes, a pair per element)
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
            const int row = min(16 * (RT * u + r) + (lane & 15), M - 1);  // rows past M: computed, not stored
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
                        a_frag16<P, VW>(rem == 0 ? rA[r] : rem == 1 ? rB[r] : rC[r], ascale, a4[r]);
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
                    for (int r = 0; r < RT; r++) a_frag16<P, VW>(odd ? rawB[r] : rawA[r], ascale, a4[r]);
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
                        for (int r = 0; r < RT; r++) acc[r][c] = mma<P>(a4[r], bb, acc[r][c], accx[r][c]);
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
