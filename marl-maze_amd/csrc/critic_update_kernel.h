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
// Included once by x3mlp.hip, inside namespace mm::x3, after gemm_parts.h and gemm_bres.h (bres_load); the
// launch (mm_critic_update) is in x3mlp.hip.
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

// one 64-wide layer of the wave's tile: A rows from its fp32 tile (k_bres's fp32-A fragments at scale s: a_frag),
// B the NT column tiles of a resident pack [2 k-steps][NT][2 planes][1 KiB]; the products in the x2 order,
// tile-interleaved (x2_mma_tiles: one wave per SIMD here)
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
        a_frag<P_X2, 4>(raw, s, a);
        const bf16x8* bp = reinterpret_cast<const bf16x8*>(sB) + (ks * NT * 2) * 64 + lane;
        bf16x8 bb[NT][2];
#pragma unroll
        for (int c = 0; c < NT; c++) bb[c][0] = bp[(c * 2) * 64], bb[c][1] = bp[(c * 2 + 1) * 64];
        x2_mma_tiles(a, bb, acc, accx);
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
            a_frag<P_X2, 2>(raw[ks][0], 1.f, af[ks]);
        }
        a_frag16<P_X2, 2>(raw[nfull][0], 1.f, at);
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
                x2_mma_tiles(af[ks], bb, h0, accx);
            }
            {
                const uint2* bp = reinterpret_cast<const uint2*>(sm + kCuT0) + lane;
                uint2 bb[4][2];
#pragma unroll
                for (int c = 0; c < 4; c++) bb[c][0] = bp[(c * 2) * 64], bb[c][1] = bp[(c * 2 + 1) * 64];
                x2_mma_tiles(at, bb, h0, accx);
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
