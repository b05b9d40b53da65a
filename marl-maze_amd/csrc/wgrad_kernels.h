// ---------------------------------------------------------------------------
// Weight gradient (see x3mlp.hip's header): dW [N, K] = cscale * sum_m (dscale dY[m, n]) X[m, k].
// Included once by x3mlp.hip, inside namespace mm::x3 (it uses Prec, mma, store_piece, x2_combine, the range
// guard and kBufOOB from there); the plan (WgPlan, wg_plan) and the launches are in x3mlp.hip.
//
// Work unit = (row slice s, column block cb of <= 17 tiles); 8 waves; per
// 32-row step every thread loads (operand, column, 8-row chunk) pieces for the
// NEXT step into registers while the waves run the current step's MFMAs from
// LDS; then it converts them into the fragment images (bf16x3 split or scaled
// fp16) with one 16-byte LDS write per plane.  Wave w owns the contiguous run
// of output tiles w * TPW .. (row-major over (n-tile, k-tile)), so its A
// fragment is re-read only when the run crosses an n-tile.  Each unit writes
// its partial [N, K] to ws[s]; mm_sum_leading sums the slices in order.
//
// Five kernels: k_wgrad (any shape, register staging), k_wgrad_rect (the actor's and critic's shapes, register
// staging), k_wgrad_dma (x2, fp32 operands by LDS-DMA), k_wgrad_tr (x2, both operands stored as planes),
// k_wgrad_mix (x2, dY as planes beside an fp32 X).  Their step schedules differ for measured reasons (DESIGN.md
// section 3); what they share is written once, first: the work unit, the barrier and the counted DMA wait, the
// per-operand DMA part with the operand rule, the fragment reads, the X conversion, the rectangle MFMA loop and
// the epilogue.  k_wgrad_rect keeps its own unit decode, MFMA loop and epilogue: any change to them re-schedules
// some of its 37 instantiations ("One set of shared parts").
// ---------------------------------------------------------------------------
constexpr int kWgWaves = 8;
constexpr int kWgThreads = 64 * kWgWaves;
constexpr int kWgMaxT = 17;                                             // tiles per side of a unit
constexpr int kWgPer = (64 * 2 * kWgMaxT + kWgThreads - 1) / kWgThreads;  // pieces per thread and step

// ---- the shared parts ------------------------------------------------------

// The work unit of a workgroup.  XCD-aware: units u and u + 8 (one XCD) are the column blocks of one slice (its
// dY rows shared in L2).  s >= nslices: no unit -- the kernel returns (the whole workgroup).
struct WgUnit {
    int s, cb;           // row slice, column block
    int m_begin, nrows;  // the slice's rows
    int col0;            // the block's first column of X
    int lane, wave;
};
__device__ __forceinline__ WgUnit wg_unit(int M, int rows, int ncb, int NTK) {
    WgUnit u;
    u.lane = threadIdx.x & 63;
    u.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    u.s = (slot / ncb) * 8 + xcd;
    u.cb = slot % ncb;
    u.m_begin = u.s * rows;
    u.nrows = min(M, u.m_begin + rows) - u.m_begin;
    u.col0 = u.cb * NTK * 16;
    return u;
}

// This wave's LDS accesses done (lgkmcnt(0) only: no wait for loads in flight, vmcnt), then the workgroup's
// barrier: LDS writes -- and the DMAs waited for by wg_wait_stage -- visible to every wave.  kClobber: also a
// compiler barrier for memory accesses, which the LDS-DMA kernels need (their DMAs' LDS writes are inline asm the
// compiler cannot see); the register-staging kernels (k_wgrad, k_wgrad_rect) leave it out, so that their
// prefetching global loads stay free to be scheduled across the barrier.
template <bool kClobber = true>
__device__ __forceinline__ void wg_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt((15 << 0) | (7 << 4) | (0 << 8) | (3 << 14));  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    if constexpr (kClobber) asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// The counted wait of the LDS-DMA kernels: this wave's DMAs of the stage read next have landed; only a later
// stage's may stay in flight -- kHi instructions for the waves that issue one more per stage (hi_wave), kLo for
// the rest; none in flight (the tail): vmcnt(0).
template <int kHi, int kLo>
__device__ __forceinline__ void wg_wait_stage(bool hi_wave, bool later_in_flight) {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (later_in_flight) {
        if (hi_wave) {
            __builtin_amdgcn_s_waitcnt(0x0F70 | (kHi & 15) | ((kHi >> 4) << 14));
        } else {
            __builtin_amdgcn_s_waitcnt(0x0F70 | (kLo & 15) | ((kLo >> 4) << 14));
        }
    } else {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void wg_wait_all() { wg_wait_stage<0, 0>(false, false); }  // no DMA left in flight

// The DMA is inline asm: the compiler then sees no LDS write it cannot place, and inserts none of its own vmcnt
// waits before LDS accesses (through the stage pointers it made every conversion wait for every DMA in flight:
// vmcnt(0), one step of prefetch).  The kernels wait for their DMAs themselves, by count (wg_wait_stage).
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t lds) {
    uint32_t save;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(save)
                 : "v"(voff), "s"(r), "s"(lds)
                 : "memory");
}
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// The buffer resource over `bytes` of an operand's slice, pinned in its SGPRs (see the operand rule).  Rows past
// the slice read past num_records and land as zeros.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_slice_rsrc(const void* p, int bytes) {
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, bytes, 0x00020000);
    asm volatile("" : "+s"(r));
    return r;
}

// The lane's byte offset, in step t, of its 16-byte piece of DMA instruction j of an operand's part: rows of
// pitch wp pieces of which 4 T hold columns (T the operand's tiles; the row padding reads out of range).
template <int wp, int T>
__device__ __forceinline__ uint32_t wg_row_off(int j, int lane, int t, int ld) {
    const int e = 64 * j + lane;  // piece inside the part
    const int r = e / wp, c = e % wp;
    return c < 4 * T ? (uint32_t)(((32 * t + r) * ld + 4 * c) * 4) : kBufOOB;
}

// One operand's LDS-DMA of a kernel with kStages raw stages: kIns 1-KiB instructions per stage, this wave's
// being j = wave + 8 k (the operand of an offset slot is a compile-time fact, so each DMA names its resource
// directly: a selected copy would be rewritten while earlier DMAs are in flight).
//
// THE OPERAND RULE ("The k_wgrad_rect zeros": a buffer load reads its operands after the
// wave has gone on, and a register rewritten in that window gave lanes zeros): an in-flight DMA's offset VGPR
// is never rewritten.  There is one offset set per stage, ob[T], and issue<T> advances it IN PLACE, by kStages
// steps, only when stage T's previous DMA was waited for (the kernel's schedule: a stage is issued again after
// the step that read it); the resource SGPRs (wg_slice_rsrc) and the offsets are held to the end of the kernel
// (hold).  tools/check_wgrad_operands.py checks the ISA of every instantiation.
template <int kIns, int kStages>
struct WgDmaPart {
    static constexpr int kSlots = (kIns + kWgWaves - 1) / kWgWaves;
    uint32_t ob[kStages][kSlots];

    template <class F>
    __device__ __forceinline__ void init(int wave, F&& lane_off) {  // lane_off(j, t): see wg_row_off
#pragma unroll
        for (int k = 0; k < kSlots; k++) {
            const int j = min(wave + kWgWaves * k, kIns - 1);  // (clamped: not issued)
#pragma unroll
            for (int t = 0; t < kStages; t++) {
                ob[t][k] = lane_off(j, t);
                asm volatile("" : "+v"(ob[t][k]));
            }
        }
    }
    // the DMA of step st into stage T, whose part starts at LDS address lds_base (step_bytes: kStages steps);
    // the caller fences its issues with sched_barrier(0), one pair around the parts it issues together
    template <int T>
    __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rs, uint32_t lds_base, int wave, int st,
                                          uint32_t step_bytes) {
#pragma unroll
        for (int k = 0; k < kSlots; k++) {
            const int j = wave + kWgWaves * k;  // wave-uniform
            if (j < kIns) {
                if (st >= kStages) asm volatile("v_add_u32 %0, %0, %1" : "+v"(ob[T][k]) : "s"(step_bytes));
                dma16(rs, ob[T][k], lds_base + 1024u * (uint32_t)j);
            }
        }
    }
    __device__ __forceinline__ void hold(__amdgpu_buffer_rsrc_t rs, uint32_t step_bytes) {
#pragma unroll
        for (int t = 0; t < kStages; t++)
#pragma unroll
            for (int k = 0; k < kSlots; k++) asm volatile("" ::"v"(ob[t][k]));
        asm volatile("" ::"s"(rs), "s"(step_bytes));
    }
};

// The transposed fragment read of an operand stored as x2 planes, straight from a raw stage (rows of pitch wp
// pieces, a piece [4 hi halves][4 lo halves]), with ds_read_b64_tr_b16: lane 4 q + p of row group c supplies
// row 8 c + q, piece p of the tile (its four columns 4 p .. 4 p + 3: the hi halves, 8 bytes on the lo halves),
// and receives, for its column l & 15, the rows 8 c .. 8 c + 3 and 8 c + 4 .. 8 c + 7 per plane -- exactly the
// fragment the image holds (wg_img_frag).  wg_tr_lane: the lane's byte offset in a stage whose part starts
// `sec` pieces in.
typedef short wg_s4v __attribute__((ext_vector_type(4)));
template <int wp>
__device__ __forceinline__ uint32_t wg_tr_lane(int lane, int sec) {
    const int tc = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    return (uint32_t)(16 * (sec + (8 * tc + tq) * wp + tp));
}
template <int wp>
__device__ __forceinline__ void wg_tr_frag(const char* stage, uint32_t lane_base, int tile, bf16x8 (&f)[3]) {
    const char* p = stage + lane_base + 64 * tile;
    constexpr int r4 = 16 * 4 * wp;  // four rows on, bytes
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const wg_s4v u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) wg_s4v*)(p + 8 * q));
        const wg_s4v v =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) wg_s4v*)(p + 8 * q + r4));
        f[q] = bf16x8{u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
    }
}

// The fragment of a tile of the image (np planes of 64 lanes x 16 bytes).
template <int np>
__device__ __forceinline__ void wg_img_frag(const uint16_t* tile, int lane, bf16x8 (&f)[3]) {
    const bf16x8* p = reinterpret_cast<const bf16x8*>(tile) + lane;
#pragma unroll
    for (int q = 0; q < np; q++) f[q] = p[64 * q];
}

// pair2 (x s -> the x2 (hi, lo) fp16 pair of two values) in NON-packed instructions, for conversions that
// run beside MFMAs: packed f32 VALU (v_pk_mul_f32 / v_pk_fma_f32, which the compiler SLP-forms from pair2's
// vector arithmetic) costs ~22-26 extra cycles per instruction next to an MFMA (MI355X_MICROARCH.md), plain
// VOP3 / VOP3P-mix instructions do not.  Same values as pair2: hi = RN16(x s); x s - hi exactly by one
// v_fma_mix_f32 reading hi's halves (x s is exact, s a power of two; the difference is exact, Sterbenz);
// times 2^11 exactly; RN16.  SCALED = false: s = 1 (no multiplies).
template <bool SCALED>
__device__ __forceinline__ void pair2_plain(float x0, float x1, float s, uint32_t& h, uint32_t& l) {
    float y0, y1;
    if constexpr (SCALED) {
        asm("v_mul_f32 %0, %4, %6\n\t"
            "v_mul_f32 %1, %5, %6\n\t"
            "v_cvt_pk_f16_f32 %2, %0, %1\n\t"
            "v_fma_mix_f32 %0, %4, %6, -%2 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mix_f32 %1, %5, %6, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
            "v_mul_f32 %0, 0x45000000, %0\n\t"
            "v_mul_f32 %1, 0x45000000, %1\n\t"
            "v_cvt_pk_f16_f32 %3, %0, %1"
            : "=&v"(y0), "=&v"(y1), "=&v"(h), "=&v"(l)
            : "v"(x0), "v"(x1), "v"(s));
    } else {
        asm("v_cvt_pk_f16_f32 %2, %4, %5\n\t"
            "v_fma_mix_f32 %0, %4, 1.0, -%2 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mix_f32 %1, %5, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
            "v_mul_f32 %0, 0x45000000, %0\n\t"
            "v_mul_f32 %1, 0x45000000, %1\n\t"
            "v_cvt_pk_f16_f32 %3, %0, %1"
            : "=&v"(y0), "=&v"(y1), "=&v"(h), "=&v"(l)
            : "v"(x0), "v"(x1));
        (void)s;
    }
}
template <bool SCALED>
__device__ __forceinline__ void store_piece_x2_plain(const float* v, float s, uint4* dst) {
    uint32_t hh[4], ll[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pair2_plain<SCALED>(v[2 * k], v[2 * k + 1], s, hh[k], ll[k]);
    dst[0] = make_uint4(hh[0], hh[1], hh[2], hh[3]);
    dst[64] = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}

// The fp32 X rows of a raw stage (32 rows x 16 NTK floats, row-major) -> the x2 image of NTK tiles at im: this
// thread's pieces (8-row chunk c, column j), scale 1.
template <int NTK>
__device__ __forceinline__ void wg_conv_x(const float* xs, uint16_t* im) {
    constexpr int kB = Prec<P_X2>::kBlk, kWB = 16 * NTK, itemsB = 64 * NTK;
    constexpr int kPerB = (itemsB + kWgThreads - 1) / kWgThreads;
#pragma unroll
    for (int q = 0; q < kPerB; q++) {
        const int e = threadIdx.x + kWgThreads * q;
        if (e < itemsB) {
            const int c = e / kWB, j = e - c * kWB;
            const float* src = xs + 8 * c * kWB + j;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = src[i * kWB];
            const int loff = (j >> 4) * kB + c * 128 + (j & 15) * 8;
            store_piece_x2_plain<false>(v, 1.f, reinterpret_cast<uint4*>(im + loff));
        }
    }
}

// The accumulators of a unit of TN x NTK tiles: wave w owns the rectangle of n-tiles RN w .. RN w + RN - 1 by
// all NTK k-tiles, plus its share of the leftover n-tiles (TN - 8 RN rows of NTK tiles, dealt round-robin).
template <int TN, int NTK>
struct WgRect {
    static constexpr int RN = TN / kWgWaves;                     // n-tiles per wave in the rectangle
    static constexpr int kRem = (TN - kWgWaves * RN) * NTK;      // leftover tiles
    static constexpr int EX = (kRem + kWgWaves - 1) / kWgWaves;  // leftover tiles per wave (max)
    static constexpr int kAcc = RN * NTK + EX;
};

// A step's MFMAs of the LDS-DMA kernels, over the rectangle and the leftovers: the RN A fragments and the one of
// the leftover tiles' n-tile held in registers, each B fragment read once and used RN times, the next k-tile's B
// fragments read while the current ones feed the MFMAs; then the wave's leftover tiles (clamped: a duplicate,
// not stored).  No runtime branch in the loop but, with kSkip, `live`: k-tiles >= live are skipped
// (workgroup-uniform).  fragA(n-tile, f) / fragB(k-tile, f) read a fragment; mid(tk) runs after k-tile tk's MFMAs.
// Plain `inline` on purpose: a forced inline runs before the calling step lambda is simplified, and that order
// re-schedules k_wgrad_dma's leftover MFMAs against their waits.  Were it ever left as a call, its array
// arguments would live in scratch: tests/test_isa_wgrad_scratch.py pins ScratchSize 0 for the four kernels.
template <int P, int TN, int NTK, bool kSkip, class FA, class FB, class Mid>
__device__ inline void wg_rect_mfma(int wave, FA&& fragA, FB&& fragB, f32x4 (&acc)[WgRect<TN, NTK>::kAcc],
                                    f32x4 (&accx)[WgRect<TN, NTK>::kAcc], int live, Mid&& mid) {
    using R = WgRect<TN, NTK>;
    constexpr int RN = R::RN, kRem = R::kRem, EX = R::EX;
    static_assert(RN > 0 && (kRem == 0 || TN - kWgWaves * RN == 1), "leftover tiles of one n-tile (one A fragment)");
    bf16x8 a[RN][3], ax[3], b[2][3];
#pragma unroll
    for (int r = 0; r < RN; r++) fragA(RN * wave + r, a[r]);
    if constexpr (EX > 0) fragA(kWgWaves * RN, ax);  // the leftover tiles' n-tile
    fragB(0, b[0]);
#pragma unroll
    for (int tk = 0; tk < NTK; tk++) {
        if (tk + 1 < NTK) fragB(tk + 1, b[(tk + 1) & 1]);  // next k-tile, ahead
        if (!kSkip || tk < live) {
#pragma unroll
            for (int r = 0; r < RN; r++)
                acc[r * NTK + tk] = mma<P>(a[r], b[tk & 1], acc[r * NTK + tk], accx[r * NTK + tk]);
        }
        mid(tk);
    }
#pragma unroll
    for (int e = 0; e < EX; e++) {
        int j = wave + kWgWaves * e;  // leftover tile j (clamped: a duplicate, not stored)
        j = j < kRem ? j : kRem - 1;
        if (!kSkip || j % NTK < live) {  // wave-uniform
            bf16x8 b1[3];
            fragB(j % NTK, b1);
            acc[RN * NTK + e] = mma<P>(ax, b1, acc[RN * NTK + e], accx[RN * NTK + e]);
        }
    }
}

// The epilogue of the LDS-DMA kernels: x2_combine, the range guard, the unit's partial to ws[s] (rectangle,
// then leftovers).  kStoredOnly = false: the guard runs over all accumulators (the clamped duplicate leftover
// tiles included: same data).  true: over the stored elements only -- the accumulators of rows >= N / columns
// >= K may hold anything (NaN patterns of a pitch padding included).  x2_combine is written in both the
// guard's loop and put(): one value, computed once (the compiler merges the two), so acc stays read-only.
template <int P, int TN, int NTK, bool kStoredOnly>
__device__ __forceinline__ void wg_store(const WgUnit& un, const f32x4 (&acc)[WgRect<TN, NTK>::kAcc],
                                         const f32x4 (&accx)[WgRect<TN, NTK>::kAcc], int N, int K, float cscale,
                                         float* ws) {
    using R = WgRect<TN, NTK>;
    constexpr int RN = R::RN, kRem = R::kRem, EX = R::EX;
    uint32_t rm = 0;
    if constexpr (!kStoredOnly) {
#pragma unroll
        for (int u = 0; u < R::kAcc; u++) range_acc<P>(rm, x2_combine<P>(acc[u], accx[u]));
        range_note<P>(rm);
    }
    float* out = ws + (size_t)un.s * N * K;
    auto put = [&](f32x4 v, f32x4 vx, int tn, int tk) {
        v = x2_combine<P>(v, vx);
        const int col = un.col0 + 16 * tk + (un.lane & 15);
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = 16 * tn + 4 * (un.lane >> 4) + g;
            if (row < N && col < K) {
                if constexpr (kStoredOnly) rm = max(rm, __float_as_uint(v[g]) & 0x7FFFFFFFu);
                out[(size_t)row * K + col] = v[g] * cscale;
            }
        }
    };
#pragma unroll
    for (int r = 0; r < RN; r++)
#pragma unroll
        for (int tk = 0; tk < NTK; tk++) put(acc[r * NTK + tk], accx[r * NTK + tk], RN * un.wave + r, tk);
#pragma unroll
    for (int e = 0; e < EX; e++) {
        const int j = un.wave + kWgWaves * e;
        if (j < kRem) put(acc[RN * NTK + e], accx[RN * NTK + e], kWgWaves * RN + j / NTK, j % NTK);
    }
    if constexpr (kStoredOnly) range_note<P>(rm);
}

// ---- k_wgrad: any shape (TN, NTK and the tile runs at run time) -------------

template <int P, int TPW>
__global__ __launch_bounds__(kWgThreads) void k_wgrad(const float* __restrict__ dy, int lddy, float dscale,
                                                      const float* __restrict__ x, int ldx, int M, int N, int K,
                                                      int TN, int NTK, int tpw, int rows, int nslices, int ncb,
                                                      float cscale, float* __restrict__ ws) {
    constexpr int kB = Prec<P>::kBlk;
    constexpr int np = Prec<P>::kPlanes;
    // two image sets [A: TN tiles | B: NTK tiles] (dynamic LDS): step st's MFMAs read set st & 1 while the
    // waves convert step st + 1 into the other set -- one barrier per step
    extern __shared__ __attribute__((aligned(16))) uint16_t img[];
    const WgUnit un = wg_unit(M, rows, ncb, NTK);
    if (un.s >= nslices) return;  // the whole workgroup
    const int lane = un.lane, wave = un.wave, nrows = un.nrows, col0 = un.col0;
    const int wA = TN * 16, wB = NTK * 16;  // staged columns per operand
    const int itemsA = 4 * wA, items = itemsA + 4 * wB;  // itemsA = 64 TN: a piece's operand is wave-uniform
    const int set = (TN + NTK) * kB;                     // uint16 per image set
    const float* const baseA = dy + (size_t)un.m_begin * lddy;
    const float* const baseB = x + (size_t)un.m_begin * ldx + col0;

    // loop-invariant per piece q: first row inside a step (8c), element offset of (8c, column) from the
    // operand's slice base, validity, and the LDS destination of its fragment piece
    int r8[kWgPer], goff[kWgPer], loff[kWgPer];
    bool ok[kWgPer];
#pragma unroll
    for (int q = 0; q < kWgPer; q++) {
        const int e = threadIdx.x + kWgThreads * q;
        const bool isA = e < itemsA;
        const int e2 = isA ? e : e - itemsA, w = isA ? wA : wB;
        const int c = e2 / w, j = e2 - c * w;  // 8-row chunk, column: consecutive threads, consecutive columns
        ok[q] = e < items && (isA ? j < N : col0 + j < K);
        r8[q] = 8 * c;
        goff[q] = ok[q] ? 8 * c * (isA ? lddy : ldx) + j : 0;
        loff[q] = (isA ? 0 : TN * kB) + (j >> 4) * kB + c * 128 + (j & 15) * 8;
    }

    float raw[kWgPer][8];
    auto load_piece = [&](int q, int r0) {  // rows r0 + 8c .. + 7 of the slice
        const bool isA = threadIdx.x + kWgThreads * q < itemsA;  // wave-uniform
        const int ld = isA ? lddy : ldx;
        const float* rowp = (isA ? baseA : baseB) + (size_t)r0 * ld;  // uniform
        int o = goff[q];
        asm volatile("" : "+v"(o));  // per step: not 40 loop-invariant addresses held in registers
        const int lim = nrows - r0 - r8[q];
#pragma unroll
        for (int i = 0; i < 8; i++) {
#ifdef WG_NO_GLOAD  // diagnostic builds only: no global loads
            raw[q][i] = ok[q] ? (float)(r0 + i) : 0.f;
#else
            raw[q][i] = (ok[q] && i < lim) ? rowp[o + i * ld] : 0.f;
#endif
        }
    };
    auto store_piece_q = [&](int q, uint16_t* dst_set) {
        if (threadIdx.x + kWgThreads * q < items) {
            const bool isA = threadIdx.x + kWgThreads * q < itemsA;
            store_piece<P>(raw[q], isA ? dscale : 1.f, reinterpret_cast<uint4*>(dst_set + loff[q]));
        }
    };

    f32x4 acc[TPW], accx[TPW];
#pragma unroll
    for (int u = 0; u < TPW; u++) acc[u] = accx[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    // wave w: the run of tiles w * tpw .. + tpw - 1 (row-major over (n-tile, k-tile)), balanced
    const int ntiles = TN * NTK, first = wave * tpw, last = min(ntiles, first + tpw);
    const int tn0 = first / NTK, tk0 = first - tn0 * NTK;
    const int nsteps = (nrows + 31) / 32;
#pragma unroll
    for (int q = 0; q < kWgPer; q++) load_piece(q, 0);
#pragma unroll
    for (int q = 0; q < kWgPer; q++) store_piece_q(q, img);
    if (nsteps > 1) {
#pragma unroll
        for (int q = 0; q < kWgPer; q++) load_piece(q, 32);
    }
    wg_barrier<false>();
    // the conversion of the next step's pieces is spread over the tile loop (VALU beside the MFMAs)
    constexpr int kEvery = TPW >= kWgPer ? TPW / kWgPer : 1;
    for (int st = 0; st < nsteps; st++) {
        const uint16_t* cur = img + (st & 1) * set;
        uint16_t* nxt = img + ((st + 1) & 1) * set;
        const bool more = st + 1 < nsteps;
        int tn = tn0, tk = tk0, curtn = -1;
        bf16x8 a[3], b[3];
#pragma unroll
        for (int u = 0; u < TPW; u++) {
#ifndef WG_NO_MFMA  // diagnostic builds only
            if (first + u < last) {
                if (tn != curtn) {
                    curtn = tn;
                    wg_img_frag<np>(cur + tn * kB, lane, a);
                }
                wg_img_frag<np>(cur + TN * kB + tk * kB, lane, b);
                acc[u] = mma<P>(a, b, acc[u], accx[u]);
            }
            if (++tk == NTK) {
                tk = 0;
                tn++;
            }
#endif
            if (more && u % kEvery == 0 && u / kEvery < kWgPer) store_piece_q(u / kEvery, nxt);
        }
        if (more) {
#pragma unroll
            for (int q = TPW / kEvery; q < kWgPer; q++) store_piece_q(q, nxt);  // (TPW < kWgPer)
            if (st + 2 < nsteps) {
#pragma unroll
                for (int q = 0; q < kWgPer; q++) load_piece(q, 32 * (st + 2));  // a whole step ahead
            }
        }
        wg_barrier<false>();  // set st & 1 read by every wave, set (st + 1) & 1 written
    }
    float* out = ws + (size_t)un.s * N * K;
    int tn = tn0, tk = tk0;
    uint32_t rm = 0;  // the range guard (range_acc)
#pragma unroll
    for (int u = 0; u < TPW; u++) {
        acc[u] = x2_combine<P>(acc[u], accx[u]);
        range_acc<P>(rm, acc[u]);  // (tiles past `last` were never accumulated: zeros)
        if (first + u < last) {
            const int col = col0 + 16 * tk + (lane & 15);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int row = 16 * tn + 4 * (lane >> 4) + g;
                if (row < N && col < K) out[(size_t)row * K + col] = acc[u][g] * cscale;
            }
        }
        if (++tk == NTK) {
            tk = 0;
            tn++;
        }
    }
    range_note<P>(rm);
}

// ---- k_wgrad_rect -----------------------------------------------------------
// Structured form of k_wgrad for the shapes the actor and critic use (TN, NTK
// compile-time): wave w owns the rectangle of n-tiles RN w .. RN w + RN - 1
// by all NTK k-tiles (its RN A fragments held in registers, each B fragment
// read once and used RN times, the next k-tile's B fragments read while the
// current ones feed the MFMAs), plus its share of the leftover n-tiles
// (TN - 8 RN rows of NTK tiles, dealt round-robin: A and B read per tile).
// No runtime branch in the MFMA loop.  Staging, double-buffered images,
// partials and the reduction are those of k_wgrad.  Its unit decode, MFMA
// loop and epilogue are its own text (the loop reads the leftover tiles' A
// per tile and converts pieces between the tiles; wg_rect_mfma and wg_store
// are the LDS-DMA kernels' forms): with the shared parts in their place some
// of the 37 instantiations were scheduled differently (more VGPRs, other
// waits), so they stay as measured.

// a staged value from its dword: fp32 (esz 4), or the fp16 half at bit offset sh (esz 2) -- selects, no branch
__device__ __forceinline__ float wg_val16(uint32_t d, uint32_t sh, bool h16) {
    const float h = (float)__builtin_bit_cast(_Float16, (unsigned short)(d >> sh));
    return h16 ? h : __uint_as_float(d);
}

// XB: bytes per X element -- 4 (fp32) or 2 (fp16: P_F16's stored activations, and the heads' x3 weight
// gradient over them; fp16 values are exact in fp32, so the staging is that of their fp32 values)
// AB: bytes per dY element -- 4, or 2 (P_F16's input gradients stored fp16 and pre-scaled: dscale 1)
template <int P, int TN, int NTK, int XB = 4, int AB = 4>
__global__ __launch_bounds__(kWgThreads) void k_wgrad_rect(const float* __restrict__ dy, int lddy, float dscale,
                                                           const float* __restrict__ x, int ldx, int M, int N, int K,
                                                           int rows, int nslices, int ncb, float cscale,
                                                           float* __restrict__ ws) {
    static_assert(XB == 4 || (XB == 2 && P != P_X2), "fp16 X: P_F16 / P_X3");
    static_assert(AB == 4 || (AB == 2 && P == P_F16), "fp16 dY: P_F16");
    constexpr bool k16 = XB == 2 || AB == 2;  // some operand fp16: dword loads + half selects
    constexpr int kB = Prec<P>::kBlk;
    constexpr int np = Prec<P>::kPlanes;
    constexpr int RN = TN / kWgWaves;                               // n-tiles per wave in the rectangle
    constexpr int kRem = (TN - kWgWaves * RN) * NTK;                // leftover tiles
    constexpr int EX = (kRem + kWgWaves - 1) / kWgWaves;            // leftover tiles per wave (max)
    constexpr int kSet = (TN + NTK) * kB;                           // uint16 per image set
    constexpr int itemsA = 64 * TN, items = itemsA + 64 * NTK;      // staged pieces per step
    constexpr int kPer = (items + kWgThreads - 1) / kWgThreads;
    extern __shared__ __attribute__((aligned(16))) uint16_t img[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int s = (slot / ncb) * 8 + xcd, cb = slot % ncb;
    if (s >= nslices) return;  // the whole workgroup
    const int m_begin = s * rows, nrows = min(M, m_begin + rows) - m_begin;
    const int col0 = cb * NTK * 16;
    const void* const baseA = reinterpret_cast<const char*>(dy) + (size_t)m_begin * lddy * AB;
    const void* const baseB = reinterpret_cast<const char*>(x) + ((size_t)m_begin * ldx + col0) * XB;

    // loads through one buffer resource per piece slot q over the slice's rows (loop-invariant, built once),
    // the step's row offset added to the lane's VGPR offset -- no per-element branch or 64-bit address.
    // EVERY OFFSET IS IN RANGE: lanes whose column is past N / K read the slice's first element (their
    // values only reach output rows >= N / columns >= K, which are never stored: an MFMA output element
    // depends on its own A row and B column only), and the rows past the slice in its last, partial step
    // read it too and are zeroed by a select.  (The round-4 forms, with out-of-range offsets or without,
    // returned zeros in the last quarter-wave of some loads; the cause was operand registers rewritten
    // while the loads were in flight: see the pinned operands below.)
    int loff[kPer], r8q[kPer], ldq[kPer];
    uint32_t voff[kPer], eszq[kPer];  // eszq: bytes per element of the slot's operand (wave-uniform)
    uint32_t hsh[kPer];               // XB 2, B slots: the bit offset of the lane's half in its dword
    bool h16q[kPer];
    __amdgpu_buffer_rsrc_t rsq[kPer];
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        const int e = threadIdx.x + kWgThreads * q;
        const bool isA = e < itemsA;
        const int e2 = isA ? e : e - itemsA, w = isA ? 16 * TN : 16 * NTK;
        const int c = e2 / w, j = e2 - c * w;
        const bool ok = e < items && (isA ? j < N : col0 + j < K);
        // fp16 X (XB 2): every load is a dword (one instruction form for A and B slots, no branch between
        // load forms -- two forms merged at a branch made the compiler wait on each batch); the lane takes
        // the half (j & 1) of the dword holding its element (ldx even: rows stay dword-aligned)
        voff[q] = ok ? (isA ? (uint32_t)AB * (uint32_t)(8 * c * lddy + j) & ~3u
                            : (uint32_t)XB * (uint32_t)(8 * c * ldx + j) & ~3u)
                     : 0u;
        h16q[q] = isA ? AB == 2 : XB == 2;  // per lane (from threadIdx, not readfirstlane): a select, not a branch
        hsh[q] = (h16q[q] && ok) ? 16u * (uint32_t)(j & 1) : 0u;
        loff[q] = (isA ? 0 : TN * kB) + (j >> 4) * kB + c * 128 + (j & 15) * 8;
        r8q[q] = 8 * c;
        // wave-uniform (itemsA = 64 TN), made scalar: a resource built from a divergent value becomes a
        // readfirstlane waterfall loop per load
        const bool isAu = __builtin_amdgcn_readfirstlane(threadIdx.x + kWgThreads * q) < itemsA;
        ldq[q] = isAu ? lddy : ldx;
        eszq[q] = isAu ? (uint32_t)AB : (uint32_t)XB;
        rsq[q] = __builtin_amdgcn_make_buffer_rsrc(isAu ? (void*)baseA : (void*)baseB, (short)0,
                                                   (int)(nrows * ldq[q] * eszq[q]), 0x00020000);
    }
    float raw[kPer][8];
    // Every operand register of a staging load stays untouched until that load has completed (DESIGN.md
    // section 4, "The k_wgrad_rect zeros": a buffer load reads the operands of its last quarter-wave after
    // the wave has gone on, and a register rewritten in that window -- the compiler reuses a load's address
    // or offset register as soon as the load has issued -- gave lanes 48-63 zeros).  So: the lane's VGPR
    // offset ob[q] is advanced IN PLACE one step at a time, just before the next batch (by then the
    // previous batch has landed: its values were converted and stored); the row strides i ld are scalar
    // offsets built once; ob, the strides and the resources are held live to the end of the kernel.
    // x2 (235 VGPRs of accumulators and pieces): one VGPR offset per slot plus eight scalar row offsets
    // i ld 4; x3 / f16 (VGPR room, and the scalar form spilled SGPRs in the f16 kernels -- a reloaded
    // spill is a fresh temporary, rewritten right after the load): one VGPR offset per (slot, row i),
    // each advanced in place.  tools/check_wgrad_operands.py checks the ISA of every instantiation.
    constexpr bool kSOff = P == P_X2;  // (x2 never has fp16 operands)
    constexpr int kNv = kSOff ? 1 : 8;
    uint32_t ob[kPer][kNv], sri[kPer][8];
#pragma unroll
    for (int q = 0; q < kPer; q++) {
#pragma unroll
        for (int i = 0; i < kNv; i++) ob[q][i] = voff[q] + eszq[q] * (uint32_t)(i * ldq[q]);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if constexpr (kSOff) asm volatile("s_mul_i32 %0, %1, %2" : "=s"(sri[q][i]) : "s"(ldq[q]), "n"(4 * i));
            else sri[q][i] = 0u;
        }
    }
    auto hold_operands = [&]() {
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            asm volatile("" ::"s"(rsq[q]));
#pragma unroll
            for (int i = 0; i < kNv; i++) asm volatile("" ::"v"(ob[q][i]));
            if constexpr (kSOff) {
#pragma unroll
                for (int i = 0; i < 8; i++) asm volatile("" ::"s"(sri[q][i]));
            }
        }
    };
    auto load_piece = [&](int q, int r0) {  // rows r0 + 8c .. + 7 of the slice; r0 = 0, 32, 64, .. in turn
        const int ld = ldq[q];
        if (r0 > 0) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < kNv; i++)
                asm volatile("v_add_u32 %0, %0, %1" : "+v"(ob[q][i]) : "s"(32 * (int)eszq[q] * ld));
        }
        if (r0 + 32 <= nrows) {  // a whole step inside the slice (wave-uniform)
#pragma unroll
            for (int i = 0; i < 8; i++) {
#ifdef WG_NO_GLOAD  // diagnostic builds only: no global loads
                raw[q][i] = (float)(r0 + i);
#else
                {
                    const uint32_t d = __builtin_amdgcn_raw_buffer_load_b32(rsq[q], ob[q][kSOff ? 0 : i], sri[q][i], 0);
                    raw[q][i] = __uint_as_float(d);  // (fp16 X: the dword's bits; converted where consumed)
                }
#endif
            }
        } else {  // the slice's last, partial step: rows past the slice read its first element, zeroed; these
                  // loads' offsets are temporaries, so they are waited for here (once per slice at most; the
                  // previous batch has landed -- it was converted and stored just before -- so nothing is in
                  // flight while the temporaries live: the markers let tools/check_wgrad_operands.py skip them)
            asm volatile(";;wg-partial-begin");
            const int lim = nrows - r0 - r8q[q];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t o = i < lim ? ob[q][0] + eszq[q] * i * ld : 0u;
                const uint32_t d = __builtin_amdgcn_raw_buffer_load_b32(rsq[q], o, 0, 0);
                raw[q][i] = i < lim ? __uint_as_float(d) : 0.f;  // (fp16 X: bits, converted where consumed; 0 -> 0)
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            asm volatile(";;wg-partial-end");
        }
    };
    auto store_piece_q = [&](int q, uint16_t* dst_set) {
        if (threadIdx.x + kWgThreads * q < items) {
            const bool isA = threadIdx.x + kWgThreads * q < itemsA;
            if constexpr (k16) {  // the fp16 halves of the loaded dwords, here where they are consumed (a
                                  // conversion right after the load would wait for it there)
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = wg_val16(__float_as_uint(raw[q][i]), hsh[q], h16q[q]);
                store_piece<P>(v, isA ? dscale : 1.f, reinterpret_cast<uint4*>(dst_set + loff[q]));
            } else {
                store_piece<P>(raw[q], isA ? dscale : 1.f, reinterpret_cast<uint4*>(dst_set + loff[q]));
            }
        }
    };
    auto frag = [&](const uint16_t* tile, bf16x8 (&f)[3]) { wg_img_frag<np>(tile, lane, f); };

    f32x4 acc[RN * NTK + EX], accx[RN * NTK + EX];
#pragma unroll
    for (int u = 0; u < RN * NTK + EX; u++) acc[u] = accx[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (nrows + 31) / 32;
#pragma unroll
    for (int q = 0; q < kPer; q++) load_piece(q, 0);
#pragma unroll
    for (int q = 0; q < kPer; q++) store_piece_q(q, img);
    if (nsteps > 1) {
#pragma unroll
        for (int q = 0; q < kPer; q++) load_piece(q, 32);
    }
    wg_barrier<false>();
    // conversion of the next step's pieces: piece q at slot q * kEvery of the tile loop (VALU beside the
    // MFMAs), the rest after it
    constexpr int kSlots = (RN > 0 ? NTK : 0) + EX;
    constexpr int kEvery = kSlots >= kPer ? kSlots / kPer : 1;
    // fp16 (cheap conversion, short MFMA phase): all after the MFMAs, so the loads issued at the end of the
    // previous step get the whole MFMA phase to arrive (measured: 264 x 460 415 -> 366 us; x3: 765 -> 788)
#if !defined(WG_NO_MFMA) && !defined(WG_CONV_LATE)
    constexpr int kDone = P != P_X3 ? 0 : ((kSlots + kEvery - 1) / kEvery < kPer ? (kSlots + kEvery - 1) / kEvery : kPer);
#else
    constexpr int kDone = 0;
#endif
    for (int st = 0; st < nsteps; st++) {
        const uint16_t* cur = img + (st & 1) * kSet;
        uint16_t* nxt = img + ((st + 1) & 1) * kSet;
        const bool more = st + 1 < nsteps;
        auto conv_at = [&](int slot) {
            if (kDone > 0 && more && slot % kEvery == 0 && slot / kEvery < kPer) store_piece_q(slot / kEvery, nxt);
        };
        auto stage_next = [&]() {  // the next step's pieces into nxt, then the loads of the step after it
            if (more) {
#pragma unroll
                for (int q = kDone; q < kPer; q++) store_piece_q(q, nxt);
                if (st + 2 < nsteps) {
#pragma unroll
                    for (int q = 0; q < kPer; q++) load_piece(q, 32 * (st + 2));
                }
            }
        };
#ifndef WG_NO_MFMA
        if constexpr (RN > 0) {
            bf16x8 a[RN][3], b[2][3];
#pragma unroll
            for (int r = 0; r < RN; r++) frag(cur + (RN * wave + r) * kB, a[r]);
            frag(cur + TN * kB, b[0]);
#pragma unroll
            for (int tk = 0; tk < NTK; tk++) {
                if (tk + 1 < NTK) frag(cur + (TN + tk + 1) * kB, b[(tk + 1) & 1]);  // next k-tile, ahead
#pragma unroll
                for (int r = 0; r < RN; r++)
                    acc[r * NTK + tk] = mma<P>(a[r], b[tk & 1], acc[r * NTK + tk], accx[r * NTK + tk]);
                conv_at(tk);
            }
        }
#pragma unroll
        for (int e = 0; e < EX; e++) {
            int j = wave + kWgWaves * e;  // leftover tile j (clamped: a duplicate, not stored)
            j = j < kRem ? j : kRem - 1;
            const int tn = kWgWaves * RN + j / NTK, tk = j % NTK;
            bf16x8 a1[3], b1[3];
            frag(cur + tn * kB, a1);
            frag(cur + (TN + tk) * kB, b1);
            acc[RN * NTK + e] = mma<P>(a1, b1, acc[RN * NTK + e], accx[RN * NTK + e]);
            conv_at((RN > 0 ? NTK : 0) + e);
        }
#endif
        stage_next();
        wg_barrier<false>();
    }
    hold_operands();
    uint32_t rm = 0;  // the range guard (range_acc; the clamped duplicate leftover tiles included: same data)
#pragma unroll
    for (int u = 0; u < RN * NTK + EX; u++) {
        acc[u] = x2_combine<P>(acc[u], accx[u]);
        range_acc<P>(rm, acc[u]);
    }
    range_note<P>(rm);
    float* out = ws + (size_t)s * N * K;
    auto put = [&](const f32x4& v, int tn, int tk) {
        const int col = col0 + 16 * tk + (lane & 15);
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = 16 * tn + 4 * (lane >> 4) + g;
            if (row < N && col < K) out[(size_t)row * K + col] = v[g] * cscale;
        }
    };
#pragma unroll
    for (int r = 0; r < RN; r++)
#pragma unroll
        for (int tk = 0; tk < NTK; tk++) put(acc[r * NTK + tk], RN * wave + r, tk);
#pragma unroll
    for (int e = 0; e < EX; e++) {
        const int j = wave + kWgWaves * e;
        if (j < kRem) put(acc[RN * NTK + e], kWgWaves * RN + j / NTK, j % NTK);
    }
}

// ---- k_wgrad_dma ------------------------------------------------------------
// k_wgrad_dma (round 6): k_wgrad_rect<P_X2, TN, NTK> with the staging taken off the registers.
//
// Why (419,430 rows, 264 x 264; phase-removed builds timed by tools/bench_wgrad_dma.py): k_wgrad_rect takes
// ~300 us.  Alone, its MFMA phase takes ~96 us (the x2 floor, 3 f16 MFMAs per product), the operand streaming
// ~132 us (5.3 TB/s) and the conversion to fp16 planes ~71 us; the kernel runs them one after the other per
// 32-row step, with one step of loads in flight in registers.
//
// Here: the raw fp32 rows go HBM -> LDS by LDS-DMA (dma16) into TWO raw stages,
// [A: 32 rows x 16 TN][B: 32 rows x 16 NTK] row-major, so two steps' bytes are in flight.  Rows past the
// slice read past the resource's num_records and land as zeros; columns past N / K read finite neighbours
// that reach only output rows / columns that are never stored.  One fragment image (k_wgrad_rect's layout).
// Per step: the MFMAs from the image; the counted wait for this wave's DMAs of the next step; barrier; the
// conversion of the next step (the dY pieces in non-packed instructions, the X pieces by wg_conv_x); barrier;
// the freed raw stage takes the DMA of the step after next.  (The form with the dY conversion between the
// MFMAs lost: DESIGN.md section 3.)
//
// The operand rule is WgDmaPart's, but this kernel's instructions run over both operands from ONE interleaved
// index (i = wave + 8 k is a dY instruction when i < kInsA: the operand of an offset slot depends on the wave),
// so it keeps its own offset sets and issue loop: one set per raw stage, advanced in place by two steps after
// its previous DMA was waited for, the resources selected per instruction from pinned SGPRs.  The MFMA order
// per output tile and the images are k_wgrad_rect's: the same partials, bit for bit.
template <int P, int TN, int NTK>
__global__ __launch_bounds__(kWgThreads) void k_wgrad_dma(const float* __restrict__ dy, int lddy, float dscale,
                                                          const float* __restrict__ x, int ldx, int M, int N, int K,
                                                          int rows, int nslices, int ncb, float cscale,
                                                          float* __restrict__ ws) {
    static_assert(P == P_X2, "k_wgrad_dma: the x2 weight gradients (fp32 operands)");
    constexpr int kB = Prec<P>::kBlk;
    constexpr int np = Prec<P>::kPlanes;
    using R = WgRect<TN, NTK>;
    constexpr int kWA = 16 * TN, kWB = 16 * NTK;            // raw row widths (floats)
    constexpr int kRawA = 32 * kWA, kRaw = 32 * (kWA + kWB);  // floats
    constexpr int kImg = (TN + NTK) * kB;                   // uint16 per image
    constexpr int kInsA = kRawA / 256, kIns = kRaw / 256;   // 1-KiB DMA instructions per stage
    constexpr int kInsW = (kIns + kWgWaves - 1) / kWgWaves;  // per wave (max)
    constexpr int kInsWmin = kIns / kWgWaves;                // per wave (min)
    constexpr int itemsA = 64 * TN;
    constexpr int kPerA = (itemsA + kWgThreads - 1) / kWgThreads;
    static_assert((2 * kRaw * 4 + kImg * 2) <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) float raw0[kRaw];
    __shared__ __attribute__((aligned(16))) float raw1[kRaw];
    __shared__ __attribute__((aligned(16))) uint16_t img[kImg];
    const WgUnit un = wg_unit(M, rows, ncb, NTK);
    if (un.s >= nslices) return;  // the whole workgroup
    const int lane = un.lane, wave = un.wave, nrows = un.nrows;
    const __amdgpu_buffer_rsrc_t rsA = wg_slice_rsrc(dy + (size_t)un.m_begin * lddy, nrows * lddy * 4);
    const __amdgpu_buffer_rsrc_t rsB =
        wg_slice_rsrc(x + (size_t)un.m_begin * ldx + un.col0, (nrows * ldx - un.col0) * 4);

    // this wave's DMA instructions i = wave + 8 k: the lane's byte offset in the step of each offset set
    uint32_t ob[2][kInsW];
#pragma unroll
    for (int k = 0; k < kInsW; k++) {
        const int i = wave + kWgWaves * k;
        const int p = 64 * i + lane;
        const bool isA = i < kInsA;
        const int e = isA ? p : p - kRawA / 4;
        const int w4 = isA ? kWA / 4 : kWB / 4;
        const int r = e / w4, c4 = e - r * w4;
        const int ld = isA ? lddy : ldx;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            ob[t][k] = (uint32_t)(((32 * t + r) * ld + 4 * c4) * 4);
            asm volatile("" : "+v"(ob[t][k]));
        }
    }
    const uint32_t stepA = 2u * 32u * (uint32_t)lddy * 4u, stepB = 2u * 32u * (uint32_t)ldx * 4u;
    auto issue = [&](auto tc, int st) {  // the DMA of step st into raw stage T (offset set T)
        constexpr int T = decltype(tc)::value;
#ifdef WG_NO_DMA  // diagnostic builds only (wrong results): no loads
        return;
#endif
        const uint32_t base = lds_addr(T ? raw1 : raw0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < kInsW; k++) {
            const int i = wave + kWgWaves * k;  // wave-uniform
            if (i < kIns) {
                if (st >= 2) asm volatile("v_add_u32 %0, %0, %1" : "+v"(ob[T][k]) : "s"(i < kInsA ? stepA : stepB));
                dma16(i < kInsA ? rsA : rsB, ob[T][k], base + 1024u * (uint32_t)i);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto wait_stage = [&](bool later_in_flight) {
        wg_wait_stage<kInsW, kInsWmin>(wave < kIns % kWgWaves || kIns % kWgWaves == 0, later_in_flight);
    };
    // a raw stage -> the image: this thread's dY pieces (8-row chunk c, column j; scaled), then its X pieces
    auto conv = [&](const float* stage) {
#ifdef WG_NO_CONV  // diagnostic builds only (wrong results): no conversion
        return;
#endif
#pragma unroll
        for (int q = 0; q < kPerA; q++) {
            const int e = threadIdx.x + kWgThreads * q;
            if (e < itemsA) {
                const int c = e / kWA, j = e - c * kWA;
                const float* src = stage + 8 * c * kWA + j;
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = src[i * kWA];
                const int loff = (j >> 4) * kB + c * 128 + (j & 15) * 8;
                store_piece_x2_plain<true>(v, dscale, reinterpret_cast<uint4*>(img + loff));
            }
        }
        wg_conv_x<NTK>(stage + kRawA, img + TN * kB);
    };

    f32x4 acc[R::kAcc], accx[R::kAcc];
#pragma unroll
    for (int u = 0; u < R::kAcc; u++) acc[u] = accx[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (nrows + 31) / 32;
    constexpr std::integral_constant<int, 0> c0{};
    constexpr std::integral_constant<int, 1> c1{};
    issue(c0, 0);
    if (nsteps > 1) issue(c1, 1);
    wait_stage(nsteps > 1);
    wg_barrier();
    conv(raw0);
    wg_barrier();
    if (nsteps > 2) issue(c0, 2);
    auto step = [&](auto tc, int st) {  // step st; raw stage 1 - T holds step st + 1 (T = st & 1)
        constexpr int T = decltype(tc)::value;
        constexpr std::integral_constant<int, 1 - T> cn{};
#ifndef WG_NO_MFMA
        wg_rect_mfma<P, TN, NTK, false>(
            wave, [&](int tn, bf16x8(&f)[3]) { wg_img_frag<np>(img + tn * kB, lane, f); },
            [&](int tk, bf16x8(&f)[3]) { wg_img_frag<np>(img + (TN + tk) * kB, lane, f); }, acc, accx, NTK, [](int) {});
#endif
        if (st + 1 < nsteps) {
            wait_stage(st + 2 < nsteps);  // step st + 1's DMAs (this wave) landed
            wg_barrier();  // the MFMAs' reads of the image are done, and step st + 1's raw is visible
            conv(T ? raw0 : raw1);
            wg_barrier();  // the image holds step st + 1; raw stage 1 - T is free
            if (st + 3 < nsteps) issue(cn, st + 3);
        }
    };
    for (int st = 0; st < nsteps; st += 2) {
        step(c0, st);
        if (st + 1 < nsteps) step(c1, st + 1);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // (every issued DMA was waited for before its conversion)
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int k = 0; k < kInsW; k++) asm volatile("" ::"v"(ob[t][k]));
    asm volatile("" ::"s"(rsA), "s"(rsB), "s"(stepA), "s"(stepB));
    wg_store<P, TN, NTK, false>(un, acc, accx, N, K, cscale, ws);
}

// ---- k_wgrad_tr -------------------------------------------------------------
// k_wgrad_tr: k_wgrad_dma for operands stored as x2 planes (dY pre-scaled, X at scale 1; see pair1) -- there is
// nothing to convert.  The plane rows go HBM -> LDS by LDS-DMA into THREE raw stages (the bytes and the
// addresses per step are k_wgrad_dma's: a plane pair is 4 bytes per element, a 16-byte piece one column group),
// and the MFMA fragments are read straight from the raw stage (wg_tr_frag) -- exactly the fragment
// k_wgrad_dma's image holds, so with the same MFMA order per output tile (wg_rect_mfma, mma<P_X2>) the partials
// are its partials, bit for bit.  No image, no conversion; per step one counted vmcnt wait for this wave's DMAs
// of that step, ONE barrier (the step's stage visible; the stage of the step before free), the DMA of the step
// after next.
//
// A stage: [A: 32 rows of pitch wpA][B: 32 rows of pitch wpB] in 16-byte pieces, a row holding 4 T pieces (T
// the operand's tiles) of [4 hi halves][4 lo halves]; wp = 4 T rounded up to 4 mod 16.  Bank rule of the
// transposed read (64 banks of 4 bytes, conflicts inside a 32-lane half = row groups c, c + 1): lane 4 q + p
// reads 8 bytes of row q at piece p of the tile, so a plane's read touches only every other 8 bytes -- 32 of
// the 64 banks -- and two cycles per half are the least this layout allows.  A pitch of 16 mod 64 dwords
// reaches that: the four rows q of a block take banks 16 q .. 16 q + 15, and rows r and r + 8 the same ones.
// (Hi and lo in separate LDS rows would read at one cycle, but then a GEMM lane's hi and lo halves lie a row
// apart in global memory; the stream hides the second cycle here.)
// Both operands' parts are whole DMA instructions (32 wp pieces, wp % 4 == 0), so an instruction reads one
// operand.  Columns past an operand's width read the neighbouring row (or zeros past num_records): whatever
// they hold -- NaN patterns included -- reaches only output rows >= N / columns >= K, which are neither
// stored nor range-checked.  Rows past the slice arrive as zeros through num_records, for both planes (a piece
// holds both).  One WgDmaPart per operand, three offset sets each.
constexpr int tr_pitch(int T) {  // 16-byte pieces per staged row
    int w = 4 * T;
    while (w % 16 != 4) w++;
    return w;
}

template <int TN, int NTK>
__global__ __launch_bounds__(kWgThreads) void k_wgrad_tr(const uint32_t* __restrict__ dy, int lddy,
                                                         const uint32_t* __restrict__ x, int ldx, int M, int N, int K,
                                                         int rows, int nslices, int ncb, float cscale,
                                                         float* __restrict__ ws) {
    constexpr int P = P_X2;
    using R = WgRect<TN, NTK>;
    constexpr int wpA = tr_pitch(TN), wpB = tr_pitch(NTK);  // row pitches, pieces
    constexpr int kSecA = 32 * wpA, kSecB = 32 * wpB;      // an operand's part of a stage
    static_assert(kSecA % 64 == 0 && kSecB % 64 == 0, "parts of whole DMA instructions");
    constexpr int kInsA = kSecA / 64, kInsB = kSecB / 64;  // DMA instructions per part
    constexpr int kStage = kSecA + kSecB;                  // pieces
    constexpr int kStages = 3;
    static_assert(kStages * kStage * 16 <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) uint4 raw[kStages * kStage];
    const WgUnit un = wg_unit(M, rows, ncb, NTK);
    if (un.s >= nslices) return;  // the whole workgroup
    const int lane = un.lane, wave = un.wave, nrows = un.nrows;
    const __amdgpu_buffer_rsrc_t rsA = wg_slice_rsrc(dy + (size_t)un.m_begin * lddy, nrows * lddy * 4);
    const __amdgpu_buffer_rsrc_t rsB =
        wg_slice_rsrc(x + (size_t)un.m_begin * ldx + un.col0, (nrows * ldx - un.col0) * 4);

    using PartA = WgDmaPart<kInsA, kStages>;
    using PartB = WgDmaPart<kInsB, kStages>;
    PartA dA;
    PartB dB;
    dA.init(wave, [&](int j, int t) { return wg_row_off<wpA, TN>(j, lane, t, lddy); });
    dB.init(wave, [&](int j, int t) { return wg_row_off<wpB, NTK>(j, lane, t, ldx); });
    const uint32_t stepA = (uint32_t)kStages * 32u * (uint32_t)lddy * 4u, stepB = (uint32_t)kStages * 32u * (uint32_t)ldx * 4u;
    auto issue = [&](auto tc, int st) {  // the DMA of step st into raw stage T (offset sets T)
        constexpr int T = decltype(tc)::value;
        const uint32_t base = lds_addr(raw + T * kStage);
        __builtin_amdgcn_sched_barrier(0);
        dA.template issue<T>(rsA, base, wave, st, stepA);
        dB.template issue<T>(rsB, base + 16u * (uint32_t)kSecA, wave, st, stepB);
        __builtin_amdgcn_sched_barrier(0);
    };
    // instructions per wave and step: the count a wave may leave in flight (the next step's)
    constexpr int kRemA = kInsA % kWgWaves, kRemB = kInsB % kWgWaves;
    static_assert(kRemA == kRemB && kRemA != 0, "waves below kRemA issue one more instruction of each operand");
    constexpr int kInsW = PartA::kSlots + PartB::kSlots, kInsWmin = kInsW - 2;
    const uint32_t laneA = wg_tr_lane<wpA>(lane, 0), laneB = wg_tr_lane<wpB>(lane, kSecA);  // bytes

    f32x4 acc[R::kAcc], accx[R::kAcc];
#pragma unroll
    for (int u = 0; u < R::kAcc; u++) acc[u] = accx[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (nrows + 31) / 32;
    constexpr std::integral_constant<int, 0> c0{};
    constexpr std::integral_constant<int, 1> c1{};
    constexpr std::integral_constant<int, 2> c2{};
    issue(c0, 0);
    if (nsteps > 1) issue(c1, 1);
    auto step = [&](auto tcur, auto tnext2, int st) {  // step st in stage T; step st + 2 goes to stage (T + 2) % 3
        constexpr int T = decltype(tcur)::value;
        wg_wait_stage<kInsW, kInsWmin>(wave < kRemA, st + 1 < nsteps);  // this wave's DMAs of step st landed
        wg_barrier();  // every wave's DMAs of the step visible; this wave's LDS reads of the step before done
        if (st + 2 < nsteps) issue(tnext2, st + 2);
        const char* stage = reinterpret_cast<const char*>(raw + T * kStage);
        wg_rect_mfma<P, TN, NTK, false>(
            wave, [&](int tn, bf16x8(&f)[3]) { wg_tr_frag<wpA>(stage, laneA, tn, f); },
            [&](int tk, bf16x8(&f)[3]) { wg_tr_frag<wpB>(stage, laneB, tk, f); }, acc, accx, NTK, [](int) {});
    };
    for (int st = 0; st < nsteps; st += 3) {
        step(c0, c2, st);
        if (st + 1 < nsteps) step(c1, c0, st + 1);
        if (st + 2 < nsteps) step(c2, c1, st + 2);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // (every issued DMA was waited for before its step)
    dA.hold(rsA, stepA);
    dB.hold(rsB, stepB);
    wg_store<P, TN, NTK, true>(un, acc, accx, N, K, cscale, ws);
}

// ---- k_wgrad_mix ------------------------------------------------------------
// k_wgrad_mix: k_wgrad_dma for dY stored as pre-scaled x2 planes beside an fp32 X (the first trunk layer:
// dW1 = dY1^T h0, 264 x 460, where h0 has no plane form).  k_wgrad_dma's plan, tile runs and MFMA order per
// output tile (wg_rect_mfma); the dY side is k_wgrad_tr's (plane rows by LDS-DMA at pitch tr_pitch(TN), A
// fragments straight from the raw stage by wg_tr_frag: nothing converted, no image part -- under k_wgrad_dma
// every one of the ncb column blocks converted the whole dY step again), the X side k_wgrad_dma's (raw fp32
// rows by LDS-DMA, wg_conv_x into an image of NTK tiles).  The fragments are the ones k_wgrad_dma's image
// holds (see wg_tr_frag), so the partials are its partials, bit for bit.
//
// LDS: two dY stages (32 rows of pitch wpA pieces) and two raw X stages (32 rows x 16 NTK floats), 2 x (34,816
// + 16,384) bytes at <17, 8>, and TWO X images (135,168 bytes in all): X runs one step further ahead than dY,
// and step st + 1's X is converted into the other image after the first k-tile's MFMAs of step st.  ONE barrier
// per step: before it the wave waited for all its DMAs (vmcnt(0)), so after it dY of step st, the raw X of step
// st + 1 and the image of step st are visible, and every wave is past step st - 1 (its A fragments read, its
// image read, its conversion's raw X read) -- free for dY of step st + 1, the raw X of step st + 2 and the
// conversion of step st + 1.  (Measured against the one-image form and k_wgrad_dma: DESIGN.md section 3, "dY1
// as planes".)  A column block's k-tiles wholly past K (the last block's three at K = 460) are skipped: they
// are never stored.  One WgDmaPart per operand, two offset sets each.  The range guard runs over the stored
// accumulators only (columns past N / K may hold anything, NaN patterns of a pitch padding included).
template <int TN, int NTK>
__global__ __launch_bounds__(kWgThreads) void k_wgrad_mix(const uint32_t* __restrict__ dy, int lddy,
                                                          const float* __restrict__ x, int ldx, int M, int N, int K,
                                                          int rows, int nslices, int ncb, float cscale,
                                                          float* __restrict__ ws) {
    constexpr int P = P_X2;
    constexpr int kB = Prec<P>::kBlk;
    using R = WgRect<TN, NTK>;
    constexpr int wpA = tr_pitch(TN);                    // dY row pitch, pieces
    constexpr int kWB = 16 * NTK;                        // X raw row width (floats)
    constexpr int kSecA = 32 * wpA, kSecB = 32 * kWB / 4;  // an operand's part of a stage, pieces
    static_assert(kSecA % 64 == 0 && kSecB % 64 == 0, "parts of whole DMA instructions");
    constexpr int kInsA = kSecA / 64, kInsB = kSecB / 64;  // DMA instructions per part
    constexpr int kImg = NTK * kB;                         // uint16
    static_assert(2 * (kSecA + kSecB) * 16 + 2 * kImg * 2 <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) uint4 rawA[2 * kSecA];
    __shared__ __attribute__((aligned(16))) uint4 rawB[2 * kSecB];
    __shared__ __attribute__((aligned(16))) uint16_t img[2 * kImg];
    const WgUnit un = wg_unit(M, rows, ncb, NTK);
    if (un.s >= nslices) return;  // the whole workgroup
    const int lane = un.lane, wave = un.wave, nrows = un.nrows;
    const int live = min(NTK, (K - un.col0 + 15) / 16);  // the block's k-tiles that reach a stored column
    const __amdgpu_buffer_rsrc_t rsA = wg_slice_rsrc(dy + (size_t)un.m_begin * lddy, nrows * lddy * 4);
    const __amdgpu_buffer_rsrc_t rsB =
        wg_slice_rsrc(x + (size_t)un.m_begin * ldx + un.col0, (nrows * ldx - un.col0) * 4);

    WgDmaPart<kInsA, 2> dA;  // dY's plane rows (the row padding: out of range)
    WgDmaPart<kInsB, 2> dB;  // X's fp32 rows, 4 NTK pieces wide
    dA.init(wave, [&](int j, int t) { return wg_row_off<wpA, TN>(j, lane, t, lddy); });
    dB.init(wave, [&](int j, int t) { return wg_row_off<kWB / 4, NTK>(j, lane, t, ldx); });
    const uint32_t stepA = 2u * 32u * (uint32_t)lddy * 4u, stepB = 2u * 32u * (uint32_t)ldx * 4u;
    auto issueA = [&](auto tc, int st) {  // the DMA of step st's dY rows into dY stage T
        constexpr int T = decltype(tc)::value;
        __builtin_amdgcn_sched_barrier(0);
        dA.template issue<T>(rsA, lds_addr(rawA + T * kSecA), wave, st, stepA);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto issueB = [&](auto tc, int st) {  // ... of its X rows into X stage T
        constexpr int T = decltype(tc)::value;
        __builtin_amdgcn_sched_barrier(0);
        dB.template issue<T>(rsB, lds_addr(rawB + T * kSecB), wave, st, stepB);
        __builtin_amdgcn_sched_barrier(0);
    };
    const uint32_t laneA = wg_tr_lane<wpA>(lane, 0);  // bytes

    f32x4 acc[R::kAcc], accx[R::kAcc];
#pragma unroll
    for (int u = 0; u < R::kAcc; u++) acc[u] = accx[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (nrows + 31) / 32;
    constexpr std::integral_constant<int, 0> c0{};
    constexpr std::integral_constant<int, 1> c1{};
    issueA(c0, 0);
    issueB(c0, 0);
    if (nsteps > 1) issueB(c1, 1);
    wg_wait_all();
    wg_barrier();
    wg_conv_x<NTK>(reinterpret_cast<const float*>(rawB), img);
    auto step = [&](auto tcur, int st) {  // step st: dY stage, image T = st & 1; raw X stage 1 - T holds step st + 1
        constexpr int T = decltype(tcur)::value;
        constexpr std::integral_constant<int, 1 - T> cn{};
        wg_barrier();
        if (st + 1 < nsteps) issueA(cn, st + 1);
        if (st + 2 < nsteps) issueB(tcur, st + 2);
        const char* stage = reinterpret_cast<const char*>(rawA + T * kSecA);
        const uint16_t* im = img + T * kImg;
        wg_rect_mfma<P, TN, NTK, true>(
            wave, [&](int tn, bf16x8(&f)[3]) { wg_tr_frag<wpA>(stage, laneA, tn, f); },
            [&](int tk, bf16x8(&f)[3]) { wg_img_frag<2>(im + tk * kB, lane, f); }, acc, accx, live, [&](int slot) {
                if (slot == 0 && st + 1 < nsteps)
                    wg_conv_x<NTK>(reinterpret_cast<const float*>(rawB + (1 - T) * kSecB), img + (1 - T) * kImg);
            });
        wg_wait_all();  // this wave's DMAs of dY (step st + 1) and X (step st + 2) landed
    };
    for (int st = 0; st < nsteps; st += 2) {
        step(c0, st);
        if (st + 1 < nsteps) step(c1, st + 1);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // (every issued DMA was waited for before its step)
    dA.hold(rsA, stepA);
    dB.hold(rsB, stepB);
    wg_store<P, TN, NTK, true>(un, acc, accx, N, K, cscale, ws);
}

// out[e] = sum over the row slices s of ws[s][e]: 16 groups of consecutive slices per element, each group's
// loads all in flight (the plain per-element loop over S = 256 slices was latency-bound: ~90 us), the
// groups then summed in order -- a fixed order, so the result is deterministic
__global__ __launch_bounds__(256) void k_wg_reduce(const float* __restrict__ ws, int S, long n,
                                                   float* __restrict__ out) {
    __shared__ float red[16][17];
    const int el = threadIdx.x & 15, g = threadIdx.x >> 4;
    const long e = blockIdx.x * 16L + el;
    const int per = (S + 15) / 16, s0 = g * per, s1 = min(S, s0 + per);
    float a = 0.f;
    if (e < n) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = s0 + i < s1 ? ws[(long)(s0 + i) * n + e] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) a += v[i];
        for (int t = s0 + 16; t < s1; t++) a += ws[(long)t * n + e];  // S > 256
    }
    red[g][el] = a;
    __syncthreads();
    if (g == 0 && e < n) {
        float t = red[0][el];
#pragma unroll
        for (int k = 1; k < 16; k++) t += red[k][el];
        out[e] = t;
    }
}
