// eval_kernels.hip -- policy evaluation on MI355X (gfx950).
//
//   k_head_act   the actor's two heads fused with the action choice, with a mode: MM_ACT_SAMPLE draws like
//                k_head_sample (rl_kernels.hip), MM_ACT_GREEDY takes the most likely action (greedy_row,
//                policy_device.h).  k_head_sample's row layout -- 8 lanes per row, the same per-lane fma order
//                and butterfly, head weights in LDS -- so the logits equal mm_heads_fwd's and
//                mm_head_sample_ex's bit for bit, and MM_ACT_SAMPLE reproduces mm_head_sample_ex.
//   k_act        the same choice from given logits (the logits-input sibling of k_sample).
//   k_eval_init / k_eval_accum  episode totals of an evaluation run: one thread per maze, one launch per env
//                step.  Every maze contributes its first `quota` episodes and no more, so mazes that finish
//                fast are not over-represented.  Every total is an integer (sums, min, max, a histogram of
//                len / shortest in quarter steps): exact, and independent of the order in which the
//                workgroups arrive.  Per workgroup the words are reduced with wavefront shuffles and LDS
//                atomics (the histogram in LDS), then one global atomic per non-empty word.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "marlmaze.h"
#include "policy_device.h"

namespace mm {

template <int MODE>
__device__ __forceinline__ float act_row(const float l[5], float kl, const uint8_t* __restrict__ mk, int row,
                                         uint64_t seed, uint64_t off, int& move, int& mark) {
    if constexpr (MODE == MM_ACT_GREEDY) return greedy_row(l, kl, mk, move, mark);
    else return sample_row(l, kl, mk, row, seed, off, move, mark);
}

// One thread per maze: rows 2i (agent 0) and 2i+1 (agent 1), as k_sample.
template <int MODE>
__global__ void k_act(const float* __restrict__ ml, const float* __restrict__ kl, const uint8_t* __restrict__ masks,
                      int M, uint64_t seed, uint64_t offset, int8_t* __restrict__ act, float* __restrict__ logp,
                      float* __restrict__ joint) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nm = (M + 1) / 2;
    if (i >= nm) return;
    float jl = 0.f;
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int row = 2 * i + a;
        if (row >= M) break;
        float l[5];
#pragma unroll
        for (int j = 0; j < 5; j++) l[j] = ml[(size_t)row * 5 + j];
        int move, mark;
        const float lp = act_row<MODE>(l, kl[row], masks + (size_t)row * MM_MASK_DIM, row, seed, offset, move, mark);
        act[2 * row] = (int8_t)move;
        act[2 * row + 1] = (int8_t)mark;
        if (logp) logp[row] = lp;
        jl += lp;
    }
    if (joint) joint[i] = jl;
}

// k_head_sample's constants and row layout (rl_kernels.hip): 8 lanes per row, each lane a 4-column stride of
// the row, 32 rows = 16 mazes per 256-thread workgroup.
constexpr int kHaLanes = 8;
constexpr int kHaRows = 32;
constexpr int kHaMaxK = 1024;

template <int MODE>
__global__ __launch_bounds__(kHaLanes* kHaRows) void k_head_act(const float* __restrict__ h, int ldh, int K,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ b,
                                                                const uint8_t* __restrict__ masks, int M,
                                                                uint64_t seed, uint64_t offset,
                                                                const uint64_t* __restrict__ offset_dev,
                                                                int8_t* __restrict__ act, float* __restrict__ logp,
                                                                float* __restrict__ joint,
                                                                float* __restrict__ logits) {
    __shared__ __attribute__((aligned(16))) float W[6 * kHaMaxK];
    constexpr int kB = 8;  // loads batched ahead of the LDS writes
    for (int e0 = threadIdx.x; e0 < 6 * K; e0 += kB * blockDim.x) {
        float t[kB];
#pragma unroll
        for (int u = 0; u < kB; u++) {
            const int e = e0 + u * blockDim.x;
            t[u] = e < 6 * K ? w[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kB; u++) {
            const int e = e0 + u * blockDim.x;
            if (e < 6 * K) W[e] = t[u];
        }
    }
    __syncthreads();
    const int j = threadIdx.x % kHaLanes;
    const int row = blockIdx.x * kHaRows + threadIdx.x / kHaLanes;
    const bool valid = row < M;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const float* hr = h + (size_t)row * ldh;
        for (int c = 4 * j; c < K; c += 4 * kHaLanes) {
            const float4 hv = *reinterpret_cast<const float4*>(hr + c);
#pragma unroll
            for (int o = 0; o < 6; o++) {
                const float4 wv = *reinterpret_cast<const float4*>(W + o * K + c);
                acc[o] = fmaf(hv.x, wv.x, acc[o]);
                acc[o] = fmaf(hv.y, wv.y, acc[o]);
                acc[o] = fmaf(hv.z, wv.z, acc[o]);
                acc[o] = fmaf(hv.w, wv.w, acc[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 6; o++) {  // butterfly over the row's 8 lanes: every lane holds the sums
#pragma unroll
        for (int d = kHaLanes / 2; d > 0; d >>= 1) acc[o] += __shfl_xor(acc[o], d);
    }
    float lp = 0.f;
    if (valid && j == 0) {
        float l[5];
#pragma unroll
        for (int o = 0; o < 5; o++) l[o] = acc[o] + b[o];
        const float kl = acc[5] + b[5];
        int move, mark;
        uint64_t off = offset;
        if constexpr (MODE == MM_ACT_SAMPLE) off += offset_dev ? *offset_dev : 0ull;
        lp = act_row<MODE>(l, kl, masks + (size_t)row * MM_MASK_DIM, row, seed, off, move, mark);
        act[2 * row] = (int8_t)move;
        act[2 * row + 1] = (int8_t)mark;
        if (logp) logp[row] = lp;
        if (logits) {
#pragma unroll
            for (int o = 0; o < 5; o++) logits[(size_t)row * 6 + o] = l[o];
            logits[(size_t)row * 6 + 5] = kl;
        }
    }
    // joint log-prob of maze row/2: rows 2i and 2i+1 are adjacent 8-lane groups
    const float other = __shfl_down(lp, kHaLanes);
    if (joint && valid && j == 0 && (row & 1) == 0) joint[row >> 1] = lp + (row + 1 < M ? other : 0.f);
}

// ---------------------------------------------------------------------------
// episode totals
// ---------------------------------------------------------------------------
typedef unsigned long long u64;
constexpr int kEvThreads = 256;
constexpr u64 kEvNone = ~0ull;  // the min word before any solved episode

__global__ void k_eval_init(u64* __restrict__ totals, int32_t* __restrict__ counted, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counted[i] = 0;
    if (i < MM_EVAL_WORDS) totals[i] = i == MM_EV_MIN_LEN_SOLVED ? kEvNone : 0ull;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}

__global__ __launch_bounds__(kEvThreads) void k_eval_accum(const uint8_t* __restrict__ done,
                                                           const float* __restrict__ reward,
                                                           const int2* __restrict__ ep_stats, int n, int quota,
                                                           int32_t* __restrict__ counted, u64* __restrict__ totals) {
    __shared__ u64 s[MM_EV_HIST0];               // the scalar words of this workgroup
    __shared__ unsigned int hist[MM_EV_HIST_BINS];  // (<= 256 episodes per workgroup and launch)
    const int tid = threadIdx.x, m = blockIdx.x * kEvThreads + tid;
    if (tid < MM_EV_HIST0) s[tid] = tid == MM_EV_MIN_LEN_SOLVED ? kEvNone : 0ull;
    if (tid < MM_EV_HIST_BINS) hist[tid] = 0u;
    __syncthreads();
    bool ev = false;
    if (m < n && done[m] != 0) {
        const int32_t c = counted[m];
        if (c < quota) {
            counted[m] = c + 1;
            ev = true;
        }
    }
    if (__any(ev)) {  // wave-uniform: most waves of most steps hold no episode end
        u64 solved = 0, len = 0, len_s = 0, short_s = 0, ratio = 0, bad = 0, mn = kEvNone, mx = 0;
        if (ev) {
            const int2 st = ep_stats[m];  // (length, shortest_path_len): k_step's pair
            len = (u64)(int64_t)st.x;
            if (reward[m] == 1.0f) {
                solved = 1;
                len_s = mn = mx = len;
                short_s = (u64)(int64_t)st.y;
                if (st.y <= 0) {
                    bad = 1;
                } else {
                    ratio = (len << 16) / (u64)st.y;  // floor(len 65536 / shortest)
                    const int64_t bin = (int64_t)(4 * (int64_t)st.x / (int64_t)st.y) - 4;
                    atomicAdd(&hist[bin < 0 ? 0 : bin > MM_EV_HIST_BINS - 1 ? MM_EV_HIST_BINS - 1 : (int)bin], 1u);
                }
            }
        }
        const u64 episodes = wave_sum(ev ? 1ull : 0ull);
        solved = wave_sum(solved);
        len = wave_sum(len);
        len_s = wave_sum(len_s);
        short_s = wave_sum(short_s);
        ratio = wave_sum(ratio);
        bad = wave_sum(bad);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const u64 a = __shfl_down(mn, d), b = __shfl_down(mx, d);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if ((tid & 63) == 0) {
            atomicAdd(&s[MM_EV_EPISODES], episodes);
            atomicAdd(&s[MM_EV_SOLVED], solved);
            atomicAdd(&s[MM_EV_TIMEOUTS], episodes - solved);
            atomicAdd(&s[MM_EV_SUM_LEN], len);
            atomicAdd(&s[MM_EV_SUM_LEN_SOLVED], len_s);
            atomicAdd(&s[MM_EV_SUM_SHORT_SOLVED], short_s);
            atomicAdd(&s[MM_EV_SUM_RATIO_Q16], ratio);
            atomicAdd(&s[MM_EV_BAD_SHORT], bad);
            atomicMin(&s[MM_EV_MIN_LEN_SOLVED], mn);
            atomicMax(&s[MM_EV_MAX_LEN_SOLVED], mx);
        }
    }
    __syncthreads();
    // one global atomic per word that this workgroup changed
    if (tid < MM_EV_HIST0) {
        const u64 v = s[tid];
        if (tid == MM_EV_MIN_LEN_SOLVED) {
            if (v != kEvNone) atomicMin(&totals[tid], v);
        } else if (tid == MM_EV_MAX_LEN_SOLVED) {
            if (v != 0) atomicMax(&totals[tid], v);
        } else if (v != 0) {
            atomicAdd(&totals[tid], v);
        }
    } else if (tid < MM_EVAL_WORDS) {
        const unsigned int v = hist[tid - MM_EV_HIST0];
        if (v != 0) atomicAdd(&totals[tid], (u64)v);
    }
}

}  // namespace mm

using namespace mm;

static bool act_mode_ok(int mode) { return mode == MM_ACT_SAMPLE || mode == MM_ACT_GREEDY; }

extern "C" int mm_act(const float* move_logits, const float* mark_logits, const uint8_t* masks, int M, int mode,
                      uint64_t seed, uint64_t offset, int8_t* actions, float* logp, float* joint_logp, void* stream) {
    if (!move_logits || !mark_logits || !masks || !actions || M < 0 || !act_mode_ok(mode)) return MM_E_ARG;
    if (M == 0) return 0;
    const int nm = (M + 1) / 2;
    const dim3 grid((nm + 255) / 256), block(256);
    if (mode == MM_ACT_GREEDY)
        hipLaunchKernelGGL(k_act<MM_ACT_GREEDY>, grid, block, 0, (hipStream_t)stream, move_logits, mark_logits, masks,
                           M, seed, offset, actions, logp, joint_logp);
    else
        hipLaunchKernelGGL(k_act<MM_ACT_SAMPLE>, grid, block, 0, (hipStream_t)stream, move_logits, mark_logits, masks,
                           M, seed, offset, actions, logp, joint_logp);
    return (int)hipGetLastError();
}

extern "C" int mm_head_act(const float* h, int ldh, int K, const float* w, const float* b, const uint8_t* masks,
                           int M, int mode, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                           int8_t* actions, float* logp, float* joint_logp, float* logits, void* stream) {
    if (!h || !w || !b || !masks || !actions || M < 0 || K <= 0 || (K & 3) || K > kHaMaxK || ldh < K || (ldh & 3) ||
        ((uintptr_t)h & 15) || !act_mode_ok(mode))
        return MM_E_ARG;
    if (M == 0) return 0;
    const dim3 grid((M + kHaRows - 1) / kHaRows), block(kHaLanes * kHaRows);
    if (mode == MM_ACT_GREEDY)
        hipLaunchKernelGGL(k_head_act<MM_ACT_GREEDY>, grid, block, 0, (hipStream_t)stream, h, ldh, K, w, b, masks, M,
                           seed, offset, offset_dev, actions, logp, joint_logp, logits);
    else
        hipLaunchKernelGGL(k_head_act<MM_ACT_SAMPLE>, grid, block, 0, (hipStream_t)stream, h, ldh, K, w, b, masks, M,
                           seed, offset, offset_dev, actions, logp, joint_logp, logits);
    return (int)hipGetLastError();
}

extern "C" int mm_eval_init(uint64_t* totals, int32_t* counted, int n, void* stream) {
    if (!totals || !counted || n < 0 || ((uintptr_t)totals & 7)) return MM_E_ARG;
    const int threads = n > MM_EVAL_WORDS ? n : MM_EVAL_WORDS;
    hipLaunchKernelGGL(k_eval_init, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<u64*>(totals), counted, n);
    return (int)hipGetLastError();
}

extern "C" int mm_eval_accum(const uint8_t* done, const float* reward, const int32_t* ep_stats, int n, int quota,
                             int32_t* counted, uint64_t* totals, void* stream) {
    if (!done || !reward || !ep_stats || !counted || !totals || n < 0 || quota < 0 || ((uintptr_t)ep_stats & 7) ||
        ((uintptr_t)totals & 7))
        return MM_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_eval_accum, dim3((n + kEvThreads - 1) / kEvThreads), dim3(kEvThreads), 0,
                       (hipStream_t)stream, done, reward, reinterpret_cast<const int2*>(ep_stats), n, quota, counted,
                       reinterpret_cast<u64*>(totals));
    return (int)hipGetLastError();
}
