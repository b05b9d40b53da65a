// eval_kernels.hip -- policy evaluation on MI355X (gfx950): the episode totals.  (The actions of an evaluation
// run come from the rollout's own kernels, k_head_act / k_act in rl_kernels.hip, in either mode.)
//
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

namespace mm {

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
