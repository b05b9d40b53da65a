// eval_kernels.hip -- policy evaluation on MI355X (gfx950): the episode totals and the totals against par.  (The
// actions of an evaluation run come from the rollout's own kernels, k_head_act / k_act in rl_kernels.hip, in
// either mode; the par times come from k_env_par in solve_kernels.hip.)
//
//   k_eval_init / k_eval_accum  episode totals of an evaluation run: one thread per maze, one launch per env
//                step.  Every maze contributes its first `quota` episodes and no more (quota_device.h).  Every
//                total is an integer (sums, min, max, a histogram of len / shortest in quarter steps): exact,
//                and independent of the order in which the workgroups arrive.
//   k_par_init / k_par_accum    the same for the exit time of the solved episodes against the par time of their
//                maze (mm_env_par's rows), on a `counted` array of its own.
//
// Both accumulate kernels are one skeleton (TotalsLds, totals_* and wave_reduce below): the 16 scalar words and
// the 16 histogram bins of the workgroup are staged in LDS, every wavefront that holds an event reduces its
// lanes' contributions word by word with shuffles and lane 0 adds them with LDS atomics (the histogram is bumped
// in LDS by the lanes themselves), then one global atomic per non-empty word.  What differs is what a lane
// contributes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "marlmaze.h"
#include "quota_device.h"

namespace mm {

typedef unsigned long long u64;
constexpr int kTotThreads = 256;
constexpr int kTotScalars = 16, kTotBins = 16;  // the scalar words, then the histogram: both sets of totals
static_assert(MM_EV_HIST0 == kTotScalars && MM_EV_HIST_BINS == kTotBins && MM_EVAL_WORDS == kTotScalars + kTotBins &&
                  MM_PAR_HIST0 == kTotScalars && MM_PAR_HIST_BINS == kTotBins && MM_PAR_WORDS == kTotScalars + kTotBins,
              "k_eval_accum and k_par_accum share one layout of their 32 words");
constexpr u64 kTotNone = ~0ull;  // a min word before anything entered it
constexpr int kNoWord = -1;      // "these totals have no min word"

template <class Op>
__device__ __forceinline__ u64 wave_reduce(u64 v, Op op) {  // lane 0 ends with the wavefront's
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_down(v, d));
    return v;
}

// counted = 0, totals = 0, the min word (if any) = kTotNone
__device__ __forceinline__ void totals_init(u64* __restrict__ totals, int32_t* __restrict__ counted, int n,
                                            int min_word) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counted[i] = 0;
    if (i < kTotScalars + kTotBins) totals[i] = i == min_word ? kTotNone : 0ull;
}

// One workgroup's share of the 32 words.  MinWord / MaxWord: the scalar words that are a minimum / a maximum
// (kNoWord: none); every other word is a sum.
struct TotalsLds {
    u64 s[kTotScalars];
    unsigned int hist[kTotBins];  // (<= 256 episodes per workgroup and launch)
};

template <int MinWord>
__device__ __forceinline__ void totals_stage(TotalsLds& L) {
    const int tid = threadIdx.x;
    if (tid < kTotScalars) L.s[tid] = tid == MinWord ? kTotNone : 0ull;
    if (tid < kTotBins) L.hist[tid] = 0u;
    __syncthreads();
}

// len against d > 0 (the shortest path, or par): one more in the histogram's bin clamp(4 len / d - 4, 0, 15);
// returns floor(len 65536 / d)
__device__ __forceinline__ u64 totals_rate(TotalsLds& L, int len, int d) {
    const int64_t bin = 4 * (int64_t)len / (int64_t)d - 4;
    atomicAdd(&L.hist[bin < 0 ? 0 : bin > kTotBins - 1 ? kTotBins - 1 : (int)bin], 1u);
    return ((u64)(int64_t)len << 16) / (u64)d;
}

// the wavefront's sum / minimum / maximum of v into scalar word w of the workgroup
__device__ __forceinline__ void totals_add(TotalsLds& L, int w, u64 v) {
    v = wave_reduce(v, [](u64 a, u64 b) { return a + b; });
    if ((threadIdx.x & 63) == 0) atomicAdd(&L.s[w], v);
}
__device__ __forceinline__ void totals_min(TotalsLds& L, int w, u64 v) {
    v = wave_reduce(v, [](u64 a, u64 b) { return b < a ? b : a; });
    if ((threadIdx.x & 63) == 0) atomicMin(&L.s[w], v);
}
__device__ __forceinline__ void totals_max(TotalsLds& L, int w, u64 v) {
    v = wave_reduce(v, [](u64 a, u64 b) { return b > a ? b : a; });
    if ((threadIdx.x & 63) == 0) atomicMax(&L.s[w], v);
}

// one global atomic per word that this workgroup changed
template <int MinWord, int MaxWord>
__device__ __forceinline__ void totals_flush(const TotalsLds& L, u64* __restrict__ totals) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < kTotScalars) {
        const u64 v = L.s[tid];
        if (tid == MinWord) {
            if (v != kTotNone) atomicMin(&totals[tid], v);
        } else if (v != 0) {
            if (tid == MaxWord) atomicMax(&totals[tid], v);
            else atomicAdd(&totals[tid], v);
        }
    } else if (tid < kTotScalars + kTotBins) {
        const unsigned int v = L.hist[tid - kTotScalars];
        if (v != 0) atomicAdd(&totals[tid], (u64)v);
    }
}

// ---------------------------------------------------------------------------
// episode totals
// ---------------------------------------------------------------------------
__global__ void k_eval_init(u64* __restrict__ totals, int32_t* __restrict__ counted, int n) {
    totals_init(totals, counted, n, MM_EV_MIN_LEN_SOLVED);
}

__global__ __launch_bounds__(kTotThreads) void k_eval_accum(const uint8_t* __restrict__ done,
                                                            const float* __restrict__ reward,
                                                            const int2* __restrict__ ep_stats, int n, int quota,
                                                            int32_t* __restrict__ counted, u64* __restrict__ totals) {
    __shared__ TotalsLds L;
    const int tid = threadIdx.x, m = blockIdx.x * kTotThreads + tid;
    totals_stage<MM_EV_MIN_LEN_SOLVED>(L);
    const bool ev = m < n && quota_claim(done[m], counted, m, quota) >= 0;
    if (__any(ev)) {  // wave-uniform: most waves of most steps hold no episode end
        u64 solved = 0, len = 0, len_s = 0, short_s = 0, ratio = 0, bad = 0, mn = kTotNone, mx = 0;
        if (ev) {
            const int2 st = ep_stats[m];  // (length, shortest_path_len): k_step's pair
            len = (u64)(int64_t)st.x;
            if (reward[m] == 1.0f) {
                solved = 1;
                len_s = mn = mx = len;
                short_s = (u64)(int64_t)st.y;
                if (st.y <= 0) bad = 1;
                else ratio = totals_rate(L, st.x, st.y);
            }
        }
        totals_add(L, MM_EV_EPISODES, ev);
        totals_add(L, MM_EV_SOLVED, solved);
        totals_add(L, MM_EV_TIMEOUTS, ev && !solved);
        totals_add(L, MM_EV_SUM_LEN, len);
        totals_add(L, MM_EV_SUM_LEN_SOLVED, len_s);
        totals_add(L, MM_EV_SUM_SHORT_SOLVED, short_s);
        totals_add(L, MM_EV_SUM_RATIO_Q16, ratio);
        totals_add(L, MM_EV_BAD_SHORT, bad);
        totals_min(L, MM_EV_MIN_LEN_SOLVED, mn);
        totals_max(L, MM_EV_MAX_LEN_SOLVED, mx);
    }
    totals_flush<MM_EV_MIN_LEN_SOLVED, MM_EV_MAX_LEN_SOLVED>(L, totals);
}

// ---------------------------------------------------------------------------
// totals of exit time against par
// ---------------------------------------------------------------------------
__global__ void k_par_init(u64* __restrict__ totals, int32_t* __restrict__ counted, int n) {
    totals_init(totals, counted, n, kNoWord);
}

__global__ __launch_bounds__(kTotThreads) void k_par_accum(const uint8_t* __restrict__ done,
                                                           const float* __restrict__ reward,
                                                           const int2* __restrict__ ep_stats,
                                                           const int32_t* __restrict__ par, int n, int quota,
                                                           int32_t* __restrict__ counted, u64* __restrict__ totals) {
    __shared__ TotalsLds L;
    const int tid = threadIdx.x, m = blockIdx.x * kTotThreads + tid;
    totals_stage<kNoWord>(L);
    // only solved episodes are rated (a timed-out one still takes its slot of the quota: the claim comes first)
    const bool ev = m < n && quota_claim(done[m], counted, m, quota) >= 0 && reward[m] == 1.0f;
    if (__any(ev)) {  // wave-uniform: most waves of most steps hold no solved episode
        u64 rated = 0, len = 0, sp = 0, ratio = 0, at = 0, below = 0, unrated = 0, mx = 0;
        if (ev) {
            const int l = ep_stats[m].x, p = par[4 * (size_t)m];
            if (p <= 0) {
                unrated = 1;
            } else {
                rated = 1;
                len = (u64)(int64_t)l;
                sp = (u64)p;
                ratio = totals_rate(L, l, p);
                at = l == p;
                below = l < p;
                mx = l > p ? (u64)(l - p) : 0ull;
            }
        }
        totals_add(L, MM_PAR_EPISODES, rated);
        totals_add(L, MM_PAR_SUM_LEN, len);
        totals_add(L, MM_PAR_SUM_PAR, sp);
        totals_add(L, MM_PAR_SUM_RATIO_Q16, ratio);
        totals_add(L, MM_PAR_AT_PAR, at);
        totals_add(L, MM_PAR_BELOW, below);
        totals_add(L, MM_PAR_UNRATED, unrated);
        totals_max(L, MM_PAR_MAX_EXCESS, mx);
    }
    totals_flush<kNoWord, MM_PAR_MAX_EXCESS>(L, totals);
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
    hipLaunchKernelGGL(k_eval_accum, dim3((n + kTotThreads - 1) / kTotThreads), dim3(kTotThreads), 0,
                       (hipStream_t)stream, done, reward, reinterpret_cast<const int2*>(ep_stats), n, quota, counted,
                       reinterpret_cast<u64*>(totals));
    return (int)hipGetLastError();
}

extern "C" int mm_par_init(uint64_t* totals, int32_t* counted, int n, void* stream) {
    if (!totals || !counted || n < 0 || ((uintptr_t)totals & 7) || ((uintptr_t)counted & 3)) return MM_E_ARG;
    const int threads = n > MM_PAR_WORDS ? n : MM_PAR_WORDS;
    hipLaunchKernelGGL(k_par_init, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<u64*>(totals), counted, n);
    return (int)hipGetLastError();
}

extern "C" int mm_par_accum(const uint8_t* done, const float* reward, const int32_t* ep_stats, const int32_t* par,
                            int n, int quota, int32_t* counted, uint64_t* totals, void* stream) {
    if (!done || !reward || !ep_stats || !par || !counted || !totals || n < 0 || quota < 0 ||
        ((uintptr_t)reward & 3) || ((uintptr_t)ep_stats & 7) || ((uintptr_t)par & 3) || ((uintptr_t)counted & 3) ||
        ((uintptr_t)totals & 7))
        return MM_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_par_accum, dim3((n + kTotThreads - 1) / kTotThreads), dim3(kTotThreads), 0,
                       (hipStream_t)stream, done, reward, reinterpret_cast<const int2*>(ep_stats), par, n, quota,
                       counted, reinterpret_cast<u64*>(totals));
    return (int)hipGetLastError();
}
