// elog_kernels.hip -- the episode log on MI355X (gfx950): one record of MM_ELOG_WORDS int32 per finished episode,
// written where the episode ran.
//
// k_step regenerates a finished maze in the same launch (auto_reset = 1), so what an episode did is gone by the
// time the host could look.  The log is a tracker between the step and the reset: after mm_env_step(...,
// auto_reset = 2) k_elog_step folds the post-step agents, maze and actions into a small running state per maze
// and, where done[m] != 0, turns that state into the episode's record; after the reset k_elog_start clears the
// state of the mazes that were reset and takes in their spawn cells and open-cell count.
//
// Running state: `state_words` = kElScalars + 2 * ceil(layout_stride / 32) int32 per maze, stored WORD-MAJOR: word
// k of maze m is state[k * n + m].  k_elog_step is one lane per maze, so every scalar word is read and written
// by 64 consecutive lanes as 256 contiguous bytes; maze-major rows (34 words = 136 bytes at 10x10 mazes) would put
// every lane on a line of its own.  The two visit bitmaps (one bit per layout cell and agent) cost one
// read-modify-write of one word per agent and step, written back only when the bit is new.  A PHASE word says which
// of the four milestones (key gone, agent 0 / 1 knows the end, team exit-ready) have been stamped, so a step reads
// one word for them, not four, and writes a T_* word once per episode.  The three counters are read with it and
// written only by a step that marks or stays.  Popcounts run only at done.
//
//   k_elog_init   log = -1, counted = 0, state = 0
//   k_elog_start  a wavefront per 64 mazes finds the selected ones with one ballot, then works on them one at a
//                 time with all 64 lanes: the layout's w * h bytes are counted (cell & 3) != 1 with a wavefront
//                 reduction, and the lanes write the maze's state words
//   k_elog_step   one lane per maze, one launch per env step
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "env_device.h"
#include "marlmaze.h"
#include "quota_device.h"

namespace mm {

constexpr int kElThreads = 256;
// the scalar words of a maze's running state; the bitmaps of agent 0 and agent 1 follow
enum { kElPhase, kElTKey, kElFetcher, kElTKnow0, kElTKnow1, kElTReady, kElOpen, kElMarks0, kElMarks1, kElStays, kElScalars };
constexpr int kPhKey = 1, kPhKnow0 = 2, kPhKnow1 = 4, kPhReady = 8;  // kElPhase: this milestone has its T_* word

__host__ __device__ inline int elog_bm_words(int stride) { return (stride + 31) >> 5; }

// x, y and flags of an agent from the first four bytes of its record (x, y, dir, flags: one aligned load)
static_assert(offsetof(mm_agent_t, x) == 0 && offsetof(mm_agent_t, y) == 1 && offsetof(mm_agent_t, flags) == 3 &&
                  sizeof(mm_agent_t) == 32 && sizeof(mm_maze_t) == 32,
              "k_elog_* read the head of the 32-byte records");
struct ElAgent {
    int x, y, flags;
};
__device__ __forceinline__ ElAgent elog_agent(const mm_agent_t* a) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(a);
    return ElAgent{(int)(int8_t)(v & 0xff), (int)(int8_t)(v >> 8 & 0xff), (int)(v >> 24)};
}
// the agent's cell in its bitmap, -1 when it is not a cell of this layout (nothing is then written)
__device__ __forceinline__ int elog_cell(const ElAgent& a, int w, int stride) {
    const int c = a.y * w + a.x;
    return (a.x >= 0 && a.y >= 0 && a.x < w && c < stride) ? c : -1;
}

__global__ __launch_bounds__(kElThreads) void k_elog_init(int32_t* __restrict__ log, size_t nlog,
                                                          int32_t* __restrict__ counted, size_t n,
                                                          int32_t* __restrict__ state, size_t nstate) {
    const size_t i0 = (size_t)blockIdx.x * kElThreads + threadIdx.x, step = (size_t)gridDim.x * kElThreads;
    for (size_t i = i0; i < nlog; i += step) log[i] = -1;
    for (size_t i = i0; i < n; i += step) counted[i] = 0;
    for (size_t i = i0; i < nstate; i += step) state[i] = 0;
}

__global__ __launch_bounds__(kElThreads) void k_elog_start(mm_env_t env, const uint8_t* __restrict__ select,
                                                           int32_t* __restrict__ state, int sw) {
    const int n = env.n, stride = env.layout_stride, bw = elog_bm_words(stride);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long base = ((long)blockIdx.x * (kElThreads / 64) + wave) * 64; base < n;
         base += (long)gridDim.x * kElThreads) {
        const long mi = base + lane;
        unsigned long long todo = __ballot(mi < n && (!select || select[mi] != 0));
        while (todo) {  // wavefront-uniform: the selected mazes of this chunk, one at a time
            const int m = (int)base + __builtin_ctzll(todo);
            todo &= todo - 1;
            const mm_maze_t* mz = env.mazes + m;
            const int w = min(max((int)mz->w, 0), MM_MAX_SIDE), h = min(max((int)mz->h, 0), MM_MAX_SIDE);
            const int nc = min(w * h, stride);
            const uint8_t* L = env.layout + (size_t)m * stride;
            int open = 0;
            for (int c = lane; c < nc; c += 64) open += (L[c] & 3) != 1;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) open += __shfl_xor(open, d);
            const ElAgent a0 = elog_agent(env.agents + 2 * (size_t)m), a1 = elog_agent(env.agents + 2 * (size_t)m + 1);
            const int c0 = elog_cell(a0, w, stride), c1 = elog_cell(a1, w, stride);
            const bool k0 = a0.flags & MM_AF_KNOWS_END, k1 = a1.flags & MM_AF_KNOWS_END;  // the reset's observation
            for (int k = lane; k < sw; k += 64) {
                int32_t v = 0;  // the counters, and every bitmap word but the spawn cells'
                if (k == kElPhase) v = (k0 ? kPhKnow0 : 0) | (k1 ? kPhKnow1 : 0);
                else if (k == kElTKey || k == kElFetcher || k == kElTReady) v = -1;
                else if (k == kElTKnow0) v = k0 ? 0 : -1;
                else if (k == kElTKnow1) v = k1 ? 0 : -1;
                else if (k == kElOpen) v = open;
                else if (k >= kElScalars) {
                    const int j = k - kElScalars, a = j >= bw, c = a ? c1 : c0;
                    if (c >= 0 && (c >> 5) == j - a * bw) v = (int32_t)(1u << (c & 31));
                }
                state[(size_t)k * n + m] = v;
            }
        }
    }
}

__global__ __launch_bounds__(kElThreads) void k_elog_step(mm_env_t env, const char4* __restrict__ act,
                                                          const uint8_t* __restrict__ done,
                                                          const float* __restrict__ reward,
                                                          const int2* __restrict__ ep_stats,
                                                          const int32_t* __restrict__ par, int quota,
                                                          int32_t* __restrict__ counted, int32_t* state,
                                                          int32_t* __restrict__ log) {
    const int n = env.n, m = blockIdx.x * kElThreads + threadIdx.x;
    if (m >= n) return;
    const int stride = env.layout_stride, bw = elog_bm_words(stride);
    int32_t* S = state + m;  // word k of this maze: S[k * n]
    const size_t N = (size_t)n;
    const ElAgent a0 = elog_agent(env.agents + 2 * (size_t)m), a1 = elog_agent(env.agents + 2 * (size_t)m + 1);
    const mm_maze_t* mz = env.mazes + m;
    const int t = mz->t, w = mz->w, kx = mz->kx;
    const char4 ac = act[m];  // (move, mark) of agent 0, of agent 1: the bytes as given
    // every load that depends on nothing is issued here, before the first store (`state` may alias itself, so a
    // load placed after a store would wait for it): the launch is one lane per maze, a few wavefronts per CU, and its
    // time is its chain of dependent memory round trips, not its bytes
    const int ph0 = S[kElPhase * N];
    const int marks0 = S[kElMarks0 * N], marks1 = S[kElMarks1 * N], stays = S[kElStays * N];
    const uint8_t dn = done[m];
    // the cells the agents stand on: the second round trip
    const int cell[2] = {elog_cell(a0, w, stride), elog_cell(a1, w, stride)};
    int32_t* bp[2];
    int32_t bo[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        bp[a] = S + (size_t)(kElScalars + a * bw + (max(cell[a], 0) >> 5)) * N;  // cell < stride: word < bw
        bo[a] = *bp[a];
    }
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int32_t v = bo[a] | (int32_t)(1u << (cell[a] & 31));
        if (cell[a] >= 0 && v != bo[a]) *bp[a] = v;
    }
    // milestones: each T_* word is written by the first step that finds its condition true
    int ph = ph0;
    if (!(ph & kPhKey) && kx < 0) {
        ph |= kPhKey;
        S[kElTKey * N] = t;
        S[kElFetcher * N] = (a0.flags & MM_AF_HAS_KEY) ? 0 : (a1.flags & MM_AF_HAS_KEY) ? 1 : -1;
    }
    if (!(ph & kPhKnow0) && (a0.flags & MM_AF_KNOWS_END)) {
        ph |= kPhKnow0;
        S[kElTKnow0 * N] = t;
    }
    if (!(ph & kPhKnow1) && (a1.flags & MM_AF_KNOWS_END)) {
        ph |= kPhKnow1;
        S[kElTKnow1 * N] = t;
    }
    constexpr int kReady = MM_AF_KNOWS_END | MM_AF_TEAM_KEY;
    if (!(ph & kPhReady) && (a0.flags & a1.flags & kReady) == kReady) {
        ph |= kPhReady;
        S[kElTReady * N] = t;
    }
    if (ph != ph0) S[kElPhase * N] = ph;
    const int mk0 = ac.y == 1, mk1 = ac.w == 1, st = (ac.x == 4) + (ac.z == 4);
    if (mk0) S[kElMarks0 * N] = marks0 + 1;
    if (mk1) S[kElMarks1 * N] = marks1 + 1;
    if (st) S[kElStays * N] = stays + st;
    if (dn == 0) return;
    // the episode ended with this step: its record, if the maze still has quota (quota_device.h; `counted` is
    // read here, after the running state's stores, and only by the lanes whose episode ended)
    const int32_t c = quota_claim(dn, counted, m, quota);
    if (c < 0) return;
    int n0 = 0, n1 = 0, nb = 0;
    for (int k = 0; k < bw; k++) {
        const uint32_t b0 = (uint32_t)S[(size_t)(kElScalars + k) * N], b1 = (uint32_t)S[(size_t)(kElScalars + bw + k) * N];
        n0 += __popc(b0);
        n1 += __popc(b1);
        nb += __popc(b0 & b1);
    }
    const int2 es = ep_stats[m];
    int32_t r[MM_ELOG_WORDS];
    r[MM_ELOG_LEN] = es.x;
    r[MM_ELOG_SHORTEST] = es.y;
    r[MM_ELOG_SOLVED] = reward[m] == 1.0f;
    r[MM_ELOG_PAR] = par ? par[4 * (size_t)m] : -1;
    r[MM_ELOG_T_KEY] = S[kElTKey * N];
    r[MM_ELOG_FETCHER] = S[kElFetcher * N];
    r[MM_ELOG_T_KNOW0] = S[kElTKnow0 * N];
    r[MM_ELOG_T_KNOW1] = S[kElTKnow1 * N];
    r[MM_ELOG_T_READY] = S[kElTReady * N];
    r[MM_ELOG_CELLS0] = n0;
    r[MM_ELOG_CELLS1] = n1;
    r[MM_ELOG_CELLS_BOTH] = nb;
    r[MM_ELOG_OPEN] = S[kElOpen * N];
    r[MM_ELOG_MARKS0] = marks0 + mk0;
    r[MM_ELOG_MARKS1] = marks1 + mk1;
    r[MM_ELOG_STAYS] = stays + st;
    int4* row = reinterpret_cast<int4*>(log + ((size_t)m * quota + c) * MM_ELOG_WORDS);  // c < quota: inside log
#pragma unroll
    for (int q = 0; q < MM_ELOG_WORDS / 4; q++) row[q] = make_int4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
}

constexpr int kElGrid = 4096;  // workgroups of the grid-stride kernels

}  // namespace mm

using namespace mm;

extern "C" long mm_elog_state_words(int layout_stride) {
    if (layout_stride <= 0) return MM_E_ARG;
    return kElScalars + 2L * elog_bm_words(layout_stride);
}

extern "C" int mm_elog_init(int32_t* log, int32_t* counted, int32_t* state, int n, int quota, long state_words,
                            void* stream) {
    if (!log || !counted || !state || n < 0 || quota < 0 || state_words <= kElScalars || ((uintptr_t)log & 15) ||
        ((uintptr_t)counted & 3) || ((uintptr_t)state & 3))
        return MM_E_ARG;
    if (n == 0) return 0;
    const size_t nlog = (size_t)n * quota * MM_ELOG_WORDS, nstate = (size_t)n * state_words;
    const size_t most = nlog > nstate ? nlog : nstate, blocks = (most + kElThreads - 1) / kElThreads;
    hipLaunchKernelGGL(k_elog_init, dim3(blocks < (size_t)kElGrid ? (unsigned)blocks : kElGrid), dim3(kElThreads), 0,
                       (hipStream_t)stream, log, nlog, counted, (size_t)n, state, nstate);
    return (int)hipGetLastError();
}

extern "C" int mm_elog_start(const mm_env_t* env, const uint8_t* select, int32_t* state, long state_words,
                             void* stream) {
    int e = check_env(env);
    if (e) return e;
    if (!state || ((uintptr_t)state & 3) || state_words != mm_elog_state_words(env->layout_stride)) return MM_E_ARG;
    const int blocks = (env->n + kElThreads - 1) / kElThreads;  // a wavefront per 64 mazes
    hipLaunchKernelGGL(k_elog_start, dim3(blocks < kElGrid ? blocks : kElGrid), dim3(kElThreads), 0,
                       (hipStream_t)stream, *env, select, state, (int)state_words);
    return (int)hipGetLastError();
}

extern "C" int mm_elog_step(const mm_env_t* env, const int8_t* actions, const uint8_t* done, const float* reward,
                            const int32_t* ep_stats, const int32_t* par, int quota, int32_t* counted, int32_t* state,
                            long state_words, int32_t* log, void* stream) {
    int e = check_env(env);
    if (e) return e;
    if (!actions || !done || !reward || !ep_stats || !counted || !state || !log || quota < 0 ||
        state_words != mm_elog_state_words(env->layout_stride) || ((uintptr_t)actions & 3) ||
        ((uintptr_t)reward & 3) || ((uintptr_t)ep_stats & 7) || ((uintptr_t)par & 3) || ((uintptr_t)counted & 3) ||
        ((uintptr_t)state & 3) || ((uintptr_t)log & 15))
        return MM_E_ARG;
    hipLaunchKernelGGL(k_elog_step, dim3((env->n + kElThreads - 1) / kElThreads), dim3(kElThreads), 0,
                       (hipStream_t)stream, *env, reinterpret_cast<const char4*>(actions), done, reward,
                       reinterpret_cast<const int2*>(ep_stats), par, quota, counted, state, log);
    return (int)hipGetLastError();
}
