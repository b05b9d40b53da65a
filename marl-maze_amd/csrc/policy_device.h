// policy_device.h -- the per-row device code of the actor's heads (networks.py:38-41) and of PPO.get_action
// (PPO.py:170-186), once: act_row (the action of one agent row, drawn or most likely) and the heads' row GEMV
// (heads_fma4, heads_row_dot, heads_butterfly, heads_finish).  Its callers are k_act, k_head_act and k_heads_fwd
// (rl_kernels.hip) and k_trunk3's fused heads (x3mlp.hip), so the rollout's, the update's and the fused trunk's
// logits, and every kernel's draws and log-probs, are equal bit for bit because they are the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "marlmaze.h"

namespace mm {

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

// One agent row of PPO.get_action (PPO.py:170-186): a move among the legal ones and a mark where it is
// allowed; returns the per-agent log-prob log pi(a|s).
//   MM_ACT_SAMPLE  masked categorical move (inverse-CDF draw), Bernoulli mark.  The draws are Philox of
//                  counter (offset, row): the same row gets the same numbers in every kernel.
//   MM_ACT_GREEDY  no draws (row, seed and offset are unused).  Move: the lowest index among the legal moves
//                  whose logit is the maximum (torch.argmax's first occurrence).  Mark: allowed and
//                  mark_logit > 0 (sigmoid > 0.5; a logit of exactly 0 does not mark).
template <int MODE>
__device__ __forceinline__ float act_row(const float ml[5], float kl, const uint8_t* __restrict__ mk, int row,
                                         uint64_t seed, uint64_t offset, int& move, int& mark) {
    constexpr bool kDraw = MODE == MM_ACT_SAMPLE;
    uint4 rnd = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (kDraw)
        rnd = philox(make_uint4((uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)row, 0u),
                     make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    float l[5];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        l[j] = mk[j] ? ml[j] : -INFINITY;  // masked_fill(~mask, -inf)
        mx = fmaxf(mx, l[j]);
    }
    float p[5], sum = 0.f;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        p[j] = mk[j] ? expf(l[j] - mx) : 0.f;
        sum += p[j];
    }
    // mv: the move; alt: the legal move taken when none was picked -- the last one (rounding left the target at
    // or above the whole sum) / the first one (the legal logits are all NaN: fmaxf skipped them, lp is NaN)
    int mv = -1, alt = -1;
    if constexpr (kDraw) {  // inverse-CDF draw over the allowed moves
        const float target = u01(rnd.x) * sum;
        float c = 0.f;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            if (!mk[j]) continue;
            alt = j;
            c += p[j];
            if (mv < 0 && target < c) mv = j;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 5; j++) {
            if (!mk[j]) continue;
            if (alt < 0) alt = j;
            if (mv < 0 && l[j] == mx) mv = j;
        }
    }
    if (mv < 0) mv = alt;
    float lp;
    if (mv < 0) {  // no legal move: the reference's Categorical is undefined (NaN)
        mv = 4;
        lp = NAN;
    } else {
        lp = (l[mv] - mx) - logf(sum);  // Categorical.log_prob = logit - logsumexp
    }
    // mark ~ Bernoulli(sigmoid(mark_logit)) if allowed else 0 (PPO.py:179-181)
    int mk5 = 0;
    float pm = 0.f;
    if (mk[5]) {
        pm = 1.f / (1.f + expf(-kl));
        mk5 = (kDraw ? u01(rnd.y) < pm : kl > 0.f) ? 1 : 0;
    }
    lp += logf(mk5 ? pm : 1.f - pm);
    move = mv;
    mark = mk5;
    return lp;
}

// ---------------------------------------------------------------------------
// The heads on one row: logits = h W^T + b for the concatenated heads W = [move_head; mark_head] (6 rows).
// kHeadLanes lanes a row: lane j takes columns 4 j .. 4 j + 3 of every 32 (a row's lanes read 128 contiguous
// bytes per step), each output an fmaf chain in column order (heads_fma4), then a butterfly in which every lane
// gets the sums (heads_butterfly).  This order IS the logits' value: every kernel that computes them goes through
// these two, whether it walks the row (heads_row_dot) or holds its loads in registers (k_heads_fwd<NS > 0>).
// ---------------------------------------------------------------------------
constexpr int kHeadLanes = 8;

// Four columns of a row: hv against the six weight rows at Wc (LDS, `pitch` floats apart).
__device__ __forceinline__ void heads_fma4(const float4& hv, const float* Wc, int pitch, float (&acc)[6]) {
#pragma unroll
    for (int o = 0; o < 6; o++) {
        const float4 wv = *reinterpret_cast<const float4*>(Wc + o * pitch);
        acc[o] = fmaf(hv.x, wv.x, acc[o]);
        acc[o] = fmaf(hv.y, wv.y, acc[o]);
        acc[o] = fmaf(hv.z, wv.z, acc[o]);
        acc[o] = fmaf(hv.w, wv.w, acc[o]);
    }
}

// One lane's share of a row: hr: the row's K values (global or LDS); W: the head weights in LDS, `pitch` floats
// a row; j: the lane within the row; acc: the six sums, zero on entry.  heads_butterfly follows, in all lanes.
__device__ __forceinline__ void heads_row_dot(const float* hr, int K, const float* W, int pitch, int j,
                                              float (&acc)[6]) {
    for (int c = 4 * j; c < K; c += 4 * kHeadLanes)
        heads_fma4(*reinterpret_cast<const float4*>(hr + c), W + c, pitch, acc);
}

__device__ __forceinline__ void heads_butterfly(float (&acc)[6]) {
#pragma unroll
    for (int o = 0; o < 6; o++) {
#pragma unroll
        for (int d = kHeadLanes / 2; d > 0; d >>= 1) acc[o] += __shfl_xor(acc[o], d);
    }
}

// After the butterfly: the row's first lane (`lead`: valid and j == 0) adds the bias, picks the action and stores
// it with its log-prob and, where asked, the logits; then the joint log-prob of maze row / 2, whose rows 2i and
// 2i + 1 are adjacent lane groups (the group's first row is even).  Called by all lanes (the shuffle).
// offset_dev: a device base added to offset in sample mode (graph replays advance it).
template <int MODE>
__device__ __forceinline__ void heads_finish(const float (&acc)[6], const float* __restrict__ b,
                                             const uint8_t* __restrict__ masks, int row, int M, bool lead,
                                             uint64_t seed, uint64_t offset, const uint64_t* __restrict__ offset_dev,
                                             int8_t* __restrict__ act, float* __restrict__ logp,
                                             float* __restrict__ joint, float* __restrict__ logits) {
    float lp = 0.f;
    if (lead) {
        float l[5];
#pragma unroll
        for (int o = 0; o < 5; o++) l[o] = acc[o] + b[o];
        const float kl = acc[5] + b[5];
        int move, mark;
        if constexpr (MODE == MM_ACT_SAMPLE) offset += offset_dev ? *offset_dev : 0ull;
        lp = act_row<MODE>(l, kl, masks + (size_t)row * MM_MASK_DIM, row, seed, offset, move, mark);
        act[2 * row] = (int8_t)move;
        act[2 * row + 1] = (int8_t)mark;
        if (logp) logp[row] = lp;
        if (logits) {
#pragma unroll
            for (int o = 0; o < 5; o++) logits[(size_t)row * 6 + o] = l[o];
            logits[(size_t)row * 6 + 5] = kl;
        }
    }
    const float other = __shfl_down(lp, kHeadLanes);
    if (joint && lead && (row & 1) == 0) joint[row >> 1] = lp + (row + 1 < M ? other : 0.f);
}

}  // namespace mm
