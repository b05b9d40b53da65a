// quota_device.h -- the quota rule of the evaluation's per-maze accumulators (k_eval_accum, k_par_accum,
// k_elog_step), each on a `counted` array of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

// Every maze contributes its FIRST `quota` episodes and nothing else, so mazes that finish fast are not
// over-represented.  `done_m` is done[m] of the step: where an episode ended and the maze still has quota, take
// the next slot and return its index (0 .. quota - 1); otherwise -1, and counted[m] is not touched.  One lane
// per maze, so the read-modify-write needs no atomic.
__device__ __forceinline__ int32_t quota_claim(uint8_t done_m, int32_t* __restrict__ counted, int m, int quota) {
    if (done_m == 0) return -1;
    const int32_t c = counted[m];
    if (c >= quota) return -1;
    counted[m] = c + 1;
    return c;
}

}  // namespace mm
