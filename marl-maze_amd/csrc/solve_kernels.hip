// solve_kernels.hip -- distance fields and par times of the batched mazes on MI355X (gfx950).
//
// Kernels
//   k_env_dist  one 64-lane wavefront per maze (a workgroup of exactly one wavefront, as k_reset): the distance
//               field of one target cell by a level-synchronous breadth-first search.  The maze's cells (one byte
//               each: passable, and which of the four neighbours are), the int16 field, the queue of reached cells
//               and a bitmap of them live in LDS.  Every reached cell enters the queue once, in the order reached,
//               so the frontier of a level is a slice of the queue: lane i expands the i-th cell of the slice,
//               claims each passable neighbour with an LDS atomic on the bitmap (one claimant, also where a
//               hand-made layout has cycles), gives it the level and appends it.  A maze is a tree with frontiers
//               of a few cells, so a level costs a handful of dependent LDS operations, not a scan of the maze.
//               The search ends at the first empty frontier, at the latest after w * h levels.
//   k_env_par   the same search for two targets at once, the end and the key (two fields in LDS, one barrier pair
//               per level for both), then a handful of reads at the two spawn cells and the key: the par time of
//               the maze (marlmaze.h).  The fields are not written out.  (The totals of exit time against these
//               par times are an evaluation's: k_par_accum in eval_kernels.hip.)
//
// The number of levels differs from maze to maze.  A workgroup is one wavefront, so __syncthreads() is local to
// the wavefront of one maze and a maze that finishes early cannot strand a barrier that another still waits at.
// Every loop bound comes from the clamped sizes (w, h <= MM_MAX_SIDE), never from the layout's contents: a corrupt
// layout gives -1 entries, not a long run, and every LDS index is below w * h <= min(layout_stride, 1681).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_device.h"
#include "marlmaze.h"

namespace mm {

constexpr int kSolveCells = MM_MAX_SIDE * MM_MAX_SIDE;
static_assert(kSolveCells < 32767, "levels and cell indices are int16");
constexpr int kNbOpen = 16;  // cell byte: bit 4 = passable, bits 0-3 = neighbour N, E, S, W (maze.py:19) passable

// The workgroup's LDS, carved from the dynamic allocation for `cap` cells: the environment's layout_stride, not
// MM_MAX_SIDE^2, so that 10x10 mazes (361 cells) take 2 to 3.4 KB a wavefront and the CU's wavefront slots fill.
template <int NF>
struct SolveLds {
    uint32_t* seen[NF];  // [cap / 32] bit c: cell c has been reached (the NF bitmaps are contiguous)
    int* tail;           // [NF] entries in the queue
    int16_t* dist[NF];   // [cap]
    int16_t* queue[NF];  // [cap] the reached cells in the order reached (each once: at most w * h entries)
    uint8_t* nb;         // [cap]
};

__host__ __device__ inline int solve_cap(int stride) {  // cells to hold, a multiple of 32
    return ((stride < kSolveCells ? stride : kSolveCells) + 31) & ~31;
}
template <int NF>
__host__ __device__ inline int solve_lds_bytes(int cap) {
    return NF * (cap / 32) * 4 + 8 + NF * 2 * cap * 2 + cap;
}
template <int NF>
__device__ __forceinline__ SolveLds<NF> solve_carve(uint8_t* base, int cap) {
    SolveLds<NF> s;
    uint32_t* words = reinterpret_cast<uint32_t*>(base);
#pragma unroll
    for (int f = 0; f < NF; f++) s.seen[f] = words + f * (cap / 32);
    s.tail = reinterpret_cast<int*>(words + NF * (cap / 32));
    int16_t* h = reinterpret_cast<int16_t*>(words + NF * (cap / 32) + 2);
#pragma unroll
    for (int f = 0; f < NF; f++) {
        s.dist[f] = h + 2 * f * cap;
        s.queue[f] = h + (2 * f + 1) * cap;
    }
    s.nb = reinterpret_cast<uint8_t*>(h + 2 * NF * cap);
    return s;
}

extern __shared__ __attribute__((aligned(16))) uint8_t solve_smem[];

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }  // wavefront-uniform
__device__ __forceinline__ int clamp_side(int v) { return v < 0 ? 0 : v > MM_MAX_SIDE ? MM_MAX_SIDE : v; }

// Stage maze L (w x h, both clamped) into s.nb, set every field to -1 and clear the bitmaps.
template <int NF>
__device__ void solve_stage(const SolveLds<NF>& s, const uint8_t* __restrict__ L, int w, int h, int marks_block,
                            int cap) {
    const int lane = threadIdx.x, nc = w * h;
    uint32_t open = 0;  // bit k: cell lane + 64 k is passable
    for (int k = 0, c = lane; c < nc; k++, c += 64) {
        const int v = L[c] & 3;
        const bool o = marks_block ? v == 0 : v != 1;
        s.nb[c] = o ? kNbOpen : 0;
        open |= (uint32_t)o << k;
#pragma unroll
        for (int f = 0; f < NF; f++) s.dist[f][c] = -1;
    }
    for (int i = lane; i < NF * (cap / 32); i += 64) s.seen[0][i] = 0u;
    __syncthreads();
    // the neighbour bits of the passable cells (an impassable cell, a target even, is never expanded).  Other
    // lanes read bit 4 of a byte while its owner rewrites it with the same bit 4: byte stores, so they see it
    // either way.
    for (uint32_t p = open; p; p &= p - 1) {
        const int c = lane + 64 * __builtin_ctz(p);
        const int y = c / w, x = c - y * w;
        int b = kNbOpen;
        b |= (y > 0 && (s.nb[c - w] & kNbOpen)) ? 1 : 0;
        b |= (x < w - 1 && (s.nb[c + 1] & kNbOpen)) ? 2 : 0;
        b |= (y < h - 1 && (s.nb[c + w] & kNbOpen)) ? 4 : 0;
        b |= (x > 0 && (s.nb[c - 1] & kNbOpen)) ? 8 : 0;
        s.nb[c] = (uint8_t)b;
    }
    __syncthreads();
}

// NF searches at once over the staged maze: field f from the cell tc[f] (inside the grid; 0 whatever its value).
template <int NF>
__device__ void solve_bfs(const SolveLds<NF>& s, int w, int nc, const int (&tc)[NF]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int f = 0; f < NF; f++) {
        if (lane == f) {
            s.dist[f][tc[f]] = 0;
            s.queue[f][0] = (int16_t)tc[f];
            s.seen[f][tc[f] >> 5] = 1u << (tc[f] & 31);
            s.tail[f] = 1;
        }
    }
    __syncthreads();
    int head[NF], tail[NF];
#pragma unroll
    for (int f = 0; f < NF; f++) head[f] = 0, tail[f] = 1;
    for (int level = 1; level <= nc; level++) {
        bool any = false;
#pragma unroll
        for (int f = 0; f < NF; f++) {
            const int cnt = tail[f] - head[f];  // wavefront-uniform
            any |= cnt > 0;
            for (int i = lane; i < cnt; i += 64) {
                const int c = s.queue[f][head[f] + i];
                const int b = s.nb[c];
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    if (!(b >> d & 1)) continue;
                    const int c2 = c + (d == 0 ? -w : d == 1 ? 1 : d == 2 ? w : -1);
                    const uint32_t bit = 1u << (c2 & 31);
                    if (atomicOr(&s.seen[f][c2 >> 5], bit) & bit) continue;  // reached before (or by another lane)
                    s.dist[f][c2] = (int16_t)level;
                    s.queue[f][atomicAdd(&s.tail[f], 1)] = (int16_t)c2;  // every cell is claimed once: < w * h
                }
            }
        }
        if (!any) break;
        __syncthreads();
#pragma unroll
        for (int f = 0; f < NF; f++) {
            head[f] = tail[f];
            tail[f] = uni(s.tail[f]);
        }
        __syncthreads();  // every lane holds the new tail before the next level appends
    }
}

__global__ __launch_bounds__(64) void k_env_dist(mm_env_t env, const int16_t* __restrict__ targets,
                                                 const uint8_t* __restrict__ select, int marks_block,
                                                 int16_t* __restrict__ out) {
    const int lane = threadIdx.x, stride = env.layout_stride, cap = solve_cap(stride);
    const SolveLds<1> s = solve_carve<1>(solve_smem, cap);
    for (int m = blockIdx.x; m < env.n; m += gridDim.x) {
        if (select && !select[m]) continue;
        const mm_maze_t mz = env.mazes[m];
        const int w = uni(clamp_side(mz.w)), h = uni(clamp_side(mz.h)), nc = w * h;
        const int tx = uni(targets[2 * m]), ty = uni(targets[2 * m + 1]);
        const bool ok = nc > 0 && nc <= stride && tx >= 0 && tx < w && ty >= 0 && ty < h;
        if (ok) {
            solve_stage(s, env.layout + (size_t)m * stride, w, h, marks_block, cap);
            const int tc[1] = {ty * w + tx};
            solve_bfs<1>(s, w, nc, tc);
        }
        int16_t* row = out + (size_t)m * stride;
        for (int c = lane; c < stride; c += 64) row[c] = (ok && c < nc) ? s.dist[0][c] : (int16_t)-1;
        __syncthreads();  // the next maze of this workgroup restages the LDS
    }
}

__global__ __launch_bounds__(64) void k_env_par(mm_env_t env, const uint8_t* __restrict__ select,
                                                int32_t* __restrict__ out) {
    const int lane = threadIdx.x, stride = env.layout_stride, cap = solve_cap(stride);
    const SolveLds<2> s = solve_carve<2>(solve_smem, cap);
    for (int m = blockIdx.x; m < env.n; m += gridDim.x) {
        if (select && !select[m]) continue;
        const mm_maze_t mz = env.mazes[m];
        const int w = uni(clamp_side(mz.w)), h = uni(clamp_side(mz.h)), nc = w * h;
        const int ex = uni(mz.ex), ey = uni(mz.ey), kx = uni(mz.kx), ky = uni(mz.ky);
        auto inb = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h; };
        const bool ok = nc > 0 && nc <= stride && inb(ex, ey) && inb(kx, ky);  // kx < 0: no key
        int par = -1, fetcher = -1, fetch = -1, other = -1;
        if (ok) {
            solve_stage(s, env.layout + (size_t)m * stride, w, h, 0, cap);
            const int tc[2] = {ey * w + ex, ky * w + kx};
            solve_bfs<2>(s, w, nc, tc);
            const int x0 = mz.sx, y0 = mz.sy, x1 = mz.spawn1 & 0xff, y1 = (mz.spawn1 >> 8) & 0xff;
            if (lane == 0 && inb(x0, y0) && inb(x1, y1)) {
                const int c0 = y0 * w + x0, c1 = y1 * w + x1;
                const int ke = s.dist[0][tc[1]];                      // d(key, end)
                const int e0 = s.dist[0][c0], e1 = s.dist[0][c1];     // d(s_a, end)
                const int k0 = s.dist[1][c0], k1 = s.dist[1][c1];     // d(s_a, key)
                if ((ke | e0 | e1 | k0 | k1) >= 0) {
                    const int cand0 = max(k0 + ke, e1), cand1 = max(k1 + ke, e0);
                    fetcher = cand1 < cand0;  // agent 0 wins a tie
                    par = fetcher ? cand1 : cand0;
                    fetch = (fetcher ? k1 : k0) + ke;
                    other = fetcher ? e0 : e1;
                }
            }
        }
        if (lane == 0) {
            int32_t* row = out + 4 * (size_t)m;
            row[0] = par;
            row[1] = fetcher;
            row[2] = fetch;
            row[3] = other;
        }
        __syncthreads();  // the next maze of this workgroup restages the LDS
    }
}

constexpr int kSolveGrid = 1 << 16;  // workgroups (mazes in flight); more mazes take turns

}  // namespace mm

using namespace mm;

extern "C" int mm_env_dist(const mm_env_t* env, const int16_t* targets, const uint8_t* select, int marks_block,
                           int16_t* dist, void* stream) {
    int e = check_env(env);
    if (e) return e;
    if (!targets || !dist || ((uintptr_t)targets & 1) || ((uintptr_t)dist & 1)) return MM_E_ARG;
    hipLaunchKernelGGL(k_env_dist, dim3(env->n < kSolveGrid ? env->n : kSolveGrid), dim3(64),
                       solve_lds_bytes<1>(solve_cap(env->layout_stride)), (hipStream_t)stream, *env, targets, select, marks_block != 0, dist);
    return (int)hipGetLastError();
}

extern "C" int mm_env_par(const mm_env_t* env, const uint8_t* select, int32_t* par, void* stream) {
    int e = check_env(env);
    if (e) return e;
    if (!par || ((uintptr_t)par & 3)) return MM_E_ARG;
    hipLaunchKernelGGL(k_env_par, dim3(env->n < kSolveGrid ? env->n : kSolveGrid), dim3(64),
                       solve_lds_bytes<2>(solve_cap(env->layout_stride)), (hipStream_t)stream, *env, select, par);
    return (int)hipGetLastError();
}
