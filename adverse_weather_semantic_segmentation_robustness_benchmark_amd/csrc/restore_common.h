// restore_common.h — what every restoration front-end shares (DESIGN.md §10n–§10q): dehaze.hip, dehaze_guided.hip, relight.hip,
// deocclude.hip and estimate.hip.  The scalar steps of include/awseg_restore.h, the counter epilogue, the launchers' common
// refusals, and the separable window minimum of the tile kernels.  Once each: every translation unit must produce the same bits.
#ifndef AWSEG_RESTORE_COMMON_H
#define AWSEG_RESTORE_COMMON_H
#include "awseg_common.h"
#include "../../include/awseg_restore.h"
#include <float.h>
#include <math.h>

// The window loops: 2 r taps beside the first, two per trip (minima, maxima and integer sums do not mind the order), four trips
// unrolled, so that eight LDS reads are in flight where a plain loop waits for each.
#define AWSEG_TAPS _Pragma("unroll 4")

namespace {

constexpr int kTH = AWSEG_DEHAZE_TILE_H, kTW = AWSEG_DEHAZE_TILE_W;      // the tile of every tile kernel
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / AWSEG_WAVE;
static_assert(kTW % 4 == 0, "a tile row is whole float4s");

__device__ __forceinline__ float unit(float x, float sd, float mean) { return fminf(fmaxf(x * sd + mean, 0.0f), 1.0f); }
__device__ __forceinline__ uint32_t not_finite(float x) { return fabsf(x) <= FLT_MAX ? 0u : 1u; }

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// The frame's own slot, 1 + cond[img] where that is a slot; -1: none.
__device__ __forceinline__ int slot_of(int n_slots, const int32_t* __restrict__ cond, int64_t img)
{
    int slot = -1;
    if (cond) { const int c = cond[img]; if (c >= 0 && c + 1 < n_slots) slot = c + 1; }
    return slot;
}

// One row of counters into slot 0 and the frame's own slot.  int64 sums: the order of the atomics does not matter.
template <int ROW>
__device__ __forceinline__ void add_row(int64_t* __restrict__ stats, int slot, const long long (&row)[ROW])
{
#pragma unroll
    for (int k = 0; k < ROW; ++k) {
        if (!row[k]) continue;
        atomicAdd((unsigned long long*)&stats[k], (unsigned long long)row[k]);
        if (slot > 0) atomicAdd((unsigned long long*)&stats[(int64_t)slot * ROW + k], (unsigned long long)row[k]);
    }
}

template <int ROW>
__device__ __forceinline__ void add_row(int64_t* __restrict__ stats, int n_slots, const int32_t* __restrict__ cond, int64_t img,
                                        const long long (&row)[ROW])
{
    add_row(stats, slot_of(n_slots, cond, img), row);
}

// The (2r+1)^2 window minimum of a staged map, separably, by a block of THREADS.  G: dz_args or dc_args (r, halo, pad, sw, rows, q,
// c1).  In: b0 [g.rows][g.sw] staged (column pad - halo is pixel x0 - halo), behind a barrier.  Out: b0 [kTH + 2 q][c1] = the
// minimum at pixel (y0 - q + ii, x0 - q + j); OUTSIDE: -inf outside the frame (such positions take part in no maximum).  Ends with
// a barrier.  PAIRED: two taps per trip under AWSEG_TAPS, which the 512-thread kernels gain from; the dehazer's 256-thread kernels
// lose by it at r = 7 and keep the plain loop (profiles/restore_refactor_kernel_bench_hip_events.log).  No staged value is NaN (each
// went through unit()), so the order of the taps does not matter.
template <int THREADS, bool OUTSIDE, bool PAIRED, class G>
__device__ __forceinline__ void window_minimum(int H, int W, int y0, int x0, const G& g, float* __restrict__ b0, float* __restrict__ b1)
{
    const int tid = threadIdx.x, taps = 2 * g.r;
    const int rows_e = kTH + 2 * g.q;
    // minimum along the row: column j of b1 is pixel x0 - q + j
    for (int i = tid; i < g.rows * g.c1; i += THREADS) {
        const int row = i / g.c1, j = i - row * g.c1;
        const float* p = b0 + row * g.sw + (g.pad - g.halo) + j;
        float m = p[0];
        if constexpr (PAIRED) { AWSEG_TAPS for (int k = 1; k <= taps; k += 2) m = fminf(m, fminf(p[k], p[k + 1])); }
        else { for (int k = 1; k <= taps; ++k) m = fminf(m, p[k]); }
        b1[i] = m;
    }
    __syncthreads();
    // minimum down the column: row ii of b0 [rows_e][c1] is pixel row y0 - q + ii
    for (int i = tid; i < rows_e * g.c1; i += THREADS) {
        const int ii = i / g.c1, j = i - ii * g.c1;
        const float* p = b1 + i;
        float m = p[0];
        if constexpr (PAIRED) { AWSEG_TAPS for (int k = 1; k <= taps; k += 2) m = fminf(m, fminf(p[k * g.c1], p[(k + 1) * g.c1])); }
        else { for (int k = 1; k <= taps; ++k) m = fminf(m, p[k * g.c1]); }
        if constexpr (OUTSIDE) {
            const int yy = y0 - g.q + ii, xx = x0 - g.q + j;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) m = -INFINITY;
        }
        b0[i] = m;
    }
    __syncthreads();
}

inline bool is_finite(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }
inline bool in_unit(float v) { return v > 0.0f && v <= 1.0f; }             // NaN fails
inline bool in_closed_unit(float v) { return v >= 0.0f && v <= 1.0f; }

// The refusals every restoration launcher shares, in the order every entry point keeps; fills g's normalisation.  own_pointers:
// the launcher's outputs (and its workspace where it needs one) are there; own_parameters: its own parameters are in range.
#define AWSEG_RESTORE_CHECKS(g, own_pointers, own_parameters)                                                                   \
    if (!image || !mean || !std || !stats || !(own_pointers)) return AWSEG_EINVAL;                                              \
    if (channels != 3 || batch < 0 || height < 1 || width < 1 || n_slots < 1) return AWSEG_EINVAL;                              \
    if (!(own_parameters)) return AWSEG_EINVAL;                                                                                 \
    for (int c = 0; c < 3; ++c) {                                                                                               \
        if (!(std[c] > 0.0f && std[c] <= FLT_MAX) || !is_finite(mean[c])) return AWSEG_EINVAL;                                  \
        (g).mean[c] = mean[c];                                                                                                  \
        (g).std[c] = std[c];                                                                                                    \
    }                                                                                                                           \
    if (batch > 65535 || height > INT32_MAX / width) return AWSEG_ERANGE;      /* grid.y or grid.z; H * W >= 2^31 */            \
    if (workspace && !awseg_aligned(workspace, 8)) return AWSEG_EALIGN;        /* NULL: refused above where bytes are needed */ \
    if (batch == 0) return 0

}  // namespace
#endif  // AWSEG_RESTORE_COMMON_H
