// weightgrid.hip — ensemble weight sweep: the mIoU counters of argmax(w0 * seg1 + w1 * seg2) at every weight pair of a grid, and
// how the two members' own predictions split the labelled pixels, per condition slot, in one pass over the member logits
// (DESIGN.md §10m).  The mIoU per grid point, the best and the fitted weighting and the member shares are host math on these
// integer counts (evaluation/metrics.py weight_grid_metrics_from_stats).
//
// Per labelled pixel (label neither ignore_index nor outside [0, C)):
//   for each grid point g:  r_c = awseg_combine<0>(seg1_c, seg2_c, w[g][0], w[g][1], false, 0)   (two products, one sum, each rounded)
//                           pred_g = argmax r under awseg_amax_step      -> predicted[pred_g] += 1, hit[pred_g] += (pred_g == label)
//   m1 / m2 = argmax of seg1 / seg2 alone under the same rule (raw logits: 0 * inf is NaN at the grid's ends)
//                                                                       -> labelled[label], both / only m1 / only m2 right, m1 != m2
// Built with -ffp-contract=off like metrics.hip, whose combine kernels these predictions equal at the model's own weights.
//
// Issue-bound: G x C combines and argmax steps per pixel against 8 B per class.  A lane keeps its pixel's 2 x C logits in registers
// and walks the grid, whose weights are kernel arguments (scalar loads); the maps are read once.  Counters: predicted[c] and hit[c]
// of one grid point are touched for the SAME c (a hit is a prediction of the label), so they share one 64-bit LDS cell (predicted
// in the low half, hits in the high half: neither half can carry, a block counts fewer than 2^31 pixels) and take one ds_add_u64
// per pixel and grid point.  Across lanes the adds stay plain LDS atomics: merging the lanes of a wave by ballot and shuffle cost
// more than the same-address adds it saved in failure.hip (see there), and coherent (trained-like) maps time like random ones here.
// grid.y = frame, so a block serves one slot pair; it flushes its non-zero cells once with 64-bit global atomics into slot 0 and
// the frame's slot.
//
// Launch shape, measured at 8 x 19 x 1024 x 2048 (profiles/weightgrid_kernel_bench_hip_events.log): the pass wants waves, not
// pixels per lane.  At 18 points and four 256-thread blocks per CU, one pixel per lane (50 VGPRs) takes 1.07 ms, two (91 VGPRs,
// with the lane merging its pixels of one prediction into one add) 1.34 ms, four (177 VGPRs, two waves per SIMD) 1.83 ms.  With one
// pixel per lane, 512 threads x 4 resident blocks per CU (8 waves per SIMD asked for, 7 fit) takes 0.95 ms, as 256 x 8 does with
// twice the flushes; 512 x 2, 256 x 4 and 1024 x 2 take 1.07 ms.  So: one pixel per lane, 512 threads, and the 16-byte alignment
// the contract asks for is not used by the loads.
#include "awseg_logitscan.h"

namespace {

constexpr int kThreads = 512;
constexpr int kBlocksPerCU = 4;             // resident per CU: 8 waves per SIMD asked for (50 VGPRs: profiles/weightgrid_resource_usage.log)
constexpr int kC = 19;
constexpr int kMaxPoints = AWSEG_WGRID_MAX_POINTS;
constexpr int kMisc = 4 * kC + 3;           // labelled | both right | only m1 | only m2 | {out of range, NaN pixel, m1 != m2}

struct wgrid_weights { float w0[kMaxPoints], w1[kMaxPoints]; };     // kernel arguments: wave-uniform scalar loads

// block (x, img) walks frame img, one pixel per lane
template <int LDT>
__global__ __launch_bounds__(kThreads)
void wgrid_kernel(const float* __restrict__ seg1, const float* __restrict__ seg2, int64_t hw, const wgrid_weights wt, int n_points,
                  const void* __restrict__ label, int ignore_index, const int32_t* __restrict__ cond, int n_slots,
                  long long* __restrict__ stats)
{
    extern __shared__ unsigned long long s_cell[];          // [n_points][kC]: predicted | hit << 32, then uint32 s_misc[kMisc]
    uint32_t* s_misc = reinterpret_cast<uint32_t*>(s_cell + n_points * kC);
    for (int i = threadIdx.x; i < n_points * kC; i += kThreads) s_cell[i] = 0ull;
    for (int i = threadIdx.x; i < kMisc; i += kThreads) s_misc[i] = 0u;
    __syncthreads();

    const int64_t img = blockIdx.y;
    const float* a = seg1 + img * kC * hw;
    const float* d = seg2 + img * kC * hw;
    for (int64_t p0 = (int64_t)blockIdx.x * kThreads; p0 < hw; p0 += (int64_t)gridDim.x * kThreads) {
        const int64_t p = p0 + threadIdx.x;
        const bool live = p < hw;
        const int64_t t = live ? awseg_ld_label<LDT>(label, img * hw + p) : (int64_t)ignore_index;
        const bool in = t >= 0 && t < kC;
        const int y = (in && t != ignore_index) ? (int)t : -1;      // the label of a labelled pixel, -1 otherwise
        if (t != ignore_index && !in) atomicAdd(&s_misc[4 * kC + 0], 1u);
        if (__ballot(y >= 0) == 0ull) continue;             // nothing to count in this wave (wave-uniform)

        float x[kC], z[kC];
#pragma unroll
        for (int c = 0; c < kC; ++c) {
            x[c] = live ? a[(int64_t)c * hw + p] : 0.f;
            z[c] = live ? d[(int64_t)c * hw + p] : 0.f;
        }
        {   // the members on their own
            float b1 = x[0], b2 = z[0];
            int m1 = 0, m2 = 0;
            bool nan = (b1 != b1) || (b2 != b2);
#pragma unroll
            for (int c = 1; c < kC; ++c) {
                awseg_amax_step(x[c], c, b1, m1);
                awseg_amax_step(z[c], c, b2, m2);
                nan |= (x[c] != x[c]) || (z[c] != z[c]);
            }
            if (y >= 0) {
                atomicAdd(&s_misc[y], 1u);
                const bool r1 = m1 == y, r2 = m2 == y;
                if (r1 || r2) atomicAdd(&s_misc[(r1 && r2 ? 1 : (r1 ? 2 : 3)) * kC + y], 1u);
                if (nan) atomicAdd(&s_misc[4 * kC + 1], 1u);
                if (m1 != m2) atomicAdd(&s_misc[4 * kC + 2], 1u);
            }
        }
        for (int g = 0; g < n_points; ++g) {
            const float w0 = wt.w0[g], w1 = wt.w1[g];
            float best = awseg_combine<0>(x[0], z[0], w0, w1, false, 0.f);
            int pred = 0;
#pragma unroll
            for (int c = 1; c < kC; ++c) awseg_amax_step(awseg_combine<0>(x[c], z[c], w0, w1, false, 0.f), c, best, pred);
            if (y >= 0) atomicAdd(&s_cell[g * kC + pred], 1ull + ((unsigned long long)(pred == y) << 32));
        }
    }
    __syncthreads();

    // flush: stats[slot][g][c] = hits, [g][kC + c] = predicted; rows n_points .. n_points + 2 from s_misc; non-zero values only
    int slot = -1;
    if (cond) { const int cv = cond[img]; if (cv >= 0 && cv + 1 < n_slots) slot = cv + 1; }
    const int64_t slot_stride = (int64_t)AWSEG_WGRID_ROWS(n_points) * 2 * kC;
    unsigned long long* out0 = reinterpret_cast<unsigned long long*>(stats);
    unsigned long long* out1 = slot > 0 ? out0 + slot * slot_stride : nullptr;
    for (int i = threadIdx.x; i < n_points * kC; i += kThreads) {
        const unsigned long long val = s_cell[i];
        if (!val) continue;
        const int g = i / kC, c = i - g * kC;
        const unsigned long long hit = val >> 32, predicted = val & 0xFFFFFFFFull;
        const int64_t o = (int64_t)g * 2 * kC + c;
        if (hit) { atomicAdd(&out0[o], hit); if (out1) atomicAdd(&out1[o], hit); }
        atomicAdd(&out0[o + kC], predicted);
        if (out1) atomicAdd(&out1[o + kC], predicted);
    }
    for (int i = threadIdx.x; i < kMisc; i += kThreads) {
        const unsigned long long val = s_misc[i];
        if (!val) continue;
        // labelled, both: row n_points; only m1, only m2: row n_points + 1 (each [c], [kC + c]); the three singles: row n_points + 2
        const int64_t o = (int64_t)n_points * 2 * kC + i;
        atomicAdd(&out0[o], val);
        if (out1) atomicAdd(&out1[o], val);
    }
}

size_t lds_bytes(int n_points) { return sizeof(unsigned long long) * (size_t)n_points * kC + sizeof(uint32_t) * kMisc; }

}  // namespace

AWSEG_API int awseg_ensemble_weight_grid_stats(const float* seg1, const float* seg2, int64_t batch, int num_classes, int64_t hw,
                                               const float* weights, int n_points, const void* label, int label_dtype,
                                               int ignore_index, const int32_t* cond, int64_t* stats, int n_slots,
                                               awseg_stream_t stream)
{
    if (!seg1 || !seg2 || !weights || !label || !stats) return AWSEG_EINVAL;
    if (batch < 1 || num_classes < 1 || hw < 1 || n_slots < 1) return AWSEG_EINVAL;
    if (n_points < 1 || n_points > kMaxPoints) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    wgrid_weights wt;
    for (int g = 0; g < kMaxPoints; ++g) {
        const float w0 = g < n_points ? weights[2 * g] : 0.f, w1 = g < n_points ? weights[2 * g + 1] : 0.f;
        if (!(w0 >= 0.f) || !(w0 <= 3.4028234663852886e38f) || !(w1 >= 0.f) || !(w1 <= 3.4028234663852886e38f)) return AWSEG_EINVAL;
        wt.w0[g] = w0; wt.w1[g] = w1;
    }
    if (num_classes != kC || hw > INT32_MAX || batch > 65535) return AWSEG_ERANGE;
    if ((hw & 3) || !awseg_aligned(seg1, 16) || !awseg_aligned(seg2, 16)) return AWSEG_EALIGN;
    const dim3 grid((unsigned)awseg_blocks_per_image(hw, kThreads, batch, kBlocksPerCU), (unsigned)batch), block(kThreads);
    return awseg_by_label(label_dtype, [&](auto L) {
        hipLaunchKernelGGL(wgrid_kernel<decltype(L)::value>, grid, block, lds_bytes(n_points), awseg_s(stream), seg1, seg2, hw, wt,
                           n_points, label, ignore_index, cond, n_slots, (long long*)stats);
        AWSEG_LAUNCH_CHECK();
        return 0;
    });
}
