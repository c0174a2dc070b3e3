// calib.hip — streaming temperature calibration: the per-pixel NLL and the ECE bins of the evaluated logits at every temperature
// of a grid, per condition slot, in one pass over the logits (replaces the per-pixel part of PKG/evaluation/metrics.py:266-321,
// ConfidenceCalibration.temperature_scale + optimize_temperature, which holds every logit of the evaluation set in memory).
//
// Per pixel with label != 255 (metrics.py:170), r = the logits the existing ECE sees, d_c = r_c - max r (computed once):
//   for each grid temperature t_k:  sum_k = sum_c exp(d_c / t_k)   (class order, exp2(d_c * log2(e)/t_k): __expf's own form)
//                                   conf_k = 1.0f / sum_k           -> ECE bin (lo, hi] {count, conf in units of 2^-30, correct}
//                                   nll_k  = log(sum_k) - d_y / t_k -> round(nll_k * 2^20), clamped at 2^11 (counted)
// At t_k == 1.0f every operation of the confidence is the one awseg_ece_accumulate / ensemble_stats_kernel performs, so the bins
// are bit-identical to theirs.
//
// Issue-bound: K x C exponentials per pixel against 4 B per logit.  The pixel's C logits (x 4 pixels per lane on the C = 19
// fast path; every CMAX instantiation keeps them in registers, no scratch) stay there while the lane walks the grid; the
// per-temperature constants are kernel arguments (SGPRs).  No per-lane LDS atomics: per temperature the wave first sums its
// 64 x 4 contributions (one 64-bit shuffle-tree sum for the NLL, one per DISTINCT bin for the ECE — neighbouring pixels share a
// bin, so that loop is short; the shuffles are ds_bpermute on the LDS pipe, and the bin search reads the staged edges from LDS),
// then one lane adds the wave's total to the block's LDS accumulators.  A block flushes its non-zero accumulators into the int64
// output with one global atomic each, into slot 0 and slot 1 + cond[img]: integer sums, independent of launch geometry and order.
#include "awseg_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerCU = 4;
constexpr int kMaxTemps = AWSEG_CALIB_MAX_TEMPS;
constexpr int kMaxClasses = AWSEG_CALIB_MAX_CLASSES;
constexpr float kLog2e = 0x1.715476p+0f;                    // the constant __expf multiplies by (exp(x) = exp2(log2e * x))
constexpr float kLn2 = 0x1.62e430p-1f;
constexpr float kNllScale = (float)(1 << AWSEG_CALIB_NLL_FRAC_BITS);
constexpr float kNllCap = (float)AWSEG_CALIB_NLL_CAP;
constexpr unsigned long long kNllCapQ = (unsigned long long)AWSEG_CALIB_NLL_CAP << AWSEG_CALIB_NLL_FRAC_BITS;
constexpr unsigned long long kLow40 = (1ull << 40) - 1;

// per-temperature constants, host-computed in float32 (IEEE division: the same values the device's `/` gives):
// t, s = log2(e)/t (exponent scale; == kLog2e exactly at t = 1), inv = 1/t.  Kernel arguments: wave-uniform scalar loads.
struct tgrid_consts { float t[kMaxTemps], s[kMaxTemps], inv[kMaxTemps]; };

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// MODE: 0 weighted, 2 mean (r = combine(seg1, seg2) [/T], ensemble_stats_kernel's roundings), 3 single logits (seg2 unused).
// PX pixels per lane (4: float4 loads, C = CT = 19; 1: any C <= CMAX).  Block (x, img) walks image img; temperatures [k0, k0 + kc).
template <int MODE, int LDT, int PX, int CT, int CMAX>
__global__ __launch_bounds__(kThreads)
void tgrid_kernel(const float* __restrict__ seg1, const float* __restrict__ seg2, int C, int64_t hw,
                  const float* __restrict__ weights, const float* __restrict__ temperature, const void* __restrict__ label,
                  const tgrid_consts tc, int k0, int kc, int n_temps, const float* __restrict__ edges, int n_bins,
                  const int32_t* __restrict__ cond, int n_slots, long long* __restrict__ stats)
{
    // LDS: nll[kc] | sat | nonfinite << 32 [kc] | count | correct << 32 [kc][n_bins] | conf q30 [kc][n_bins] | valid, oor | edges
    extern __shared__ unsigned long long s_mem[];
    unsigned long long* s_nll = s_mem;
    unsigned long long* s_sn = s_nll + kc;
    unsigned long long* s_cc = s_sn + kc;
    unsigned long long* s_q = s_cc + kc * n_bins;
    unsigned long long* s_misc = s_q + kc * n_bins;
    float* s_edges = reinterpret_cast<float*>(s_misc + 2);
    const int n_acc = 2 * kc + 2 * kc * n_bins + 2;
    for (int i = threadIdx.x; i < n_acc; i += kThreads) s_mem[i] = 0ull;
    for (int i = threadIdx.x; i <= n_bins; i += kThreads) s_edges[i] = edges[i];
    __syncthreads();

    if (CT > 0) C = CT;
    const int lane = threadIdx.x & 63;
    const int64_t img = blockIdx.y;
    const float* a = seg1 + img * C * hw;
    const float* dd = (MODE == 3) ? nullptr : seg2 + img * C * hw;
    float w0 = 0.f, w1 = 0.f, T = 1.f;
    const bool has_t = (MODE != 3) && temperature != nullptr;
    if (MODE == 0) { w0 = weights[0]; w1 = weights[1]; }
    if (has_t) T = temperature[0];

    const int64_t nvec = hw / PX;
    // block-uniform trip count: every lane of a wave takes part in the ballots and shuffles, lanes past the end as label 255
    for (int64_t v0 = (int64_t)blockIdx.x * kThreads; v0 < nvec; v0 += (int64_t)gridDim.x * kThreads) {
        const int64_t v = v0 + threadIdx.x;
        const bool live = v < nvec;
        const int64_t p = v * PX;
        int64_t y[PX];
        bool valid[PX], nll_ok[PX];
        bool lane_valid = false, lane_nll = false;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            y[j] = live ? awseg_ld_label<LDT>(label, img * hw + p + j) : 255;
            valid[j] = y[j] != 255;
            nll_ok[j] = valid[j] && y[j] >= 0 && y[j] < C;
            lane_valid |= valid[j];
            lane_nll |= nll_ok[j];
        }
        if (__ballot(lane_valid) == 0ull) continue;                 // nothing to count in this wave (wave-uniform)
        const bool any_nll = __ballot(lane_nll) != 0ull;

        // r, its argmax under the rule of the kernel whose ECE this one reproduces, d = r - max r
        float d[CMAX][PX];
        int bi[PX];
        float m[PX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c >= C) continue;                           // (not break: keeps the walk fully unrolled, d[] in registers)
            float x[PX], yv[PX];
            if (!live) {
#pragma unroll
                for (int j = 0; j < PX; ++j) { x[j] = 0.f; yv[j] = 0.f; }
            } else if constexpr (PX == 4) {
                const float4 xv = *reinterpret_cast<const float4*>(a + (int64_t)c * hw + p);
                x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w;
                if (MODE != 3) {
                    const float4 q = *reinterpret_cast<const float4*>(dd + (int64_t)c * hw + p);
                    yv[0] = q.x; yv[1] = q.y; yv[2] = q.z; yv[3] = q.w;
                }
            } else {
                x[0] = a[(int64_t)c * hw + p];
                if (MODE != 3) yv[0] = dd[(int64_t)c * hw + p];
            }
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                float rv;
                // four separately rounded float32 operations (built with -ffp-contract=off), as ensemble_stats_kernel
                if (MODE == 0) { float u = w0 * x[j]; float q = w1 * yv[j]; rv = u + q; }
                else if (MODE == 2) { float u = x[j] + yv[j]; rv = u / 2.f; }
                else rv = x[j];
                if (has_t) rv = rv / T;
                d[c][j] = rv;
                if (c == 0) { m[j] = rv; bi[j] = 0; }
                else if (MODE == 3) { if (rv > m[j]) { m[j] = rv; bi[j] = c; } }   // ece_kernel (metrics.hip)
                else awseg_amax_step(rv, c, m[j], bi[j]);                        // torch's argmax rule: ensemble_stats_kernel (with confusion)
            }
        }
        float dy[PX];
        bool correct[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            dy[j] = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if (c >= C) continue;                           // (not break: keeps the walk fully unrolled, d[] in registers)
                d[c][j] = d[c][j] - m[j];
                if ((int64_t)c == y[j]) dy[j] = d[c][j];
            }
            // the correctness test of the kernel reproduced: ece_kernel on registers / ensemble compare with (int)label, its strided form in int64
            correct[j] = (PX == 4 || MODE != 3) ? (bi[j] == (int)y[j]) : ((int64_t)bi[j] == y[j]);
        }
        {   // temperature-independent block counters: pixels entering the NLL, out-of-range labels (ECE only)
            unsigned long long nv = 0, no = 0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                nv += __popcll(__ballot(nll_ok[j]));
                no += __popcll(__ballot(valid[j] && !nll_ok[j]));
            }
            if (lane == 0) {
                if (nv) atomicAdd(&s_misc[0], nv);
                if (no) atomicAdd(&s_misc[1], no);
            }
        }

        for (int k = 0; k < kc; ++k) {
            const float t = tc.t[k], s = tc.s[k], inv = tc.inv[k];
            float conf[PX];
            unsigned long long nacc = 0;                            // nll q20 (bits 0-39) | saturated << 40 | non-finite << 52
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                float sum = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;                           // (not break: keeps the walk fully unrolled, d[] in registers)
                    sum += __builtin_amdgcn_exp2f(d[c][j] * s);
                }
                conf[j] = 1.0f / sum;
                if (nll_ok[j]) {
                    // d_y / t to within an ulp (one correction step: an unrounded 1/t would bias every pixel's NLL the same way)
                    const float q = dy[j] * inv;
                    const float e = fmaf(-q, t, dy[j]);
                    const float zy = fmaf(e, inv, q);
                    const float nll = kLn2 * __builtin_amdgcn_logf(sum) - zy;    // v_log_f32 = log2; sum in [1, C]
                    if (!(fabsf(nll) <= 3.0e38f)) nacc += 1ull << 52;
                    else if (nll > kNllCap) nacc += kNllCapQ + (1ull << 40);
                    else nacc += (unsigned long long)rintf(fmaxf(nll, 0.f) * kNllScale);
                }
            }
            if (any_nll) {
                nacc = wave_sum_u64(nacc);
                if (lane == 0 && nacc) {
                    atomicAdd(&s_nll[k], nacc & kLow40);
                    const unsigned long long sn = ((nacc >> 40) & 0xFFFull) | ((nacc >> 52) << 32);
                    if (sn) atomicAdd(&s_sn[k], sn);
                }
            }
            // ECE: one wave sum per distinct bin (count << 40 | correct << 52 | conf q30; a wave has <= 256 pixels)
            int bin[PX];
            unsigned pend = 0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                bin[j] = valid[j] ? awseg_ece_find_bin(conf[j], s_edges, n_bins) : -1;
                if (bin[j] >= 0) pend |= 1u << j;
            }
            unsigned long long* cc = s_cc + (int64_t)k * n_bins;
            unsigned long long* cq = s_q + (int64_t)k * n_bins;
            for (;;) {
                const unsigned long long lanes = __ballot(pend != 0u);
                if (!lanes) break;
                const int src = __ffsll((long long)lanes) - 1;
                int mine = -1;
#pragma unroll
                for (int j = PX - 1; j >= 0; --j) if ((pend >> j) & 1u) mine = bin[j];
                const int b0 = __shfl(mine, src, 64);
                unsigned long long acc = 0;
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    if (((pend >> j) & 1u) && bin[j] == b0) {
                        acc += awseg_conf_q30(conf[j]) + (1ull << 40) + ((unsigned long long)correct[j] << 52);
                        pend &= ~(1u << j);
                    }
                }
                acc = wave_sum_u64(acc);
                if (lane == src) {
                    atomicAdd(&cc[b0], ((acc >> 40) & 0xFFFull) | ((acc >> 52) << 32));
                    atomicAdd(&cq[b0], acc & kLow40);
                }
            }
        }
    }
    __syncthreads();

    // flush: out[slot][k0 + k][4 + 3 n_bins] = {count, nll q20, saturated, non-finite, n_bins x {count, conf q30, correct}},
    // out[slot][n_temps][0] = out-of-range labels (added by the launch of the first chunk only)
    int slot = -1;
    if (cond) { const int cv = cond[img]; if (cv >= 0 && cv + 1 < n_slots) slot = cv + 1; }
    const int R = 4 + 3 * n_bins;
    const int64_t slot_stride = (int64_t)(n_temps + 1) * R;
    const unsigned long long valid_px = s_misc[0];
    for (int i = threadIdx.x; i < kc * R; i += kThreads) {
        const int k = i / R, f = i - k * R;
        unsigned long long val;
        if (f == 0) val = valid_px - (s_sn[k] >> 32);
        else if (f == 1) val = s_nll[k];
        else if (f == 2) val = s_sn[k] & 0xFFFFFFFFull;
        else if (f == 3) val = s_sn[k] >> 32;
        else {
            const int b = (f - 4) / 3, w = (f - 4) - 3 * b;
            const unsigned long long c2 = s_cc[(int64_t)k * n_bins + b];
            val = w == 0 ? (c2 & 0xFFFFFFFFull) : (w == 1 ? s_q[(int64_t)k * n_bins + b] : (c2 >> 32));
        }
        if (val) {
            const int64_t o = (int64_t)(k0 + k) * R + f;
            atomicAdd((unsigned long long*)&stats[o], val);
            if (slot > 0) atomicAdd((unsigned long long*)&stats[slot * slot_stride + o], val);
        }
    }
    if (k0 == 0 && threadIdx.x == 0 && s_misc[1]) {
        const int64_t o = (int64_t)n_temps * R;
        atomicAdd((unsigned long long*)&stats[o], s_misc[1]);
        if (slot > 0) atomicAdd((unsigned long long*)&stats[slot * slot_stride + o], s_misc[1]);
    }
}

constexpr size_t kLdsBudget = 48 * 1024;     // four 256-thread blocks per CU at K = 100, 15 bins (27 KB)

size_t lds_bytes(int kc, int n_bins) { return sizeof(unsigned long long) * (2 * (size_t)kc + 2 * (size_t)kc * n_bins + 2) + sizeof(float) * 65; }

int check_common(int64_t batch, int num_classes, int64_t hw, const void* label, int label_dtype, const float* temps, int n_temps,
                 const float* edges, int n_bins, const int64_t* stats, int n_slots)
{
    if (!label || !temps || !edges || !stats) return AWSEG_EINVAL;
    if (batch < 1 || batch > 65535 || hw < 1 || num_classes < 1 || num_classes > kMaxClasses || n_slots < 1) return AWSEG_EINVAL;
    if (n_temps < 1 || n_temps > kMaxTemps || n_bins < 1 || n_bins > 64) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    for (int k = 0; k < n_temps; ++k)
        if (!(temps[k] > 0.f) || !(temps[k] <= 3.4028234663852886e38f)) return AWSEG_EINVAL;   // NaN, <= 0, inf
    return 0;
}

struct tgrid_launch {                                     // the arguments of one entry point, as the kernel takes them
    const float *seg1, *seg2; int64_t batch; int C; int64_t hw; const float *weights, *temperature; const void* label;
    const int32_t* cond; const float* temps; int n_temps; const float* edges; int n_bins; int64_t* stats; int n_slots; hipStream_t s;
};

template <int MODE, int LDT, int PX, int CT, int CMAX>
int launch_chunks(const tgrid_launch& g)
{
    auto kern = tgrid_kernel<MODE, LDT, PX, CT, CMAX>;
    int kc_max = g.n_temps;
    while (kc_max > 1 && lds_bytes(kc_max, g.n_bins) > kLdsBudget) --kc_max;
    dim3 grid((unsigned)awseg_blocks_per_image(g.hw / PX, kThreads, g.batch, kBlocksPerCU), (unsigned)g.batch), block(kThreads);
    for (int k0 = 0; k0 < g.n_temps; k0 += kc_max) {        // more temperatures x bins than the LDS budget holds: re-read the logits
        const int kc = g.n_temps - k0 < kc_max ? g.n_temps - k0 : kc_max;
        tgrid_consts tc;
        for (int k = 0; k < kMaxTemps; ++k) {
            const float t = k < kc ? g.temps[k0 + k] : 1.0f;
            tc.t[k] = t; tc.s[k] = kLog2e / t; tc.inv[k] = 1.0f / t;
        }
        hipLaunchKernelGGL(kern, grid, block, lds_bytes(kc, g.n_bins), g.s, g.seg1, g.seg2, g.C, g.hw, g.weights, g.temperature, g.label, tc,
                           k0, kc, g.n_temps, g.edges, g.n_bins, g.cond, g.n_slots, (long long*)g.stats);
        AWSEG_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

AWSEG_API int awseg_temperature_grid_stats(const float* logits, int64_t batch, int num_classes, int64_t hw, const void* label,
                                           int label_dtype, const int32_t* cond, const float* temps, int n_temps,
                                           const float* edges, int n_bins, int64_t* stats, int n_slots, awseg_stream_t stream)
{
    if (!logits) return AWSEG_EINVAL;
    if (int rc = check_common(batch, num_classes, hw, label, label_dtype, temps, n_temps, edges, n_bins, stats, n_slots)) return rc;
    const tgrid_launch g = { logits, nullptr, batch, num_classes, hw, nullptr, nullptr, label, cond, temps, n_temps, edges, n_bins, stats,
                             n_slots, awseg_s(stream) };
    const bool vec19 = (num_classes == 19) && !(hw & 3) && awseg_aligned(logits, 16);   // the ECE's condition for its vector kernel
    return awseg_by_label(label_dtype, [&](auto L) {
        constexpr int l = decltype(L)::value;
        if (vec19) return launch_chunks<3, l, 4, 19, 19>(g);
        if (num_classes <= 8) return launch_chunks<3, l, 1, 0, 8>(g);
        if (num_classes <= 16) return launch_chunks<3, l, 1, 0, 16>(g);
        if (num_classes <= 32) return launch_chunks<3, l, 1, 0, 32>(g);
        return launch_chunks<3, l, 1, 0, 64>(g);
    });
}

AWSEG_API int awseg_ensemble_temperature_grid_stats(const float* seg1, const float* seg2, int64_t batch, int num_classes, int64_t hw,
                                                    int mode, const float* weights, const float* temperature, const void* label,
                                                    int label_dtype, const int32_t* cond, const float* temps, int n_temps,
                                                    const float* edges, int n_bins, int64_t* stats, int n_slots,
                                                    awseg_stream_t stream)
{
    if (!seg1 || !seg2) return AWSEG_EINVAL;
    if (int rc = check_common(batch, num_classes, hw, label, label_dtype, temps, n_temps, edges, n_bins, stats, n_slots)) return rc;
    if (num_classes != 19) return AWSEG_ERANGE;                  // awseg_combine_confusion_stats' eligibility
    if (mode != AWSEG_COMBINE_WEIGHTED && mode != AWSEG_COMBINE_MEAN) return AWSEG_ERANGE;
    if (mode == AWSEG_COMBINE_WEIGHTED && !weights) return AWSEG_EINVAL;
    if ((hw & 3) || !awseg_aligned(seg1, 16) || !awseg_aligned(seg2, 16)) return AWSEG_EALIGN;
    const tgrid_launch g = { seg1, seg2, batch, 19, hw, weights, temperature, label, cond, temps, n_temps, edges, n_bins, stats, n_slots,
                             awseg_s(stream) };
    return awseg_by_combine_mode(mode, [&](auto M) { return awseg_by_label(label_dtype, [&](auto L) {
        return launch_chunks<decltype(M)::value, decltype(L)::value, 4, 19, 19>(g);
    }); });
}
