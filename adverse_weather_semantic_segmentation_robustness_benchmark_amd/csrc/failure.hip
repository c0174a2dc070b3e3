// failure.hip — failure-detection counters: per condition slot and per uncertainty score, a histogram of the score split by
// "the prediction was right / wrong", in one pass over the member logits.  AUROC, its computed uncertainty, AURC
// and excess AURC are host math on these integer counts (evaluation/metrics.py failure_metrics_from_hist).
//
// Scores (float32, higher = less certain), per pixel with a label in [0, C):
//   0 mi        H(m) - (H(p1) + H(p2))/2, m = (p1 + p2)/2: ensemble_stats_kernel's expressions, operation for operation
//   1 entropy   H(m) = -sum m log(m + 1e-8)
//   2 variance  sum_c (p1_c - p2_c)^2 / 2
//   3 msp       1 - 1.0f / sum exp(r - max r), r = combine(seg1, seg2)/T as ensemble_stats_kernel forms it, or read from `combined`
// rows 0-2 are flagged by argmax(m) != label, row 3 by argmax(r) != label (first maximum).  The single-model form fills rows 1
// and 3 from softmax(logits).  Built with -ffp-contract=off like metrics.hip.
//
// Bin = clamp((int32(bits(s)) - (105 << 23)) >> 16, 0, 3071): 24 octaves of 128 steps from 2^-22 to 4.0, three integer
// instructions, every edge an exact float32.
//
// Shape.  grid.y = frame, so a block serves one slot pair.  The block's histogram lives in LDS as uint32 (4 x 2 x 3072 x 4 B =
// 96 KB: one block per CU, hence 1024 threads = four waves per SIMD on the C = 19 path) and is flushed once: non-zero cells only,
// 64-bit global atomics into slot 0 and the frame's slot.  A lane adds its four cells with plain LDS atomics.  Measured at
// 8 x 19 x 1024 x 2048 (profiles/failure_kernel_bench_hip_events.log): merging the lanes of a wave that hold the
// same cell into one add (ballot + shuffle, one or two rounds) costs 1.8 - 3.2 ms against 0.73 - 1.08 ms without, on random and
// on trained-like logits alike (most of a wave in bin 0 of three rows there): the LDS unit absorbs the same-address adds, the
// ballots do not come free.  Of the launch shapes, 1024 threads x one pixel per lane (0.73 / 0.77 ms; the compiler's figures are in
// DESIGN.md 10e) beat 512 x 4 (0.75 / 0.78), 512 x 2 (0.81 / 0.82) and 1024 x 2 (1.05 / 1.08, 157 - 184 spilled registers).  So
// the C = 19 path needs no vector loads and takes any hw; the one-pass statistics kernel takes 0.71 ms on the same tensors.
#include "awseg_common.h"

namespace {

constexpr int kBins = AWSEG_FAIL_BINS;
constexpr int kBinBase = 105 << 23;                         // bits of 2^-22
constexpr int kCells = 2 * kBins;                           // one score: [flag][bin]

__device__ __forceinline__ int fail_bin(float s)
{
    int i = (int)__float_as_uint(s);                        // a negative float is a negative int32: bin 0
    i = i < kBinBase ? kBinBase : i;                        // (clamped BEFORE the subtraction: -0.0f is INT32_MIN)
    const int b = (i - kBinBase) >> 16;
    return b > kBins - 1 ? kBins - 1 : b;
}

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= 3.4028234663852886e38f); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// MODE: 0 weighted, 2 mean (r = combine(seg1, seg2) [/T], ensemble_stats_kernel's roundings), 4 r read from `comb`,
//       3 single logits (seg2, comb unused; rows entropy and msp only).
// TH threads, PX pixels per lane (4: 16-byte loads, single logits at C = 19; 1: any hw), CT > 0: the class count, unrolled.
template <int MODE, int LDT, int TH, int PX, int CT, int CMAX>
__global__ __launch_bounds__(TH)
void failure_kernel(const float* __restrict__ seg1, const float* __restrict__ seg2, const float* __restrict__ comb, int C, int64_t hw,
                    const float* __restrict__ weights, const float* __restrict__ temperature, const void* __restrict__ label,
                    const int32_t* __restrict__ cond, int n_slots, long long* __restrict__ stats)
{
    constexpr int NR = MODE == 3 ? 2 : AWSEG_FAIL_SCORES;   // score rows this kernel fills (single: entropy, msp)
    extern __shared__ uint32_t s_hist[];                    // [NR][2][kBins], then {counted, non-finite, out of range}
    uint32_t* s_misc = s_hist + NR * kCells;
    for (int i = threadIdx.x; i < NR * kCells + 3; i += TH) s_hist[i] = 0u;
    __syncthreads();

    if (CT > 0) C = CT;
    const int lane = threadIdx.x & (AWSEG_WAVE - 1);
    const int64_t img = blockIdx.y;
    const float* a = seg1 + img * C * hw;
    const float* d = MODE == 3 ? nullptr : seg2 + img * C * hw;
    const float* cb = MODE == 4 ? comb + img * C * hw : nullptr;
    float w0 = 0.f, w1 = 0.f, T = 1.f;
    const bool has_t = (MODE == 0 || MODE == 2) && temperature != nullptr;
    if (MODE == 0) { w0 = weights[0]; w1 = weights[1]; }
    if (has_t) T = temperature[0];
    uint32_t n_px = 0, n_bad = 0, n_oor = 0;

    typedef float lvec __attribute__((ext_vector_type(PX > 1 ? PX : 2)));
    const int64_t nvec = hw / PX;
    for (int64_t v0 = (int64_t)blockIdx.x * TH; v0 < nvec; v0 += (int64_t)gridDim.x * TH) {
        const int64_t v = v0 + threadIdx.x;
        const bool live = v < nvec;
        const int64_t p = live ? v * PX : 0;
        float x[CMAX][PX], y[MODE == 3 ? 1 : CMAX][PX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c >= C) continue;                           // (not break: keeps the walk fully unrolled, the vectors in registers)
            if constexpr (PX > 1) {
                const lvec xv = live ? *reinterpret_cast<const lvec*>(a + (int64_t)c * hw + p) : (lvec)(0.f);
#pragma unroll
                for (int k = 0; k < PX; ++k) x[c][k] = xv[k];
                if constexpr (MODE != 3) {
                    const lvec yv = live ? *reinterpret_cast<const lvec*>(d + (int64_t)c * hw + p) : (lvec)(0.f);
#pragma unroll
                    for (int k = 0; k < PX; ++k) y[c][k] = yv[k];
                }
            } else {
                x[c][0] = live ? a[(int64_t)c * hw + p] : 0.f;
                if constexpr (MODE != 3) y[c][0] = live ? d[(int64_t)c * hw + p] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const int64_t t = live ? awseg_ld_label<LDT>(label, img * hw + p + k) : 255;
            const bool lab_ok = t >= 0 && t < C;
            n_oor += (t != 255 && !lab_ok) ? 1u : 0u;
            bool bad = false;
            int b_ent, b_msp, f_mean, f_r;                  // bins and error flags
            int b_mi = 0, b_var = 0;
            if constexpr (MODE == 3) {
                // softmax(logits): the maximum, exponentials and their sum in class order as ece_kernel (metrics.hip) forms them
                float m = x[0][k]; int bi = 0;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;
                    bad |= not_finite(x[c][k]);
                    if (c > 0 && x[c][k] > m) { m = x[c][k]; bi = c; }
                }
                float z = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;
                    x[c][k] = __expf(x[c][k] - m);
                    z += x[c][k];
                }
                const float conf = 1.0f / z;
                float h = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;
                    const float pc = x[c][k] * conf;
                    h -= pc * __logf(pc + 1e-8f);
                }
                b_ent = fail_bin(h);
                b_msp = fail_bin(1.0f - conf);
                f_mean = f_r = ((int64_t)bi != t) ? 1 : 0;
            } else {
                // r, its first maximum and sum-exp: the calibration part of ensemble_stats_kernel
                float rmax = -INFINITY, rsum = 0.f; int rarg = 0;
                float r[CMAX];
                float m1 = x[0][k], m2 = y[0][k];
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;
                    float rv;
                    if (MODE == 0) { float u = w0 * x[c][k]; float q = w1 * y[c][k]; rv = u + q; }
                    else if (MODE == 2) { float u = x[c][k] + y[c][k]; rv = u / 2.f; }
                    else { rv = live ? cb[(int64_t)c * hw + p + k] : 0.f; bad |= not_finite(rv); }
                    if (has_t) rv = rv / T;
                    r[c] = rv;
                    if (c == 0 || rv > rmax) { rmax = rv; rarg = c; }
                    bad |= not_finite(x[c][k]) || not_finite(y[c][k]);
                    m1 = fmaxf(m1, x[c][k]); m2 = fmaxf(m2, y[c][k]);
                }
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;
                    rsum += __expf(r[c] - rmax);
                }
                const float conf = 1.0f / rsum;
                // member softmaxes and entropies, the mixture entropy and the argmax of the mean probability: the disagreement
                // part of ensemble_stats_kernel (see there for the logarithm-free member entropy)
                float z1 = 0.f, z2 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;
                    const float d1 = x[c][k] - m1, d2 = y[c][k] - m2;
                    x[c][k] = __expf(d1); y[c][k] = __expf(d2);
                    z1 += x[c][k]; z2 += y[c][k];
                    t1 = fmaf(x[c][k], d1, t1); t2 = fmaf(y[c][k], d2, t2);
                }
                const float i1 = 1.0f / z1, i2 = 1.0f / z2;
                const float h1 = __logf(z1) - t1 * i1, h2 = __logf(z2) - t2 * i2;
                float hm = 0.f, mbest = -1.f, var = 0.f; int marg = 0;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c >= C) continue;
                    const float p1 = x[c][k] * i1, p2 = y[c][k] * i2;
                    const float mp = (p1 + p2) * 0.5f;
                    hm -= mp * __logf(mp + 1e-8f);
                    if (mp > mbest) { mbest = mp; marg = c; }
                    const float dp = p1 - p2;
                    var += dp * dp;
                }
                const float score = hm - (h1 + h2) * 0.5f;
                b_mi = fail_bin(score);
                b_ent = fail_bin(hm);
                b_var = fail_bin(var * 0.5f);
                b_msp = fail_bin(1.0f - conf);
                f_mean = (marg != (int)t) ? 1 : 0;
                f_r = (rarg != (int)t) ? 1 : 0;
            }
            const bool on = lab_ok && !bad;
            n_px += on ? 1u : 0u;
            n_bad += (lab_ok && bad) ? 1u : 0u;
            if constexpr (MODE == 3) {
                if (on) atomicAdd(&s_hist[f_mean * kBins + b_ent], 1u);
                if (on) atomicAdd(&s_hist[kCells + f_r * kBins + b_msp], 1u);
            } else {
                if (on) atomicAdd(&s_hist[AWSEG_FAIL_MI * kCells + f_mean * kBins + b_mi], 1u);
                if (on) atomicAdd(&s_hist[AWSEG_FAIL_ENTROPY * kCells + f_mean * kBins + b_ent], 1u);
                if (on) atomicAdd(&s_hist[AWSEG_FAIL_VARIANCE * kCells + f_mean * kBins + b_var], 1u);
                if (on) atomicAdd(&s_hist[AWSEG_FAIL_MSP * kCells + f_r * kBins + b_msp], 1u);
            }
        }
    }
    n_px = wave_sum_u32(n_px); n_bad = wave_sum_u32(n_bad); n_oor = wave_sum_u32(n_oor);
    if (lane == 0) {
        if (n_px) atomicAdd(&s_misc[0], n_px);
        if (n_bad) atomicAdd(&s_misc[1], n_bad);
        if (n_oor) atomicAdd(&s_misc[2], n_oor);
    }
    __syncthreads();

    // flush: stats[slot][score][flag][bin], then {counted, non-finite, out of range, 0}; non-zero cells only
    int slot = -1;
    if (cond) { const int cv = cond[img]; if (cv >= 0 && cv + 1 < n_slots) slot = cv + 1; }
    for (int i = threadIdx.x; i < NR * kCells + 3; i += TH) {
        const uint32_t val = s_hist[i];
        if (!val) continue;
        int64_t o;
        if (i >= NR * kCells) o = (int64_t)AWSEG_FAIL_SCORES * kCells + (i - NR * kCells);
        else if (MODE == 3) o = (int64_t)(i < kCells ? AWSEG_FAIL_ENTROPY : AWSEG_FAIL_MSP) * kCells + (i < kCells ? i : i - kCells);
        else o = i;
        atomicAdd((unsigned long long*)&stats[o], (unsigned long long)val);
        if (slot > 0) atomicAdd((unsigned long long*)&stats[(int64_t)slot * AWSEG_FAIL_ROW + o], (unsigned long long)val);
    }
}

struct fail_launch {                                      // the arguments of one entry point, as the kernel takes them
    const float *seg1, *seg2, *comb; int64_t batch; int C; int64_t hw; const float *weights, *temperature; const void* label;
    const int32_t* cond; int64_t* stats; int n_slots; hipStream_t s;
};

template <int MODE, int LDT, int TH, int PX, int CT, int CMAX>
int launch(const fail_launch& g)
{
    auto kern = failure_kernel<MODE, LDT, TH, PX, CT, CMAX>;
    constexpr int NR = MODE == 3 ? 2 : AWSEG_FAIL_SCORES;
    const size_t lds = ((size_t)NR * kCells + 3) * sizeof(uint32_t);
    // resident blocks per CU: one 96 KB histogram (ensemble); two 512-thread blocks of the single kernel (48 KB each; its
    // 102 registers at C = 19 allow four waves per SIMD)
    const int bpi = awseg_blocks_per_image(g.hw / PX, TH, g.batch, MODE == 3 ? 2 : 1);
    // (per launch, not once: the attribute belongs to the current device's copy of the kernel)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
        return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)bpi, (unsigned)g.batch), dim3(TH), lds, g.s, g.seg1, g.seg2, g.comb, g.C, g.hw, g.weights,
                       g.temperature, g.label, g.cond, g.n_slots, (long long*)g.stats);
    AWSEG_LAUNCH_CHECK();
    return 0;
}

template <int MODE>
int launch_ensemble(const fail_launch& g, int label_dtype)
{
    return awseg_by_label(label_dtype, [&](auto L) {
        if (g.C == 19) return launch<MODE, decltype(L)::value, 1024, 1, 19, 19>(g);
        return launch<MODE, decltype(L)::value, 512, 1, 0, AWSEG_MAX_CLASSES>(g);
    });
}

int check_common(int64_t batch, int num_classes, int64_t hw, const void* label, int label_dtype, const int64_t* stats, int n_slots)
{
    if (!label || !stats) return AWSEG_EINVAL;
    if (batch < 0 || num_classes < 1 || hw < 1 || n_slots < 1) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    return 0;
}

}  // namespace

AWSEG_API int awseg_ensemble_failure_stats(const float* seg1, const float* seg2, const float* combined, int64_t batch, int num_classes,
                                           int64_t hw, int mode, const float* weights, const float* temperature, const void* label,
                                           int label_dtype, const int32_t* cond, int64_t* stats, int n_slots, awseg_stream_t stream)
{
    if (!seg1 || !seg2) return AWSEG_EINVAL;
    if (int rc = check_common(batch, num_classes, hw, label, label_dtype, stats, n_slots)) return rc;
    if (!combined) {
        if (mode != AWSEG_COMBINE_WEIGHTED && mode != AWSEG_COMBINE_MEAN) return AWSEG_EINVAL;   // MAXCONF: hand over `combined`
        if (mode == AWSEG_COMBINE_WEIGHTED && !weights) return AWSEG_EINVAL;
    }
    if (num_classes > AWSEG_MAX_CLASSES || hw > INT32_MAX || batch > 65535) return AWSEG_ERANGE;
    if (batch == 0) return 0;
    const fail_launch g = { seg1, seg2, combined, batch, num_classes, hw, weights, temperature, label, cond, stats, n_slots, awseg_s(stream) };
    if (combined) return launch_ensemble<4>(g, label_dtype);
    return awseg_by_combine_mode(mode, [&](auto M) { return launch_ensemble<decltype(M)::value>(g, label_dtype); });
}

AWSEG_API int awseg_failure_stats(const float* logits, int64_t batch, int num_classes, int64_t hw, const void* label, int label_dtype,
                                  const int32_t* cond, int64_t* stats, int n_slots, awseg_stream_t stream)
{
    if (!logits) return AWSEG_EINVAL;
    if (int rc = check_common(batch, num_classes, hw, label, label_dtype, stats, n_slots)) return rc;
    if (num_classes > AWSEG_CALIB_MAX_CLASSES || hw > INT32_MAX || batch > 65535) return AWSEG_ERANGE;
    if (batch == 0) return 0;
    const fail_launch g = { logits, nullptr, nullptr, batch, num_classes, hw, nullptr, nullptr, label, cond, stats, n_slots, awseg_s(stream) };
    const bool vec = num_classes == 19 && !(hw & 3) && awseg_aligned(logits, 16);
    return awseg_by_label(label_dtype, [&](auto L) {
        constexpr int l = decltype(L)::value;
        if (vec) return launch<3, l, 512, 4, 19, 19>(g);
        if (num_classes <= 32) return launch<3, l, 512, 1, 0, 32>(g);
        return launch<3, l, 512, 1, 0, 64>(g);
    });
}
