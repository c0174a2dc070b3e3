// deptheval.hip — depth error sums of the evaluated depth maps against the loader's depth target, per condition slot and per
// prediction series, in one pass.  The ensemble's depth tail (depth_up_combine_kernel, backbone.hip) writes the
// upsampled DeepLab map and the combined map at full resolution only for them to be read back; here both values are formed in
// registers with that kernel's own expressions and roundings (built with -ffp-contract=off like it) and neither map is written.
//
// Series: one (d1) when d2_low is NULL, else three: 0 ensemble, 1 d1 (SegFormer), 2 upsampled d2 (DeepLab).
// Per pixel, t = target:  non-finite (t or any series value) -> counted, nothing else;  t < min_depth -> masked, nothing else;
// else per series p:  q = max(p, min_depth), g = float32(log(q) - log(t)) (float64 logarithms), r = max(q / t, t / q),
//     sums of |p-t|, (p-t)^2, |p-t|/t, (p-t)^2/t, g (signed), g^2 and the counts r < 1.25, r < 1.25^2, r < 1.25^3.
// Every real term is rounded to nearest in units of 2^-20 and clamped at 2^11 in magnitude (a clamped term counted as saturated):
// integer sums only, so the counters do not depend on launch geometry, batch split or rank count.
//
// 8 B/px of HBM (d1, target; the stride-16 map is 1/256 of that and lives in L2) against four float64 logarithms and twelve
// IEEE float32 divisions per pixel.  grid.y = frame, so a block serves one slot.  Each lane walks its pixels (four per step
// from 16-byte loads when W % 4 == 0: the four share their source rows) and keeps every accumulator in registers: 6 int64 sums
// + 4 uint32 counts per series, 3 uint32 pixel counts.  Nothing is reduced per pixel: one shuffle-tree sum per accumulator at the end of the block's
// strip, LDS across the four waves, one 64-bit global atomicAdd per non-zero counter per block and slot.
#include "awseg_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / AWSEG_WAVE;
constexpr int kRow = AWSEG_DEPTH_ROW;
constexpr int kSums = 6;                                    // |e|, e^2, |e|/t, e^2/t, g, g^2
constexpr float kScale = (float)(1 << AWSEG_DEPTH_FRAC_BITS);
constexpr float kCap = (float)AWSEG_DEPTH_CAP;

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// a non-negative term -> units of 2^-20, round to nearest (x * 2^20 is exact in float32 below the cap); +inf clamps like any term.
// The result is at most 2^31: one 32-bit conversion (a float -> int64 conversion is a dozen instructions), widened for the sum.
__device__ __forceinline__ long long quant(float x, uint32_t& sat)
{
    if (x > kCap) { x = kCap; ++sat; }
    return (long long)(uint32_t)rintf(x * kScale);
}

__device__ __forceinline__ long long quant_signed(float x, uint32_t& sat)
{
    float m = fabsf(x);
    if (m > kCap) { m = kCap; ++sat; }
    const long long q = (long long)(uint32_t)rintf(m * kScale);
    return x < 0.f ? -q : q;
}

struct series_acc {
    long long s[kSums];
    uint32_t c[4];                                          // delta1, delta2, delta3, saturated terms
};

// g = log(q) - log(t) rounded ONCE to float32: the two logarithms are taken in float64.  Float32 logarithms are within an ulp
// but not unbiased (measured: mean error -0.24e-6 at log(1e-3), the value every prediction under the floor shares), and the
// mean of g^2 = (log q - log t)^2 multiplies that bias by 2|g|; every other operation is float32.
__device__ __forceinline__ void series_terms(float p, float t, double log_t, float min_depth, series_acc& a)
{
    const float e = p - t;
    const float ae = fabsf(e), se = e * e;
    const float q = fmaxf(p, min_depth);
    const float g = (float)(log((double)q) - log_t);
    const float r = fmaxf(q / t, t / q);
    a.s[0] += quant(ae, a.c[3]);
    a.s[1] += quant(se, a.c[3]);
    a.s[2] += quant(ae / t, a.c[3]);
    a.s[3] += quant(se / t, a.c[3]);
    a.s[4] += quant_signed(g, a.c[3]);
    a.s[5] += quant(g * g, a.c[3]);
    a.c[0] += r < 1.25f;
    a.c[1] += r < 1.5625f;
    a.c[2] += r < 1.953125f;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// NS series (1 or 3), PX pixels per lane per step (4: W % 4 == 0, d1 and target 16-byte aligned; 1: anything).
template <int NS, int PX>
__global__ __launch_bounds__(kThreads)
void depth_eval_kernel(const float* __restrict__ d1, const float* __restrict__ d2_low, int h, int w, int H, int W, float sy, float sx,
                       const float* __restrict__ weights, const float* __restrict__ target, float min_depth,
                       const int32_t* __restrict__ cond, int n_slots, long long* __restrict__ stats)
{
    __shared__ unsigned long long s_red[kWaves][NS * kRow];
    const int64_t hw = (int64_t)H * W;
    const int64_t frame = (int64_t)blockIdx.y * hw;
    const float* lo = NS == 3 ? d2_low + (int64_t)blockIdx.y * h * w : nullptr;
    const float w0 = (NS == 3 && weights) ? weights[0] : 0.f, w1 = (NS == 3 && weights) ? weights[1] : 0.f;

    series_acc acc[NS];
    uint32_t n_valid = 0, n_masked = 0, n_bad = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[s].s[k] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[s].c[k] = 0u;
    }

    const int64_t n_items = hw / PX;
    for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < n_items; it += (int64_t)gridDim.x * kThreads) {
        const int p = (int)(it * PX);                       // hw < 2^31 (launcher)
        float a[PX], t[PX];
        if constexpr (PX == 4) {
            const float4 av = *reinterpret_cast<const float4*>(d1 + frame + p);
            const float4 tv = *reinterpret_cast<const float4*>(target + frame + p);
            a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
            t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
        } else {
            a[0] = d1[frame + p];
            t[0] = target[frame + p];
        }
        float v[PX], m[PX];
        if constexpr (NS == 3) {
            // depth_up_combine_kernel's expressions, operation for operation (torch area_pixel_compute_source_index,
            // align_corners=false); the PX pixels of a step lie in one row, so the row terms are formed once
            const int y = p / W, x = p - y * W;
            float fy = sy * ((float)y + 0.5f) - 0.5f; fy = fy < 0.f ? 0.f : fy;
            int y0 = (int)fy; y0 = y0 < h - 1 ? y0 : h - 1;
            const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
            const float ly1 = fy - (float)y0, ly0 = 1.0f - ly1;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                float fx = sx * ((float)(x + j) + 0.5f) - 0.5f; fx = fx < 0.f ? 0.f : fx;
                int x0 = (int)fx; x0 = x0 < w - 1 ? x0 : w - 1;
                const int x1 = x0 + (x0 < w - 1 ? 1 : 0);
                const float lx1 = fx - (float)x0, lx0 = 1.0f - lx1;
                v[j] = ly0 * (lx0 * lo[y0 * w + x0] + lx1 * lo[y0 * w + x1]) + ly1 * (lx0 * lo[y1 * w + x0] + lx1 * lo[y1 * w + x1]);
                m[j] = weights ? (w0 * a[j] + w1 * v[j]) : ((a[j] + v[j]) / 2.0f);
            }
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            bool fin = finite_f32(t[j]) && finite_f32(a[j]);
            if constexpr (NS == 3) fin = fin && finite_f32(v[j]) && finite_f32(m[j]);
            if (!fin) { ++n_bad; continue; }
            if (t[j] < min_depth) { ++n_masked; continue; }
            ++n_valid;
            const double log_t = log((double)t[j]);
            if constexpr (NS == 3) {
                series_terms(m[j], t[j], log_t, min_depth, acc[0]);
                series_terms(a[j], t[j], log_t, min_depth, acc[1]);
                series_terms(v[j], t[j], log_t, min_depth, acc[2]);
            } else {
                series_terms(a[j], t[j], log_t, min_depth, acc[0]);
            }
        }
    }

    // block sum: shuffle tree per accumulator, one LDS row per wave
    const int lane = threadIdx.x & (AWSEG_WAVE - 1), wave = threadIdx.x / AWSEG_WAVE;
    const unsigned long long px[3] = { wave_sum_u64(n_valid), wave_sum_u64(n_masked), wave_sum_u64(n_bad) };
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        unsigned long long row[kRow];
        row[AWSEG_DEPTH_VALID] = px[0]; row[AWSEG_DEPTH_MASKED] = px[1]; row[AWSEG_DEPTH_NONFINITE] = px[2];
#pragma unroll
        for (int k = 0; k < kSums; ++k) row[AWSEG_DEPTH_SUM_ABS + k] = wave_sum_u64((unsigned long long)acc[s].s[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) row[AWSEG_DEPTH_DELTA1 + k] = wave_sum_u64(acc[s].c[k]);
        row[AWSEG_DEPTH_SATURATED] = wave_sum_u64(acc[s].c[3]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kRow; ++k) s_red[wave][s * kRow + k] = row[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < NS * kRow) {
        unsigned long long sum = 0;                         // two's complement: the signed log sum adds like the others
#pragma unroll
        for (int k = 0; k < kWaves; ++k) sum += s_red[k][threadIdx.x];
        if (sum) {
            int slot = -1;
            if (cond) { const int c = cond[blockIdx.y]; if (c >= 0 && c + 1 < n_slots) slot = c + 1; }
            const int s = threadIdx.x / kRow, f = threadIdx.x - s * kRow;
            const int64_t o = (int64_t)s * kRow + f;
            atomicAdd((unsigned long long*)&stats[o], sum);
            if (slot > 0) atomicAdd((unsigned long long*)&stats[(int64_t)slot * AWSEG_DEPTH_SERIES * kRow + o], sum);
        }
    }
}

}  // namespace

AWSEG_API int awseg_depth_eval_stats(const float* d1, const float* d2_low, int batch, int low_height, int low_width, int height,
                                     int width, const float* weights, const float* target, float min_depth, const int32_t* cond,
                                     int64_t* stats, int n_slots, awseg_stream_t stream)
{
    if (!d1 || !target || !stats) return AWSEG_EINVAL;
    if (batch < 0 || height < 1 || width < 1 || n_slots < 1) return AWSEG_EINVAL;
    if (d2_low && (low_height < 1 || low_width < 1)) return AWSEG_EINVAL;
    if (!(min_depth > 0.f) || !(min_depth <= 3.4028234663852886e38f)) return AWSEG_EINVAL;      // NaN, <= 0, inf
    if (batch == 0) return 0;
    const int64_t hw = (int64_t)height * width;
    if (batch > 65535 || hw > INT32_MAX || (d2_low && (int64_t)low_height * low_width > INT32_MAX)) return AWSEG_ERANGE;
    const bool vec = !(width & 3) && awseg_aligned(d1, 16) && awseg_aligned(target, 16);
    // 256 CUs x 8 resident blocks over the whole batch, grid-stride beyond (a lane then walks 8 steps at 8 x 1024 x 2048)
    dim3 grid((unsigned)awseg_blocks_per_image(vec ? hw / 4 : hw, kThreads, batch, 8), (unsigned)batch), block(kThreads);
    // torch area_pixel_compute_scale(in, out, align_corners=false, scale=None) = (float)in / out, as awseg_depth_upsample_combine
    const float sy = d2_low ? (float)low_height / (float)height : 1.f, sx = d2_low ? (float)low_width / (float)width : 1.f;
    hipStream_t s = awseg_s(stream);
    awseg_by_flag(d2_low != nullptr, [&](auto THREE) { awseg_by_flag(vec, [&](auto VEC) {
        hipLaunchKernelGGL((depth_eval_kernel<decltype(THREE)::value ? 3 : 1, decltype(VEC)::value ? 4 : 1>), grid, block, 0, s, d1, d2_low,
                           low_height, low_width, height, width, sy, sx, weights, target, min_depth, cond, n_slots, (long long*)stats);
    }); });
    AWSEG_LAUNCH_CHECK();
    return 0;
}
