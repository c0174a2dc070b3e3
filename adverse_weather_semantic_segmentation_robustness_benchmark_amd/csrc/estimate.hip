// estimate.hip — which restoration a frame needs, from its pixels alone: the mean dark channel (a veil: fog), the
// red-to-blue ratio of the channel means with the mean luma (a dark blue cast: night) and the share of top-hat seeds (bright
// occluders: rain, snow), and the first rule of include/awseg_restore.h that matches.  Every float step is the one the header
// states; everything summed is an integer, so every output bit is what numpy gives, whatever the grid.
//
// awseg_weather_estimate: a clear of the frames' records and two kernels on the caller's stream, no host synchronisation.
//   estimate_kernel   512 threads on the dehazer's 32 x 64 tiles: the detection kernel of deocclude.hip at d = 0 (deocclude_tiles.h:
//                     one staged plane with a halo of 2 r, one scratch plane, separable minima and maxima, the channels one after
//                     another) without the dilation and the mask.  A thread keeps, for its 4 pixels, the running minimum of the
//                     top-hats, of v_c and of e_c (the dark channel: minima commute, so the minimum over the channels of the window
//                     minima is the window minimum of the minimum over the channels) and the growing luma; it sums its pixels'
//                     fixed-point terms in 32 bits (4 * 2^16), a wave's and a block's sums (2048 * 2^16 = 2^27) fit as well.  One
//                     block-level reduction, then one 64-bit atomic per quantity into the frame's record.
//   route_kernel      one thread per frame: the descriptors in double from the record, the route, and the frame's row into slot 0
//                     and its own slot.
// LDS: [TH + 4 r][TW + 2 pad] + [TH + 4 r][TW + 2 r] floats (pad = 2 r rounded up to whole float4s): 41.8 KB at r = 7 (three
// resident blocks per CU, 24 waves), 81.7 KB at r = 15 (one, 8 waves).  Every pass reads 32-bit words that are consecutive across a wave's
// lanes (the column passes index the planes linearly in the thread's index), so a 32-lane half hits 32 distinct banks; only a half
// that straddles a row wrap of a row pass can take a second cycle.  There is no scratch.
#include "deocclude_tiles.h"

namespace {

constexpr int kERow = AWSEG_ESTIMATE_ROW;
constexpr int kPerThread = kTH * kTW / kDetectThreads;                     // pixels of the tile per thread
constexpr int kSums = 7;                                                   // Q_dark, Q_l, Q_0, Q_1, Q_2, N_seed, non-finite values
static_assert(kTH * kTW % kDetectThreads == 0, "every thread owns the same number of pixels");
static_assert((int64_t)kTH * kTW * 65536 < (int64_t)1 << 31, "a block's fixed-point sums fit 32 bits");

struct es_record { long long sum[kSums], pad; };                           // per frame, the workspace
static_assert(sizeof(es_record) == AWSEG_ESTIMATE_FRAME_RECORD, "the size the workspace query states");

struct es_rule { float cast_max, luma_max, dark_min, seed_min; };

// grid = (tiles_x * tiles_y, B).
template <bool VEC>
__global__ __launch_bounds__(kDetectThreads)
void estimate_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dc_args g, es_record* __restrict__ records)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* b0 = reinterpret_cast<float*>(lds_raw);                         // [rows][sw]
    float* b1 = b0 + g.rows * g.sw;                                        // [rows][c1]
    __shared__ uint32_t red[kDetectWaves][kSums];
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const float* frame = image + img * 3 * hw;
    float h[kPerThread], m[kPerThread], dark[kPerThread], l[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) { h[k] = m[k] = dark[k] = INFINITY; l[k] = 0.0f; }
    uint32_t sum[kSums] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    uint32_t bad = 0;
    for (int c = 0; c < 3; ++c) {
        stage_channel<VEC>(frame + c * hw, H, W, y0, x0, g, pick(g.std, c), pick(g.mean, c), b0, bad);
        __syncthreads();
        const float weight = c == 0 ? 0.299f : c == 1 ? 0.587f : 0.114f;
        float v[kPerThread];                                               // v_c at this thread's pixels, before b0 is reused
        uint32_t q = 0;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int idx = tid + k * kDetectThreads;
            const int i = idx / kTW, j = idx - i * kTW;
            v[k] = b0[(g.halo + i) * g.sw + g.pad + j];                     // +inf outside the frame
            if (y0 + i < H && x0 + j < W) {
                q += (uint32_t)(int32_t)rintf(v[k] * 65536.0f);
                l[k] = c == 0 ? weight * v[k] : l[k] + weight * v[k];       // (0.299 v_0 + 0.587 v_1) + 0.114 v_2, one operation a step
                m[k] = fminf(m[k], v[k]);
            }
        }
        if (c == 0) sum[2] += q; else if (c == 1) sum[3] += q; else sum[4] += q;
        window_minimum<kDetectThreads, true, true>(H, W, y0, x0, g, b0, b1);       // e_c on the tile plus r, -inf outside the frame
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int idx = tid + k * kDetectThreads;
            const int i = idx / kTW, j = idx - i * kTW;
            if (y0 + i < H && x0 + j < W) dark[k] = fminf(dark[k], b0[(g.q + i) * g.c1 + g.q + j]);
        }
        maximum_row_pass(g, b0, b1);                                       // its barrier also stands behind the reads of e_c above
        // maximum down the column at this thread's pixels: o_c.  The next channel's staging writes b0 only, and its row pass
        // writes b1 after a barrier.
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int idx = tid + k * kDetectThreads;
            const int i = idx / kTW, j = idx - i * kTW;
            if (y0 + i < H && x0 + j < W) h[k] = fminf(h[k], v[k] - maximum_down(b1, idx, g));
        }
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int idx = tid + k * kDetectThreads;
        const int i = idx / kTW, j = idx - i * kTW;
        if (y0 + i < H && x0 + j < W) {
            sum[0] += (uint32_t)(int32_t)rintf(dark[k] * 65536.0f);
            sum[1] += (uint32_t)(int32_t)rintf(l[k] * 65536.0f);
            sum[5] += h[k] > g.threshold && m[k] >= g.bright_min ? 1u : 0u;
        }
    }
    sum[6] = bad;
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
#pragma unroll
    for (int s = 0; s < kSums; ++s) {
        const uint32_t t = awseg_wave_sum_u32(sum[s]);
        if (lane == 0) red[wave][s] = t;
    }
    __syncthreads();
    if (tid < kSums) {
        uint32_t t = 0;
        for (int w = 0; w < kDetectWaves; ++w) t += red[w][tid];
        if (t) atomicAdd((unsigned long long*)&records[img].sum[tid], (unsigned long long)t);
    }
}

// One thread per frame.
__global__ __launch_bounds__(AWSEG_WAVE)
void route_kernel(const es_record* __restrict__ records, int batch, int64_t hw, const es_rule rule, const int32_t* __restrict__ cond,
                  int32_t* __restrict__ route, float* __restrict__ descriptors, int64_t* __restrict__ stats, int n_slots)
{
    const int b = blockIdx.x * AWSEG_WAVE + threadIdx.x;
    if (b >= batch) return;
    const es_record rec = records[b];
    const double P = (double)hw * 65536.0;
    const float D = (float)((double)rec.sum[0] / P), L = (float)((double)rec.sum[1] / P);
    const float M0 = (float)((double)rec.sum[2] / P), M1 = (float)((double)rec.sum[3] / P), M2 = (float)((double)rec.sum[4] / P);
    const float O = (float)((double)rec.sum[5] / (double)hw);
    int to = 0;
    if (M0 < rule.cast_max * M2 && L < rule.luma_max) to = 2;
    else if (D > rule.dark_min) to = 1;
    else if (O > rule.seed_min) to = 3;
    route[b] = to;
    float* d = descriptors + (int64_t)b * AWSEG_ESTIMATE_DESCRIPTORS;
    d[0] = D; d[1] = L; d[2] = M0; d[3] = M1; d[4] = M2; d[5] = O;
    long long row[kERow] = { 1, (long long)hw, rec.sum[0], rec.sum[1], rec.sum[2], rec.sum[3], rec.sum[4], rec.sum[5], rec.sum[6],
                             to == 0, to == 1, to == 2, to == 3 };
    add_row(stats, n_slots, cond, b, row);
}

inline bool below_one(float v) { return v >= 0.0f && v < 1.0f; }

}  // namespace

AWSEG_API int64_t awseg_weather_estimate_workspace(int64_t batch)
{
    return (batch > 0 ? batch : 0) * (int64_t)sizeof(es_record);
}

AWSEG_API int awseg_weather_estimate(const float* image, int64_t batch, int channels, int64_t height, int64_t width, const float* mean,
                                     const float* std, int radius, float threshold, float bright_min, float cast_max, float luma_max,
                                     float dark_min, float seed_min, const int32_t* cond, int32_t* route, float* descriptors,
                                     int64_t* stats, int n_slots, void* workspace, awseg_stream_t stream)
{
    dc_args g = {};
    AWSEG_RESTORE_CHECKS(g, route && descriptors && workspace,
                         radius >= 1 && radius <= AWSEG_DEHAZE_MAX_RADIUS && in_unit(threshold) && in_closed_unit(bright_min)
                             && cast_max > 0.0f && cast_max <= 4.0f && in_unit(luma_max) && below_one(dark_min) && below_one(seed_min));
    g.threshold = threshold;
    g.bright_min = bright_min;
    hipStream_t s = awseg_s(stream);
    const int H = (int)height, W = (int)width;
    const int tiles_x = (W + kTW - 1) / kTW, tiles = tiles_x * ((H + kTH - 1) / kTH);
    const bool vec = (W % 4 == 0) && awseg_aligned(image, 16);
    es_record* records = static_cast<es_record*>(workspace);
    geometry(radius, 0, g);
    auto kern = vec ? estimate_kernel<true> : estimate_kernel<false>;
    const size_t lds = detect_lds(g);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return AWSEG_EINVAL;                                               // the last refusal: nothing has touched the workspace yet
    hipError_t e = hipMemsetAsync(records, 0, (size_t)batch * sizeof(es_record), s);      // the blocks add to them
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)batch), dim3(kDetectThreads), lds, s, image, H, W, tiles_x, g, records);
    AWSEG_LAUNCH_CHECK();
    const es_rule rule = { cast_max, luma_max, dark_min, seed_min };
    hipLaunchKernelGGL(route_kernel, dim3((unsigned)((batch + AWSEG_WAVE - 1) / AWSEG_WAVE)), dim3(AWSEG_WAVE), 0, s,
                       (const es_record*)records, (int)batch, (int64_t)H * W, rule, cond, route, descriptors, stats, n_slots);
    AWSEG_LAUNCH_CHECK();
    return 0;
}
