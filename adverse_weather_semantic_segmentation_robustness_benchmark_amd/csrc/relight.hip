// relight.hip — night relighting of the frames the model sees: contrast-limited adaptive histogram equalisation of the luma
// (CLAHE; Zuiderveld 1994, the algorithm of OpenCV's createCLAHE) with a grey-world white balance, the arithmetic
// include/awseg_restore.h states step by step: every output bit is what numpy float32 gives.
//
// awseg_relight: one clear and three kernels on the caller's stream, no host synchronisation, no block waits for another.
//   A  histogram_kernel   streaming.  grid = (strips, tiles_y, B): a block walks rows y0_i + blockIdx.x, + gridDim.x, ... of tile row i
//                         over the whole width, counts the bins in one LDS histogram per tile column with plain LDS atomics (merging
//                         the runs of equal bins among a thread's four pixels first was measured and made no difference, on
//                         night-like frames that crowd a few bins as on random ones: README) and adds the non-zero words to the
//                         tiles' histograms with integer atomics; the frame's channel sums and non-finite count likewise.
//   B  tables_kernel      grid = (tiles + 1, B), one thread per bin: clip, sum the excess, redistribute once, prefix-scan, table.
//                         The last block of a frame computes the gains and adds the frame's own counters.
//   C  apply_kernel       streaming.  grid = (strips, tiles_y + 1, B): band k of rows lies between the centres of tile rows k - 1 and
//                         k, so a block needs the tables of two tile rows only; it stages them in LDS as one 32-bit word per (tile
//                         column, bin) (upper row in the low half, lower row in the high half: 1 KB per tile column, 16 KB at most),
//                         interpolates, applies the gain and the white balance and adds its sums to the slots' rows.
// The tile and band bounds travel in the kernel arguments (host integers: no division per pixel); a pixel finds its tile column
// from a multiplied guess corrected against the bounds in LDS.
#include "restore_common.h"                                               // v_c, the reductions, the counter epilogue, the refusals

namespace {

constexpr int kBins = 256;
constexpr int kRow = AWSEG_RELIGHT_ROW;
constexpr int kMaxT = AWSEG_RELIGHT_MAX_TILES;
static_assert(kThreads == kBins, "one thread per bin in tables_kernel");
static_assert(AWSEG_RELIGHT_TILE_BYTES == kBins * (sizeof(uint32_t) + sizeof(uint16_t)), "a histogram and a table per tile");

struct rl_record {                                                         // per frame, at the head of the workspace
    long long sum[3], nonfinite;
    float gain[3], pad;
};
static_assert(sizeof(rl_record) == AWSEG_RELIGHT_FRAME_RECORD, "the size the workspace query states");

struct rl_args {
    float mean[3], std[3];
    float clip, max_gain;
    int wb, ty, tx;
    int yb[kMaxT + 1], xb[kMaxT + 1];                                      // tile i = rows [yb[i], yb[i + 1]), tile j = columns [xb[j], xb[j + 1])
    int ry[kMaxT + 2], rx[kMaxT + 2];                                      // band k = [ry[k], ry[k + 1]): the positions with exactly k centres at or before them
    float cy[kMaxT], cx[kMaxT];                                            // the tiles' centres
};

__device__ __forceinline__ float luma(float v0, float v1, float v2) { return (0.299f * v0 + 0.587f * v1) + 0.114f * v2; }
__device__ __forceinline__ int bin_of(float l) { return min((int)(l * 255.0f), 255); }

// k with b[k] <= p < b[k + 1] among the n intervals of b (n + 1 non-decreasing bounds, b[0] <= p < b[n]; empty ones are stepped over).
__device__ __forceinline__ int interval_of(const int* b, int n, int p, int guess)
{
    int k = min(max(guess, 0), n - 1);
    while (p < b[k]) --k;
    while (p >= b[k + 1]) ++k;
    return k;
}

__device__ __forceinline__ unsigned char* histograms(unsigned char* ws, int64_t batch) { return ws + batch * (int64_t)sizeof(rl_record); }
__device__ __forceinline__ unsigned char* tables(unsigned char* ws, int64_t batch, int tiles)
{
    return histograms(ws, batch) + batch * tiles * (int64_t)(kBins * sizeof(uint32_t));
}

// A.  grid = (strips, tiles_y, B).
template <bool VEC>
__global__ __launch_bounds__(kThreads)
void histogram_kernel(const float* __restrict__ image, int H, int W, const rl_args g, unsigned char* __restrict__ ws)
{
    __shared__ uint32_t hist[kMaxT * kBins];
    __shared__ int xb[kMaxT + 1];
    __shared__ long long red[kWaves][4];
    const int tid = threadIdx.x, ti = blockIdx.y;
    const int64_t img = blockIdx.z, hw = (int64_t)H * W;
    for (int i = tid; i < g.tx * kBins; i += kThreads) hist[i] = 0;
    if (tid <= g.tx) xb[tid] = g.xb[tid];
    __syncthreads();
    const float* frame = image + img * 3 * hw;
    const float scale = (float)g.tx / (float)W;
    const int y1 = g.yb[ti + 1];
    long long s0 = 0, s1 = 0, s2 = 0;
    uint32_t bad = 0;
    auto take = [&](float x0, float x1, float x2) {
        bad += not_finite(x0) + not_finite(x1) + not_finite(x2);
        const float v0 = unit(x0, g.std[0], g.mean[0]), v1 = unit(x1, g.std[1], g.mean[1]), v2 = unit(x2, g.std[2], g.mean[2]);
        s0 += (long long)rintf(v0 * 65536.0f);
        s1 += (long long)rintf(v1 * 65536.0f);
        s2 += (long long)rintf(v2 * 65536.0f);
        return bin_of(luma(v0, v1, v2));
    };
    for (int y = g.yb[ti] + (int)blockIdx.x; y < y1; y += (int)gridDim.x) {
        const float* row = frame + (int64_t)y * W;
        if constexpr (VEC) {
            for (int q = tid; q < W / 4; q += kThreads) {
                const int x = 4 * q;
                const float4 a = *reinterpret_cast<const float4*>(row + x);
                const float4 b = *reinterpret_cast<const float4*>(row + hw + x);
                const float4 c = *reinterpret_cast<const float4*>(row + 2 * hw + x);
                const int bins[4] = { take(a.x, b.x, c.x), take(a.y, b.y, c.y), take(a.z, b.z, c.z), take(a.w, b.w, c.w) };
                int j = interval_of(xb, g.tx, x, (int)((float)x * scale));
                atomicAdd(&hist[j * kBins + bins[0]], 1u);
#pragma unroll
                for (int k = 1; k < 4; ++k) {                              // tiles are never empty: one pixel on is at most one tile on
                    if (x + k >= xb[j + 1]) ++j;
                    atomicAdd(&hist[j * kBins + bins[k]], 1u);
                }
            }
        } else {
            for (int x = tid; x < W; x += kThreads) {
                const int bin = take(row[x], row[hw + x], row[2 * hw + x]);
                atomicAdd(&hist[interval_of(xb, g.tx, x, (int)((float)x * scale)) * kBins + bin], 1u);
            }
        }
    }
    __syncthreads();
    const int tiles = g.ty * g.tx;
    uint32_t* out = reinterpret_cast<uint32_t*>(histograms(ws, gridDim.z)) + (img * tiles + (int64_t)ti * g.tx) * kBins;
    for (int i = tid; i < g.tx * kBins; i += kThreads)
        if (hist[i]) atomicAdd(&out[i], hist[i]);
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
    s0 = wave_sum_i64(s0); s1 = wave_sum_i64(s1); s2 = wave_sum_i64(s2);
    const long long nf = wave_sum_i64((long long)bad);
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = nf; }
    __syncthreads();
    if (tid < 4) {
        rl_record* rec = reinterpret_cast<rl_record*>(ws) + img;
        long long t = 0;
        for (int w = 0; w < kWaves; ++w) t += red[w][tid];
        long long* dst = tid < 3 ? &rec->sum[tid] : &rec->nonfinite;
        if (t) atomicAdd((unsigned long long*)dst, (unsigned long long)t);
    }
}

// B.  grid = (tiles + 1, B): block t < tiles makes tile t's table, block `tiles` the frame's gains and its own counters.
__global__ __launch_bounds__(kThreads)
void tables_kernel(int H, int W, const rl_args g, unsigned char* __restrict__ ws, const int32_t* __restrict__ cond,
                   float* __restrict__ gains, int64_t* __restrict__ stats, int n_slots)
{
    __shared__ uint32_t scan[2][kBins];
    __shared__ uint32_t part[kWaves];
    const int tid = threadIdx.x, tiles = g.ty * g.tx, t = blockIdx.x;
    const int64_t img = blockIdx.y, batch = gridDim.y;
    rl_record* rec = reinterpret_cast<rl_record*>(ws) + img;
    if (t == tiles) {
        if (tid != 0) return;
        const double px = (double)((int64_t)H * W) * 65536.0;
        const float m0 = (float)((double)rec->sum[0] / px), m1 = (float)((double)rec->sum[1] / px), m2 = (float)((double)rec->sum[2] / px);
        const float grey = ((m0 + m1) + m2) / 3.0f;
        float k[3] = { 1.0f, 1.0f, 1.0f };
        if (g.wb) {
            k[0] = fminf(fmaxf(grey / fmaxf(m0, 1.0f / 256.0f), 0.25f), 4.0f);
            k[1] = fminf(fmaxf(grey / fmaxf(m1, 1.0f / 256.0f), 0.25f), 4.0f);
            k[2] = fminf(fmaxf(grey / fmaxf(m2, 1.0f / 256.0f), 0.25f), 4.0f);
        }
        long long row[kRow] = { 1, 0, 0, 0, 0, 0, 0, rec->nonfinite, 0, 0 };
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rec->gain[c] = k[c];
            gains[img * 3 + c] = k[c];
            row[1 + c] = (long long)rintf(k[c] * 65536.0f);
        }
        add_row(stats, n_slots, cond, img, row);
        return;
    }
    const uint32_t* hist = reinterpret_cast<const uint32_t*>(histograms(ws, batch)) + (img * tiles + t) * kBins;
    uint16_t* lut = reinterpret_cast<uint16_t*>(tables(ws, batch, tiles)) + (img * tiles + t) * kBins;
    const int i = t / g.tx, j = t - i * g.tx;
    const uint32_t n = (uint32_t)(g.yb[i + 1] - g.yb[i]) * (uint32_t)(g.xb[j + 1] - g.xb[j]);
    const uint32_t limit = (uint32_t)max(1, (int)((g.clip * (float)n) / 256.0f));
    const uint32_t count = hist[tid];
    uint32_t over = awseg_wave_sum_u32(count > limit ? count - limit : 0u);
    if ((tid & (AWSEG_WAVE - 1)) == 0) part[tid / AWSEG_WAVE] = over;
    __syncthreads();
    uint32_t excess = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) excess += part[w];
    uint32_t h = min(count, limit) + excess / kBins;
    const uint32_t rest = excess % kBins;
    if (rest) {
        const uint32_t step = kBins / rest;                                  // >= 1: rest < 256
        if ((uint32_t)tid % step == 0 && (uint32_t)tid / step < rest) h += 1;
    }
    int src = 0;
    scan[0][tid] = h;
    __syncthreads();
    for (int off = 1; off < kBins; off <<= 1) {                            // inclusive scan
        const uint32_t v = scan[src][tid] + (tid >= off ? scan[src][tid - off] : 0u);
        scan[src ^ 1][tid] = v;
        src ^= 1;
        __syncthreads();
    }
    const uint64_t cdf = scan[src][tid];
    lut[tid] = (uint16_t)((cdf * 65535ull + n / 2) / n);
}

struct rl_out { float r0, r1, r2; };

// C.  grid = (strips, tiles_y + 1, B).
template <bool VEC>
__global__ __launch_bounds__(kThreads)
void apply_kernel(const float* __restrict__ image, int H, int W, const rl_args g, const unsigned char* __restrict__ ws,
                  const int32_t* __restrict__ cond, float* __restrict__ restored, int64_t* __restrict__ stats, int n_slots)
{
    __shared__ uint32_t lut[kMaxT * kBins];
    __shared__ int rx[kMaxT + 2];
    __shared__ float cx[kMaxT];
    __shared__ long long red[kWaves][5];
    const int tid = threadIdx.x, band = blockIdx.y, tiles = g.ty * g.tx;
    const int64_t img = blockIdx.z, batch = gridDim.z, hw = (int64_t)H * W;
    const int y_end = g.ry[band + 1];
    if (g.ry[band] + (int)blockIdx.x >= y_end) return;                     // the whole block: no barrier has been met
    const int i0 = max(band - 1, 0), i1 = min(band, g.ty - 1);
    {
        const unsigned char* region = tables(const_cast<unsigned char*>(ws), batch, tiles);
        const uint16_t* all = reinterpret_cast<const uint16_t*>(region) + img * tiles * kBins;
        const uint16_t* up = all + (int64_t)i0 * g.tx * kBins;
        const uint16_t* down = all + (int64_t)i1 * g.tx * kBins;
        for (int i = tid; i < g.tx * kBins; i += kThreads) lut[i] = (uint32_t)up[i] | ((uint32_t)down[i] << 16);
        if (tid <= g.tx + 1) rx[tid] = g.rx[tid];
        if (tid < g.tx) cx[tid] = g.cx[tid];
    }
    __syncthreads();
    const rl_record* rec = reinterpret_cast<const rl_record*>(ws) + img;
    const float k0 = rec->gain[0], k1 = rec->gain[1], k2 = rec->gain[2];
    const float cy0 = g.cy[i0], cy1 = g.cy[i1];
    const float scale = (float)g.tx / (float)W;
    const float* frame = image + img * 3 * hw;
    float* out = restored + img * 3 * hw;
    long long n_px = 0, l_in = 0, l_out = 0, capped = 0, saturated = 0;
    // one pixel at column x of band kx, row weight wy
    auto pixel = [&](float x0, float x1, float x2, int x, int kx, float wy) -> rl_out {
        const float v0 = unit(x0, g.std[0], g.mean[0]), v1 = unit(x1, g.std[1], g.mean[1]), v2 = unit(x2, g.std[2], g.mean[2]);
        const float l = luma(v0, v1, v2);
        const int bin = bin_of(l);
        const int j0 = max(kx - 1, 0), j1 = min(kx, g.tx - 1);
        const float wx = j0 != j1 ? ((float)x - cx[j0]) / (cx[j1] - cx[j0]) : 0.0f;
        const uint32_t left = lut[j0 * kBins + bin], right = lut[j1 * kBins + bin];
        const float a = (float)(left & 0xFFFFu), b = (float)(right & 0xFFFFu), c = (float)(left >> 16), d = (float)(right >> 16);
        const float top = a + wx * (b - a);
        const float bot = c + wx * (d - c);
        const float lp = (top + wy * (bot - top)) / 65535.0f;
        const float raw = lp / fmaxf(l, 1.0f / 256.0f);
        const float gain = fminf(raw, g.max_gain);
        const float u0 = (v0 * k0) * gain, u1 = (v1 * k1) * gain, u2 = (v2 * k2) * gain;
        const float j_0 = fminf(fmaxf(u0, 0.0f), 1.0f), j_1 = fminf(fmaxf(u1, 0.0f), 1.0f), j_2 = fminf(fmaxf(u2, 0.0f), 1.0f);
        n_px += 1;
        l_in += (long long)rintf(l * 65536.0f);
        l_out += (long long)rintf(fminf(luma(j_0, j_1, j_2), 1.0f) * 65536.0f);
        capped += raw > g.max_gain ? 1 : 0;
        saturated += (u0 > 1.0f ? 1 : 0) + (u1 > 1.0f ? 1 : 0) + (u2 > 1.0f ? 1 : 0);
        return { (j_0 - g.mean[0]) / g.std[0], (j_1 - g.mean[1]) / g.std[1], (j_2 - g.mean[2]) / g.std[2] };
    };
    for (int y = g.ry[band] + (int)blockIdx.x; y < y_end; y += (int)gridDim.x) {
        const float wy = i0 != i1 ? ((float)y - cy0) / (cy1 - cy0) : 0.0f;
        const int64_t p = (int64_t)y * W;
        if constexpr (VEC) {
            for (int q = tid; q < W / 4; q += kThreads) {
                const int x = 4 * q;
                const float4 a = *reinterpret_cast<const float4*>(frame + p + x);
                const float4 b = *reinterpret_cast<const float4*>(frame + hw + p + x);
                const float4 c = *reinterpret_cast<const float4*>(frame + 2 * hw + p + x);
                int kx = interval_of(rx, g.tx + 1, x, (int)((float)x * scale));
                const rl_out w0 = pixel(a.x, b.x, c.x, x, kx, wy);
                while (x + 1 >= rx[kx + 1]) ++kx;                          // bands may be empty; rx[tiles_x + 1] = W stops the walk
                const rl_out w1 = pixel(a.y, b.y, c.y, x + 1, kx, wy);
                while (x + 2 >= rx[kx + 1]) ++kx;
                const rl_out w2 = pixel(a.z, b.z, c.z, x + 2, kx, wy);
                while (x + 3 >= rx[kx + 1]) ++kx;
                const rl_out w3 = pixel(a.w, b.w, c.w, x + 3, kx, wy);
                *reinterpret_cast<float4*>(out + p + x) = { w0.r0, w1.r0, w2.r0, w3.r0 };
                *reinterpret_cast<float4*>(out + hw + p + x) = { w0.r1, w1.r1, w2.r1, w3.r1 };
                *reinterpret_cast<float4*>(out + 2 * hw + p + x) = { w0.r2, w1.r2, w2.r2, w3.r2 };
            }
        } else {
            for (int x = tid; x < W; x += kThreads) {
                const int kx = interval_of(rx, g.tx + 1, x, (int)((float)x * scale));
                const rl_out w = pixel(frame[p + x], frame[hw + p + x], frame[2 * hw + p + x], x, kx, wy);
                out[p + x] = w.r0;
                out[hw + p + x] = w.r1;
                out[2 * hw + p + x] = w.r2;
            }
        }
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
    n_px = wave_sum_i64(n_px); l_in = wave_sum_i64(l_in); l_out = wave_sum_i64(l_out);
    capped = wave_sum_i64(capped); saturated = wave_sum_i64(saturated);
    if (lane == 0) { red[wave][0] = n_px; red[wave][1] = l_in; red[wave][2] = l_out; red[wave][3] = capped; red[wave][4] = saturated; }
    __syncthreads();
    if (tid == 0) {
        long long row[kRow] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int w = 0; w < kWaves; ++w) {
            row[4] += red[w][0]; row[5] += red[w][1]; row[6] += red[w][2]; row[8] += red[w][3]; row[9] += red[w][4];
        }
        add_row(stats, n_slots, cond, img, row);
    }
}

inline bool in_range(float v, float lo, float hi) { return v >= lo && v <= hi; }       // NaN fails

// Strips per band: enough blocks to fill the chip `resident` times over the whole launch, at most one per row of the tallest band.
inline int strips(int64_t bands, int64_t batch, int tallest, int resident)
{
    int64_t s = ((int64_t)AWSEG_CUS * resident + bands * batch - 1) / (bands * batch);
    if (s > tallest) s = tallest;
    if (s < 1) s = 1;
    return (int)s;
}

}  // namespace

AWSEG_API int64_t awseg_relight_workspace(int64_t batch, int tiles_y, int tiles_x)
{
    if (batch < 1) batch = 1;
    if (tiles_y < 1) tiles_y = 1;
    if (tiles_x < 1) tiles_x = 1;
    return batch * ((int64_t)AWSEG_RELIGHT_FRAME_RECORD + (int64_t)tiles_y * tiles_x * AWSEG_RELIGHT_TILE_BYTES);
}

AWSEG_API int awseg_relight(const float* image, int64_t batch, int channels, int64_t height, int64_t width, const float* mean,
                            const float* std, int tiles_y, int tiles_x, float clip_limit, float max_gain, int white_balance,
                            const int32_t* cond, float* restored, float* gains, int64_t* stats, int n_slots, void* workspace,
                            awseg_stream_t stream)
{
    rl_args g = {};
    AWSEG_RESTORE_CHECKS(g, restored && gains && workspace,
                         tiles_y >= 1 && tiles_y <= kMaxT && tiles_x >= 1 && tiles_x <= kMaxT && tiles_y <= height && tiles_x <= width
                             && in_range(clip_limit, 1.0f, 64.0f) && in_range(max_gain, 1.0f, 64.0f)
                             && (white_balance == 0 || white_balance == 1));
    hipStream_t s = awseg_s(stream);
    const int H = (int)height, W = (int)width;
    g.clip = clip_limit;
    g.max_gain = max_gain;
    g.wb = white_balance;
    g.ty = tiles_y;
    g.tx = tiles_x;
    // bounds, centres and bands of one axis; band k begins at the first position at or after centre k - 1: 2 p >= lo + hi - 1
    auto axis = [](int size, int n, int* bound, int* band, float* centre) {
        for (int i = 0; i <= n; ++i) bound[i] = (int)(((int64_t)i * size) / n);
        band[0] = 0;
        for (int i = 0; i < n; ++i) {
            const int64_t twice = (int64_t)bound[i] + bound[i + 1] - 1;
            centre[i] = (float)twice * 0.5f;
            band[i + 1] = (int)((twice + 1) / 2);
        }
        band[n + 1] = size;
    };
    axis(H, tiles_y, g.yb, g.ry, g.cy);
    axis(W, tiles_x, g.xb, g.rx, g.cx);
    const int tiles = tiles_y * tiles_x;
    unsigned char* ws = (unsigned char*)workspace;
    // the records and the histograms: the kernels add to them.  The tables behind them are written whole.
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)batch * (sizeof(rl_record) + (size_t)tiles * kBins * sizeof(uint32_t)), s);
    if (e != hipSuccess) return (int)e;
    const bool vec = (W % 4 == 0) && awseg_aligned(image, 16) && awseg_aligned(restored, 16);
    const int tallest = (H + tiles_y - 1) / tiles_y;
    dim3 block(kThreads);
    {
        auto kern = vec ? histogram_kernel<true> : histogram_kernel<false>;
        dim3 grid((unsigned)strips(tiles_y, batch, tallest, 4), (unsigned)tiles_y, (unsigned)batch);
        hipLaunchKernelGGL(kern, grid, block, 0, s, image, H, W, g, ws);
        AWSEG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tables_kernel, dim3((unsigned)tiles + 1, (unsigned)batch), block, 0, s, H, W, g, ws, cond, gains, stats, n_slots);
    AWSEG_LAUNCH_CHECK();
    {
        auto kern = vec ? apply_kernel<true> : apply_kernel<false>;
        dim3 grid((unsigned)strips(tiles_y + 1, batch, tallest + 1, 8), (unsigned)tiles_y + 1, (unsigned)batch);
        hipLaunchKernelGGL(kern, grid, block, 0, s, image, H, W, g, (const unsigned char*)ws, cond, restored, stats, n_slots);
        AWSEG_LAUNCH_CHECK();
    }
    return 0;
}
