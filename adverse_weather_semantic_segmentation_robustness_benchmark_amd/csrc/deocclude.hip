// deocclude.hip — rain and snow removal in front of the model: bright occluders narrower than a window, found by the
// white top-hat of every channel and filled from their unmasked neighbours; the arithmetic include/awseg_restore.h states step by
// step: every output bit is what numpy gives.
//
// awseg_deocclude: two kernels on the caller's stream, no host synchronisation, no block waits for another.  Both run on the tiles
// of the dehazer (restore_common.h: the tile, v_c, the reductions and the window minimum) and walk the three channels one after another
// through one staged plane and one scratch plane, so that the LDS stays what one channel needs.  The detection kernel's geometry,
// staging and window passes live in deocclude_tiles.h, which estimate.hip (awseg_weather_estimate) shares.
//   detect_kernel   512 threads.  Per channel: stages v_c for the tile plus a halo of 2 r + d (+inf outside the frame), takes the (2r+1)^2 minimum
//                   separably on the tile plus r + d, then the (2r+1)^2 maximum of the minima (-inf outside the frame) on the tile
//                   plus d, and folds v_c - o_c and v_c into the running minima h and b, which a thread keeps in registers for its
//                   (at most 5) positions of the tile plus d.  Then the seeds go to LDS, are dilated separably by d and written as
//                   the mask.  Counts frames, pixels, seeds and the input values that are not finite.
//   fill_kernel     256 threads.  Per channel: stages one word per position of the tile plus r: q_c with bit 24 set where the position is inside
//                   the frame and unmasked, 0 elsewhere.  A row sum of at most 31 such words keeps the sum of q (< 2^21) and the
//                   count (< 2^5) apart; the column pass unpacks them before it adds.  Then J_c and the normalised output for the
//                   tile's pixels.  Counts the masked pixels, those left unfilled and the change.
// LDS: detect [TH + 2 halo][TW + 2 pad] + [TH + 2 halo][TW + 2 (r + d)] floats (pad = halo rounded up to whole float4s): 52.6 KB
// at r = 9, d = 1 (three resident blocks per CU, 24 waves), 86.8 KB at r = 15, d = 2 (one, 8 waves); fill [TH + 2 r][TW + 2 pad + TW] words: 30.4 KB at
// r = 9, 39.7 KB at r = 15.
#include "deocclude_tiles.h"                                              // the geometry, the staging and the window passes

namespace {

constexpr int kDRow = AWSEG_DEOCCLUDE_ROW;
constexpr int kMaxDilate = AWSEG_DEOCCLUDE_MAX_DILATE;
constexpr int kRing = ((kTH + 2 * kMaxDilate) * (kTW + 2 * kMaxDilate) + kDetectThreads - 1) / kDetectThreads;    // positions of the tile plus d per thread
constexpr uint32_t kOne = 1u << 24, kSumMask = kOne - 1;                   // the count above the sum of q in a staged word
static_assert((2 * AWSEG_DEHAZE_MAX_RADIUS + 1) * 65536 < (int)kOne, "a row sum of q stays below the count");
static_assert(kTH * kTW % kThreads == 0, "every thread owns the same number of pixels");

size_t fill_lds(const dc_args& g) { return (size_t)g.frows * (g.fsw + kTW) * sizeof(uint32_t); }

// Pass A.  grid = (tiles_x * tiles_y, B).
template <bool VEC>
__global__ __launch_bounds__(kDetectThreads)
void detect_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dc_args g, const int32_t* __restrict__ cond,
                   uint8_t* __restrict__ mask, int64_t* __restrict__ stats, int n_slots)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* b0 = reinterpret_cast<float*>(lds_raw);                         // [rows][sw]
    float* b1 = b0 + g.rows * g.sw;                                        // [rows][c1]
    __shared__ long long red[kDetectWaves][3];
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const float* frame = image + img * 3 * hw;
    const int eh = kTH + 2 * g.d, n_e = eh * g.c2;                          // the tile plus d: where the seeds are needed
    float h[kRing], b[kRing];
#pragma unroll
    for (int k = 0; k < kRing; ++k) h[k] = b[k] = INFINITY;
    uint32_t bad = 0;
    for (int c = 0; c < 3; ++c) {
        stage_channel<VEC>(frame + c * hw, H, W, y0, x0, g, pick(g.std, c), pick(g.mean, c), b0, bad);
        __syncthreads();
        float v[kRing];                                                    // v_c at this thread's positions, before b0 is reused
#pragma unroll
        for (int k = 0; k < kRing; ++k) {
            const int idx = tid + k * kDetectThreads;
            v[k] = INFINITY;
            if (idx < n_e) {
                const int i = idx / g.c2, j = idx - i * g.c2;
                v[k] = b0[(g.halo - g.d + i) * g.sw + (g.pad - g.d) + j];
            }
        }
        window_minimum<kDetectThreads, true, true>(H, W, y0, x0, g, b0, b1);       // e_c on the tile plus q, -inf outside the frame
        maximum_row_pass(g, b0, b1);
        // maximum down the column at this thread's positions: o_c, folded into the running minima.  The next channel's staging
        // writes b0 only, and its row pass writes b1 after a barrier.
#pragma unroll
        for (int k = 0; k < kRing; ++k) {
            const int idx = tid + k * kDetectThreads;
            if (idx < n_e) {
                h[k] = fminf(h[k], v[k] - maximum_down(b1, idx, g));
                b[k] = fminf(b[k], v[k]);
            }
        }
    }
    // the seeds on the tile plus d (0 outside the frame), dilated by d along the row, then down the column
    uint32_t* s0 = reinterpret_cast<uint32_t*>(b0);                        // [eh][c2]
    uint32_t* s1 = reinterpret_cast<uint32_t*>(b1);                        // [eh][kTW]
    long long n_seed = 0, n_px = 0;
#pragma unroll
    for (int k = 0; k < kRing; ++k) {
        const int idx = tid + k * kDetectThreads;
        if (idx < n_e) {
            const int i = idx / g.c2, j = idx - i * g.c2;
            const int yy = y0 - g.d + i, xx = x0 - g.d + j;
            const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const bool seed = inside && h[k] > g.threshold && b[k] >= g.bright_min;
            s0[idx] = seed ? 1u : 0u;
            if (seed && i >= g.d && i < g.d + kTH && j >= g.d && j < g.d + kTW) n_seed += 1;
        }
    }
    __syncthreads();
    for (int i = tid; i < eh * kTW; i += kDetectThreads) {
        const int ii = i / kTW, j = i - ii * kTW;
        const uint32_t* p = s0 + ii * g.c2 + j;
        uint32_t m = p[0];
        for (int k = 1; k <= 2 * g.d; ++k) m |= p[k];
        s1[i] = m;
    }
    __syncthreads();
    uint8_t* mk = mask + img * hw;
    if constexpr (VEC) {
        for (int i = tid; i < kTH * (kTW / 4); i += kDetectThreads) {
            const int row = i / (kTW / 4), col = (i - row * (kTW / 4)) * 4;
            const int yy = y0 + row, xx = x0 + col;
            if (yy < H && xx < W) {
                uint4 m = *reinterpret_cast<const uint4*>(s1 + row * kTW + col);
                for (int k = 1; k <= 2 * g.d; ++k) {
                    const uint4 w = *reinterpret_cast<const uint4*>(s1 + (row + k) * kTW + col);
                    m.x |= w.x; m.y |= w.y; m.z |= w.z; m.w |= w.w;
                }
                *reinterpret_cast<uint32_t*>(mk + (int64_t)yy * W + xx) = m.x | (m.y << 8) | (m.z << 16) | (m.w << 24);
                n_px += 4;
            }
        }
    } else {
        for (int i = tid; i < kTH * kTW; i += kDetectThreads) {
            const int row = i / kTW, col = i - row * kTW;
            const int yy = y0 + row, xx = x0 + col;
            if (yy < H && xx < W) {
                uint32_t m = s1[i];
                for (int k = 1; k <= 2 * g.d; ++k) m |= s1[i + k * kTW];
                mk[(int64_t)yy * W + xx] = (uint8_t)m;
                n_px += 1;
            }
        }
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
    n_seed = wave_sum_i64(n_seed);
    n_px = wave_sum_i64(n_px);
    bad = awseg_wave_sum_u32(bad);
    if (lane == 0) { red[wave][0] = n_px; red[wave][1] = n_seed; red[wave][2] = (long long)bad; }
    __syncthreads();
    if (tid == 0) {
        long long row[kDRow] = { 0, 0, 0, 0, 0, 0, 0 };
        for (int w = 0; w < kDetectWaves; ++w) { row[1] += red[w][0]; row[2] += red[w][1]; row[6] += red[w][2]; }
        if (blockIdx.x == 0) row[0] = 1;                                   // the frame, once
        add_row(stats, n_slots, cond, img, row);
    }
}

// J_c and the normalised output of one pixel from its window's S_c and N.  `first` (0 or 1): the channel that counts the pixel itself.
// The counters are a thread's own: at most 8 pixels and 24 changes of at most 2^16, so 32 bits hold them.
__device__ __forceinline__ float fill_pixel(float x, uint32_t masked, uint32_t S, uint32_t N, float sd, float mean, uint32_t first,
                                            uint32_t& n_masked, uint32_t& n_unfilled, uint32_t& change)
{
    const float v = unit(x, sd, mean);
    const bool filled = masked != 0u && N > 0u;
    const float J = filled ? (float)((double)S / ((double)(N > 0u ? N : 1u) * 65536.0)) : v;
    const int32_t moved = (int32_t)rintf(J * 65536.0f) - (int32_t)rintf(v * 65536.0f);       // 0 where J is v
    n_masked += masked != 0u ? first : 0u;
    n_unfilled += masked != 0u && N == 0u ? first : 0u;
    change += (uint32_t)(moved < 0 ? -moved : moved);
    return (J - mean) / sd;
}

__device__ __forceinline__ uint32_t fill_word(float x, uint32_t masked, float sd, float mean)
{
    return masked ? 0u : ((uint32_t)(int32_t)rintf(unit(x, sd, mean) * 65536.0f) | kOne);
}

// Pass B.  grid = (tiles_x * tiles_y, B).
template <bool VEC>
__global__ __launch_bounds__(kThreads)
void fill_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dc_args g, const uint8_t* __restrict__ mask,
                 const int32_t* __restrict__ cond, float* __restrict__ restored, int64_t* __restrict__ stats, int n_slots)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    uint32_t* p0 = reinterpret_cast<uint32_t*>(lds_raw);                   // [frows][fsw]: q | count, 0 where masked or outside
    uint32_t* r0 = p0 + g.frows * g.fsw;                                   // [frows][kTW]: their row sums
    __shared__ long long red[kWaves][3];
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const int tid = threadIdx.x, taps = 2 * g.r;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const uint8_t* mk = mask + img * hw;
    uint32_t n_masked = 0, n_unfilled = 0, change = 0;
    for (int c = 0; c < 3; ++c) {
        const float* plane = image + (img * 3 + c) * hw;
        float* out = restored + (img * 3 + c) * hw;
        const float sd = pick(g.std, c), mean = pick(g.mean, c);
        const uint32_t first = c == 0 ? 1u : 0u;
        if constexpr (VEC) {
            const int groups = g.fsw / 4;
            for (int i = tid; i < g.frows * groups; i += kThreads) {
                const int row = i / groups, col = (i - row * groups) * 4;
                const int yy = y0 - g.r + row, xx = x0 - g.fpad + col;
                uint4 o = { 0u, 0u, 0u, 0u };
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    const int64_t p = (int64_t)yy * W + xx;
                    const float4 a = *reinterpret_cast<const float4*>(plane + p);
                    const uint32_t m = *reinterpret_cast<const uint32_t*>(mk + p);
                    o = { fill_word(a.x, m & 0xFFu, sd, mean), fill_word(a.y, (m >> 8) & 0xFFu, sd, mean),
                          fill_word(a.z, (m >> 16) & 0xFFu, sd, mean), fill_word(a.w, m >> 24, sd, mean) };
                }
                *reinterpret_cast<uint4*>(p0 + row * g.fsw + col) = o;
            }
        } else {
            for (int i = tid; i < g.frows * g.fsw; i += kThreads) {
                const int row = i / g.fsw, col = i - row * g.fsw;
                const int yy = y0 - g.r + row, xx = x0 - g.fpad + col;
                uint32_t o = 0u;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    const int64_t p = (int64_t)yy * W + xx;
                    o = fill_word(plane[p], mk[p], sd, mean);
                }
                p0[row * g.fsw + col] = o;
            }
        }
        __syncthreads();
        for (int i = tid; i < g.frows * kTW; i += kThreads) {              // sums along the row: at most 31 words, sum and count stay apart
            const int row = i / kTW, j = i - row * kTW;
            const uint32_t* p = p0 + row * g.fsw + (g.fpad - g.r) + j;
            uint32_t s = p[0];
            AWSEG_TAPS for (int k = 1; k <= taps; k += 2) s += p[k] + p[k + 1];
            r0[i] = s;
        }
        __syncthreads();
        // sums down the column, unpacked, and the pixels.  The next channel's staging writes p0 only, and its row pass writes r0
        // after a barrier.
        if constexpr (VEC) {
            for (int i = tid; i < kTH * (kTW / 4); i += kThreads) {
                const int row = i / (kTW / 4), col = (i - row * (kTW / 4)) * 4;
                const int yy = y0 + row, xx = x0 + col;
                if (yy < H && xx < W) {
                    uint4 S = { 0u, 0u, 0u, 0u }, N = { 0u, 0u, 0u, 0u };
                    AWSEG_TAPS for (int k = 0; k <= taps; ++k) {
                        const uint4 w = *reinterpret_cast<const uint4*>(r0 + (row + k) * kTW + col);
                        S.x += w.x & kSumMask; S.y += w.y & kSumMask; S.z += w.z & kSumMask; S.w += w.w & kSumMask;
                        N.x += w.x >> 24; N.y += w.y >> 24; N.z += w.z >> 24; N.w += w.w >> 24;
                    }
                    const int64_t p = (int64_t)yy * W + xx;
                    const float4 a = *reinterpret_cast<const float4*>(plane + p);
                    const uint32_t m = *reinterpret_cast<const uint32_t*>(mk + p);
                    *reinterpret_cast<float4*>(out + p) = { fill_pixel(a.x, m & 0xFFu, S.x, N.x, sd, mean, first, n_masked, n_unfilled, change),
                                                            fill_pixel(a.y, (m >> 8) & 0xFFu, S.y, N.y, sd, mean, first, n_masked, n_unfilled, change),
                                                            fill_pixel(a.z, (m >> 16) & 0xFFu, S.z, N.z, sd, mean, first, n_masked, n_unfilled, change),
                                                            fill_pixel(a.w, m >> 24, S.w, N.w, sd, mean, first, n_masked, n_unfilled, change) };
                }
            }
        } else {
            for (int i = tid; i < kTH * kTW; i += kThreads) {
                const int row = i / kTW, col = i - row * kTW;
                const int yy = y0 + row, xx = x0 + col;
                if (yy < H && xx < W) {
                    uint32_t S = 0u, N = 0u;
                    AWSEG_TAPS for (int k = 0; k <= taps; ++k) {
                        const uint32_t w = r0[i + k * kTW];
                        S += w & kSumMask;
                        N += w >> 24;
                    }
                    const int64_t p = (int64_t)yy * W + xx;
                    out[p] = fill_pixel(plane[p], mk[p], S, N, sd, mean, first, n_masked, n_unfilled, change);
                }
            }
        }
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
    n_masked = awseg_wave_sum_u32(n_masked);                               // a wave's sums: at most 64 * 24 * 2^16 < 2^32
    n_unfilled = awseg_wave_sum_u32(n_unfilled);
    change = awseg_wave_sum_u32(change);
    if (lane == 0) { red[wave][0] = n_masked; red[wave][1] = n_unfilled; red[wave][2] = change; }
    __syncthreads();
    if (tid == 0) {
        long long row[kDRow] = { 0, 0, 0, 0, 0, 0, 0 };
        for (int w = 0; w < kWaves; ++w) { row[3] += red[w][0]; row[4] += red[w][1]; row[5] += red[w][2]; }
        add_row(stats, n_slots, cond, img, row);
    }
}

}  // namespace

AWSEG_API int64_t awseg_deocclude_workspace(int64_t batch, int64_t height, int64_t width)
{
    (void)batch; (void)height; (void)width;
    return 0;                                                              // the mask is all that one kernel leaves for the other
}

AWSEG_API int awseg_deocclude(const float* image, int64_t batch, int channels, int64_t height, int64_t width, const float* mean,
                              const float* std, int radius, float threshold, float bright_min, int dilate, const int32_t* cond,
                              float* restored, uint8_t* mask, int64_t* stats, int n_slots, void* workspace, awseg_stream_t stream)
{
    dc_args g = {};
    AWSEG_RESTORE_CHECKS(g, restored && mask,                                  // workspace: no bytes, so NULL will do
                         radius >= 1 && radius <= AWSEG_DEHAZE_MAX_RADIUS && dilate >= 0 && dilate <= kMaxDilate && in_unit(threshold)
                             && in_closed_unit(bright_min));
    g.threshold = threshold;
    g.bright_min = bright_min;
    hipStream_t s = awseg_s(stream);
    const int H = (int)height, W = (int)width;
    const int tiles_x = (W + kTW - 1) / kTW, tiles = tiles_x * ((H + kTH - 1) / kTH);
    const bool vec = (W % 4 == 0) && awseg_aligned(image, 16) && awseg_aligned(restored, 16) && awseg_aligned(mask, 4);
    geometry(radius, dilate, g);
    dim3 grid((unsigned)tiles, (unsigned)batch);
    {
        auto kern = vec ? detect_kernel<true> : detect_kernel<false>;
        const size_t lds = detect_lds(g);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return AWSEG_EINVAL;
        hipLaunchKernelGGL(kern, grid, dim3(kDetectThreads), lds, s, image, H, W, tiles_x, g, cond, mask, stats, n_slots);
        AWSEG_LAUNCH_CHECK();
    }
    {
        auto kern = vec ? fill_kernel<true> : fill_kernel<false>;
        const size_t lds = fill_lds(g);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return AWSEG_EINVAL;
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, s, image, H, W, tiles_x, g, (const uint8_t*)mask, cond, restored, stats, n_slots);
        AWSEG_LAUNCH_CHECK();
    }
    return 0;
}
