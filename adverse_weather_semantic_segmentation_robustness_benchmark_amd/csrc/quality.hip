// quality.hip — image-quality counters of a corrupted frame against its clean twin: the error terms of PSNR and the
// luminance / contrast-structure factors of SSIM (Wang et al. 2004: 11 x 11 Gaussian window, valid windows only), as int64 sums of
// float32 terms in units of 2^-24.
//
// awseg_image_quality: a tile kernel like boundary.hip.  A block owns AWSEG_IQ_TILE_H x AWSEG_IQ_TILE_W window centres (a window is
// addressed by its top-left pixel) of one frame and loops over the channels.  Per channel:
//   1. stage x = image * std + mean and y likewise from the twin for the tile plus its 10-pixel apron in LDS (16-byte loads when the
//      rows allow, scalar otherwise); the error terms of the pixels the tile owns come from the same loaded values, so every input
//      byte is read from HBM once, the apron excepted;
//   2. horizontal pass: the five maps x, y, x*x, y*y, x*y filtered along the row, one (row, centre column) per lane, into LDS;
//   3. vertical pass on the horizontal sums, one centre per lane, then l, cs, s and their fixed-point terms.
// Per-lane int64 sums are reduced over the wave (shuffles) and the block (LDS); block (x, y) writes one int64 partial row that
// image_quality_fold_kernel sums into slot 0 and slot 1 + cond[b]: integer sums only, so the result does not depend on the grid.
// LDS: 2 x 42 x 76 x 4 (x, y) + 5 x 42 x 64 x 4 (horizontal sums) + 4 x 10 x 8 = 79616 B: two resident blocks in a CU's 160 KiB.
#include "awseg_common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int kTH = AWSEG_IQ_TILE_H, kTW = AWSEG_IQ_TILE_W;                // window centres per tile
constexpr int kApron = 10;                                                 // an 11-tap window reaches 10 pixels past its first
constexpr int kRows = kTH + kApron;                                        // staged rows
constexpr int kSW = 76;                                                    // staged columns: kTW + 10, rounded up to whole float4s
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / AWSEG_WAVE;
constexpr int kTaps = 11;
constexpr int kRow = AWSEG_IQ_ROW;
constexpr size_t kLdsBytes = (size_t)(2 * kRows * kSW + 5 * kRows * kTW) * sizeof(float) + (size_t)kWaves * kRow * sizeof(long long);
static_assert(kTW == AWSEG_WAVE, "one wave per row of centres");
static_assert(kSW % 4 == 0 && kSW >= kTW + kApron, "the staged row holds the apron in whole float4s");
static_assert(2 * kLdsBytes <= 160 * 1024, "two resident blocks per CU");

struct iq_args {
    float mean[4], std[4];
    float taps[kTaps];
    float c1, c2;
};

struct iq_sums {                                                           // one lane's share of a row, [0] (frames) excepted
    uint32_t n_err = 0, bad_err = 0, n_win = 0, bad_win = 0;               // named, and updated without branches: the compiler
    long long abs_q = 0, sq_q = 0, l_q = 0, cs_q = 0, s_q = 0;             // turns "one of two array cells" into an indexed scratch access
    __device__ __forceinline__ long long get(int k) const
    {
        switch (k) {
        case 1: return n_err;
        case 2: return abs_q;
        case 3: return sq_q;
        case 4: return bad_err;
        case 5: return n_win;
        case 6: return l_q;
        case 7: return cs_q;
        case 8: return s_q;
        default: return bad_win;
        }
    }
};

__device__ __forceinline__ void error_term(float a, float b, float sd, iq_sums& s)
{
    const float d = (a - b) * sd;
    const float ad = fabsf(d);
    const bool ok = ad <= 2.0f;                                            // NaN fails this
    s.n_err += ok ? 1u : 0u;
    s.bad_err += ok ? 0u : 1u;
    s.abs_q += ok ? (long long)rintf(ad * 16777216.0f) : 0;
    s.sq_q += ok ? (long long)rintf((d * d) * 16777216.0f) : 0;
}

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// grid = (tiles_x * tiles_y, B); block (t, b) writes partial[(b * gridDim.x + t)][AWSEG_IQ_ROW].
// VEC: W % 4 == 0 and image, ref_images 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(kThreads)
void image_quality_kernel(const float* __restrict__ image, const float* __restrict__ ref_images, int n_refs, int channels, int H, int W,
                          int tiles_x, const int32_t* __restrict__ frame_ref, const iq_args g, long long* __restrict__ partial,
                          int64_t* __restrict__ oob)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* sx = reinterpret_cast<float*>(lds_raw);                         // [kRows][kSW]
    float* sy = sx + kRows * kSW;                                          // [kRows][kSW]
    float* hs = sy + kRows * kSW;                                          // [5][kRows][kTW]
    long long* red = reinterpret_cast<long long*>(hs + 5 * kRows * kTW);   // [kWaves][kRow]

    const int64_t img = blockIdx.y;
    const int tid = threadIdx.x;
    long long* dst = partial + (img * gridDim.x + blockIdx.x) * kRow;
    const int r = frame_ref[img];
    if (r < 0 || r >= n_refs) {                                            // no clean twin: the frame is skipped (uniform over the block)
        if (tid < kRow) dst[tid] = 0;
        if (r >= n_refs && blockIdx.x == 0 && tid == 0) atomicAdd((unsigned long long*)oob, (unsigned long long)((int64_t)H * W));
        return;
    }
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int tiles_y = gridDim.x / tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    // the pixels whose error terms this tile counts: its kTH x kTW pixels, and what lies beyond them in the last tile row / column
    const int own_rows = ty == tiles_y - 1 ? kRows : kTH, own_cols = tx == tiles_x - 1 ? kSW : kTW;
    const int64_t hw = (int64_t)H * W;
    iq_sums s;

    for (int c = 0; c < channels; ++c) {
        const float* ip = image + (img * channels + c) * hw;
        const float* rp = ref_images + ((int64_t)r * channels + c) * hw;
        // (selected, not indexed: a run-time index into the kernel arguments would put them in scratch)
        const float mean = c == 0 ? g.mean[0] : c == 1 ? g.mean[1] : c == 2 ? g.mean[2] : g.mean[3];
        const float sd = c == 0 ? g.std[0] : c == 1 ? g.std[1] : c == 2 ? g.std[2] : g.std[3];
        // 1. stage (pixels outside the frame: zeros no measured window reads)
        if constexpr (VEC) {
            constexpr int kGroups = kSW / 4;
            for (int i = tid; i < kRows * kGroups; i += kThreads) {
                const int row = i / kGroups, col = (i - row * kGroups) * 4;
                const int yy = y0 + row, xx = x0 + col;                    // W % 4 == 0 and x0 % 4 == 0: a group is inside or outside
                float4 a = { 0.0f, 0.0f, 0.0f, 0.0f }, b = a;
                if (yy < H && xx < W) {
                    const float4 ia = *reinterpret_cast<const float4*>(ip + (int64_t)yy * W + xx);
                    const float4 ib = *reinterpret_cast<const float4*>(rp + (int64_t)yy * W + xx);
                    if (row < own_rows && col < own_cols) {
                        error_term(ia.x, ib.x, sd, s); error_term(ia.y, ib.y, sd, s);
                        error_term(ia.z, ib.z, sd, s); error_term(ia.w, ib.w, sd, s);
                    }
                    a = { ia.x * sd + mean, ia.y * sd + mean, ia.z * sd + mean, ia.w * sd + mean };
                    b = { ib.x * sd + mean, ib.y * sd + mean, ib.z * sd + mean, ib.w * sd + mean };
                }
                *reinterpret_cast<float4*>(sx + row * kSW + col) = a;
                *reinterpret_cast<float4*>(sy + row * kSW + col) = b;
            }
        } else {
            for (int i = tid; i < kRows * kSW; i += kThreads) {
                const int row = i / kSW, col = i - row * kSW;
                const int yy = y0 + row, xx = x0 + col;
                float a = 0.0f, b = 0.0f;
                if (yy < H && xx < W) {
                    const float ia = ip[(int64_t)yy * W + xx], ib = rp[(int64_t)yy * W + xx];
                    if (row < own_rows && col < own_cols) error_term(ia, ib, sd, s);
                    a = ia * sd + mean;
                    b = ib * sd + mean;
                }
                sx[row * kSW + col] = a;
                sy[row * kSW + col] = b;
            }
        }
        __syncthreads();
        // 2. horizontal pass: a wave takes one staged row, a lane one centre column
        for (int i = tid; i < kRows * kTW; i += kThreads) {
            const int row = i / kTW, col = i - row * kTW;
            if (y0 + row >= H || x0 + col + kApron >= W) continue;         // no measured window reads this sum
            const float* px = sx + row * kSW + col;
            const float* py = sy + row * kSW + col;
            float x = px[0], y = py[0];
            float ax = g.taps[0] * x, ay = g.taps[0] * y, axx = g.taps[0] * (x * x), ayy = g.taps[0] * (y * y), axy = g.taps[0] * (x * y);
#pragma unroll
            for (int k = 1; k < kTaps; ++k) {
                x = px[k]; y = py[k];
                const float t = g.taps[k];
                ax = ax + t * x;
                ay = ay + t * y;
                axx = axx + t * (x * x);
                ayy = ayy + t * (y * y);
                axy = axy + t * (x * y);
            }
            float* h = hs + row * kTW + col;
            h[0] = ax; h[kRows * kTW] = ay; h[2 * kRows * kTW] = axx; h[3 * kRows * kTW] = ayy; h[4 * kRows * kTW] = axy;
        }
        __syncthreads();
        // 3. vertical pass and the window terms
        for (int i = tid; i < kTH * kTW; i += kThreads) {
            const int cy = i / kTW, cx = i - cy * kTW;
            if (y0 + cy + kApron >= H || x0 + cx + kApron >= W) continue;
            const float* h = hs + cy * kTW + cx;
            float m[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float* hq = h + q * kRows * kTW;
                float acc = g.taps[0] * hq[0];
#pragma unroll
                for (int k = 1; k < kTaps; ++k) acc = acc + g.taps[k] * hq[k * kTW];
                m[q] = acc;
            }
            const float mx = m[0], my = m[1];
            const float vx = m[2] - mx * mx, vy = m[3] - my * my, cxy = m[4] - mx * my;
            const float l = ((2.0f * mx) * my + g.c1) / ((mx * mx + my * my) + g.c1);
            const float cs = (2.0f * cxy + g.c2) / ((vx + vy) + g.c2);
            const float sv = l * cs;
            const bool ok = fabsf(l) <= 2.0f && fabsf(cs) <= 2.0f && fabsf(sv) <= 2.0f;
            s.n_win += ok ? 1u : 0u;
            s.bad_win += ok ? 0u : 1u;
            s.l_q += ok ? (long long)rintf(l * 16777216.0f) : 0;
            s.cs_q += ok ? (long long)rintf(cs * 16777216.0f) : 0;
            s.s_q += ok ? (long long)rintf(sv * 16777216.0f) : 0;
        }
        __syncthreads();                                                   // the next channel overwrites sx, sy and hs
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
#pragma unroll
    for (int k = 1; k < kRow; ++k) {
        const long long t = wave_sum_i64(s.get(k));
        if (lane == 0) red[wave * kRow + k] = t;
    }
    __syncthreads();
    if (tid < kRow) {
        long long t = 0;
        if (tid == 0) t = blockIdx.x == 0 ? 1 : 0;                         // frames
        else for (int w = 0; w < kWaves; ++w) t += red[w * kRow + tid];
        dst[tid] = t;
    }
}

// grid = B, block = kThreads: sum the frame's per-tile rows into slot 0 and slot 1 + cond[b].
__global__ __launch_bounds__(kThreads)
void image_quality_fold_kernel(const long long* __restrict__ partial, int tiles, const int32_t* __restrict__ cond, int n_slots,
                               int64_t* __restrict__ stats)
{
    __shared__ long long red[kWaves][kRow];
    const int img = blockIdx.x, tid = threadIdx.x;
    const long long* src = partial + (int64_t)img * tiles * kRow;
    long long v[kRow];
#pragma unroll
    for (int k = 0; k < kRow; ++k) v[k] = 0;
    for (int t = tid; t < tiles; t += kThreads) {
#pragma unroll
        for (int k = 0; k < kRow; ++k) v[k] += src[(int64_t)t * kRow + k];
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
#pragma unroll
    for (int k = 0; k < kRow; ++k) {
        const long long t = wave_sum_i64(v[k]);
        if (lane == 0) red[wave][k] = t;
    }
    __syncthreads();
    if (tid < kRow) {
        long long t = 0;
        for (int w = 0; w < kWaves; ++w) t += red[w][tid];
        if (t) {
            int slot = -1;
            if (cond) { const int c = cond[img]; if (c >= 0 && c + 1 < n_slots) slot = c + 1; }
            atomicAdd((unsigned long long*)&stats[tid], (unsigned long long)t);
            if (slot > 0) atomicAdd((unsigned long long*)&stats[(int64_t)slot * kRow + tid], (unsigned long long)t);
        }
    }
}

int64_t tiles_of(int64_t n, int tile)                                      // tiles of window centres along one side; one when there is no window
{
    const int64_t centres = n - kApron;
    return centres < 1 ? 1 : (centres + tile - 1) / tile;
}

bool is_finite(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }

}  // namespace

AWSEG_API int64_t awseg_image_quality_workspace(int64_t batch, int channels, int64_t height, int64_t width)
{
    (void)channels;                                                        // the block loops over the channels
    if (batch < 1) batch = 1;
    if (height < 1) height = 1;
    if (width < 1) width = 1;
    return batch * tiles_of(height, kTH) * tiles_of(width, kTW) * kRow * (int64_t)sizeof(long long);
}

AWSEG_API int awseg_image_quality(const float* image, const float* ref_images, int n_refs, int64_t batch, int channels,
                                  int64_t height, int64_t width, const int32_t* frame_ref, const float* mean, const float* std,
                                  const float* taps, float c1, float c2, const int32_t* cond, int64_t* stats, int n_slots,
                                  int64_t* oob, void* workspace, awseg_stream_t stream)
{
    if (!image || !ref_images || !frame_ref || !mean || !std || !taps || !stats || !oob || !workspace) return AWSEG_EINVAL;
    if (n_refs < 1 || batch < 0 || height < 1 || width < 1 || channels < 1 || channels > 4 || n_slots < 1) return AWSEG_EINVAL;
    iq_args g = {};
    for (int c = 0; c < channels; ++c) {
        if (!(std[c] > 0.0f && std[c] <= FLT_MAX) || !is_finite(mean[c])) return AWSEG_EINVAL;
        g.mean[c] = mean[c];
        g.std[c] = std[c];
    }
    for (int k = 0; k < kTaps; ++k) {
        if (!is_finite(taps[k])) return AWSEG_EINVAL;
        g.taps[k] = taps[k];
    }
    if (!(c1 > 0.0f && c1 <= FLT_MAX) || !(c2 > 0.0f && c2 <= FLT_MAX)) return AWSEG_EINVAL;
    g.c1 = c1;
    g.c2 = c2;
    if (batch > 65535 || height > INT32_MAX / width) return AWSEG_ERANGE;      // grid.y; H * W >= 2^31
    if (batch == 0) return 0;
    hipStream_t s = awseg_s(stream);
    const int tiles_x = (int)tiles_of(width, kTW);
    const int tiles = (int)(tiles_of(height, kTH) * tiles_x);                  // the count the workspace query assumed
    const bool vec = (width % 4 == 0) && awseg_aligned(image, 16) && awseg_aligned(ref_images, 16);
    long long* partial = (long long*)workspace;
    dim3 grid((unsigned)tiles, (unsigned)batch), block(kThreads);
    auto kern = vec ? image_quality_kernel<true> : image_quality_kernel<false>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes) != hipSuccess)
        return AWSEG_EINVAL;
    hipLaunchKernelGGL(kern, grid, block, kLdsBytes, s, image, ref_images, n_refs, channels, (int)height, (int)width, tiles_x, frame_ref,
                       g, partial, oob);
    AWSEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(image_quality_fold_kernel, dim3((unsigned)batch), block, 0, s, partial, tiles, cond, n_slots, stats);
    AWSEG_LAUNCH_CHECK();
    return 0;
}
