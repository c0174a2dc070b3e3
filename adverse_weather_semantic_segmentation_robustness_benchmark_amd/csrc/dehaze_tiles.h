// dehaze_tiles.h — what the dehazing kernels of dehaze.hip (awseg_dehaze) and dehaze_guided.hip (awseg_dehaze_guided) share
// (DESIGN.md §10n, §10n-bis): the per-frame record, the tile geometry, the staging of min_c v_c (/ A_c) with its halo, the separable
// window passes, passes A (dark channel, bins, histogram) and B (airlight sums), and the recovery arithmetic.  Every step is the
// one include/awseg_restore.h states; both translation units must produce the same bits from it.
#ifndef AWSEG_DEHAZE_TILES_H
#define AWSEG_DEHAZE_TILES_H
#include "restore_common.h"                                               // v_c, the reductions, the window minimum, the refusals

namespace {

constexpr int kRow = AWSEG_DEHAZE_ROW;
constexpr int kBins = 256;
static_assert(kThreads == kBins, "one thread per histogram word");

struct dz_record {                                                         // per frame, at the head of the workspace
    uint32_t hist[kBins];
    long long sum[3], n, nonfinite;
};
static_assert(sizeof(dz_record) == AWSEG_DEHAZE_FRAME_RECORD, "the size the workspace query states");

struct dz_args {
    float mean[3], std[3];
    float omega, t_min, a_min;
    int r, halo, pad, sw, rows, q, c1;                                     // see geometry()
};

// halo: pixels staged around the tile; pad: halo rounded up to whole float4s; sw: staged columns; rows: staged rows;
// q = halo - r: the ring of window minima the maximum pass reads around the tile; c1 = kTW + 2 q.
void geometry(int r, int refine, dz_args& g)
{
    g.r = r;
    g.halo = refine ? 2 * r : r;
    g.pad = (g.halo + 3) & ~3;
    g.sw = kTW + 2 * g.pad;
    g.rows = kTH + 2 * g.halo;
    g.q = g.halo - r;
    g.c1 = kTW + 2 * g.q;
}
size_t lds_bytes(const dz_args& g) { return (size_t)g.rows * (g.sw + g.c1) * sizeof(float); }

template <bool DIV>
__device__ __forceinline__ float min_of(float x0, float x1, float x2, const dz_args& g, float a0, float a1, float a2)
{
    float v0 = unit(x0, g.std[0], g.mean[0]), v1 = unit(x1, g.std[1], g.mean[1]), v2 = unit(x2, g.std[2], g.mean[2]);
    if constexpr (DIV) { v0 = v0 / a0; v1 = v1 / a1; v2 = v2 / a2; }
    return fminf(fminf(v0, v1), v2);
}

// b0 [g.rows][g.sw] = min_c over the tile and its halo, +inf outside the frame.  COUNT: `bad` += the tile's own values that are not finite.
template <bool VEC, bool DIV, bool COUNT>
__device__ __forceinline__ void stage(const float* __restrict__ frame, int64_t hw, int H, int W, int y0, int x0, const dz_args& g,
                                      float a0, float a1, float a2, float* __restrict__ b0, uint32_t& bad)
{
    const int tid = threadIdx.x;
    if constexpr (VEC) {
        const int groups = g.sw / 4;
        for (int i = tid; i < g.rows * groups; i += kThreads) {
            const int row = i / groups, col = (i - row * groups) * 4;
            const int yy = y0 - g.halo + row, xx = x0 - g.pad + col;         // W % 4 == 0 and (x0 - pad) % 4 == 0: a group is inside or outside
            float4 o = { INFINITY, INFINITY, INFINITY, INFINITY };
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float* p = frame + (int64_t)yy * W + xx;
                const float4 a = *reinterpret_cast<const float4*>(p);
                const float4 b = *reinterpret_cast<const float4*>(p + hw);
                const float4 c = *reinterpret_cast<const float4*>(p + 2 * hw);
                if constexpr (COUNT) {
                    if (row >= g.halo && row < g.halo + kTH && col >= g.pad && col < g.pad + kTW)
                        bad += not_finite(a.x) + not_finite(a.y) + not_finite(a.z) + not_finite(a.w) + not_finite(b.x) + not_finite(b.y)
                             + not_finite(b.z) + not_finite(b.w) + not_finite(c.x) + not_finite(c.y) + not_finite(c.z) + not_finite(c.w);
                }
                o = { min_of<DIV>(a.x, b.x, c.x, g, a0, a1, a2), min_of<DIV>(a.y, b.y, c.y, g, a0, a1, a2),
                      min_of<DIV>(a.z, b.z, c.z, g, a0, a1, a2), min_of<DIV>(a.w, b.w, c.w, g, a0, a1, a2) };
            }
            *reinterpret_cast<float4*>(b0 + row * g.sw + col) = o;
        }
    } else {
        for (int i = tid; i < g.rows * g.sw; i += kThreads) {
            const int row = i / g.sw, col = i - row * g.sw;
            const int yy = y0 - g.halo + row, xx = x0 - g.pad + col;
            float o = INFINITY;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float* p = frame + (int64_t)yy * W + xx;
                const float a = p[0], b = p[hw], c = p[2 * hw];
                if constexpr (COUNT) {
                    if (row >= g.halo && row < g.halo + kTH && col >= g.pad && col < g.pad + kTW)
                        bad += not_finite(a) + not_finite(b) + not_finite(c);
                }
                o = min_of<DIV>(a, b, c, g, a0, a1, a2);
            }
            b0[row * g.sw + col] = o;
        }
    }
}

// The window passes on the staged map.  On return b0 holds [kTH][kTW] (row stride kTW): the (2r+1)^2 minimum at the tile's pixels, or
// (REFINE) the (2r+1)^2 maximum of those minima.  Begins and ends with a barrier.
template <bool REFINE>
__device__ __forceinline__ void window_passes(int H, int W, int y0, int x0, const dz_args& g, float* __restrict__ b0, float* __restrict__ b1)
{
    const int tid = threadIdx.x, taps = 2 * g.r;
    const int rows_e = kTH + 2 * g.q;
    __syncthreads();
    window_minimum<kThreads, REFINE, false>(H, W, y0, x0, g, b0, b1);   // the plain tap loops: see there
    if constexpr (REFINE) {
        for (int i = tid; i < rows_e * kTW; i += kThreads) {               // maximum along the row
            const int ii = i / kTW, j = i - ii * kTW;
            const float* p = b0 + ii * g.c1 + j;
            float m = p[0];
            for (int k = 1; k <= taps; ++k) m = fmaxf(m, p[k]);
            b1[i] = m;
        }
        __syncthreads();
        for (int i = tid; i < kTH * kTW; i += kThreads) {                  // maximum down the column
            const float* p = b1 + i;
            float m = p[0];
            for (int k = 1; k <= taps; ++k) m = fmaxf(m, p[k * kTW]);
            b0[i] = m;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t bin_of(float dark) { return (uint32_t)(int)(dark * 255.0f); }

// A.  grid = (tiles_x * tiles_y, B).  ws: B records, then B x H x W bins.
template <bool VEC>
__global__ __launch_bounds__(kThreads)
void dark_channel_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dz_args g, unsigned char* __restrict__ ws)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* b0 = reinterpret_cast<float*>(lds_raw);                         // [rows][sw]
    float* b1 = b0 + g.rows * g.sw;                                        // [rows][c1]
    __shared__ uint32_t hist[kBins];
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const int tid = threadIdx.x;
    dz_record* rec = reinterpret_cast<dz_record*>(ws) + img;
    unsigned char* bins = ws + (int64_t)gridDim.y * (int64_t)sizeof(dz_record) + img * hw;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    uint32_t bad = 0;
    hist[tid] = 0;
    stage<VEC, false, true>(image + img * 3 * hw, hw, H, W, y0, x0, g, 1.0f, 1.0f, 1.0f, b0, bad);
    window_passes<false>(H, W, y0, x0, g, b0, b1);
    if constexpr (VEC) {
        for (int i = tid; i < kTH * (kTW / 4); i += kThreads) {
            const int row = i / (kTW / 4), col = (i - row * (kTW / 4)) * 4;
            const int yy = y0 + row, xx = x0 + col;
            if (yy < H && xx < W) {
                const float4 d = *reinterpret_cast<const float4*>(b0 + row * kTW + col);
                const uint32_t k0 = bin_of(d.x), k1 = bin_of(d.y), k2 = bin_of(d.z), k3 = bin_of(d.w);
                atomicAdd(&hist[k0], 1u); atomicAdd(&hist[k1], 1u); atomicAdd(&hist[k2], 1u); atomicAdd(&hist[k3], 1u);
                *reinterpret_cast<uint32_t*>(bins + (int64_t)yy * W + xx) = k0 | (k1 << 8) | (k2 << 16) | (k3 << 24);
            }
        }
    } else {
        for (int i = tid; i < kTH * kTW; i += kThreads) {
            const int row = i / kTW, col = i - row * kTW;
            const int yy = y0 + row, xx = x0 + col;
            if (yy < H && xx < W) {
                const uint32_t k = bin_of(b0[i]);
                atomicAdd(&hist[k], 1u);
                bins[(int64_t)yy * W + xx] = (unsigned char)k;
            }
        }
    }
    __syncthreads();
    if (hist[tid]) atomicAdd(&rec->hist[tid], hist[tid]);
    bad = awseg_wave_sum_u32(bad);
    if ((tid & (AWSEG_WAVE - 1)) == 0 && bad) atomicAdd((unsigned long long*)&rec->nonfinite, (unsigned long long)bad);
}

// B.  grid = (blocks per frame, B).  VEC4: H * W % 4 == 0, four bins per 32-bit load.
template <bool VEC4>
__global__ __launch_bounds__(kThreads)
void airlight_kernel(const float* __restrict__ image, int64_t hw, const dz_args g, unsigned char* __restrict__ ws)
{
    __shared__ uint32_t hist[kBins];
    __shared__ int b_star;
    __shared__ long long red[kWaves][4];
    const int64_t img = blockIdx.y;
    const int tid = threadIdx.x;
    dz_record* rec = reinterpret_cast<dz_record*>(ws) + img;
    const unsigned char* bins = ws + (int64_t)gridDim.y * (int64_t)sizeof(dz_record) + img * hw;
    const float* frame = image + img * 3 * hw;
    hist[tid] = rec->hist[tid];
    if (tid == 0) b_star = 0;
    __syncthreads();
    const uint64_t n_top = (uint64_t)((hw + 999) / 1000);
    uint64_t suffix = 0;
    for (int k = tid; k < kBins; ++k) suffix += hist[k];
    if (suffix >= n_top) atomicMax(&b_star, tid);                          // bin 0's suffix is H * W >= n_top
    __syncthreads();
    const uint32_t lo = (uint32_t)b_star;
    long long s0 = 0, s1 = 0, s2 = 0, n = 0;
    auto take = [&](int64_t p) {
        s0 += (long long)rintf(unit(frame[p], g.std[0], g.mean[0]) * 65536.0f);
        s1 += (long long)rintf(unit(frame[hw + p], g.std[1], g.mean[1]) * 65536.0f);
        s2 += (long long)rintf(unit(frame[2 * hw + p], g.std[2], g.mean[2]) * 65536.0f);
        n += 1;
    };
    const int64_t first = (int64_t)blockIdx.x * kThreads + tid, step = (int64_t)gridDim.x * kThreads;
    if constexpr (VEC4) {
        const uint32_t* words = reinterpret_cast<const uint32_t*>(bins);
        for (int64_t i = first; i < hw / 4; i += step) {
            const uint32_t w = words[i];
            if ((w & 0xFFu) >= lo) take(4 * i);
            if (((w >> 8) & 0xFFu) >= lo) take(4 * i + 1);
            if (((w >> 16) & 0xFFu) >= lo) take(4 * i + 2);
            if ((w >> 24) >= lo) take(4 * i + 3);
        }
    } else {
        for (int64_t i = first; i < hw; i += step)
            if (bins[i] >= lo) take(i);
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
    s0 = wave_sum_i64(s0); s1 = wave_sum_i64(s1); s2 = wave_sum_i64(s2); n = wave_sum_i64(n);
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = n; }
    __syncthreads();
    if (tid < 4) {
        long long t = 0;
        for (int w = 0; w < kWaves; ++w) t += red[w][tid];
        long long* dst = tid < 3 ? &rec->sum[tid] : &rec->n;
        if (t) atomicAdd((unsigned long long*)dst, (unsigned long long)t);
    }
}

__device__ __forceinline__ float airlight_of(long long s, long long n, float a_min, bool& floored)
{
    const float a = (float)((double)s / ((double)n * 65536.0));
    floored = floored || a < a_min;
    return fmaxf(a, a_min);
}

struct dz_pixel { float r0, r1, r2; };

// J and the normalised output of one pixel at the transmission t.
__device__ __forceinline__ dz_pixel recover_at(float t, float x0, float x1, float x2, const dz_args& g, float a0, float a1, float a2, long long& t_q)
{
    t_q += (long long)rintf(t * 65536.0f);
    const float v0 = unit(x0, g.std[0], g.mean[0]), v1 = unit(x1, g.std[1], g.mean[1]), v2 = unit(x2, g.std[2], g.mean[2]);
    const float j0 = fminf(fmaxf((v0 - a0) / t + a0, 0.0f), 1.0f);
    const float j1 = fminf(fmaxf((v1 - a1) / t + a1, 0.0f), 1.0f);
    const float j2 = fminf(fmaxf((v2 - a2) / t + a2, 0.0f), 1.0f);
    return { (j0 - g.mean[0]) / g.std[0], (j1 - g.mean[1]) / g.std[1], (j2 - g.mean[2]) / g.std[2] };
}

__device__ __forceinline__ dz_pixel recover(float o, float x0, float x1, float x2, const dz_args& g, float a0, float a1, float a2, long long& t_q)
{
    return recover_at(fmaxf(1.0f - g.omega * o, g.t_min), x0, x1, x2, g, a0, a1, a2, t_q);
}

// The refusals awseg_dehaze and awseg_dehaze_guided share; fills g's normalisation and parameters.  own_pointers and own_parameters:
// what the one has and the other has not (refine; guided_stats, the guided radius and eps).
#define AWSEG_DEHAZE_CHECKS(own_pointers, own_parameters)                                                                     \
    dz_args g = {};                                                                                                             \
    AWSEG_RESTORE_CHECKS(g, restored && airlight && workspace && (own_pointers),                                                \
                         radius >= 1 && radius <= AWSEG_DEHAZE_MAX_RADIUS && (own_parameters) && in_unit(omega) && in_unit(t_min) \
                             && in_unit(airlight_min));                                                                         \
    g.omega = omega;                                                                                                            \
    g.t_min = t_min;                                                                                                            \
    g.a_min = airlight_min

// Clears the frames' records and runs passes A and B on `s`: afterwards every record holds its frame's airlight sums and the bin
// map is written.  Leaves g at geometry(radius, 0).
inline int estimate_airlight(const float* image, int64_t batch, int H, int W, int radius, dz_args& g, bool vec, unsigned char* ws,
                             hipStream_t s)
{
    const int64_t hw = (int64_t)H * W;
    const int tiles_x = (W + kTW - 1) / kTW, tiles = tiles_x * ((H + kTH - 1) / kTH);
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)batch * sizeof(dz_record), s);     // histograms and sums: the kernels add to them
    if (e != hipSuccess) return (int)e;
    dim3 grid((unsigned)tiles, (unsigned)batch), block(kThreads);
    geometry(radius, 0, g);
    {
        auto kern = vec ? dark_channel_kernel<true> : dark_channel_kernel<false>;
        const size_t lds = lds_bytes(g);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return AWSEG_EINVAL;
        hipLaunchKernelGGL(kern, grid, block, lds, s, image, H, W, tiles_x, g, ws);
        AWSEG_LAUNCH_CHECK();
    }
    {
        const bool vec4 = hw % 4 == 0;                                         // the frame's bins then begin on a 4-byte boundary
        const int bpi = awseg_blocks_per_image(vec4 ? hw / 4 : hw, kThreads, batch, 8);
        auto kern = vec4 ? airlight_kernel<true> : airlight_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)bpi, (unsigned)batch), block, 0, s, image, hw, g, ws);
        AWSEG_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace
#endif  // AWSEG_DEHAZE_TILES_H
