// deocclude_tiles.h — what the detection kernel of deocclude.hip (awseg_deocclude) and the tile kernel of estimate.hip
// (awseg_weather_estimate) share: the geometry of a 32 x 64 tile with a halo of 2 r + d, the staging of one
// channel's v_c, and the maximum passes of the opening in LDS.  Every step is the one include/awseg_restore.h states; both
// translation units must produce the same bits from it.  On top of restore_common.h: the tile, v_c, the reductions and the window
// minimum, which these kernels run at 512 threads with -inf outside the frame.
#ifndef AWSEG_DEOCCLUDE_TILES_H
#define AWSEG_DEOCCLUDE_TILES_H
#include "restore_common.h"

namespace {

constexpr int kDetectThreads = 512;                                        // the detection kernel: twice the waves per staged tile
constexpr int kDetectWaves = kDetectThreads / AWSEG_WAVE;

struct dc_args {
    float mean[3], std[3];
    float threshold, bright_min;
    int r, d;
    int halo, pad, sw, rows, q, c1, c2;                                    // detection, see geometry()
    int fpad, fsw, frows;                                                  // fill
};

// Detection: halo = 2 r + d pixels staged around the tile, pad = halo rounded up to whole float4s, sw staged columns, rows staged
// rows; q = r + d: the ring of minima the maximum pass reads; c1 = TW + 2 q; c2 = TW + 2 d: the columns the seeds are needed on.
// Fill: a halo of r, fpad, fsw and frows likewise.
void geometry(int r, int d, dc_args& g)
{
    g.r = r;
    g.d = d;
    g.halo = 2 * r + d;
    g.pad = (g.halo + 3) & ~3;
    g.sw = kTW + 2 * g.pad;
    g.rows = kTH + 2 * g.halo;
    g.q = r + d;
    g.c1 = kTW + 2 * g.q;
    g.c2 = kTW + 2 * d;
    g.fpad = (r + 3) & ~3;
    g.fsw = kTW + 2 * g.fpad;
    g.frows = kTH + 2 * r;
}
size_t detect_lds(const dc_args& g) { return (size_t)g.rows * (g.sw + g.c1) * sizeof(float); }

// a[c] of a kernel argument without an indexed (scratch) copy of it
__device__ __forceinline__ float pick(const float (&a)[3], int c) { return c == 0 ? a[0] : c == 1 ? a[1] : a[2]; }

// b0 [g.rows][g.sw] = v_c over the tile and its halo, +inf outside the frame; `bad` += the tile's own values that are not finite.
template <bool VEC>
__device__ __forceinline__ void stage_channel(const float* __restrict__ plane, int H, int W, int y0, int x0, const dc_args& g, float sd,
                                              float mean, float* __restrict__ b0, uint32_t& bad)
{
    const int tid = threadIdx.x;
    if constexpr (VEC) {
        const int groups = g.sw / 4;
        for (int i = tid; i < g.rows * groups; i += kDetectThreads) {
            const int row = i / groups, col = (i - row * groups) * 4;
            const int yy = y0 - g.halo + row, xx = x0 - g.pad + col;         // W % 4 == 0 and (x0 - pad) % 4 == 0: a group is inside or outside
            float4 o = { INFINITY, INFINITY, INFINITY, INFINITY };
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float4 a = *reinterpret_cast<const float4*>(plane + (int64_t)yy * W + xx);
                if (row >= g.halo && row < g.halo + kTH && col >= g.pad && col < g.pad + kTW)
                    bad += not_finite(a.x) + not_finite(a.y) + not_finite(a.z) + not_finite(a.w);
                o = { unit(a.x, sd, mean), unit(a.y, sd, mean), unit(a.z, sd, mean), unit(a.w, sd, mean) };
            }
            *reinterpret_cast<float4*>(b0 + row * g.sw + col) = o;
        }
    } else {
        for (int i = tid; i < g.rows * g.sw; i += kDetectThreads) {
            const int row = i / g.sw, col = i - row * g.sw;
            const int yy = y0 - g.halo + row, xx = x0 - g.pad + col;
            float o = INFINITY;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float a = plane[(int64_t)yy * W + xx];
                if (row >= g.halo && row < g.halo + kTH && col >= g.pad && col < g.pad + kTW) bad += not_finite(a);
                o = unit(a, sd, mean);
            }
            b0[row * g.sw + col] = o;
        }
    }
}

// The maximum of the minima along the row.  In: b0 of window_minimum.  Out: b1 [kTH + 2 q][c2], column j = pixel x0 - d + j; ends
// with a barrier.  The maximum down the column is the caller's: it takes it at its own positions only.
__device__ __forceinline__ void maximum_row_pass(const dc_args& g, const float* __restrict__ b0, float* __restrict__ b1)
{
    const int tid = threadIdx.x, taps = 2 * g.r;
    const int rows_e = kTH + 2 * g.q;
    for (int i = tid; i < rows_e * g.c2; i += kDetectThreads) {
        const int ii = i / g.c2, j = i - ii * g.c2;
        const float* p = b0 + ii * g.c1 + j;
        float m = p[0];
        AWSEG_TAPS for (int k = 1; k <= taps; k += 2) m = fmaxf(m, fmaxf(p[k], p[k + 1]));
        b1[i] = m;
    }
    __syncthreads();
}

// o_c at position idx of b1 [.][c2]: the maximum down the column of maximum_row_pass's rows.
__device__ __forceinline__ float maximum_down(const float* __restrict__ b1, int idx, const dc_args& g)
{
    const int taps = 2 * g.r;
    const float* p = b1 + idx;
    float m = p[0];
    AWSEG_TAPS for (int t = 1; t <= taps; t += 2) m = fmaxf(m, fmaxf(p[t * g.c2], p[(t + 1) * g.c2]));
    return m;
}

}  // namespace
#endif  // AWSEG_DEOCCLUDE_TILES_H
