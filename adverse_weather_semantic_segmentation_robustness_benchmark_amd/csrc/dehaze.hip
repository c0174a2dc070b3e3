// dehaze.hip — dark-channel-prior dehazing of the frames the model sees (He, Sun, Tang 2009), the arithmetic
// include/awseg_restore.h states step by step: every output bit is what numpy float32 gives.
//
// awseg_dehaze: three kernels on the caller's stream, no host synchronisation, no block waits for another.  A, B and the pieces of C
// that awseg_dehaze_guided (dehaze_guided.hip) uses as well live in dehaze_tiles.h; C itself and the launcher are here.
//   A  dark_channel_kernel   tile kernel like quality.hip.  A block owns AWSEG_DEHAZE_TILE_H x AWSEG_DEHAZE_TILE_W pixels of one frame,
//                            stages m = min_c v_c for the tile plus a halo of r in LDS (+inf outside the frame: such positions take part
//                            in no minimum), takes the (2r+1)^2 minimum separably (along the row, then down the column), stores one
//                            uint8 bin per pixel and counts the bins in an LDS histogram that it adds to the frame's 256 words.
//   B  airlight_kernel       every block recomputes b* from the frame's histogram, walks its share of the bin map and sums
//                            rintf(v_c * 65536) over the pixels with bin >= b* (int64: exact, order-free).
//   C  recover_kernel        the same tile kernel on n = min_c v_c / A_c with a halo of r (refine 0) or 2 r (refine 1: minimum, then
//                            maximum of the minima, -inf outside the frame), then t, J and the normalised output for the tile's pixels;
//                            sum of rintf(t * 65536) and the pixel count per block, added to the slots' rows.  Block 0 of a frame adds
//                            the frame's own counters and writes its airlight.
// LDS of A and C: two float maps, [TH + 2 halo][TW + 2 pad] (pad = halo rounded up to whole float4s, so that a staged row begins on a
// 16-byte boundary of the frame's row) and [TH + 2 halo][TW + 2 (halo - r)]: 16.9 KB for A at r = 7, 41.8 KB for C at r = 7 with
// refine (three resident blocks per CU), 81.7 KB at r = 15 with refine (one).
#include "dehaze_tiles.h"

namespace {

// C.  grid = (tiles_x * tiles_y, B).
template <bool VEC, bool REFINE>
__global__ __launch_bounds__(kThreads)
void recover_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dz_args g, const unsigned char* __restrict__ ws,
                    const int32_t* __restrict__ cond, float* __restrict__ restored, float* __restrict__ airlight,
                    int64_t* __restrict__ stats, int n_slots)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* b0 = reinterpret_cast<float*>(lds_raw);
    float* b1 = b0 + g.rows * g.sw;
    __shared__ long long red[kWaves][2];
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const int tid = threadIdx.x;
    const dz_record* rec = reinterpret_cast<const dz_record*>(ws) + img;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const float* frame = image + img * 3 * hw;
    float* out = restored + img * 3 * hw;
    bool floored = false;
    const long long n_sel = rec->n;
    const float a0 = airlight_of(rec->sum[0], n_sel, g.a_min, floored);
    const float a1 = airlight_of(rec->sum[1], n_sel, g.a_min, floored);
    const float a2 = airlight_of(rec->sum[2], n_sel, g.a_min, floored);
    uint32_t unused = 0;
    stage<VEC, true, false>(frame, hw, H, W, y0, x0, g, a0, a1, a2, b0, unused);
    window_passes<REFINE>(H, W, y0, x0, g, b0, b1);
    long long t_q = 0, n_px = 0;
    if constexpr (VEC) {
        for (int i = tid; i < kTH * (kTW / 4); i += kThreads) {
            const int row = i / (kTW / 4), col = (i - row * (kTW / 4)) * 4;
            const int yy = y0 + row, xx = x0 + col;
            if (yy < H && xx < W) {
                const int64_t p = (int64_t)yy * W + xx;
                const float4 o = *reinterpret_cast<const float4*>(b0 + row * kTW + col);
                const float4 a = *reinterpret_cast<const float4*>(frame + p);
                const float4 b = *reinterpret_cast<const float4*>(frame + hw + p);
                const float4 c = *reinterpret_cast<const float4*>(frame + 2 * hw + p);
                const dz_pixel w0 = recover(o.x, a.x, b.x, c.x, g, a0, a1, a2, t_q), w1 = recover(o.y, a.y, b.y, c.y, g, a0, a1, a2, t_q);
                const dz_pixel w2 = recover(o.z, a.z, b.z, c.z, g, a0, a1, a2, t_q), w3 = recover(o.w, a.w, b.w, c.w, g, a0, a1, a2, t_q);
                *reinterpret_cast<float4*>(out + p) = { w0.r0, w1.r0, w2.r0, w3.r0 };
                *reinterpret_cast<float4*>(out + hw + p) = { w0.r1, w1.r1, w2.r1, w3.r1 };
                *reinterpret_cast<float4*>(out + 2 * hw + p) = { w0.r2, w1.r2, w2.r2, w3.r2 };
                n_px += 4;
            }
        }
    } else {
        for (int i = tid; i < kTH * kTW; i += kThreads) {
            const int row = i / kTW, col = i - row * kTW;
            const int yy = y0 + row, xx = x0 + col;
            if (yy < H && xx < W) {
                const int64_t p = (int64_t)yy * W + xx;
                const dz_pixel w = recover(b0[i], frame[p], frame[hw + p], frame[2 * hw + p], g, a0, a1, a2, t_q);
                out[p] = w.r0;
                out[hw + p] = w.r1;
                out[2 * hw + p] = w.r2;
                n_px += 1;
            }
        }
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
    t_q = wave_sum_i64(t_q);
    n_px = wave_sum_i64(n_px);
    if (lane == 0) { red[wave][0] = n_px; red[wave][1] = t_q; }
    __syncthreads();
    if (tid == 0) {
        long long row[kRow] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int w = 0; w < kWaves; ++w) { row[4] += red[w][0]; row[5] += red[w][1]; }
        if (blockIdx.x == 0) {                                             // the frame's own counters, once
            row[0] = 1;
            row[1] = (long long)rintf(a0 * 65536.0f);
            row[2] = (long long)rintf(a1 * 65536.0f);
            row[3] = (long long)rintf(a2 * 65536.0f);
            row[6] = rec->nonfinite;
            row[7] = floored ? 1 : 0;
            airlight[img * 3] = a0;
            airlight[img * 3 + 1] = a1;
            airlight[img * 3 + 2] = a2;
        }
        add_row(stats, n_slots, cond, img, row);
    }
}

}  // namespace

#ifndef AWSEG_RESTORE_HEADER_HASH
#define AWSEG_RESTORE_HEADER_HASH 0ULL
#endif
AWSEG_API uint64_t awseg_restore_header_hash(void) { return AWSEG_RESTORE_HEADER_HASH; }     // csrc/build.py: 60 bits of sha256(include/awseg_restore.h)

AWSEG_API int64_t awseg_dehaze_workspace(int64_t batch, int64_t height, int64_t width)
{
    if (batch < 1) batch = 1;
    if (height < 1) height = 1;
    if (width < 1) width = 1;
    return batch * ((int64_t)AWSEG_DEHAZE_FRAME_RECORD + height * width);
}

AWSEG_API int awseg_dehaze(const float* image, int64_t batch, int channels, int64_t height, int64_t width, const float* mean,
                           const float* std, int radius, float omega, float t_min, float airlight_min, int refine,
                           const int32_t* cond, float* restored, float* airlight, int64_t* stats, int n_slots, void* workspace,
                           awseg_stream_t stream)
{
    AWSEG_DEHAZE_CHECKS(true, refine == 0 || refine == 1);
    hipStream_t s = awseg_s(stream);
    const int H = (int)height, W = (int)width;
    const int tiles_x = (W + kTW - 1) / kTW, tiles = tiles_x * ((H + kTH - 1) / kTH);
    const bool vec = (W % 4 == 0) && awseg_aligned(image, 16) && awseg_aligned(restored, 16);
    unsigned char* ws = (unsigned char*)workspace;
    const int rc = estimate_airlight(image, batch, H, W, radius, g, vec, ws, s);
    if (rc != 0) return rc;
    dim3 grid((unsigned)tiles, (unsigned)batch), block(kThreads);
    geometry(radius, refine, g);
    {
        auto kern = vec ? (refine ? recover_kernel<true, true> : recover_kernel<true, false>)
                        : (refine ? recover_kernel<false, true> : recover_kernel<false, false>);
        const size_t lds = lds_bytes(g);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return AWSEG_EINVAL;
        hipLaunchKernelGGL(kern, grid, block, lds, s, image, H, W, tiles_x, g, (const unsigned char*)ws, cond, restored, airlight, stats,
                           n_slots);
        AWSEG_LAUNCH_CHECK();
    }
    return 0;
}
