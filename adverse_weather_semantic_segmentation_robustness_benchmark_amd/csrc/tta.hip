// tta.hip — the two steps between the forwards of test-time augmentation: awseg_tta_view makes a rescaled and
// mirrored view of the frames, awseg_tta_accumulate takes a view's logits back to the frame's geometry and folds them into a running
// average.  The arithmetic is the one include/awseg_restore.h states step by step (align_corners = False bilinear, one float32
// operation per step, no contraction): every output bit is what numpy float32 gives.  It is NOT awseg_upsample_bilinear's, which is
// pinned to torch's fmaf form.
//
// One streaming kernel for both, no LDS, no block waits for another.  An item is four consecutive destination pixels of one row of
// one plane; a lane takes items tid, tid + stride, ... of a grid capped by awseg_grid_1d.  The row's two source rows and weights are
// formed once per item, the columns once per pixel.
//   VEC     W % 4 == 0 and a 16-byte aligned destination: the four pixels are one 16-byte load (the modes that read the accumulator)
//           and one 16-byte store.  Otherwise scalar accesses and a ragged last group; the same bits either way.
//   EQUAL   source and destination have one size: no blend, the value itself.  With W % 4 == 0 and an aligned source the four values
//           are one 16-byte load, mirrored: the group that ends where this one's mirror image begins, its components reversed.
//   else    four gathered taps per pixel through the cache (neighbouring lanes read neighbouring columns; going up, a source value
//           is read by several pixels of the same wave).
#include "awseg_common.h"
#include "../../include/awseg_restore.h"
#include <float.h>

namespace {

constexpr int kThreads = 256;
constexpr int kView = -1;                                                  // dst = U: awseg_tta_view; the others are AWSEG_TTA_*

struct tta_args {
    int h, w, H, W;                                                        // source and destination size
    int groups;                                                            // ceil(W / 4)
    int flip_dst, flip_src;                                                // mirror the destination column (view) / the source columns (accumulate)
    int src_vec;                                                           // EQUAL: 16-byte loads of the source
    float sy, sx, weight;
    unsigned items;                                                        // planes * H * groups < 2^31
};

// One axis: position p of the destination -> the two source positions and their weights.
__device__ __forceinline__ void taps(float scale, int p, int n, int& p0, int& p1, float& l0, float& l1)
{
    const float f = fmaxf(scale * ((float)p + 0.5f) - 0.5f, 0.0f);
    p0 = min((int)f, n - 1);
    p1 = p0 + (p0 < n - 1 ? 1 : 0);
    l1 = f - (float)p0;
    l0 = 1.0f - l1;
}

// l * v, and +0 for a tap of weight zero: a non-finite neighbour that takes no part must not turn the pixel into NaN.
__device__ __forceinline__ float term(float l, float v) { return l != 0.0f ? l * v : 0.0f; }

template <int MODE>
__device__ __forceinline__ float fold(float u, float a, float weight)
{
    if constexpr (MODE == kView) return u;
    else if constexpr (MODE == AWSEG_TTA_SET) return weight * u;
    else if constexpr (MODE == AWSEG_TTA_ADD) return a + weight * u;
    else return weight * a + weight * u;
}

template <int MODE, bool VEC, bool EQUAL>
__global__ __launch_bounds__(kThreads)
void tta_kernel(const float* __restrict__ src, float* __restrict__ dst, const tta_args g)
{
    constexpr bool READS = MODE == AWSEG_TTA_ADD || MODE == AWSEG_TTA_SCALE_ADD;
    const unsigned stride = gridDim.x * kThreads;
    const int64_t src_plane = (int64_t)g.h * g.w, dst_plane = (int64_t)g.H * g.W;
    for (unsigned item = blockIdx.x * kThreads + threadIdx.x; item < g.items; item += stride) {
        const unsigned row = item / (unsigned)g.groups;                    // plane * H + y
        const int x0 = 4 * (int)(item - row * (unsigned)g.groups);
        const unsigned plane = row / (unsigned)g.H;
        const int y = (int)(row - plane * (unsigned)g.H);
        const float* s = src + plane * src_plane;
        float* d = dst + plane * dst_plane + (int64_t)y * g.W + x0;
        const int n = VEC ? 4 : min(4, g.W - x0);
        float u[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, a[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        if constexpr (READS) {
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(d);
                a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (k < n) a[k] = d[k];
            }
        }
        if constexpr (EQUAL) {
            const bool mirror = (g.flip_dst | g.flip_src) != 0;
            const float* r = s + (int64_t)y * g.w;
            if (g.src_vec) {                                               // W % 4 == 0: the mirrored group is a whole one
                const float4 t = *reinterpret_cast<const float4*>(r + (mirror ? g.w - 4 - x0 : x0));
                if (mirror) { u[0] = t.w; u[1] = t.z; u[2] = t.y; u[3] = t.x; }
                else { u[0] = t.x; u[1] = t.y; u[2] = t.z; u[3] = t.w; }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (k < n) u[k] = r[mirror ? g.w - 1 - (x0 + k) : x0 + k];
            }
        } else {
            int y0, y1;
            float ly0, ly1;
            taps(g.sy, y, g.h, y0, y1, ly0, ly1);
            const float* r0 = s + (int64_t)y0 * g.w;
            const float* r1 = s + (int64_t)y1 * g.w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= n) continue;
                const int x = x0 + k;
                int c0, c1;
                float lx0, lx1;
                taps(g.sx, g.flip_dst ? g.W - 1 - x : x, g.w, c0, c1, lx0, lx1);
                if (g.flip_src) { c0 = g.w - 1 - c0; c1 = g.w - 1 - c1; }
                const float top = term(lx0, r0[c0]) + term(lx1, r0[c1]);
                const float bot = term(lx0, r1[c0]) + term(lx1, r1[c1]);
                u[k] = term(ly0, top) + term(ly1, bot);
            }
        }
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(d) = { fold<MODE>(u[0], a[0], g.weight), fold<MODE>(u[1], a[1], g.weight),
                                              fold<MODE>(u[2], a[2], g.weight), fold<MODE>(u[3], a[3], g.weight) };
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < n) d[k] = fold<MODE>(u[k], a[k], g.weight);
        }
    }
}

template <int MODE>
int launch(const float* src, float* dst, const tta_args& g, bool vec, bool equal, hipStream_t s)
{
    auto kern = vec ? (equal ? tta_kernel<MODE, true, true> : tta_kernel<MODE, true, false>)
                    : (equal ? tta_kernel<MODE, false, true> : tta_kernel<MODE, false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)awseg_grid_1d((int64_t)g.items, kThreads)), dim3(kThreads), 0, s, src, dst, g);
    AWSEG_LAUNCH_CHECK();
    return 0;
}

// The refusals both launchers share, and the geometry.  0: go on.
int prepare(const float* src, int64_t batch, int channels, int64_t src_height, int64_t src_width, const float* dst, int64_t height,
            int64_t width, int flip, tta_args& g, bool& vec, bool& equal)
{
    if (!src || !dst || src == dst) return AWSEG_EINVAL;
    if (batch < 1 || channels < 1 || src_height < 1 || src_width < 1 || height < 1 || width < 1) return AWSEG_EINVAL;
    if (flip != 0 && flip != 1) return AWSEG_EINVAL;
    if (!awseg_aligned(src, 4) || !awseg_aligned(dst, 4)) return AWSEG_EALIGN;
    const int64_t groups = (width + 3) / 4;
    if (src_height > INT32_MAX / src_width || height > INT32_MAX / width) return AWSEG_ERANGE;        // a plane of 2^31 pixels
    if (batch > INT32_MAX / channels || batch * channels > (int64_t)INT32_MAX / (height * groups)) return AWSEG_ERANGE;
    g.h = (int)src_height; g.w = (int)src_width; g.H = (int)height; g.W = (int)width;
    g.groups = (int)groups;
    g.items = (unsigned)(batch * channels * height * groups);
    g.sy = (float)src_height / (float)height;
    g.sx = (float)src_width / (float)width;
    equal = src_height == height && src_width == width;
    vec = width % 4 == 0 && awseg_aligned(dst, 16);
    g.src_vec = equal && width % 4 == 0 && awseg_aligned(src, 16) ? 1 : 0;
    return 0;
}

}  // namespace

AWSEG_API int awseg_tta_view(const float* src, int64_t batch, int channels, int64_t src_height, int64_t src_width, float* dst,
                             int64_t height, int64_t width, int flip, awseg_stream_t stream)
{
    tta_args g = {};
    bool vec = false, equal = false;
    if (channels > AWSEG_TTA_VIEW_MAX_CHANNELS) return AWSEG_EINVAL;
    const int rc = prepare(src, batch, channels, src_height, src_width, dst, height, width, flip, g, vec, equal);
    if (rc) return rc;
    g.flip_dst = flip;
    g.weight = 1.0f;
    return launch<kView>(src, dst, g, vec, equal, awseg_s(stream));
}

AWSEG_API int awseg_tta_accumulate(const float* src, int64_t batch, int channels, int64_t src_height, int64_t src_width, float* acc,
                                   int64_t height, int64_t width, int flip, float weight, int mode, awseg_stream_t stream)
{
    tta_args g = {};
    bool vec = false, equal = false;
    if (mode != AWSEG_TTA_SET && mode != AWSEG_TTA_ADD && mode != AWSEG_TTA_SCALE_ADD) return AWSEG_EINVAL;
    if (!(weight >= -FLT_MAX && weight <= FLT_MAX)) return AWSEG_EINVAL;
    const int rc = prepare(src, batch, channels, src_height, src_width, acc, height, width, flip, g, vec, equal);
    if (rc) return rc;
    g.flip_src = flip;
    g.weight = weight;
    hipStream_t s = awseg_s(stream);
    if (mode == AWSEG_TTA_SET) return launch<AWSEG_TTA_SET>(src, acc, g, vec, equal, s);
    if (mode == AWSEG_TTA_ADD) return launch<AWSEG_TTA_ADD>(src, acc, g, vec, equal, s);
    return launch<AWSEG_TTA_SCALE_ADD>(src, acc, g, vec, equal, s);
}
