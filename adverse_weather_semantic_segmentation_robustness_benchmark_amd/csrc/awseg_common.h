// awseg_common.h — shared device/host helpers for libawseg_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <type_traits>
#include "../../include/awseg.h"

#define AWSEG_API extern "C" __attribute__((visibility("default")))

#define AWSEG_WAVE 64
#define AWSEG_CUS 256

// Launch check: kernels are enqueued asynchronously, so only launch-time errors surface here.
#define AWSEG_LAUNCH_CHECK()                                  \
    do {                                                      \
        hipError_t e__ = hipGetLastError();                   \
        if (e__ != hipSuccess) return (int)e__;               \
    } while (0)

static inline hipStream_t awseg_s(awseg_stream_t s) { return (hipStream_t)s; }

// CU count of the CURRENT device (a process may drive several): asked once per ordinal, AWSEG_CUS where the runtime cannot say.
inline int awseg_cu_count()
{
    static std::atomic<int> cached[16];                       // zero-initialised; ordinals past the array ask every time
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AWSEG_CUS;
    const bool slot = dev >= 0 && dev < 16;
    if (slot && (n_cu = cached[dev].load(std::memory_order_relaxed)) > 0) return n_cu;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu < 1) return AWSEG_CUS;
    if (slot) cached[dev].store(n_cu, std::memory_order_relaxed);
    return n_cu;
}

// p is aligned to `bytes` (a power of two): the test every vector-load path makes of its bases
static inline bool awseg_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// Memory-bound grids: cap at 8 resident 256-thread blocks per CU and grid-stride the rest
// (cdna_hip_programming.md Guideline 11).
static inline int awseg_grid_1d(int64_t work_items, int per_block, int max_blocks = AWSEG_CUS * 8)
{
    int64_t b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

// 64-lane wavefront reductions (shuffle tree, no LDS).
__device__ __forceinline__ double awseg_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ float awseg_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ float awseg_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t awseg_wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// label load for the two dtypes the reference produces (uint8 from the loader, int64 in its tests)
template <int DT> __device__ __forceinline__ int64_t awseg_ld_label(const void* p, int64_t i)
{
    if (DT == AWSEG_U8) return (int64_t)((const uint8_t*)p)[i];
    return ((const int64_t*)p)[i];
}

// torch's argmax update rule (metrics.hip's combine and one-pass statistics kernels; their prediction maps are what
// consistency.hip compares): take v when v > best, or v is NaN and best is not.
__device__ __forceinline__ void awseg_amax_step(float v, int c, float& best, int& bi)
{
    if (!(v <= best) && !(best != best)) { best = v; bi = c; }
}

// erf to 1.5e-7 absolute (Abramowitz & Stegun 7.1.26: 1 - (a1 t + ... + a5 t^5) exp(-x^2), t = 1 / (1 + p |x|)) with the hardware
// reciprocal and exp2: 14 vector instructions, two of them transcendental.  The library erff is ~40 (two range branches, both
// evaluated and selected): the depthwise 3x3 + GELU kernel of backbone.hip spent 160 of its ~200 instructions per output quad
// there and was bound by them, not by memory.  GELU error <= 0.5 |x| x 3e-7: two orders inside the 1e-4 gate
// (AWSEG_GELU_EXACT=1: erff).  backbone.hip and the Mix-FFN tile kernel of mixffn.hip.
__device__ __forceinline__ float awseg_erf_as(float x)
{
    const float ax = __builtin_fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    p = p * t;
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * ax * ax);
    const float r = fmaf(-p, e, 1.0f);
    return __builtin_copysignf(r, x);
}
// torch GELU (erf form) on the fast erf
__device__ __forceinline__ float awseg_gelu(float v) { return 0.5f * v * (1.0f + awseg_erf_as(v * 0.70710678118654752440f)); }

// Border indices of the stencil kernels (weather.hip, depth.hip): scipy 'reflect' (d c b a | a b c d | d c b a) ...
__device__ __forceinline__ int awseg_reflect_sym(int i, int n)
{
    if (n == 1) return 0;
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}
// ... and OpenCV BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) at any offset (cv::borderInterpolate)
__device__ __forceinline__ int awseg_reflect_101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// ECE confidence sums in FIXED POINT, units of 2^-30 (metrics.hip, calib.hip): a float32 confidence in [2^-7, 1] is a multiple
// of 2^-30, so conf * 2^30 is an exact integer and integer sums do not depend on the order of the atomics.
__device__ __forceinline__ unsigned long long awseg_conf_q30(float conf) { return (unsigned long long)(conf * 1073741824.0f); }

// Bin of a confidence on the reference's float32 linspace, bins (lo, hi] (metrics.py:179-188): the uniform-grid guess is
// checked against the staged edges with the reference's own comparisons and moved by one where rounding put it next door;
// anything else (edges that are not a uniform grid) falls back to the linear scan.  -1 = in no bin.
__device__ __forceinline__ int awseg_ece_find_bin(float conf, const float* s_edges, int n_bins)
{
    int b = (int)ceilf(conf * (float)n_bins) - 1;
    b = b < 0 ? 0 : (b > n_bins - 1 ? n_bins - 1 : b);
    if (!(conf > s_edges[b])) b = b > 0 ? b - 1 : 0;
    else if (!(conf <= s_edges[b + 1])) b = b < n_bins - 1 ? b + 1 : b;
    if (conf > s_edges[b] && conf <= s_edges[b + 1]) return b;
    for (int k = 0; k < n_bins; ++k)
        if (conf > s_edges[k] && conf <= s_edges[k + 1]) return k;
    return -1;
}

// Blocks per image of a grid (blocks_per_image, batch): enough for `lane_items` items at one per thread, at most
// resident_per_cu resident blocks on each of 256 CUs over the whole batch (the kernels stride beyond), at least one.
// A launch and its workspace query call this with the same arguments.
inline int awseg_blocks_per_image(int64_t lane_items, int threads, int64_t batch, int resident_per_cu)
{
    int64_t want = (lane_items + threads - 1) / threads;
    int64_t cap = (AWSEG_CUS * resident_per_cu + batch - 1) / batch;
    if (cap < 1) cap = 1;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    return (int)want;
}

// Template arguments from run-time values: f(std::integral_constant<int, AWSEG_U8 or AWSEG_I64>), f(std::bool_constant<flag>),
// f(std::integral_constant<int, 0 or 2>) for AWSEG_COMBINE_WEIGHTED / AWSEG_COMBINE_MEAN (the kernels' MODE; the callers have
// refused every other mode); the callee reads decltype(arg)::value.  Each returns what f returns.
template <typename F> inline auto awseg_by_label(int label_dtype, F&& f)
{
    if (label_dtype == AWSEG_U8) return f(std::integral_constant<int, AWSEG_U8>());
    return f(std::integral_constant<int, AWSEG_I64>());
}
template <typename F> inline auto awseg_by_flag(bool flag, F&& f)
{
    if (flag) return f(std::true_type());
    return f(std::false_type());
}
template <typename F> inline auto awseg_by_combine_mode(int mode, F&& f)
{
    if (mode == AWSEG_COMBINE_WEIGHTED) return f(std::integral_constant<int, 0>());
    return f(std::integral_constant<int, 2>());
}

// Philox4x32-7 counter-based generator (Salmon et al., Random123: 7 rounds pass BigCrush) for the
// throughput-mode noise; parity mode takes host draws instead.  One call = four uint32.
struct awseg_philox {
    __device__ __forceinline__ static void gen(uint64_t seed, uint64_t ctr, uint32_t stream, uint32_t out[4])
    {
        const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
        uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = stream, c3 = 0x9E3779B9u;
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
            uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
            uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
            c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    }
};
// two uint32 -> one N(0,1) pair (Box-Muller in float32 on the hardware transcendental units:
// v_log_f32 is log2, v_sin/v_cos take their argument in revolutions).  Distribution-only parity.
__device__ __forceinline__ void awseg_box_muller(uint32_t a, uint32_t b, float& n0, float& n1)
{
    float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);
    float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    float r = __builtin_amdgcn_sqrtf(-1.38629436111989061883f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1), ln = log2 * ln2
    n0 = r * __builtin_amdgcn_cosf(u2);
    n1 = r * __builtin_amdgcn_sinf(u2);
}
// One uint32 -> one N(0,1) pair from its two 16-bit halves.  The noise these feed is quantised to
// 8 bits at sigma <= 1 LSB (night) or smoothed by a 17x17 Gaussian (fog depth), so 16-bit uniforms
// (tails truncated at 4.7 sigma) are ample and halve the Philox calls per pixel.
__device__ __forceinline__ void awseg_box_muller16(uint32_t a, float& n0, float& n1)
{
    float u1 = ((float)(a & 0xFFFFu) + 0.5f) * (1.0f / 65536.0f);
    float u2 = (float)(a >> 16) * (1.0f / 65536.0f);
    float r = __builtin_amdgcn_sqrtf(-1.38629436111989061883f * __builtin_amdgcn_logf(u1));
    n0 = r * __builtin_amdgcn_cosf(u2);
    n1 = r * __builtin_amdgcn_sinf(u2);
}
__device__ __forceinline__ float awseg_u01(uint32_t a) { return (float)(a >> 8) * (1.0f / 16777216.0f); }

// gemm_split3.hip (the LDS-DMA split-operand GEMM), called from gemm_split.hip
int awseg_gemm_split3_weights(const float* w, int n, int k, uint16_t* w3, const unsigned* trailer, hipStream_t stream);
bool awseg_gemm_split3_eligible(int64_t m, int n, int k, const void* x, const void* out, const void* residual, const void* bias);
// dual: the A operand continues in a second source behind column k1 (gemm_split3.hip g3_args: x2, K1, x2H, x2W, x2s, x2Ho, x2Wo)
struct awseg_g3_dual { const float* x2; int k1; int h, w, stride, ho, wo; int64_t bytes; const float* x3 = nullptr; const float* x4 = nullptr; };   // bytes: of ONE piece
int awseg_gemm_split3_launch(const float* x, const uint16_t* w3, const unsigned* trailer, const float* bias, const float* residual,
                             int act, float* out, int64_t m, int n, int k, int cus, hipStream_t stream, const int* conv = nullptr,
                             bool bf16 = false, const awseg_g3_dual* dual = nullptr);
int awseg_gemm_split3_bn(int n);
int64_t awseg_gemm_split3_image_rows(int n);
int awseg_gemm_bf16_3_weights(const float* w, int n, int k, uint16_t* w3, hipStream_t stream);
