// dehaze_guided.hip — dark-channel dehazing with the guided-filter refinement of the transmission (He, Sun, Tang 2010/2013;
// DESIGN.md §10n-bis), the arithmetic include/awseg_restore.h states step by step: every output bit is what numpy float32 gives,
// the order of the box sums' additions included.
//
// awseg_dehaze_guided: five kernels on the caller's stream, no host synchronisation, no block waits for another.
//   A, B  dark_channel_kernel, airlight_kernel of dehaze_tiles.h, as awseg_dehaze launches them.
//   P  patch_kernel          pass C's staging and (2r+1)^2 minimum of n = min_c v_c / A_c; stores p = 1 - omega * e to the workspace.
//   Q  coefficient_kernel    a block owns kTH x kTW pixels, stages the guide g (recomputed from the frame) and p with a halo of R, +0.0f
//                            outside the frame, and forms S(g), S(p), S(g g), S(g p) one after another through one row-sum buffer:
//                            a row pass (every staged row, the tile's columns) and a column pass (the tile's pixels).  Then a, b to
//                            the workspace.
//   T  transmission_kernel   stages a and b the same way, forms M(a), M(b), q = M(a) g + M(b), t, J, the outputs and the counters.
// A thread of Q and T owns four adjacent columns: in the row pass it walks its 2R + 4 staged values once (16-byte LDS reads), each
// value joining the up to four running sums whose window holds it — every sum still adds its own 2R + 1 terms left to right; in the
// column pass it reads one 16-byte group of row sums per window row.
// LDS of Q and T: two float maps [kTH + 2R][sw], sw = kTW + 2R rounded up to whole float4s, and the row sums [kTH + 2R][kTW]:
// 104.5 KB at R = 28, 120 KB at R = 32 (one resident block of 512 threads per CU), 42 KB at R = 8 (three).
#include "dehaze_tiles.h"

namespace {

constexpr int kGThreads = 512;                                             // Q and T: one thread per four adjacent pixels of the tile
constexpr int kGWaves = kGThreads / AWSEG_WAVE;
constexpr int kGroups = kTW / 4;                                           // float4 groups per tile row
constexpr int kGRow = AWSEG_GUIDED_ROW;
static_assert(kGThreads == kTH * kGroups, "one thread per float4 group of the tile");

struct gf_args {
    int R, rows, sw;                                                       // staged rows kTH + 2R; staged columns, whole float4s
    float eps;
};

void guided_geometry(int R, float eps, gf_args& f)
{
    f.R = R;
    f.rows = kTH + 2 * R;
    f.sw = (kTW + 2 * R + 3) & ~3;
    f.eps = eps;
}
size_t guided_lds_bytes(const gf_args& f) { return (size_t)f.rows * (2 * f.sw + kTW) * sizeof(float); }

__device__ __forceinline__ float guide_of(float x0, float x1, float x2, const dz_args& g)
{
    const float v0 = unit(x0, g.std[0], g.mean[0]), v1 = unit(x1, g.std[1], g.mean[1]), v2 = unit(x2, g.std[2], g.mean[2]);
    return (0.299f * v0 + 0.587f * v1) + 0.114f * v2;
}

// P.  grid = (tiles_x * tiles_y, B).  pmap [B][H*W].
template <bool VEC>
__global__ __launch_bounds__(kThreads)
void patch_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dz_args g, const unsigned char* __restrict__ ws,
                  float* __restrict__ pmap)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* b0 = reinterpret_cast<float*>(lds_raw);
    float* b1 = b0 + g.rows * g.sw;
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const int tid = threadIdx.x;
    const dz_record* rec = reinterpret_cast<const dz_record*>(ws) + img;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    bool floored = false;
    const long long n_sel = rec->n;
    const float a0 = airlight_of(rec->sum[0], n_sel, g.a_min, floored);
    const float a1 = airlight_of(rec->sum[1], n_sel, g.a_min, floored);
    const float a2 = airlight_of(rec->sum[2], n_sel, g.a_min, floored);
    uint32_t unused = 0;
    stage<VEC, true, false>(image + img * 3 * hw, hw, H, W, y0, x0, g, a0, a1, a2, b0, unused);
    window_passes<false>(H, W, y0, x0, g, b0, b1);
    float* out = pmap + img * hw;
    for (int i = tid; i < kTH * kTW; i += kThreads) {
        const int row = i / kTW, col = i - row * kTW;
        const int yy = y0 + row, xx = x0 + col;
        if (yy < H && xx < W) out[(int64_t)yy * W + xx] = 1.0f - g.omega * b0[i];
    }
}

// What the box sum adds at a staged position: the first map, the second, the first squared, or their product.
enum { kFirst = 0, kSecond = 1, kSquare = 2, kProduct = 3 };

template <int WHAT>
__device__ __forceinline__ float4 terms(const float* __restrict__ m0, const float* __restrict__ m1, int at)
{
    float4 u = {}, v = {};
    if constexpr (WHAT != kSecond) u = *reinterpret_cast<const float4*>(m0 + at);
    if constexpr (WHAT == kSecond || WHAT == kProduct) v = *reinterpret_cast<const float4*>(m1 + at);
    if constexpr (WHAT == kFirst) return u;
    if constexpr (WHAT == kSecond) return v;
    if constexpr (WHAT == kSquare) return { u.x * u.x, u.y * u.y, u.z * u.z, u.w * u.w };
    return { u.x * v.x, u.y * v.y, u.z * v.z, u.w * v.w };
}

// Sum m of the four (k - m = 0: it begins with this value; 0 < k - m <= 2R: it adds it; otherwise the value is outside its window).
__device__ __forceinline__ void join(float (&acc)[4], float v, int k, int taps)
{
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int d = k - m;
        if (d == 0) acc[m] = v;
        else if (d > 0 && d <= taps) acc[m] = acc[m] + v;
    }
}

// S(x) at the thread's four pixels (tile row tid / kGroups, columns 4 (tid % kGroups) ..+3), x chosen by WHAT from the staged maps
// m0, m1 [f.rows][f.sw] (column 0 is pixel x0 - R).  hs [f.rows][kTW] takes the row sums.  Begins and ends with a barrier.
template <int WHAT>
__device__ __forceinline__ float4 box_sum(const float* __restrict__ m0, const float* __restrict__ m1, float* __restrict__ hs, const gf_args& f)
{
    const int tid = threadIdx.x, taps = 2 * f.R;
    const int chunks = (taps + 4 + 3) / 4;                                 // a thread's 2R + 4 staged values, in float4s
    __syncthreads();
    for (int i = tid; i < f.rows * kGroups; i += kGThreads) {
        const int row = i / kGroups, j = (i - row * kGroups) * 4;
        const int at = row * f.sw + j;
        float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int c = 0; c < chunks; ++c) {
            const float4 v = terms<WHAT>(m0, m1, at + 4 * c);
            const int k = 4 * c;
            if (c >= 1 && k + 3 <= taps) {                                 // every one of the four windows holds all four values
                acc[0] = acc[0] + v.x; acc[1] = acc[1] + v.x; acc[2] = acc[2] + v.x; acc[3] = acc[3] + v.x;
                acc[0] = acc[0] + v.y; acc[1] = acc[1] + v.y; acc[2] = acc[2] + v.y; acc[3] = acc[3] + v.y;
                acc[0] = acc[0] + v.z; acc[1] = acc[1] + v.z; acc[2] = acc[2] + v.z; acc[3] = acc[3] + v.z;
                acc[0] = acc[0] + v.w; acc[1] = acc[1] + v.w; acc[2] = acc[2] + v.w; acc[3] = acc[3] + v.w;
            } else {
                join(acc, v.x, k, taps); join(acc, v.y, k + 1, taps); join(acc, v.z, k + 2, taps); join(acc, v.w, k + 3, taps);
            }
        }
        *reinterpret_cast<float4*>(hs + row * kTW + j) = { acc[0], acc[1], acc[2], acc[3] };
    }
    __syncthreads();
    const float* p = hs + (tid / kGroups) * kTW + (tid % kGroups) * 4;    // window row 0 of tile row tid / kGroups is staged row the same
    float4 s = *reinterpret_cast<const float4*>(p);
    for (int k = 1; k <= taps; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(p + k * kTW);
        s.x = s.x + v.x; s.y = s.y + v.y; s.z = s.z + v.z; s.w = s.w + v.w;
    }
    __syncthreads();
    return s;
}

// The positions of the (2R+1)-window around `at` that lie in [0, size).
__device__ __forceinline__ int in_frame(int at, int R, int size) { return min(at + R, size - 1) - max(at - R, 0) + 1; }

__device__ __forceinline__ float4 window_counts(int yy, int xx, int R, int H, int W)
{
    const int ny = in_frame(yy, R, H);
    return { (float)(ny * in_frame(xx, R, W)), (float)(ny * in_frame(xx + 1, R, W)), (float)(ny * in_frame(xx + 2, R, W)),
             (float)(ny * in_frame(xx + 3, R, W)) };                       // columns >= W: counts nobody uses
}

__device__ __forceinline__ float4 quotient(float4 s, float4 n) { return { s.x / n.x, s.y / n.y, s.z / n.z, s.w / n.w }; }

// Q.  grid = (tiles_x * tiles_y, B), kGThreads.  pmap, amap, bmap [B][H*W].
__global__ __launch_bounds__(kGThreads)
void coefficient_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dz_args g, const gf_args f,
                        const float* __restrict__ pmap, float* __restrict__ amap, float* __restrict__ bmap)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* mg_ = reinterpret_cast<float*>(lds_raw);                        // the guide   [rows][sw]
    float* mp_ = mg_ + f.rows * f.sw;                                      // p           [rows][sw]
    float* hs = mp_ + f.rows * f.sw;                                       // row sums    [rows][kTW]
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const float* frame = image + img * 3 * hw;
    const float* pin = pmap + img * hw;
    for (int i = tid; i < f.rows * f.sw; i += kGThreads) {
        const int row = i / f.sw, col = i - row * f.sw;
        const int yy = y0 - f.R + row, xx = x0 - f.R + col;
        float gv = 0.0f, pv = 0.0f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const int64_t at = (int64_t)yy * W + xx;
            gv = guide_of(frame[at], frame[hw + at], frame[2 * hw + at], g);
            pv = pin[at];
        }
        mg_[i] = gv;
        mp_[i] = pv;
    }
    const float4 sg = box_sum<kFirst>(mg_, mp_, hs, f);
    const float4 sp = box_sum<kSecond>(mg_, mp_, hs, f);
    const float4 sgg = box_sum<kSquare>(mg_, mp_, hs, f);
    const float4 sgp = box_sum<kProduct>(mg_, mp_, hs, f);
    const int row = tid / kGroups, col = (tid % kGroups) * 4;
    const int yy = y0 + row, xx = x0 + col;
    if (yy >= H || xx >= W) return;
    const float4 n = window_counts(yy, xx, f.R, H, W);
    const float4 mg = quotient(sg, n), mp = quotient(sp, n), mgg = quotient(sgg, n), mgp = quotient(sgp, n);
    const float mgs[4] = { mg.x, mg.y, mg.z, mg.w }, mps[4] = { mp.x, mp.y, mp.z, mp.w };
    const float mggs[4] = { mgg.x, mgg.y, mgg.z, mgg.w }, mgps[4] = { mgp.x, mgp.y, mgp.z, mgp.w };
    const int64_t at = img * hw + (int64_t)yy * W + xx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (xx + k >= W) break;
        const float var = mggs[k] - mgs[k] * mgs[k];
        const float cov = mgps[k] - mgs[k] * mps[k];
        const float a = cov / (var + f.eps);
        amap[at + k] = a;
        bmap[at + k] = mps[k] - a * mgs[k];
    }
}

// T.  grid = (tiles_x * tiles_y, B), kGThreads.
template <bool VEC>
__global__ __launch_bounds__(kGThreads)
void transmission_kernel(const float* __restrict__ image, int H, int W, int tiles_x, const dz_args g, const gf_args f,
                         const unsigned char* __restrict__ ws, const float* __restrict__ pmap, const float* __restrict__ amap,
                         const float* __restrict__ bmap, const int32_t* __restrict__ cond, float* __restrict__ restored,
                         float* __restrict__ airlight, float* __restrict__ transmission, int64_t* __restrict__ stats,
                         int64_t* __restrict__ guided_stats, int n_slots)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* ma_ = reinterpret_cast<float*>(lds_raw);                        // a           [rows][sw]
    float* mb_ = ma_ + f.rows * f.sw;                                      // b           [rows][sw]
    float* hs = mb_ + f.rows * f.sw;                                       // row sums    [rows][kTW]
    __shared__ long long red[kGWaves][5];
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
    {
        const float* ain = amap + img * hw;
        const float* bin = bmap + img * hw;
        for (int i = tid; i < f.rows * f.sw; i += kGThreads) {
            const int row = i / f.sw, col = i - row * f.sw;
            const int yy = y0 - f.R + row, xx = x0 - f.R + col;
            float av = 0.0f, bv = 0.0f;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const int64_t at = (int64_t)yy * W + xx;
                av = ain[at];
                bv = bin[at];
            }
            ma_[i] = av;
            mb_[i] = bv;
        }
    }
    const float4 sa = box_sum<kFirst>(ma_, mb_, hs, f);
    const float4 sb = box_sum<kSecond>(ma_, mb_, hs, f);
    const int row = tid / kGroups, col = (tid % kGroups) * 4;
    const int yy = y0 + row, xx = x0 + col;
    long long t_q = 0, n_px = 0, over = 0, under = 0, moved = 0;
    if (yy < H && xx < W) {
        const float4 n = window_counts(yy, xx, f.R, H, W);
        const float4 ma4 = quotient(sa, n), mb4 = quotient(sb, n);
        const float ma[4] = { ma4.x, ma4.y, ma4.z, ma4.w }, mb[4] = { mb4.x, mb4.y, mb4.z, mb4.w };
        const int64_t at = (int64_t)yy * W + xx;
        const float* pin = pmap + img * hw + at;
        float x[3][4], tt[4];
        dz_pixel w[4];
        const int live = VEC ? 4 : min(4, W - xx);                         // VEC: W % 4 == 0, a group is inside or outside
        if constexpr (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(frame + c * hw + at);
                x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) x[c][k] = k < live ? frame[c * hw + at + k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tt[k] = 0.0f;
            w[k] = { 0.0f, 0.0f, 0.0f };
            if (k >= live) continue;
            const float gv = guide_of(x[0][k], x[1][k], x[2][k], g);
            const float q = ma[k] * gv + mb[k];
            const float t = fmaxf(fminf(q, 1.0f), g.t_min);
            over += q > 1.0f ? 1 : 0;
            under += q < g.t_min ? 1 : 0;
            moved += (long long)rintf(fabsf(t - fmaxf(pin[k], g.t_min)) * 65536.0f);
            n_px += 1;
            tt[k] = t;
            w[k] = recover_at(t, x[0][k], x[1][k], x[2][k], g, a0, a1, a2, t_q);
        }
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(out + at) = { w[0].r0, w[1].r0, w[2].r0, w[3].r0 };
            *reinterpret_cast<float4*>(out + hw + at) = { w[0].r1, w[1].r1, w[2].r1, w[3].r1 };
            *reinterpret_cast<float4*>(out + 2 * hw + at) = { w[0].r2, w[1].r2, w[2].r2, w[3].r2 };
            if (transmission) *reinterpret_cast<float4*>(transmission + img * hw + at) = { tt[0], tt[1], tt[2], tt[3] };
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= live) continue;
                out[at + k] = w[k].r0;
                out[hw + at + k] = w[k].r1;
                out[2 * hw + at + k] = w[k].r2;
                if (transmission) transmission[img * hw + at + k] = tt[k];
            }
        }
    }
    const int lane = tid & (AWSEG_WAVE - 1), wave = tid / AWSEG_WAVE;
    t_q = wave_sum_i64(t_q); n_px = wave_sum_i64(n_px); over = wave_sum_i64(over); under = wave_sum_i64(under); moved = wave_sum_i64(moved);
    if (lane == 0) { red[wave][0] = n_px; red[wave][1] = t_q; red[wave][2] = over; red[wave][3] = under; red[wave][4] = moved; }
    __syncthreads();
    if (tid == 0) {
        long long row_d[kRow] = { 0, 0, 0, 0, 0, 0, 0, 0 }, row_g[kGRow] = { 0, 0, 0, 0 };
        for (int v = 0; v < kGWaves; ++v) {
            row_d[4] += red[v][0]; row_d[5] += red[v][1];
            row_g[0] += red[v][2]; row_g[1] += red[v][3]; row_g[2] += red[v][4]; row_g[3] += red[v][0];
        }
        if (blockIdx.x == 0) {                                             // the frame's own counters, once
            row_d[0] = 1;
            row_d[1] = (long long)rintf(a0 * 65536.0f);
            row_d[2] = (long long)rintf(a1 * 65536.0f);
            row_d[3] = (long long)rintf(a2 * 65536.0f);
            row_d[6] = rec->nonfinite;
            row_d[7] = floored ? 1 : 0;
            airlight[img * 3] = a0;
            airlight[img * 3 + 1] = a1;
            airlight[img * 3 + 2] = a2;
        }
        const int slot = slot_of(n_slots, cond, img);                      // one read of cond for both rows
        add_row(stats, slot, row_d);
        add_row(guided_stats, slot, row_g);
    }
}

int64_t ceil8(int64_t x) { return (x + 7) & ~(int64_t)7; }

}  // namespace

AWSEG_API int64_t awseg_dehaze_guided_workspace(int64_t batch, int64_t height, int64_t width)
{
    if (batch < 1) batch = 1;
    if (height < 1) height = 1;
    if (width < 1) width = 1;
    return ceil8(batch * ((int64_t)AWSEG_DEHAZE_FRAME_RECORD + height * width)) + 3 * ceil8(4 * batch * height * width);
}

AWSEG_API int awseg_dehaze_guided(const float* image, int64_t batch, int channels, int64_t height, int64_t width, const float* mean,
                                  const float* std, int radius, float omega, float t_min, float airlight_min, int guided_radius,
                                  float guided_eps, const int32_t* cond, float* restored, float* airlight, float* transmission,
                                  int64_t* stats, int64_t* guided_stats, int n_slots, void* workspace, awseg_stream_t stream)
{
    AWSEG_DEHAZE_CHECKS(guided_stats != nullptr, guided_radius >= 1 && guided_radius <= AWSEG_GUIDED_MAX_RADIUS
                                                     && guided_eps >= 1e-4f && guided_eps <= 1.0f);      // NaN fails
    hipStream_t s = awseg_s(stream);
    const int H = (int)height, W = (int)width;
    const int64_t hw = height * width;
    const int tiles_x = (W + kTW - 1) / kTW, tiles = tiles_x * ((H + kTH - 1) / kTH);
    const bool vec = (W % 4 == 0) && awseg_aligned(image, 16) && awseg_aligned(restored, 16)
                     && (!transmission || awseg_aligned(transmission, 16));
    unsigned char* ws = (unsigned char*)workspace;
    const int64_t map_bytes = ceil8(4 * batch * hw);
    float* pmap = reinterpret_cast<float*>(ws + ceil8(batch * ((int64_t)AWSEG_DEHAZE_FRAME_RECORD + hw)));
    float* amap = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(pmap) + map_bytes);
    float* bmap = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(amap) + map_bytes);
    const int rc = estimate_airlight(image, batch, H, W, radius, g, vec, ws, s);
    if (rc != 0) return rc;
    dim3 grid((unsigned)tiles, (unsigned)batch);
    {
        auto kern = vec ? patch_kernel<true> : patch_kernel<false>;
        const size_t lds = lds_bytes(g);                                       // geometry(radius, 0): what estimate_airlight left
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return AWSEG_EINVAL;
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, s, image, H, W, tiles_x, g, (const unsigned char*)ws, pmap);
        AWSEG_LAUNCH_CHECK();
    }
    gf_args f = {};
    guided_geometry(guided_radius, guided_eps, f);
    const size_t lds = guided_lds_bytes(f);
    {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(coefficient_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
            != hipSuccess)
            return AWSEG_EINVAL;
        hipLaunchKernelGGL(coefficient_kernel, grid, dim3(kGThreads), lds, s, image, H, W, tiles_x, g, f, (const float*)pmap, amap, bmap);
        AWSEG_LAUNCH_CHECK();
    }
    {
        auto kern = vec ? transmission_kernel<true> : transmission_kernel<false>;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return AWSEG_EINVAL;
        hipLaunchKernelGGL(kern, grid, dim3(kGThreads), lds, s, image, H, W, tiles_x, g, f, (const unsigned char*)ws, (const float*)pmap,
                           (const float*)amap, (const float*)bmap, cond, restored, airlight, transmission, stats, guided_stats, n_slots);
        AWSEG_LAUNCH_CHECK();
    }
    return 0;
}
