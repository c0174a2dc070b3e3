// boundary.hip — boundary-band segmentation counters (trimap mIoU / Boundary IoU per condition slot): for every
// labelled pixel the ring of its edge distance in the label map and in the prediction map (include/awseg.h gives the definitions),
// histogrammed into conf / inter / pr per (slot, ring).
//
// "Some valid pixel within Chebyshev distance d holds another class" is a test on the SET of classes in the (2d+1)^2 window, and a
// set of classes <= 32 is one uint32: a pixel becomes 1 << class (0 when it is invalid or outside the frame: neutral for OR), the
// window set is a separable OR, and e(p) <= d  <=>  window & ~(1 << M(p)) != 0.  (The window min / max of the header's equivalent
// form are the lowest and the highest bit of that word.)
//
// A block stages a 32 x 64 tile of one map plus a halo of the widest band as such words into LDS, and for each width d_k runs the
// two 1-D passes through `window8`: a lane owns 8 consecutive outputs of a line and reads the 8 + 2d inputs once (the part common
// to all 8 windows is ORed once, the rest are a suffix and a prefix OR), instead of 8 (2d + 1).  The row pass walks lanes down the
// rows (odd row pitch: no bank conflict), the column pass across the columns.  The hit count over the widths is the ring (the
// windows are nested).  The label map and the prediction map go through the same LDS one after the other; their rings stay in
// registers.  Then each lane merges its 8 vertically adjacent pixels into runs of equal (rings, classes) before the per-block LDS
// histogram; the block's partials and their fold into the int64 slots are the map scan's (awseg_mapscan.h):
// integer sums only, so the counts do not depend on grid shape, batch split or rank count.
#include "awseg_mapscan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kResident = 4;                                              // blocks per CU the grid is capped at
constexpr int kTH = 32, kTW = 64;                                         // tile; kThreads lanes x 8 rows
constexpr int kPer = 8;                                                   // outputs per lane per window8
constexpr int kHP = kTW + 1;                                              // row pitch of the row-pass result (odd)

struct Widths { int d[AWSEG_BOUNDARY_MAX_WIDTHS]; int n; };

// out[o] = OR of p[(o + i) * stride] over i in [-d, d], o = 0 .. 7.
__device__ __forceinline__ void window8(const uint32_t* p, int stride, int d, uint32_t (&out)[kPer])
{
    if (d == 1) {
        uint32_t r[kPer + 2];
#pragma unroll
        for (int i = 0; i < kPer + 2; ++i) r[i] = p[(i - 1) * stride];
#pragma unroll
        for (int o = 0; o < kPer; ++o) out[o] = r[o] | r[o + 1] | r[o + 2];
    } else if (d == 2) {
        uint32_t r[kPer + 4];
#pragma unroll
        for (int i = 0; i < kPer + 4; ++i) r[i] = p[(i - 2) * stride];
#pragma unroll
        for (int o = 0; o < kPer; ++o) out[o] = r[o] | r[o + 1] | r[o + 2] | r[o + 3] | r[o + 4];
    } else {                                                              // d >= 3: every window holds [7 - d, d] (empty at d = 3)
        uint32_t core = 0;
        for (int i = kPer - 1 - d; i <= d; ++i) core |= p[i * stride];
        uint32_t acc = 0;
        out[kPer - 1] = core;
#pragma unroll
        for (int o = kPer - 2; o >= 0; --o) { acc |= p[(o - d) * stride]; out[o] = core | acc; }       // [o - d, 6 - d]
        acc = 0;
#pragma unroll
        for (int o = 1; o < kPer; ++o) { acc |= p[(o + d) * stride]; out[o] |= acc; }                   // [d + 1, o + d]
    }
}

// grid = (blocks_per_image, B); block x of image y walks tiles x, x + gridDim.x, ... and writes
// partial[(y * gridDim.x + x)][(n + 1) * (C * C + 2 C)].  Dynamic LDS: staged | row-pass result | histogram.
template <int LDT>
__global__ __launch_bounds__(kThreads)
void boundary_kernel(const uint8_t* __restrict__ pred, const void* __restrict__ label, int ignore_index, int H, int W, int C,
                     const Widths wd, int tiles_x, int tiles, uint32_t* __restrict__ partial, int64_t* __restrict__ oob)
{
    extern __shared__ uint32_t smem[];
    const int n = wd.n, R = wd.d[n - 1];
    const int SR = kTH + 2 * R, SP = kTW + 2 * R + 1;                     // staged rows, staged row pitch (odd)
    const int SW = kTW + 2 * R;                                           // staged row width
    uint32_t* staged = smem;
    uint32_t* hbuf = staged + SR * SP;
    uint32_t* hist = hbuf + SR * kHP;
    const int row = C * C + 2 * C, nh = (n + 1) * row;
    awseg_scan_zero<kThreads>(hist, nh);
    const int64_t img = blockIdx.y, hw = (int64_t)H * W;
    const uint8_t* pp = pred + img * hw;
    const int x = threadIdx.x & (kTW - 1), y0 = (threadIdx.x / kTW) * kPer;
    uint32_t bad = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * kTH, tx0 = (tile % tiles_x) * kTW;
        uint32_t ctr[2][kPer];                                            // the lane's own pixels as class bits: label, prediction
        int ring[2][kPer];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            __syncthreads();                                              // the previous map's passes (and the zeroing) are done
            for (int i = threadIdx.x; i < SR * SW; i += kThreads) {
                const int r = i / SW, c = i - r * SW;                     // (stepping r and c without the division measured 3 % slower)
                const int gy = ty0 - R + r, gx = tx0 - R + c;
                uint32_t bit = 0;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    const int64_t at = (int64_t)gy * W + gx;
                    if (m == 0) {
                        const int64_t t = awseg_ld_label<LDT>(label, img * hw + at);
                        if (t != ignore_index && t >= 0 && t < C) bit = 1u << (int)t;
                    } else {
                        const int v = pp[at];
                        if (v < C) bit = 1u << v;
                    }
                }
                staged[r * SP + c] = bit;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kPer; ++j) { ctr[m][j] = staged[(R + y0 + j) * SP + R + x]; ring[m][j] = n; }
            for (int k = 0; k < n; ++k) {
                const int d = wd.d[k];
                const int rows = kTH + 2 * d;                             // the column pass reads rows R - d .. R + kTH + d - 1
                for (int i = threadIdx.x; i < rows * (kTW / kPer); i += kThreads) {
                    const int seg = i / rows, r = R - d + (i - seg * rows);
                    uint32_t o8[kPer];
                    window8(staged + r * SP + R + seg * kPer, 1, d, o8);
#pragma unroll
                    for (int j = 0; j < kPer; ++j) hbuf[r * kHP + seg * kPer + j] = o8[j];
                }
                __syncthreads();
                uint32_t v8[kPer];
                window8(hbuf + (R + y0) * kHP + x, kHP, d, v8);
#pragma unroll
                for (int j = 0; j < kPer; ++j) ring[m][j] -= (v8[j] & ~ctr[m][j]) != 0u;
                __syncthreads();                                          // before the next width overwrites hbuf
            }
        }
        // runs of equal (label ring, prediction ring, label, prediction) down the lane's 8 rows: one set of LDS adds per run.  Open-coded:
        // on awseg_run (awseg_mapscan.h) the same registers and occupancy came out, and 1.2 % more time in every run
        // (profiles/mapscan_kernel_bench_hip_events.log)
        uint32_t run_key = ~0u, run = 0;
#pragma unroll
        for (int j = 0; j <= kPer; ++j) {
            uint32_t key = ~0u;
            if (j < kPer && ctr[0][j]) {                                  // labelled (a pixel outside the frame is staged as 0)
                if (!ctr[1][j]) ++bad;                                    // a value no argmax over C classes produces
                else key = ((uint32_t)ring[0][j] << 24) | ((uint32_t)ring[1][j] << 16) | ((uint32_t)(__ffs(ctr[0][j]) - 1) << 8)
                           | (uint32_t)(__ffs(ctr[1][j]) - 1);
            }
            if (key == run_key && j < kPer) { ++run; continue; }
            if (run_key != ~0u) {
                const int rl = run_key >> 24, rp = (run_key >> 16) & 0xFF, t = (run_key >> 8) & 0xFF, p = run_key & 0xFF;
                atomicAdd(&hist[rl * row + t * C + p], run);
                atomicAdd(&hist[rp * row + C * C + C + p], run);
                if (t == p) atomicAdd(&hist[(rl > rp ? rl : rp) * row + C * C + t], run);
            }
            run_key = key; run = 1;
        }
    }
    awseg_scan_count_bad(bad, oob);
    awseg_scan_store<kThreads>(hist, nh, partial);
}

int64_t bnd_tiles(int height, int width) { return (int64_t)((height + kTH - 1) / kTH) * ((width + kTW - 1) / kTW); }

int bnd_blocks_per_image(int64_t tiles, int64_t batch) { return awseg_blocks_per_image(tiles, 1, batch, kResident); }   // a block per tile

int bnd_row(int num_classes, int n_widths) { return (n_widths + 1) * (num_classes * num_classes + 2 * num_classes); }

}  // namespace

AWSEG_API int64_t awseg_boundary_workspace(int64_t batch, int num_classes, int height, int width, int n_widths)
{
    if (batch < 1) batch = 1;
    if (height < 1) height = 1;
    if (width < 1) width = 1;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) num_classes = AWSEG_MAX_CLASSES;
    if (n_widths < 1 || n_widths > AWSEG_BOUNDARY_MAX_WIDTHS) n_widths = AWSEG_BOUNDARY_MAX_WIDTHS;
    return (int64_t)bnd_blocks_per_image(bnd_tiles(height, width), batch) * batch * bnd_row(num_classes, n_widths) * (int64_t)sizeof(uint32_t);
}

AWSEG_API int awseg_boundary_stats(const uint8_t* pred, const void* label, int label_dtype, int ignore_index, int64_t batch,
                                   int height, int width, int num_classes, const int32_t* widths, int n_widths,
                                   const int32_t* cond, int64_t* stats, int n_slots, int64_t* oob, void* workspace,
                                   awseg_stream_t stream)
{
    if (!pred || !label || !widths || !stats || !oob || !workspace) return AWSEG_EINVAL;
    if (batch < 1 || height < 1 || width < 1 || n_slots < 1) return AWSEG_EINVAL;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    if (n_widths < 1 || n_widths > AWSEG_BOUNDARY_MAX_WIDTHS) return AWSEG_EINVAL;
    Widths wd = {};
    wd.n = n_widths;
    for (int k = 0; k < n_widths; ++k) {
        if (widths[k] < 1 || widths[k] > AWSEG_BOUNDARY_MAX_RADIUS || (k && widths[k] <= widths[k - 1])) return AWSEG_EINVAL;
        wd.d[k] = widths[k];
    }
    if (batch > 65535 || (int64_t)height * width > INT32_MAX) return AWSEG_ERANGE;     // grid.y; uint32 per-block partials
    hipStream_t s = awseg_s(stream);
    const int64_t tiles = bnd_tiles(height, width);
    const int bpi = bnd_blocks_per_image(tiles, batch);                               // same count the workspace query assumed
    const int row = bnd_row(num_classes, n_widths);
    const int R = wd.d[n_widths - 1];
    const size_t lds = ((size_t)(kTH + 2 * R) * (kTW + 2 * R + 1 + kHP) + row) * sizeof(uint32_t);   // <= 63232 B
    uint32_t* partial = (uint32_t*)workspace;
    dim3 grid(bpi, (unsigned)batch), block(kThreads);
    const int tiles_x = (width + kTW - 1) / kTW;
    awseg_by_label(label_dtype, [&](auto L) {
        hipLaunchKernelGGL((boundary_kernel<decltype(L)::value>), grid, block, lds, s, pred, label, ignore_index, height, width,
                           num_classes, wd, tiles_x, (int)tiles, partial, oob);
    });
    AWSEG_LAUNCH_CHECK();
    return awseg_fold_u32_launch(partial, batch, bpi, row, cond, n_slots, true, stats, s);
}
