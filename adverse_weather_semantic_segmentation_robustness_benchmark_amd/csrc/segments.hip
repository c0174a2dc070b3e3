// segments.hip — segment-level counters: the 8-connected components of the label map and of the prediction map of
// every frame, and per component its area and its coverage by the other map (include/awseg.h gives the definitions), histogrammed
// per (slot, class, size bucket, coverage cell).
//
// Components cross tile seams, so the labelling is a union-find over a parent array L in the workspace (one per side; index and
// value are pixel indices y * W + x WITHIN the frame, -1 = in no segment), built by four kernels on one stream:
//   tile    a block per 32 x 64 tile (boundary.hip's tiling) labels the tile in LDS (row runs of 8, then unions across run ends and
//           rows with LDS atomicMin), sums area / hits per tile-local root in LDS, and writes L (the tile-local root of every pixel)
//           and the sums at the roots' cells (0 everywhere else: a non-zero area marks a tile-local root);
//   seam    one lane per pixel beside a tile seam unions it with its same-class neighbours in the next tile;
//   gather  every tile-local root that is no final root adds its sums into its final root's cells and points straight at it;
//   emit    every final root (L[i] == i) adds 1 to its stats cell; every pixel's id is its final root.
// No block waits for another: the order between the passes is the kernel boundary.  The invariant is L[i] <= i (the smaller
// index becomes the parent; tile-local roots are the minimum of their tile-local component), so every step of a find and every
// retry of a union goes to a strictly smaller index and ends by itself; the final root is the component's minimum index.
// Integers only.
#include "awseg_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kResident = 8;                                              // blocks per CU the per-pixel grids are capped at
constexpr int kTH = 32, kTW = 64, kTile = kTH * kTW;                      // tile; kThreads lanes x 8 rows
constexpr int kPer = 8;
constexpr int kNone = 0xFF;                                               // class code of a pixel in no segment
constexpr int kCells = AWSEG_SEGMENT_CELLS, kBuckets = AWSEG_SEGMENT_BUCKETS;
constexpr int kSmall = 2;                                                 // size buckets the emit pass histograms in LDS first

// The workspace: per side (0 label, 1 prediction) the parent array, area and hits; the label side's reference hits; the class codes.
struct Work {
    int32_t* L[2];
    uint32_t* area[2];
    uint32_t* hit[2];
    uint32_t* ref;
    uint8_t* cls[2];
};

Work carve(void* workspace, int64_t n)
{
    Work w;
    uint32_t* p = (uint32_t*)workspace;
    w.L[0] = (int32_t*)p; w.L[1] = (int32_t*)(p + n);
    w.area[0] = p + 2 * n; w.area[1] = p + 3 * n;
    w.hit[0] = p + 4 * n; w.hit[1] = p + 5 * n;
    w.ref = p + 6 * n;
    w.cls[0] = (uint8_t*)(p + 7 * n); w.cls[1] = w.cls[0] + n;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------- LDS union-find
__device__ __forceinline__ int lds_find(volatile int* par, int i)
{
    for (int p = par[i]; p != i; p = par[i]) i = p;
    return i;
}
// Lock-free: find both roots, atomicMin the larger root's cell with the smaller; if someone moved that cell first, go on from what
// it held (its old parent must end up joined to the smaller root as well).  Every retry starts from a smaller index.
__device__ __forceinline__ void lds_union(int* par, int a, int b)
{
    for (;;) {
        a = lds_find(par, a); b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

// ------------------------------------------------------------------------------------------------------------- global union-find
// Agent-scope atomic loads and updates: the parent array is shared by blocks on every XCD, whose L2s are not coherent for plain
// accesses within a launch.
__device__ __forceinline__ int agent_find(int32_t* L, int i)
{
    for (int p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); p != i;
         p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) i = p;
    return i;
}
__device__ __forceinline__ void agent_union(int32_t* L, int a, int b)
{
    for (;;) {
        a = agent_find(L, a); b = agent_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}
// after the seam pass (a kernel boundary behind every update): plain loads
__device__ __forceinline__ int plain_find(const int32_t* L, int i)
{
    for (int p = L[i]; p != i; p = L[i]) i = p;
    return i;
}

// cov(h, A) = 0 when h == 0, else 1 + floor(4 h / A): floor(4 h / A) counts the j in 1 .. 4 with 4 h >= j A (64-bit)
__device__ __forceinline__ int seg_cov(uint32_t h, uint32_t a)
{
    if (h == 0) return 0;
    const uint64_t h4 = 4ull * h, A = a;
    return 1 + (int)(h4 >= A) + (int)(h4 >= 2 * A) + (int)(h4 >= 3 * A) + (int)(h4 >= 4 * A);
}
__device__ __forceinline__ int seg_bucket(uint32_t a)
{
    const int s = (31 - __clz((int)a)) >> 1;
    return s < kBuckets - 1 ? s : kBuckets - 1;
}

// ---------------------------------------------------------------------------------------------------------------------- tile pass
// grid = (blocks_per_image, B); block x of image y walks tiles x, x + gridDim.x, ...  LDS 26 KB: class codes | parents | area << 16
// + hits | reference hits, used by the label side and then by the prediction side.
template <int LDT>
__global__ __launch_bounds__(kThreads)
void segment_tile_kernel(const uint8_t* __restrict__ pred, const void* __restrict__ label, int ignore_index, int H, int W, int C,
                         const uint8_t* __restrict__ ref_maps, int n_refs, const int32_t* __restrict__ frame_ref, int tiles_x,
                         int tiles, const Work wk, int64_t* __restrict__ oob)
{
    __shared__ uint8_t cls[kTile];
    __shared__ int par[kTile];
    __shared__ uint32_t sum_ah[kTile];                                    // area << 16 | hits: both <= 2048
    __shared__ uint32_t sum_ref[kTile];
    const int64_t img = blockIdx.y, hw = (int64_t)H * W, first = img * hw;
    const uint8_t* pp = pred + first;
    const uint8_t* rp = nullptr;
    if (ref_maps && frame_ref) {
        const int r = frame_ref[img];
        if (r >= 0 && r < n_refs) rp = ref_maps + (int64_t)r * hw;
        else if (r >= n_refs && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long*)oob, (unsigned long long)hw);
    }
    const int x = threadIdx.x & (kTW - 1), y0 = (threadIdx.x / kTW) * kPer;
    uint32_t bad = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * kTH, tx0 = (tile % tiles_x) * kTW;
        const int gx = tx0 + x;
        int code[2][kPer];                                                // the lane's pixels: label class, prediction class (kNone: none)
        uint32_t hits = 0, rhits = 0, inside = 0;                         // bit j: prediction == label; reference == label; in the frame
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int gy = ty0 + y0 + j;
            code[0][j] = code[1][j] = kNone;
            if (gy < H && gx < W) {
                inside |= 1u << j;
                const int64_t at = (int64_t)gy * W + gx;
                const int64_t t = awseg_ld_label<LDT>(label, first + at);
                if (t != ignore_index && t >= 0 && t < C) {               // live
                    const int p = pp[at];
                    code[0][j] = (int)t;
                    if (p < C) { code[1][j] = p; hits |= (uint32_t)(p == (int)t) << j; }
                    else ++bad;
                    if (rp) {
                        const int rv = rp[at];
                        if (rv < C) rhits |= (uint32_t)(rv == (int)t) << j;
                        else ++bad;
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            __syncthreads();                                              // the previous side (or tile) is done with the LDS
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int i = (y0 + j) * kTW + x;
                cls[i] = (uint8_t)code[m][j]; sum_ah[i] = 0u; sum_ref[i] = 0u;
            }
            __syncthreads();
            {   // row runs: a lane owns 8 consecutive pixels of a row; each points at the first pixel of its run within the 8
                const int base = (threadIdx.x >> 3) * kTW + (threadIdx.x & 7) * kPer;
                int start = base, prev = cls[base];
                par[base] = prev == kNone ? -1 : base;
#pragma unroll
                for (int k = 1; k < kPer; ++k) {
                    const int c = cls[base + k];
                    if (c == kNone) par[base + k] = -1;
                    else { if (c != prev) start = base + k; par[base + k] = start; }
                    prev = c;
                }
            }
            __syncthreads();
            // unions across the run ends and with the row above.  A neighbour pair is skipped where another pair joins the same
            // two runs: N covers NW and NE (they sit beside N in its row), and a pixel whose W neighbour has the same pair to join
            // (W with NW for N and for NW; E with NE) leaves it to that neighbour, down to the one that has none.
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int c = code[m][j];
                if (c == kNone) continue;
                const int r = y0 + j, i = r * kTW + x;
                const bool wm = x > 0 && cls[i - 1] == c;
                if (wm && (x & (kPer - 1)) == 0) lds_union(par, i, i - 1);
                if (r == 0) continue;
                const bool nwm = x > 0 && cls[i - kTW - 1] == c;
                if (cls[i - kTW] == c) {
                    if (!(wm && nwm)) lds_union(par, i, i - kTW);
                } else {
                    if (nwm && !wm) lds_union(par, i, i - kTW - 1);
                    if (x < kTW - 1 && cls[i - kTW + 1] == c && cls[i + 1] != c) lds_union(par, i, i - kTW + 1);
                }
            }
            __syncthreads();
            // the tile-local root of every pixel, and the sums per root: runs of one root down the lane's 8 rows add once
            int root[kPer];
            int run_root = -1;
            uint32_t run_ah = 0, run_ref = 0;
#pragma unroll
            for (int j = 0; j <= kPer; ++j) {
                int rt = -1;
                if (j < kPer) {
                    if (code[m][j] != kNone) rt = lds_find(par, (y0 + j) * kTW + x);
                    root[j] = rt;
                }
                if (rt != run_root) {
                    if (run_root >= 0) {
                        atomicAdd(&sum_ah[run_root], run_ah);
                        if (m == 0 && run_ref) atomicAdd(&sum_ref[run_root], run_ref);
                    }
                    run_root = rt; run_ah = 0; run_ref = 0;
                }
                if (j < kPer && rt >= 0) { run_ah += (1u << 16) | ((hits >> j) & 1u); run_ref += (rhits >> j) & 1u; }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                if (!((inside >> j) & 1u)) continue;
                const int i = (y0 + j) * kTW + x, rt = root[j];
                const int64_t at = first + (int64_t)(ty0 + y0 + j) * W + gx;
                wk.L[m][at] = rt < 0 ? -1 : (ty0 + (rt >> 6)) * W + tx0 + (rt & (kTW - 1));      // a pixel of this tile: inside the frame
                const uint32_t ah = rt == i ? sum_ah[i] : 0u;
                wk.area[m][at] = ah >> 16;
                wk.hit[m][at] = ah & 0xFFFFu;
                if (m == 0) wk.ref[at] = rt == i ? sum_ref[i] : 0u;
                wk.cls[m][at] = (uint8_t)code[m][j];
            }
        }
    }
    bad = awseg_wave_sum_u32(bad);
    if ((threadIdx.x & (AWSEG_WAVE - 1)) == 0 && bad) atomicAdd((unsigned long long*)oob, (unsigned long long)bad);
}

// ---------------------------------------------------------------------------------------------------------------------- seam pass
// The pixels beside a seam: the first row of every tile row but the first (n_h = (tiles_y - 1) * W of them per frame), then the
// columns left and right of every vertical seam (n_v = (tiles_x - 1) * 2 * H; those already in the first list are skipped).  Each
// looks at its W, NW, N and NE neighbours (the other four are some other pixel's) and unions with those of its class in ANOTHER
// tile; N covers NW and NE as in the tile pass.  grid = (blocks, B).
__global__ __launch_bounds__(kThreads)
void segment_seam_kernel(int H, int W, int n_h, int n_v, const Work wk)
{
    const int64_t first = (int64_t)blockIdx.y * H * W;
    for (int item = blockIdx.x * kThreads + threadIdx.x; item < n_h + n_v; item += gridDim.x * kThreads) {
        int y, x;
        if (item < n_h) { y = (item / W + 1) * kTH; x = item % W; }
        else {
            const int v = item - n_h, col = v / H;
            y = v % H; x = (col / 2 + 1) * kTW - (col & 1);
            if (y > 0 && (y & (kTH - 1)) == 0) continue;
        }
        const int i = y * W + x;
        const bool top = y > 0 && (y & (kTH - 1)) == 0, left = x > 0 && (x & (kTW - 1)) == 0, right = x < W - 1 && (x & (kTW - 1)) == kTW - 1;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const uint8_t* cls = wk.cls[m] + first;
            int32_t* L = wk.L[m] + first;
            const int c = cls[i];
            if (c == kNone) continue;
            if (left && cls[i - 1] == c) agent_union(L, i, i - 1);
            if (y == 0) continue;
            if (cls[i - W] == c) {
                if (top) agent_union(L, i, i - W);
            } else {
                if ((top || left) && x > 0 && cls[i - W - 1] == c) agent_union(L, i, i - W - 1);
                if ((top || right) && x < W - 1 && cls[i - W + 1] == c) agent_union(L, i, i - W + 1);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- gather pass
// A tile-local root (area != 0) that is no final root adds its sums into its final root's cells: one set of atomics per tile-local
// component.  It then points straight at the final root (any mix of old and new parents still leads there), so the emit pass finds
// every pixel's id in two steps.  grid = (blocks, B).
__global__ __launch_bounds__(kThreads)
void segment_gather_kernel(int hw, const Work wk)
{
    const int64_t first = (int64_t)blockIdx.y * hw;
    for (int64_t at = (int64_t)blockIdx.x * kThreads + threadIdx.x; at < hw; at += (int64_t)gridDim.x * kThreads) {
        const int i = (int)at;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const uint32_t a = wk.area[m][first + i];
            if (a == 0u) continue;
            int32_t* L = wk.L[m] + first;
            if (L[i] == i) continue;
            const int r = plain_find(L, i);
            atomicAdd(&wk.area[m][first + r], a);
            const uint32_t h = wk.hit[m][first + i];
            if (h) atomicAdd(&wk.hit[m][first + r], h);
            if (m == 0) {
                const uint32_t g = wk.ref[first + i];
                if (g) atomicAdd(&wk.ref[first + r], g);
            }
            L[i] = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- emit pass
// Every final root adds 1 to stats[slot][class][bucket][cell] for slot 0 and the frame's condition slot: segments below 16 pixels
// (buckets 0 and 1: all of them on maps of independent pixels) through a per-block LDS histogram, the rest straight to memory.
// Every pixel's id goes to the id maps that were asked for.  grid = (blocks, B); dynamic LDS C * kSmall * kCells uint32.
__global__ __launch_bounds__(kThreads)
void segment_emit_kernel(int hw, int C, const uint8_t* __restrict__ ref_maps, int n_refs, const int32_t* __restrict__ frame_ref,
                         const int32_t* __restrict__ cond, int64_t* __restrict__ stats, int n_slots, int32_t* __restrict__ label_ids,
                         int32_t* __restrict__ pred_ids, const Work wk)
{
    extern __shared__ uint32_t hist[];
    const int small = C * kSmall * kCells;
    for (int k = threadIdx.x; k < small; k += kThreads) hist[k] = 0u;
    __syncthreads();
    const int64_t img = blockIdx.y, first = img * hw;
    bool has_ref = false;
    if (ref_maps && frame_ref) { const int r = frame_ref[img]; has_ref = r >= 0 && r < n_refs; }
    const int64_t row = (int64_t)C * kBuckets * kCells;
    int64_t* slot = nullptr;
    if (cond) { const int cd = cond[img]; if (cd >= 0 && cd < n_slots - 1) slot = stats + (1 + (int64_t)cd) * row; }
    int32_t* ids[2] = { label_ids, pred_ids };
    for (int64_t px = (int64_t)blockIdx.x * kThreads + threadIdx.x; px < hw; px += (int64_t)gridDim.x * kThreads) {
        const int i = (int)px;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int32_t* L = wk.L[m] + first;
            const int p = L[i];
            if (p == i) {
                const uint32_t a = wk.area[m][first + i], h = wk.hit[m][first + i];
                const int c = wk.cls[m][first + i], s = seg_bucket(a);
                const int cell = m == 0 ? seg_cov(h, a) * 7 + (has_ref ? seg_cov(wk.ref[first + i], a) : 6) : 42 + seg_cov(h, a);
                if (s < kSmall) atomicAdd(&hist[(c * kSmall + s) * kCells + cell], 1u);
                else {
                    const int64_t at = ((int64_t)c * kBuckets + s) * kCells + cell;
                    atomicAdd((unsigned long long*)&stats[at], 1ull);
                    if (slot) atomicAdd((unsigned long long*)&slot[at], 1ull);
                }
            }
            if (ids[m]) ids[m][first + i] = p < 0 ? -1 : (p == i ? i : plain_find(L, p));
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < small; k += kThreads) {
        const uint32_t n = hist[k];
        if (!n) continue;
        const int cs = k / kCells, cell = k - cs * kCells, c = cs / kSmall, s = cs - c * kSmall;
        const int64_t at = ((int64_t)c * kBuckets + s) * kCells + cell;
        atomicAdd((unsigned long long*)&stats[at], (unsigned long long)n);
        if (slot) atomicAdd((unsigned long long*)&slot[at], (unsigned long long)n);
    }
}

int64_t seg_tiles(int height, int width) { return (int64_t)((height + kTH - 1) / kTH) * ((width + kTW - 1) / kTW); }

}  // namespace

AWSEG_API int64_t awseg_segment_workspace(int64_t batch, int height, int width)
{
    if (batch < 1) batch = 1;
    if (height < 1) height = 1;
    if (width < 1) width = 1;
    return batch * height * width * (int64_t)AWSEG_SEGMENT_WORKSPACE_PER_PIXEL;
}

AWSEG_API int awseg_segment_stats(const uint8_t* pred, const void* label, int label_dtype, int ignore_index, int64_t batch, int height,
                                  int width, int num_classes, const uint8_t* ref_maps, int n_refs, const int32_t* frame_ref,
                                  const int32_t* cond, int64_t* stats, int n_slots, int64_t* oob, int32_t* label_ids,
                                  int32_t* pred_ids, void* workspace, awseg_stream_t stream)
{
    if (!pred || !label || !stats || !oob || !workspace) return AWSEG_EINVAL;
    if (batch < 1 || height < 1 || width < 1 || n_slots < 1) return AWSEG_EINVAL;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    if (ref_maps && frame_ref && n_refs < 1) return AWSEG_EINVAL;
    if (batch > 65535 || (int64_t)height * width > INT32_MAX) return AWSEG_ERANGE;     // grid.y; int32 pixel indices within a frame
    hipStream_t s = awseg_s(stream);
    const int hw = height * width;
    const Work wk = carve(workspace, batch * hw);
    const int tiles_x = (width + kTW - 1) / kTW, tiles_y = (height + kTH - 1) / kTH;
    const int64_t tiles = seg_tiles(height, width);
    dim3 block(kThreads);
    dim3 tile_grid(awseg_blocks_per_image(tiles, 1, batch, kResident), (unsigned)batch);
    awseg_by_label(label_dtype, [&](auto L) {
        hipLaunchKernelGGL((segment_tile_kernel<decltype(L)::value>), tile_grid, block, 0, s, pred, label, ignore_index, height, width,
                           num_classes, ref_maps, n_refs, frame_ref, tiles_x, (int)tiles, wk, oob);
    });
    AWSEG_LAUNCH_CHECK();
    const int64_t n_h = (int64_t)(tiles_y - 1) * width, n_v = (int64_t)(tiles_x - 1) * 2 * height;      // both < 2 hw / 32
    if (n_h + n_v > 0) {
        dim3 seam_grid(awseg_blocks_per_image(n_h + n_v, kThreads, batch, kResident), (unsigned)batch);
        hipLaunchKernelGGL(segment_seam_kernel, seam_grid, block, 0, s, height, width, (int)n_h, (int)n_v, wk);
        AWSEG_LAUNCH_CHECK();
    }
    dim3 pixel_grid(awseg_blocks_per_image(hw, kThreads, batch, kResident), (unsigned)batch);
    if (n_h + n_v > 0) {                                                  // one tile: every tile-local root is final
        hipLaunchKernelGGL(segment_gather_kernel, pixel_grid, block, 0, s, hw, wk);
        AWSEG_LAUNCH_CHECK();
    }
    const size_t lds = (size_t)num_classes * kSmall * kCells * sizeof(uint32_t);       // <= 12 KB
    hipLaunchKernelGGL(segment_emit_kernel, pixel_grid, block, lds, s, hw, num_classes, ref_maps, n_refs, frame_ref, cond, stats,
                       n_slots, label_ids, pred_ids, wk);
    AWSEG_LAUNCH_CHECK();
    return 0;
}
