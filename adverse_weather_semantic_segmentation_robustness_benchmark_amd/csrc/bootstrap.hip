// bootstrap.hip — the two device passes of the frame bootstrap: per-frame IoU counters, and their replicate sums
// under a paired resampling of the source frames.
//
// awseg_frame_iou_counts is consistency.hip's scan with one map less: each lane owns 16 consecutive pixels (one 16-byte load per
// map when every row base is 16-byte aligned and hw % 16 == 0, byte loads otherwise), merges its (label, prediction) pairs into
// runs in registers and touches the per-block LDS row [C intersection | C label | C prediction] once per run.  Blocks write uint32
// partials; a second launch folds them into the int64 table row frame_row[b] names.  Integer sums only.
//
// awseg_bootstrap_counts runs one block per replicate: the replicate's draws (Philox4x32-7, stream kBootStream, index =
// mulhi32(word, n)) are staged in LDS once, kBootDraws at a time, then every thread owns output cells (slot, column) and walks the
// draws — no atomics, one fixed order, 64-bit accumulators; slot 0 is folded from the block's own cells at the end.
#include "awseg_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 16;                                                  // pixels per lane per step
constexpr int kRowMax = 3 * AWSEG_MAX_CLASSES;
constexpr uint32_t kBootStream = 0x0B07u;                                 // weather.hip owns 0x0F06, 0x0F07, 0x0A17, 0x0DE5
constexpr int kBootDraws = AWSEG_BOOTSTRAP_STAGED_DRAWS;                  // draws staged in LDS per pass (16 KB); larger n is chunked
static_assert(kBootDraws % 4 == 0, "a Philox call fills four consecutive draws");

__device__ __forceinline__ void unpack16(const uint4 q, int (&v)[kPer])
{
    const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[k] = (int)((w[k >> 2] >> ((k & 3) * 8)) & 0xFF);
}

// grid = (blocks_per_image, B); block x of image y writes partial[(y * gridDim.x + x)][3 C].
// VEC: hw % 16 == 0 and pred and label 16-byte aligned (every row base then is); else byte loads.
template <int LDT, bool VEC>
__global__ __launch_bounds__(kThreads)
void frame_iou_kernel(const uint8_t* __restrict__ pred, const void* __restrict__ label, int ignore_index, int64_t hw, int C,
                      const int32_t* __restrict__ frame_row, int64_t n_rows, uint32_t* __restrict__ partial, int64_t* __restrict__ oob)
{
    __shared__ uint32_t hist[kRowMax];
    const int row = 3 * C;
    for (int i = threadIdx.x; i < row; i += kThreads) hist[i] = 0u;
    __syncthreads();
    const int64_t img = blockIdx.y;
    const int64_t r = frame_row[img];
    uint32_t bad = 0;
    if (r >= 0 && r < n_rows) {
        const uint8_t* pp = pred + img * hw;
        const int64_t lb = img * hw;
        const int64_t nchunk = (hw + kPer - 1) / kPer;
        for (int64_t ch = (int64_t)blockIdx.x * kThreads + threadIdx.x; ch < nchunk; ch += (int64_t)gridDim.x * kThreads) {
            const int64_t base = ch * kPer;
            int pv[kPer];
            int64_t lv[kPer];
            if constexpr (VEC) {
                unpack16(*reinterpret_cast<const uint4*>(pp + base), pv);
                if constexpr (LDT == AWSEG_U8) {
                    int l8[kPer];
                    unpack16(*reinterpret_cast<const uint4*>((const uint8_t*)label + lb + base), l8);
#pragma unroll
                    for (int k = 0; k < kPer; ++k) lv[k] = l8[k];
                } else {
                    const longlong2* lp = reinterpret_cast<const longlong2*>((const int64_t*)label + lb + base);
#pragma unroll
                    for (int k = 0; k < kPer / 2; ++k) { const longlong2 q = lp[k]; lv[2 * k] = q.x; lv[2 * k + 1] = q.y; }
                }
            } else {
#pragma unroll
                for (int k = 0; k < kPer; ++k) {
                    const bool in = base + k < hw;
                    pv[k] = in ? (int)pp[base + k] : 0;
                    lv[k] = in ? awseg_ld_label<LDT>(label, lb + base + k) : (int64_t)ignore_index;
                }
            }
            int run_t = -1, run_p = -1;
            uint32_t run = 0;
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                if (!VEC && base + k >= hw) break;
                const int pk = pv[k];
                const int64_t t = lv[k];
                const bool labelled = t != ignore_index && t >= 0 && t < C;
                if (pk >= C) ++bad;                                       // a map value no argmax over C classes produces
                if (!labelled && t != ignore_index) ++bad;                // a label that is neither a class nor the ignore value
                if (!labelled || pk >= C) continue;
                const int tk = (int)t;
                if (tk == run_t && pk == run_p) { ++run; continue; }
                if (run) {
                    atomicAdd(&hist[C + run_t], run);
                    atomicAdd(&hist[2 * C + run_p], run);
                    if (run_t == run_p) atomicAdd(&hist[run_t], run);
                }
                run_t = tk; run_p = pk; run = 1;
            }
            if (run) {
                atomicAdd(&hist[C + run_t], run);
                atomicAdd(&hist[2 * C + run_p], run);
                if (run_t == run_p) atomicAdd(&hist[run_t], run);
            }
        }
    } else if (r >= n_rows && blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd((unsigned long long*)oob, (unsigned long long)hw);    // a row the table does not have: frame not counted
    }
    bad = awseg_wave_sum_u32(bad);
    if ((threadIdx.x & (AWSEG_WAVE - 1)) == 0 && bad) atomicAdd((unsigned long long*)oob, (unsigned long long)bad);
    __syncthreads();
    uint32_t* dst = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * row;
    for (int i = threadIdx.x; i < row; i += kThreads) dst[i] = hist[i];
}

// awseg_fold_u32_partials_kernel with a row instead of a condition slot as the destination: partials [img][blocks_per_image][row]
// into table[frame_row[img]][row] (frames whose row is outside [0, n_rows) wrote zero partials and are skipped here as well).
// grid = (B, ceil(row / 64)), block = kFoldSlices * 64.
constexpr int kFoldSlices = 4;
__global__ __launch_bounds__(kFoldSlices * 64)
void frame_fold_kernel(const uint32_t* __restrict__ partial, int blocks_per_image, int row, const int32_t* __restrict__ frame_row,
                       int64_t n_rows, int64_t* __restrict__ table)
{
    __shared__ unsigned long long s_sum[kFoldSlices][64];
    const int img = blockIdx.x;
    const int kl = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int k = blockIdx.y * 64 + kl;
    const uint32_t* src = partial + (int64_t)img * blocks_per_image * row;
    unsigned long long s = 0;
    if (k < row) {
#pragma unroll 8
        for (int b = slice; b < blocks_per_image; b += kFoldSlices) s += src[(int64_t)b * row + k];
    }
    s_sum[slice][kl] = s;
    __syncthreads();
    if (slice == 0 && k < row) {
        s = 0;
#pragma unroll
        for (int j = 0; j < kFoldSlices; ++j) s += s_sum[j][kl];
        const int64_t r = frame_row[img];
        if (s && r >= 0 && r < n_rows) atomicAdd((unsigned long long*)&table[r * row + k], s);   // two frames may name one row
    }
}

int fiou_blocks_per_image(int64_t hw, int64_t batch)
{
    // 256 CUs x 4 resident blocks over the whole batch (a 2 B/px scan), grid-stride beyond: consistency.hip's rule
    int64_t want = ((hw + kPer - 1) / kPer + kThreads - 1) / kThreads;
    int64_t cap = (AWSEG_CUS * 4 + batch - 1) / batch;
    if (cap < 1) cap = 1;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    return (int)want;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// grid = R, block = kThreads.  Replicate q = r0 + blockIdx.x; out[blockIdx.x][n_slots][W].
__global__ __launch_bounds__(kThreads)
void bootstrap_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ slots, int n, int V, int W, int n_slots,
                      uint64_t seed, int64_t r0, int64_t* __restrict__ out, int64_t* __restrict__ oob)
{
    __shared__ int s_draw[kBootDraws];
    const uint64_t q = (uint64_t)(r0 + blockIdx.x);
    const uint64_t n4 = ((uint64_t)n + 3) / 4;                            // Philox calls per replicate
    const int cells = n_slots * W;                                        // host: n_slots * W <= INT32_MAX
    int64_t* dst = out + (int64_t)blockIdx.x * cells;
    if (blockIdx.x == 0) {
        // the slot table is judged once per call, not once per draw: oob does not depend on R or on the draws
        uint32_t bad = 0;
        const int nv = n * V;
        for (int e = threadIdx.x; e < nv; e += kThreads) { const int sl = slots[e]; bad += (sl < 0 || sl >= n_slots) ? 1u : 0u; }
        bad = awseg_wave_sum_u32(bad);
        if ((threadIdx.x & (AWSEG_WAVE - 1)) == 0 && bad) atomicAdd((unsigned long long*)oob, (unsigned long long)bad);
    }
    for (int j0 = 0; j0 < n; j0 += kBootDraws) {
        const int m = n - j0 < kBootDraws ? n - j0 : kBootDraws;          // draws of this pass
        __syncthreads();                                                  // the previous pass is done with s_draw
        for (int g = threadIdx.x; g < (m + 3) / 4; g += kThreads) {
            uint32_t u[4];
            awseg_philox::gen(seed, q * n4 + (uint64_t)(j0 / 4 + g), kBootStream, u);
#pragma unroll
            for (int k = 0; k < 4; ++k) s_draw[4 * g + k] = (int)__umulhi(u[k], (uint32_t)n);   // < n; bias <= n / 2^32
        }
        __syncthreads();
        // slots >= 1 only: a frame sits in slot 0 and in exactly one other slot, so slot 0 is the sum of the others (below) and
        // every table entry is read once per replicate
        for (int cell = W + threadIdx.x; cell < cells; cell += kThreads) {
            const int s = cell / W, w = cell - s * W;
            int64_t acc = 0;
            for (int j = 0; j < m; ++j) {
                const int e0 = s_draw[j] * V;                             // < n * V <= INT32_MAX
#pragma unroll 4
                for (int v = 0; v < V; ++v)
                    if (slots[e0 + v] == s) acc += table[(int64_t)(e0 + v) * W + w];   // 1 <= s < n_slots: the value is in range
            }
            if (j0 == 0) dst[cell] = acc; else dst[cell] += acc;          // this thread owns the cell
        }
    }
    __threadfence_block();
    __syncthreads();                                                      // the block's cells are written: fold them into slot 0
    for (int w = threadIdx.x; w < W; w += kThreads) {
        int64_t acc = 0;
        for (int s = 1; s < n_slots; ++s) acc += dst[(int64_t)s * W + w];
        dst[w] = acc;
    }
}

}  // namespace

AWSEG_API int64_t awseg_frame_iou_workspace(int64_t batch, int num_classes, int64_t hw)
{
    if (batch < 1) batch = 1;
    if (hw < 1) hw = 1;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) num_classes = AWSEG_MAX_CLASSES;
    return (int64_t)fiou_blocks_per_image(hw, batch) * batch * (3 * num_classes) * (int64_t)sizeof(uint32_t);
}

AWSEG_API int awseg_frame_iou_counts(const uint8_t* pred, const void* label, int label_dtype, int ignore_index, int64_t batch,
                                     int64_t hw, int num_classes, const int32_t* frame_row, int64_t* table, int64_t n_rows,
                                     int64_t* oob, void* workspace, awseg_stream_t stream)
{
    if (!pred || !label || !frame_row || !table || !oob || !workspace) return AWSEG_EINVAL;
    if (batch < 1 || hw < 1 || n_rows < 1) return AWSEG_EINVAL;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    if (batch > 65535 || hw > INT32_MAX) return AWSEG_ERANGE;                 // grid.y; uint32 per-block partials
    hipStream_t s = awseg_s(stream);
    const int bpi = fiou_blocks_per_image(hw, batch);                          // same count the workspace query assumed
    const int row = 3 * num_classes;
    const bool vec = (hw % kPer == 0) && aligned16(pred) && aligned16(label);
    uint32_t* partial = (uint32_t*)workspace;
    dim3 grid(bpi, (unsigned)batch), block(kThreads);
#define AWSEG_FIOU(L, V) \
    hipLaunchKernelGGL((frame_iou_kernel<L, V>), grid, block, 0, s, pred, label, ignore_index, hw, num_classes, frame_row, n_rows, \
                       partial, oob)
    if (label_dtype == AWSEG_U8) { if (vec) AWSEG_FIOU(AWSEG_U8, true); else AWSEG_FIOU(AWSEG_U8, false); }
    else { if (vec) AWSEG_FIOU(AWSEG_I64, true); else AWSEG_FIOU(AWSEG_I64, false); }
#undef AWSEG_FIOU
    AWSEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_fold_kernel, dim3((unsigned)batch, (row + 63) / 64), dim3(kFoldSlices * 64), 0, s, partial, bpi, row,
                       frame_row, n_rows, table);
    AWSEG_LAUNCH_CHECK();
    return 0;
}

AWSEG_API int awseg_bootstrap_counts(const int64_t* table, const int32_t* slots, int64_t n, int64_t variants, int64_t width,
                                     int64_t n_slots, uint64_t seed, int64_t r0, int64_t replicates, int64_t* out, int64_t* oob,
                                     awseg_stream_t stream)
{
    if (!table || !slots || !out || !oob) return AWSEG_EINVAL;
    if (n < 1 || variants < 1 || replicates < 1 || width < 1 || n_slots < 1 || r0 < 0) return AWSEG_EINVAL;
    // int32 entry indices in the kernel; cells per replicate and the grid are int32 as well
    if (n > INT32_MAX || variants > INT32_MAX || n * variants > INT32_MAX) return AWSEG_ERANGE;
    if (width > INT32_MAX || n_slots > INT32_MAX || width * n_slots > INT32_MAX || replicates > INT32_MAX) return AWSEG_ERANGE;
    if (r0 > INT64_MAX - replicates) return AWSEG_ERANGE;
    hipLaunchKernelGGL(bootstrap_kernel, dim3((unsigned)replicates), dim3(kThreads), 0, awseg_s(stream), table, slots, (int)n,
                       (int)variants, (int)width, (int)n_slots, seed, r0, out, oob);
    AWSEG_LAUNCH_CHECK();
    return 0;
}
