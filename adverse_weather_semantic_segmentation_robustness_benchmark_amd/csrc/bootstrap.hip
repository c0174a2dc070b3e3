// bootstrap.hip — the two device passes of the frame bootstrap: per-frame IoU counters, and their replicate sums
// under a paired resampling of the source frames.
//
// awseg_frame_iou_counts is a map scan (awseg_mapscan.h) of the prediction and the label map: a lane merges the
// (label, prediction) pairs of its 16 pixels into runs in registers and touches the per-block LDS row [C intersection | C label |
// C prediction] once per run.  Blocks write uint32 partials; the shared fold adds them into the int64 table row frame_row[b] names.
//
// awseg_bootstrap_counts runs one block per replicate: the replicate's draws (Philox4x32-7, stream kBootStream, index =
// mulhi32(word, n)) are staged in LDS once, kBootDraws at a time, then every thread owns output cells (slot, column) and walks the
// draws — no atomics, one fixed order, 64-bit accumulators; slot 0 is folded from the block's own cells at the end.
#include "awseg_mapscan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kResident = 4;                                              // blocks per CU the scan's grid is capped at (2 B/px)
constexpr int kFoldSlices = 4;                                            // a row of 3 C counters: four waves per fold block
constexpr int kPer = kAwsegScanPer;
constexpr int kRowMax = 3 * AWSEG_MAX_CLASSES;
constexpr uint32_t kBootStream = 0x0B07u;                                 // weather.hip owns 0x0F06, 0x0F07, 0x0A17, 0x0DE5
constexpr int kBootDraws = AWSEG_BOOTSTRAP_STAGED_DRAWS;                  // draws staged in LDS per pass (16 KB); larger n is chunked
static_assert(kBootDraws % 4 == 0, "a Philox call fills four consecutive draws");

struct iou_key {                                                          // a (label, prediction) pair
    int t = -1, p = -1;
    __device__ __forceinline__ bool operator==(const iou_key& o) const { return t == o.t && p == o.p; }
};

// grid = (blocks_per_image, B); block x of image y writes partial[(y * gridDim.x + x)][3 C].
// VEC: hw % 16 == 0 and pred and label 16-byte aligned (every row base then is); else byte loads.
template <int LDT, bool VEC>
__global__ __launch_bounds__(kThreads)
void frame_iou_kernel(const uint8_t* __restrict__ pred, const void* __restrict__ label, int ignore_index, int64_t hw, int C,
                      const int32_t* __restrict__ frame_row, int64_t n_rows, uint32_t* __restrict__ partial, int64_t* __restrict__ oob)
{
    __shared__ uint32_t hist[kRowMax];
    const int row = 3 * C;
    awseg_scan_zero<kThreads>(hist, row);
    __syncthreads();
    const int64_t img = blockIdx.y;
    const int64_t r = frame_row[img];
    uint32_t bad = 0;
    if (r >= 0 && r < n_rows) {
        const uint8_t* pp = pred + img * hw;
        const int64_t nchunk = (hw + kPer - 1) / kPer;
        const auto flush = [&](const iou_key& key, uint32_t n) {
            atomicAdd(&hist[C + key.t], n);
            atomicAdd(&hist[2 * C + key.p], n);
            if (key.t == key.p) atomicAdd(&hist[key.t], n);
        };
        for (int64_t ch = (int64_t)blockIdx.x * kThreads + threadIdx.x; ch < nchunk; ch += (int64_t)gridDim.x * kThreads) {
            const int64_t base = ch * kPer;
            int pv[kPer];
            int64_t lv[kPer];
            awseg_load_chunk16<LDT, VEC>(label, img * hw, base, hw, ignore_index, lv, awseg_map16{ pp, pv });
            awseg_run<iou_key> run;
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                if (!VEC && base + k >= hw) break;
                const int pk = pv[k];
                const int64_t t = lv[k];
                const bool labelled = t != ignore_index && t >= 0 && t < C;
                if (pk >= C) ++bad;                                       // a map value no argmax over C classes produces
                if (!labelled && t != ignore_index) ++bad;                // a label that is neither a class nor the ignore value
                if (!labelled || pk >= C) continue;
                run.add(iou_key{ (int)t, pk }, flush);
            }
            run.finish(flush);
        }
    } else if (r >= n_rows) {
        awseg_scan_row_outside(hw, oob);                                  // a row the table does not have: frame not counted
    }
    awseg_scan_count_bad(bad, oob);
    awseg_scan_store<kThreads>(hist, row, partial);
}

int fiou_blocks_per_image(int64_t hw, int64_t batch) { return awseg_blocks_per_image((hw + kPer - 1) / kPer, kThreads, batch, kResident); }

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
    const bool vec = (hw % kPer == 0) && awseg_aligned(pred, 16) && awseg_aligned(label, 16);
    uint32_t* partial = (uint32_t*)workspace;
    dim3 grid(bpi, (unsigned)batch), block(kThreads);
    awseg_by_label(label_dtype, [&](auto L) { awseg_by_flag(vec, [&](auto V) {
        hipLaunchKernelGGL((frame_iou_kernel<decltype(L)::value, decltype(V)::value>), grid, block, 0, s, pred, label, ignore_index, hw,
                           num_classes, frame_row, n_rows, partial, oob);
    }); });
    AWSEG_LAUNCH_CHECK();
    // frames whose row is outside [0, n_rows) wrote zero partials and are skipped by the fold as well; two frames may name one row
    return awseg_fold_u32_launch(partial, batch, bpi, row, frame_row, n_rows, false, table, s, kFoldSlices);
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
