// consistency.hip — prediction consistency of a corrupted frame against the prediction of its clean frame (the paired severity
// sweep): per condition slot, the C x C agreement matrix A[ref class][variant class] over every pixel and the four
// correct / wrong transitions over the labelled pixels.
//
// A 2-3 B/px map scan (two uint8 maps + the label map; awseg_mapscan.h).  Clean and corrupted predictions agree over
// large connected regions, so the 16 agreement indices of a lane are merged into runs in registers before they touch the per-block
// LDS histogram (one ds_add per run: one per 16 pixels in the common case); the four transition counters never touch LDS per pixel:
// they live in registers, are summed over the wave and added once per wave.
#include "awseg_mapscan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kResident = 4;                                              // blocks per CU the grid is capped at (a 2-3 B/px scan)
constexpr int kPer = kAwsegScanPer;
constexpr int kRowMax = AWSEG_MAX_CLASSES * AWSEG_MAX_CLASSES + 4;

// grid = (blocks_per_image, B); block x of image y writes partial[(y * gridDim.x + x)][C * C + 4].
// VEC: hw % 16 == 0 and pred, ref_maps and label 16-byte aligned (every row base then is); else byte loads.
template <int LDT, bool VEC>
__global__ __launch_bounds__(kThreads)
void consistency_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ ref_maps, int n_refs, int64_t hw,
                        const int32_t* __restrict__ frame_ref, const void* __restrict__ label, int ignore_index, int C,
                        uint32_t* __restrict__ partial, int64_t* __restrict__ oob)
{
    __shared__ uint32_t hist[kRowMax];
    const int bins = C * C, row = bins + 4;
    awseg_scan_zero<kThreads>(hist, row);
    __syncthreads();
    const int64_t img = blockIdx.y;
    const int r = frame_ref[img];
    // transitions over labelled pixels: both correct, reference correct + variant wrong, reference wrong + variant correct, both wrong
    uint32_t t_cc = 0, t_cw = 0, t_wc = 0, t_ww = 0, bad = 0;
    if (r >= 0 && r < n_refs) {
        const uint8_t* pp = pred + img * hw;
        const uint8_t* rp = ref_maps + (int64_t)r * hw;
        const int64_t nchunk = (hw + kPer - 1) / kPer;
        const auto flush = [&](int idx, uint32_t n) { atomicAdd(&hist[idx], n); };
        for (int64_t ch = (int64_t)blockIdx.x * kThreads + threadIdx.x; ch < nchunk; ch += (int64_t)gridDim.x * kThreads) {
            const int64_t base = ch * kPer;
            int pv[kPer], rv[kPer];
            int64_t lv[kPer];
            awseg_load_chunk16<LDT, VEC>(label, img * hw, base, hw, ignore_index, lv, awseg_map16{ pp, pv }, awseg_map16{ rp, rv });
            awseg_run<int> run;
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                if (!VEC && base + k >= hw) break;
                const int pk = pv[k], rk = rv[k];
                if (pk >= C || rk >= C) { ++bad; continue; }             // a map value no argmax over C classes produces
                run.add(rk * C + pk, flush);
                const int64_t t = lv[k];
                if (t != ignore_index && t >= 0 && t < C) {
                    const uint32_t rc = (int64_t)rk == t, vc = (int64_t)pk == t;
                    t_cc += rc & vc; t_cw += rc & (vc ^ 1u); t_wc += (rc ^ 1u) & vc; t_ww += (rc ^ 1u) & (vc ^ 1u);
                }
            }
            run.finish(flush);
        }
    } else if (r >= n_refs) {
        awseg_scan_row_outside(hw, oob);                                  // a row index the reference maps do not have: frame not counted
    }
    t_cc = awseg_wave_sum_u32(t_cc); t_cw = awseg_wave_sum_u32(t_cw); t_wc = awseg_wave_sum_u32(t_wc); t_ww = awseg_wave_sum_u32(t_ww);
    if ((threadIdx.x & (AWSEG_WAVE - 1)) == 0) {
        if (t_cc) atomicAdd(&hist[bins + 0], t_cc);
        if (t_cw) atomicAdd(&hist[bins + 1], t_cw);
        if (t_wc) atomicAdd(&hist[bins + 2], t_wc);
        if (t_ww) atomicAdd(&hist[bins + 3], t_ww);
    }
    awseg_scan_count_bad(bad, oob);
    awseg_scan_store<kThreads>(hist, row, partial);
}

int cons_blocks_per_image(int64_t hw, int64_t batch) { return awseg_blocks_per_image((hw + kPer - 1) / kPer, kThreads, batch, kResident); }

}  // namespace

AWSEG_API int64_t awseg_consistency_workspace(int64_t batch, int num_classes, int64_t hw)
{
    if (batch < 1) batch = 1;
    if (hw < 1) hw = 1;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) num_classes = AWSEG_MAX_CLASSES;
    return (int64_t)cons_blocks_per_image(hw, batch) * batch * (num_classes * num_classes + 4) * (int64_t)sizeof(uint32_t);
}

AWSEG_API int awseg_prediction_consistency(const uint8_t* pred, const uint8_t* ref_maps, int n_refs, int64_t batch, int64_t hw,
                                           const int32_t* frame_ref, const void* label, int label_dtype, int ignore_index,
                                           int num_classes, const int32_t* cond, int64_t* stats, int n_slots, int64_t* oob,
                                           void* workspace, awseg_stream_t stream)
{
    if (!pred || !ref_maps || !frame_ref || !label || !stats || !oob || !workspace) return AWSEG_EINVAL;
    if (n_refs < 1 || batch < 1 || hw < 1 || n_slots < 1) return AWSEG_EINVAL;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    if (batch > 65535 || hw > INT32_MAX) return AWSEG_ERANGE;                 // grid.y; uint32 per-block partials
    hipStream_t s = awseg_s(stream);
    const int bpi = cons_blocks_per_image(hw, batch);                          // same count the workspace query assumed
    const int row = num_classes * num_classes + 4;
    const bool vec = (hw % kPer == 0) && awseg_aligned(pred, 16) && awseg_aligned(ref_maps, 16) && awseg_aligned(label, 16);
    uint32_t* partial = (uint32_t*)workspace;
    dim3 grid(bpi, (unsigned)batch), block(kThreads);
    awseg_by_label(label_dtype, [&](auto L) { awseg_by_flag(vec, [&](auto V) {
        hipLaunchKernelGGL((consistency_kernel<decltype(L)::value, decltype(V)::value>), grid, block, 0, s, pred, ref_maps, n_refs, hw,
                           frame_ref, label, ignore_index, num_classes, partial, oob);
    }); });
    AWSEG_LAUNCH_CHECK();
    return awseg_fold_u32_launch(partial, batch, bpi, row, cond, n_slots, true, stats, s);
}
