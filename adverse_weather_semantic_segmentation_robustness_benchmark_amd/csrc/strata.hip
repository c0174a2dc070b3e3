// strata.hip — attribute a corrupted frame's errors to the pixels the corruption changed.
//
// awseg_change_strata: one uint8 stratum per pixel from the float32 frame and its clean twin: change = max over channels of
// |image - ref| * scale, stratum = the number of edges <= change.  25 B/px of traffic at three channels (2 x 3 x 4 in, 1 out) and a
// handful of compares: four pixels per lane from 16-byte loads and one packed 4-byte store when the rows allow, scalar otherwise.
//
// awseg_stratified_stats: a map scan (awseg_mapscan.h, DESIGN.md §10j: 16 pixels per lane, 16-byte loads or byte loads) of three or
// four maps; the stratum byte selects the counter row: per (slot, stratum) the C x C confusion matrix of the labelled pixels,
// the four clean / corrupted transitions, the agreeing pixels and the pixel count.  Strata are connected regions (a flake, a
// streak, the whole frame under fog), so a lane keeps the six small counters of its current stratum in registers and touches the
// per-block LDS histogram only when the stratum changes; confusion cells are merged into runs in the same way (measured against one
// LDS atomic per counter and pixel at 8 x 1024 x 2048: 0.045 against 0.146 ms on coherent maps, 0.048 against 0.047 ms on independent
// random ones; profiles/strata_kernel_bench_hip_events.log).  Blocks write uint32 partials, the shared fold adds them into the
// int64 counters: integer sums only.
#include "awseg_mapscan.h"
#include <float.h>

namespace {

constexpr int kChangeThreads = 256;
constexpr int kStatThreads = 512, kStatResident = 2;                       // two resident blocks per CU: the partials stay small
constexpr int kPer = kAwsegScanPer;                                        // pixels per lane per step (stratified_stats)
constexpr int kSmall = 6;                                                  // cc, cw, wc, ww, agree, pixels

struct change_args {
    float scale[4];
    float edges[AWSEG_MAX_STRATA - 1];
    int n_edges;
};

template <int CH>
__device__ __forceinline__ uint32_t change_stratum(const float (&a)[CH], const float (&b)[CH], const change_args& g)
{
    float m = 0.0f;
    bool nan = false;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const float d = a[c] - b[c];
        nan |= d != d;                                                     // explicit: a maximum would drop the NaN
        const float v = fabsf(d) * g.scale[c];
        if (v > m) m = v;
    }
    uint32_t s = 0;
#pragma unroll
    for (int e = 0; e < AWSEG_MAX_STRATA - 1; ++e) s += (e < g.n_edges && m >= g.edges[e]) ? 1u : 0u;
    return nan ? (uint32_t)AWSEG_STRATUM_NONE : s;
}

// grid = (blocks_per_image, B).  VEC: hw % 4 == 0, image and ref_images 16-byte aligned, out 4-byte aligned.
template <int CH, bool VEC>
__global__ __launch_bounds__(kChangeThreads)
void change_strata_kernel(const float* __restrict__ image, const float* __restrict__ ref_images, int n_refs, int64_t hw,
                          const int32_t* __restrict__ frame_ref, const change_args g, uint8_t* __restrict__ out,
                          int64_t* __restrict__ oob)
{
    const int64_t img = blockIdx.y;
    const int r = frame_ref[img];
    uint8_t* op = out + img * hw;
    const int64_t t0 = (int64_t)blockIdx.x * kChangeThreads + threadIdx.x, step = (int64_t)gridDim.x * kChangeThreads;
    if (r < 0 || r >= n_refs) {                                            // no clean twin: the frame is unmeasured
        if constexpr (VEC) {
            for (int64_t q = t0; q < hw / 4; q += step) reinterpret_cast<uint32_t*>(op)[q] = 0xFFFFFFFFu;
        } else {
            for (int64_t p = t0; p < hw; p += step) op[p] = (uint8_t)AWSEG_STRATUM_NONE;
        }
        if (r >= n_refs && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long*)oob, (unsigned long long)hw);
        return;
    }
    const float* ip = image + img * CH * hw;
    const float* rp = ref_images + (int64_t)r * CH * hw;
    if constexpr (VEC) {
        for (int64_t q = t0; q < hw / 4; q += step) {
            float4 a4[CH], b4[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                a4[c] = reinterpret_cast<const float4*>(ip + c * hw)[q];
                b4[c] = reinterpret_cast<const float4*>(rp + c * hw)[q];
            }
            float a[CH], b[CH];
            uint32_t packed = 0;
#pragma unroll
            for (int c = 0; c < CH; ++c) { a[c] = a4[c].x; b[c] = b4[c].x; }
            packed |= change_stratum<CH>(a, b, g);
#pragma unroll
            for (int c = 0; c < CH; ++c) { a[c] = a4[c].y; b[c] = b4[c].y; }
            packed |= change_stratum<CH>(a, b, g) << 8;
#pragma unroll
            for (int c = 0; c < CH; ++c) { a[c] = a4[c].z; b[c] = b4[c].z; }
            packed |= change_stratum<CH>(a, b, g) << 16;
#pragma unroll
            for (int c = 0; c < CH; ++c) { a[c] = a4[c].w; b[c] = b4[c].w; }
            packed |= change_stratum<CH>(a, b, g) << 24;
            reinterpret_cast<uint32_t*>(op)[q] = packed;
        }
    } else {
        for (int64_t p = t0; p < hw; p += step) {
            float a[CH], b[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) { a[c] = ip[c * hw + p]; b[c] = rp[c * hw + p]; }
            op[p] = (uint8_t)change_stratum<CH>(a, b, g);
        }
    }
}

// The six small counters of one stratum, kept in registers while a lane stays inside it.
struct small_run {
    int s = -1;
    uint32_t n[kSmall] = { 0, 0, 0, 0, 0, 0 };
    __device__ __forceinline__ void flush(uint32_t* hist, int row, int bins)
    {
        if (s < 0) return;
        uint32_t* dst = hist + s * row + bins;
#pragma unroll
        for (int i = 0; i < kSmall; ++i) { if (n[i]) atomicAdd(&dst[i], n[i]); n[i] = 0; }
    }
};

// grid = (blocks_per_image, B); block x of image y writes partial[(y * gridDim.x + x)][(K + 1) * (C * C + 6)].
// VEC: hw % 16 == 0 and pred, stratum, label and ref_maps (when given) 16-byte aligned; else byte loads.  PAIRED: ref_maps given.
template <int LDT, bool VEC, bool PAIRED>
__global__ __launch_bounds__(kStatThreads)
void stratified_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ stratum, int K,
                       const uint8_t* __restrict__ ref_maps, int n_refs, int64_t hw, const int32_t* __restrict__ frame_ref,
                       const void* __restrict__ label, int ignore_index, int C, uint32_t* __restrict__ partial,
                       int64_t* __restrict__ oob)
{
    extern __shared__ uint32_t hist[];
    const int bins = C * C, row = bins + kSmall, total = (K + 1) * row;
    awseg_scan_zero<kStatThreads>(hist, total);
    __syncthreads();
    const int64_t img = blockIdx.y;
    const int r = PAIRED ? frame_ref[img] : 0;
    uint32_t bad = 0;
    if (r >= 0 && r < n_refs) {
        const uint8_t* pp = pred + img * hw;
        const uint8_t* sp = stratum + img * hw;
        const uint8_t* rp = PAIRED ? ref_maps + (int64_t)r * hw : nullptr;
        const int64_t nchunk = (hw + kPer - 1) / kPer;
        small_run sm;
        awseg_run<int> run;                                                // run of equal confusion cells (stratum included)
        const auto flush = [&](int idx, uint32_t n) { atomicAdd(&hist[idx], n); };
        for (int64_t ch = (int64_t)blockIdx.x * kStatThreads + threadIdx.x; ch < nchunk; ch += (int64_t)gridDim.x * kStatThreads) {
            const int64_t base = ch * kPer;
            int pv[kPer], sv[kPer], rv[kPer];
            int64_t lv[kPer];
            const awseg_map16 pm{ pp, pv }, smap{ sp, sv }, rm{ rp, rv };
            if constexpr (PAIRED) awseg_load_chunk16<LDT, VEC>(label, img * hw, base, hw, ignore_index, lv, pm, smap, rm);
            else awseg_load_chunk16<LDT, VEC>(label, img * hw, base, hw, ignore_index, lv, pm, smap);
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                if (!VEC && base + k >= hw) break;
                const int pk = pv[k], rk = PAIRED ? rv[k] : 0;
                if (pk >= C || rk >= C) { ++bad; continue; }               // a map value no argmax over C classes produces
                const int s = sv[k] < K ? sv[k] : K;                       // >= K (AWSEG_STRATUM_NONE included): the unmeasured row
                if (s != sm.s) { sm.flush(hist, row, bins); sm.s = s; }
                sm.n[5] += 1;
                if constexpr (PAIRED) sm.n[4] += pk == rk;
                const int64_t t = lv[k];
                if (t != ignore_index && t >= 0 && t < C) {
                    run.add(s * row + (int)t * C + pk, flush);
                    if constexpr (PAIRED) {
                        const uint32_t rc = (int64_t)rk == t, vc = (int64_t)pk == t;
                        sm.n[0] += rc & vc; sm.n[1] += rc & (vc ^ 1u); sm.n[2] += (rc ^ 1u) & vc; sm.n[3] += (rc ^ 1u) & (vc ^ 1u);
                    }
                }
            }
        }
        run.finish(flush);
        sm.flush(hist, row, bins);
    } else if (r >= n_refs) {
        awseg_scan_row_outside(hw, oob);                                   // a row index the reference maps do not have: frame not counted
    }
    awseg_scan_count_bad(bad, oob);
    awseg_scan_store<kStatThreads>(hist, total, partial);
}

int strata_blocks_per_image(int64_t hw, int64_t batch) { return awseg_blocks_per_image((hw + kPer - 1) / kPer, kStatThreads, batch, kStatResident); }

}  // namespace

AWSEG_API int awseg_change_strata(const float* image, const float* ref_images, int n_refs, int64_t batch, int channels, int64_t hw,
                                  const int32_t* frame_ref, const float* scale, const float* edges, int n_strata, uint8_t* out,
                                  int64_t* oob, awseg_stream_t stream)
{
    if (!image || !ref_images || !frame_ref || !scale || !edges || !out || !oob) return AWSEG_EINVAL;
    if (n_refs < 1 || batch < 0 || hw < 1 || channels < 1 || channels > 4) return AWSEG_EINVAL;
    if (n_strata < 2 || n_strata > AWSEG_MAX_STRATA) return AWSEG_EINVAL;
    change_args g = {};
    g.n_edges = n_strata - 1;
    for (int e = 0; e < g.n_edges; ++e) {
        if (!(edges[e] >= 0.0f && edges[e] <= FLT_MAX) || (e && !(edges[e] > edges[e - 1]))) return AWSEG_EINVAL;
        g.edges[e] = edges[e];
    }
    for (int c = 0; c < channels; ++c) {
        if (!(scale[c] > 0.0f && scale[c] <= FLT_MAX)) return AWSEG_EINVAL;   // 0 x inf would make a NaN of an infinite change
        g.scale[c] = scale[c];
    }
    if (batch > 65535 || hw > INT32_MAX) return AWSEG_ERANGE;                  // grid.y
    if (batch == 0) return 0;
    hipStream_t s = awseg_s(stream);
    const bool vec = (hw % 4 == 0) && awseg_aligned(image, 16) && awseg_aligned(ref_images, 16) && awseg_aligned(out, 4);
    const int64_t items = vec ? hw / 4 : hw;
    int64_t cap = (AWSEG_CUS * 8 + batch - 1) / batch;
    const int bpi = awseg_grid_1d(items, kChangeThreads, (int)(cap < 1 ? 1 : cap));
    dim3 grid(bpi, (unsigned)batch), block(kChangeThreads);
#define AWSEG_CHG(CH, V) \
    hipLaunchKernelGGL((change_strata_kernel<CH, V>), grid, block, 0, s, image, ref_images, n_refs, hw, frame_ref, g, out, oob)
#define AWSEG_CHG_CH(CH) do { if (vec) AWSEG_CHG(CH, true); else AWSEG_CHG(CH, false); } while (0)
    switch (channels) {
    case 1: AWSEG_CHG_CH(1); break;
    case 2: AWSEG_CHG_CH(2); break;
    case 3: AWSEG_CHG_CH(3); break;
    default: AWSEG_CHG_CH(4); break;
    }
#undef AWSEG_CHG_CH
#undef AWSEG_CHG
    AWSEG_LAUNCH_CHECK();
    return 0;
}

AWSEG_API int64_t awseg_strata_workspace(int64_t batch, int num_classes, int64_t hw, int n_strata)
{
    if (batch < 1) batch = 1;
    if (hw < 1) hw = 1;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) num_classes = AWSEG_MAX_CLASSES;
    if (n_strata < 1 || n_strata > AWSEG_MAX_STRATA) n_strata = AWSEG_MAX_STRATA;
    return (int64_t)strata_blocks_per_image(hw, batch) * batch * (n_strata + 1) * (num_classes * num_classes + kSmall) *
           (int64_t)sizeof(uint32_t);
}

AWSEG_API int awseg_stratified_stats(const uint8_t* pred, const void* label, int label_dtype, int ignore_index,
                                     const uint8_t* stratum, int n_strata, const uint8_t* ref_maps, int n_refs,
                                     const int32_t* frame_ref, int64_t batch, int64_t hw, int num_classes, const int32_t* cond,
                                     int64_t* stats, int n_slots, int64_t* oob, void* workspace, awseg_stream_t stream)
{
    if (!pred || !label || !stratum || !stats || !oob || !workspace) return AWSEG_EINVAL;
    if ((ref_maps == nullptr) != (frame_ref == nullptr)) return AWSEG_EINVAL;
    if (batch < 1 || hw < 1 || n_slots < 1 || (ref_maps && n_refs < 1)) return AWSEG_EINVAL;
    if (num_classes < 1 || num_classes > AWSEG_MAX_CLASSES) return AWSEG_EINVAL;
    if (n_strata < 1 || n_strata > AWSEG_MAX_STRATA) return AWSEG_EINVAL;
    if (label_dtype != AWSEG_U8 && label_dtype != AWSEG_I64) return AWSEG_EINVAL;
    if (batch > 65535 || hw > INT32_MAX) return AWSEG_ERANGE;                 // grid.y; uint32 per-block partials
    hipStream_t s = awseg_s(stream);
    const int bpi = strata_blocks_per_image(hw, batch);                        // same count the workspace query assumed
    const int row = (n_strata + 1) * (num_classes * num_classes + kSmall);
    const bool paired = ref_maps != nullptr;
    if (!paired) n_refs = 1;                                                   // every frame is counted
    const bool vec = (hw % kPer == 0) && awseg_aligned(pred, 16) && awseg_aligned(stratum, 16) && awseg_aligned(label, 16) &&
                     (!paired || awseg_aligned(ref_maps, 16));
    uint32_t* partial = (uint32_t*)workspace;
    dim3 grid(bpi, (unsigned)batch), block(kStatThreads);
    const size_t lds = (size_t)row * sizeof(uint32_t);
    awseg_by_label(label_dtype, [&](auto L) { awseg_by_flag(vec, [&](auto V) { awseg_by_flag(paired, [&](auto P) {
        hipLaunchKernelGGL((stratified_kernel<decltype(L)::value, decltype(V)::value, decltype(P)::value>), grid, block, lds, s, pred,
                           stratum, n_strata, ref_maps, n_refs, hw, frame_ref, label, ignore_index, num_classes, partial, oob);
    }); }); });
    AWSEG_LAUNCH_CHECK();
    return awseg_fold_u32_launch(partial, batch, bpi, row, cond, n_slots, true, stats, s);
}
