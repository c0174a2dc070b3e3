// awseg_mapscan.h — the shared core of the label-map counter passes: confusion_kernel (metrics.hip),
// consistency_kernel, stratified_kernel (strata.hip), frame_iou_kernel (bootstrap.hip); boundary_kernel shares the block prologue, epilogue, grid rule and fold.
//
// A scan gives every lane 16 consecutive pixels of each uint8 map (one 16-byte load per map when hw % 16 == 0 and every base is
// 16-byte aligned, byte loads otherwise), merges equal histogram cells into runs in registers before they touch the per-block LDS
// histogram, and writes the histogram as uint32 partials [img][blocks_per_image][row] that one fold kernel (metrics.hip) adds into
// int64 counters: integer sums only, so the counts do not depend on grid shape, batch split or rank count.
#pragma once
#include "awseg_common.h"

constexpr int kAwsegScanPer = 16;                                         // pixels per lane per step

__device__ __forceinline__ void awseg_unpack16(const uint4 q, int (&v)[kAwsegScanPer])
{
    const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
    for (int k = 0; k < kAwsegScanPer; ++k) v[k] = (int)((w[k >> 2] >> ((k & 3) * 8)) & 0xFF);
}

// Elements first + base .. first + base + 15 of a uint8 or int64 label map whose frame starts at element `first` and has hw pixels.
// VEC: 16-byte loads (one, or eight longlong2), the address 16-byte aligned and base + 16 <= hw; else element loads, `fill` past hw.
template <int LDT, bool VEC>
__device__ __forceinline__ void awseg_load_label16(const void* __restrict__ label, int64_t first, int64_t base, int64_t hw,
                                                   int64_t fill, int64_t (&v)[kAwsegScanPer])
{
    if constexpr (VEC && LDT == AWSEG_U8) {
        int l8[kAwsegScanPer];
        awseg_unpack16(*reinterpret_cast<const uint4*>((const uint8_t*)label + first + base), l8);
#pragma unroll
        for (int k = 0; k < kAwsegScanPer; ++k) v[k] = l8[k];
    } else if constexpr (VEC) {
        const longlong2* lp = reinterpret_cast<const longlong2*>((const int64_t*)label + first + base);
#pragma unroll
        for (int k = 0; k < kAwsegScanPer / 2; ++k) { const longlong2 q = lp[k]; v[2 * k] = q.x; v[2 * k + 1] = q.y; }
    } else {
#pragma unroll
        for (int k = 0; k < kAwsegScanPer; ++k) v[k] = base + k < hw ? awseg_ld_label<LDT>(label, first + base + k) : fill;
    }
}

// One chunk of a scan: pixels base .. base + 15 of each uint8 map (frame base p, values into v) and of the label map.
// VEC: one 16-byte load per map; else byte loads, 0 and ignore_index past hw, every map in ONE loop over the pixels (a loop per
// map costs the three-map scans 15 VGPRs and a wave of occupancy).
struct awseg_map16 { const uint8_t* p; int (&v)[kAwsegScanPer]; };
template <int LDT, bool VEC, typename... Maps>
__device__ __forceinline__ void awseg_load_chunk16(const void* __restrict__ label, int64_t first, int64_t base, int64_t hw,
                                                   int ignore_index, int64_t (&lv)[kAwsegScanPer], Maps... maps)
{
    if constexpr (VEC) {
        (awseg_unpack16(*reinterpret_cast<const uint4*>(maps.p + base), maps.v), ...);
        awseg_load_label16<LDT, true>(label, first, base, hw, ignore_index, lv);
    } else {
#pragma unroll
        for (int k = 0; k < kAwsegScanPer; ++k) {
            const bool in = base + k < hw;
            ((maps.v[k] = in ? (int)maps.p[base + k] : 0), ...);
            lv[k] = in ? awseg_ld_label<LDT>(label, first + base + k) : (int64_t)ignore_index;
        }
    }
}

// A run of equal histogram cells: add(key, flush) extends the run or hands the finished one to flush(key, count) and starts
// the next; finish(flush) hands over what is left.  Key is anything with ==: a cell index, a pair of classes.
template <typename Key>
struct awseg_run {
    Key key = Key();
    uint32_t n = 0;
    template <typename Flush> __device__ __forceinline__ void add(const Key k, Flush&& flush)
    {
        if (k == key) { ++n; return; }                                    // n == 0: the first of a run whose key happens to be `key`
        if (n) flush(key, n);
        key = k; n = 1;
    }
    template <typename Flush> __device__ __forceinline__ void finish(Flush&& flush)
    {
        if (n) flush(key, n);
        n = 0;
    }
};

// Block prologue: zero the LDS histogram.  The caller's next __syncthreads() orders it before the first add.
template <int THREADS> __device__ __forceinline__ void awseg_scan_zero(uint32_t* hist, int cells)
{
    for (int i = threadIdx.x; i < cells; i += THREADS) hist[i] = 0u;
}
// A frame whose row index lies behind the buffer is not read: its hw pixels are counted into oob, once.
__device__ __forceinline__ void awseg_scan_row_outside(int64_t hw, int64_t* oob)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long*)oob, (unsigned long long)hw);
}
// Block epilogue: the lanes' counts of values no map may hold go to oob once per wave ...
__device__ __forceinline__ void awseg_scan_count_bad(uint32_t bad, int64_t* oob)
{
    bad = awseg_wave_sum_u32(bad);
    if ((threadIdx.x & (AWSEG_WAVE - 1)) == 0 && bad) atomicAdd((unsigned long long*)oob, (unsigned long long)bad);
}
// ... and block x of image y stores its histogram as partial[(y * gridDim.x + x)][cells].
template <int THREADS> __device__ __forceinline__ void awseg_scan_store(const uint32_t* hist, int cells, uint32_t* __restrict__ partial)
{
    __syncthreads();
    uint32_t* dst = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * cells;
    for (int i = threadIdx.x; i < cells; i += THREADS) dst[i] = hist[i];
}

// Fold uint32 partials [images][blocks_per_image][row] into int64 rows dst[n_rows][row] (metrics.hip; returns the launch error).
// total = true, the condition slots: every image goes to row 0 and, where 0 <= index[img] < n_rows - 1, to row 1 + index[img]
// (index may be null).  total = false, a table: image img goes to row index[img] where that is in [0, n_rows), nowhere otherwise.
// slices: the waves of a fold block, each sums that share of an image's partials; 16 or 4, anything else is AWSEG_EINVAL.
int awseg_fold_u32_launch(const uint32_t* partial, int64_t images, int blocks_per_image, int row, const int32_t* index,
                          int64_t n_rows, bool total, int64_t* dst, hipStream_t stream, int slices = 16);
