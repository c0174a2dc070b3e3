// awseg_logitscan.h — the shared pieces of the passes that read float32 logits [B][C][hw], used by the combine,
// ECE and one-pass statistics kernels of metrics.hip.
//
// The logit passes promise each other bit identity (the temperature grid's bins at t == 1 are the ECE bins, the failure scores are the
// one-pass statistics' expressions).  An expression is written here once only where its users keep their registers, scratch, LDS
// and occupancy (profiles/logitscan_resource_usage.log) and their speed; tgrid_kernel (calib.hip) and failure_kernel (failure.hip)
// keep their own copies of the same text, and DESIGN.md §10k gives the figures that decided it.  Built with -ffp-contract=off like
// its users, so each operation rounds on its own.
#pragma once
#include "awseg_common.h"

// The ensemble logit of one class: MODE 0 weighted (w0*x, w1*y, +), MODE 2 mean ((x+y), /2), then /T when has_t — each operation
// rounded separately (PKG/models/model.py:443-462).
template <int MODE>
__device__ __forceinline__ float awseg_combine(float x, float y, float w0, float w1, bool has_t, float T)
{
    static_assert(MODE == 0 || MODE == 2, "weighted or mean");
    float r;
    if (MODE == 0) { const float u = w0 * x; const float q = w1 * y; r = u + q; }
    else { const float u = x + y; r = u / 2.f; }
    if (has_t) r = r / T;
    return r;
}

// v = a lane's PX consecutive floats of one class plane (PX 4 / 2: one 16- / 8-byte load, the address aligned to it; 1: a scalar
// load); zeros, and no load, when the lane is past the end (live == false).
template <int PX> __device__ __forceinline__ void awseg_load_px(const float* plane, bool live, float (&v)[PX])
{
    if constexpr (PX == 1) v[0] = live ? plane[0] : 0.f;
    else {
        typedef float lvec __attribute__((ext_vector_type(PX)));
        const lvec q = live ? *reinterpret_cast<const lvec*>(plane) : (lvec)(0.f);
#pragma unroll
        for (int k = 0; k < PX; ++k) v[k] = q[k];
    }
}

// First maximum: take v when v > best (a NaN never wins, an earlier class keeps a tie) — what the ECE of single logits, the
// calibration part of the one-pass statistics and the failure scores mean by argmax.  torch's rule is awseg_amax_step.
__device__ __forceinline__ void awseg_first_max_step(float v, int c, float& best, int& bi)
{
    if (v > best) { best = v; bi = c; }
}
