// awseg_split.h — the device primitives the matrix-core kernels share (gemm_split.hip, gemm_split3.hip, attn.hip, wino.hip,
// wino_split.hip, mixffn.hip, the classifier head of heads.hip): vector types, the LDS address cast and the 16-byte LDS-DMA, the
// power-of-two helpers of the range guards, the bf16 pack and the f16 hi / lo operand split in its five flavours.
//
// THE SPLIT SCHEME.  v_mfma_f32_32x32x16_f16 issues 16x the multiply-adds per cycle of the float32-input MFMA, and a float32
// product is three f16 products once both operands are carried as a high and a low part:
//     x = xh + xl,   xh = f16(x) (11 significant bits),   xl = f16(x - xh) (the next 11; x - xh is exact in float32)
//     x * y = xh*yh + xh*yl + xl*yh                        (+ xl*yl = O(2^-22 |x y|), below float32 rounding noise, dropped)
// Every f16 product is exact in the float32 accumulator and the accumulation is float32, so the result differs from a float32
// product by operand rounding at 2^-22 instead of 2^-24: the 22-BIT CLAIM.  It holds while xl is a NORMAL f16 number.  Unscaled,
// that is |x| >= 2^-3 (below it the error is an absolute 2^-25); a kernel that cannot promise it either scales the residual,
// xl = f16((x - xh) * kLoScale), and folds kLoInv back in through a second accumulator (|x| < 2^15 then: the scaled flavour), or
// multiplies the operand by a power of two before it is split (the prescaled flavour).  The range guards of the kernels (each
// described in its own file) move a tensor that leaves those bounds back inside with an exact power of two.
//
// THE WAIT-STATE RULE.  On gfx950 a vector instruction's result needs two wait states before an MFMA reads the register as an
// operand.  hipcc pads that hazard for instructions it emitted itself and NOT behind inline asm, so a split written in asm whose
// result may go straight into an MFMA operand register ends in `s_nop 1`.  The flavours without it are for results that reach the
// matrix pipe through LDS (or memory); reusing one for a register operand gives wrong answers, not a compile error.
//
//   flavour                     high part       residual            asm ends in s_nop 1   used by
//   split_scaled_rtz            cvt_pkrtz       x kLoScale, RTZ     (plain C++)           gemm_split.hip (activations at staging, weights),
//                                                                                         attn.hip (q, k, v): operands of any magnitude
//                                                                                         below 2^15 keep 22 bits; two accumulators
//   split_unscaled_lds          cvt_pkrtz       v_fma_mix, as is    no                    wino_split.hip (V, written to LDS), heads.hip (W2
//                                                                                         to LDS; its T, horizontal weights and GEMM-1
//                                                                                         accumulators stay in registers: kept as found)
//   split_unscaled_mfma         cvt_pkrtz       v_fma_mix, as is    yes                   attn.hip (the probabilities, pre-scaled to be normal
//                                                                                         f16: straight into the PV product)
//   split_unscaled_mfma_fused   cvt_pkrtz in    v_fma_mix, as is    yes                   mixffn.hip (LayerNorm and GELU outputs, straight into
//                               the asm block                                             fc1 / fc2; one block keeps the three together)
//   split_prescaled_rne_mfma    v_fma_mix of    v_fma_mix, as is    yes                   gemm_split3.hip (fragments read from the LDS-DMA image;
//                               x s, nearest                                              one accumulator, so s = 2^4 stands in for kLoScale)
// Merging flavours changes rounding or schedules: each kernel's file says what was measured with the one it uses.
#pragma once
#include "awseg_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));

constexpr float kLoScale = 2048.0f, kLoInv = 1.0f / 2048.0f;     // scale of the scaled residual and its inverse

// ---- LDS address and LDS-DMA
// byte address of p inside the workgroup's LDS (what m0 and the ds_ instructions count in)
__device__ __forceinline__ uint32_t lds_addr(const void* p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
// 16 bytes per lane global -> LDS through a buffer descriptor (buffer_load_dwordx4 ... lds), no registers in between: lane l's
// bytes land at lds_base + 16 * l.  lds_base goes through m0 and must be WAVE-UNIFORM (a scalar register: readfirstlane what
// is computed from a lane id); the s_nop is the wait state m0 needs between its write and the load.  Source address = descriptor
// base + per-lane 32-bit byte offset voff + scalar byte offset soff; the hardware RANGE CHECK compares voff alone with the
// descriptor's size and an out-of-range lane reads zeros — that is the zero padding of the convolutions and the "rows past M"
// of the GEMMs (0x80000000 is the offset no descriptor covers), with no 64-bit address arithmetic per lane.
// Inline asm on purpose: the LDS-DMA builtins make hipcc treat every later ds_read as possibly aliasing the DMA's LDS write and
// wait vmcnt(0) right after the first MFMA of a step, which serialises the copy with the math.  The kernels order the copy
// themselves: an s_waitcnt vmcnt before the barrier in front of the first read of what was copied.
// The "memory" clobber keeps hipcc from moving ordinary loads and stores across the instruction.
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff, uint32_t lds_base)
{
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" : : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_base) : "m0", "memory");
}
// The same WITHOUT the "memory" clobber, for wino_split.hip alone: that kernel's schedule was tuned with hipcc free to move
// its LDS traffic across the DMA issue, and the clobbered form changes its device code (the other kernels' is the same either
// way).  Safe there because every read of a patch sits behind an `s_waitcnt vmcnt(n)` that does carry the clobber
// (vm_wait_keep_patch_and / vm_wait_keep / vm_wait_all) and the __syncthreads() that follows it — in front of the first
// transform, at the end of slot A of every chunk and behind the chunk loop — and a ring slot is written again only behind the
// barrier that ends the slot in which it was last read.  Moving wino_split.hip to lds_dma16 is a performance change: measure it.
__device__ __forceinline__ void lds_dma16_unfenced(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff, uint32_t lds_base)
{
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" : : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_base) : "m0");
}

// ---- powers of two and the range guards' exponents
__device__ __forceinline__ float pow2f(int e) { return __builtin_bit_cast(float, (unsigned)(127 + e) << 23); }   // -126 <= e <= 127
// Exponent e with max * 2^-e in [2^13, 2^14), from the float bits of a maximum magnitude; 0 (leave as it is) for Inf / NaN.
// The two differ in what else maps to 0:
// ... of ANY maximum (gemm_split.hip: max|w| of a whole weight tensor, whatever it is): zero AND subnormal maxima stay
// unscaled — a subnormal has no exponent field to read, and such weights are below anything a float32 product keeps.
__device__ __forceinline__ int norm_exponent_any_max(unsigned maxbits)
{
    const int ex = (int)(maxbits >> 23) & 0xff;
    if (ex == 0 || ex == 0xff) return 0;
    return ex - 127 - 13;
}
// ... of a REPORTED maximum (attn.hip: the word is written only by threads that met a value >= 2^15): zero means "nothing
// reported, operand in range"; a subnormal cannot arrive, so only the zero word is tested.
__device__ __forceinline__ int norm_exponent_reported_max(unsigned maxbits)
{
    const int ex = (int)(maxbits >> 23) & 0xff;
    if (maxbits == 0u || ex == 0xff) return 0;
    return ex - 127 - 13;
}

// ---- bf16: float32 pair -> packed bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(v2f v) { return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf2)); }
__device__ __forceinline__ unsigned pack_bf16(float a, float b) { return pack_bf16(v2f{a, b}); }

// ---- the split flavours (table above): (a, b) -> packed f16 high parts and packed f16 low parts
// Scaled residual, round toward zero (fine: the residual is exact).  Plain C++: hipcc pads its hazards.
__device__ __forceinline__ void split_scaled_rtz(float a, float b, unsigned& hi, unsigned& lo)
{
    const auto hp = __builtin_amdgcn_cvt_pkrtz(a, b);
    const h2 hh = __builtin_bit_cast(h2, hp);
    const float ra = (a - (float)hh.x) * kLoScale, rb = (b - (float)hh.y) * kLoScale;
    hi = __builtin_bit_cast(unsigned, hp);
    lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(ra, rb));
}
// Unscaled residual in three instructions: v_cvt_pkrtz_f16_f32, then one mixed-precision FMA per value — v_fma_mixlo/mixhi_f16
// computes x * 1.0 + (-hi) with the f16 source widened and the sum taken in float32 (exact: hi is x's leading bits), rounds it to
// f16 and writes one half of the destination.  (The plain form costs six: two v_cvt_f32_f16, two subtracts, a second pack.)
// NO trailing wait states: for results that go to LDS, not into an MFMA operand register.
__device__ __forceinline__ void split_unscaled_lds(float a, float b, unsigned& hi, unsigned& lo)
{
    hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(lo) : "v"(a), "v"(b), "v"(hi));
}
// The same for low parts that go STRAIGHT into an MFMA operand register (the wait-state rule).
__device__ __forceinline__ void split_unscaled_mfma(float a, float b, unsigned& hi, unsigned& lo)
{
    hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(lo) : "v"(a), "v"(b), "v"(hi));
}
// ... with the conversion inside the asm block as well: hipcc cannot schedule anything between the three.
__device__ __forceinline__ void split_unscaled_mfma_fused(float a, float b, unsigned& hi, unsigned& lo)
{
    asm("v_cvt_pkrtz_f16_f32 %0, %2, %3\n\t"
        "v_fma_mixlo_f16 %1, %2, 1.0, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(hi), "=&v"(lo) : "v"(a), "v"(b));
}
// Operand scaled by s (a scalar register) BEFORE the split, round to nearest: hi = f16(x s), lo = f16(x s - hi) (exact in float32,
// then exactly representable while normal).  Four mixed-precision FMAs, no packed-float32 instruction (those cost extra beside
// MFMAs: MI355X_MICROARCH.md cycle constants).  MFMA-safe.
__device__ __forceinline__ void split_prescaled_rne_mfma(float a, float b, float s, unsigned& hi, unsigned& lo)
{
    asm("v_fma_mixlo_f16 %0, %2, %4, 0\n\t"
        "v_fma_mixhi_f16 %0, %3, %4, 0\n\t"
        "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, %4, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(hi), "=&v"(lo) : "v"(a), "v"(b), "s"(s));
}

// eight values -> one MFMA operand pair
__device__ __forceinline__ void split8_scaled_rtz(const float* x, h8& hi, h8& lo)
{
    u32x4 H, L;
#pragma unroll
    for (int i = 0; i < 4; ++i) { unsigned h, l; split_scaled_rtz(x[2 * i], x[2 * i + 1], h, l); H[i] = h; L[i] = l; }
    hi = __builtin_bit_cast(h8, H); lo = __builtin_bit_cast(h8, L);
}
__device__ __forceinline__ void split8_unscaled_mfma(const float* x, h8& hi, h8& lo)
{
    u32x4 H, L;
#pragma unroll
    for (int i = 0; i < 4; ++i) { unsigned h, l; split_unscaled_mfma(x[2 * i], x[2 * i + 1], h, l); H[i] = h; L[i] = l; }
    hi = __builtin_bit_cast(h8, H); lo = __builtin_bit_cast(h8, L);
}
__device__ __forceinline__ void split8_unscaled_mfma_fused(const float4& p, const float4& q, h8& hi, h8& lo)
{
    u32x4 H, L; unsigned h, l;
    split_unscaled_mfma_fused(p.x, p.y, h, l); H[0] = h; L[0] = l;
    split_unscaled_mfma_fused(p.z, p.w, h, l); H[1] = h; L[1] = l;
    split_unscaled_mfma_fused(q.x, q.y, h, l); H[2] = h; L[2] = l;
    split_unscaled_mfma_fused(q.z, q.w, h, l); H[3] = h; L[3] = l;
    hi = __builtin_bit_cast(h8, H); lo = __builtin_bit_cast(h8, L);
}
