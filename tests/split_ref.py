"""Reference side of the split-operand accuracy tests (nothing in the package imports this module).

Every split-operand kernel of csrc/ carries a float32 operand x as two f16 numbers, hi = f16(x) (round toward zero,
v_cvt_pkrtz) and a low part, and forms each product from three f16 MFMA products accumulated in float32.  This module
holds the yardstick those kernels are held to and a bit-level numpy model of the three split forms, so that the yardstick
itself can be checked without a GPU (tests/test_split_ref.py).

(a) The componentwise gate.  For an output element

        e = |got - ref64| / D,     D = sum_k |x_k| |w_k| + |bias| + |residual|

D is computed in float64 and has no absolute floor: it is the natural scale of a float32 dot product's rounding error,
and ReLU being 1-Lipschitz it holds through the activation too.  A kernel passes when its largest e is within
max(4 * (largest e of its float32 twin on the same inputs), 2^-20); 2^-20 is four times the 22-bit operand rounding.

(b) The three split forms, as the kernels compute them:
  * SCALED low part (gemm_split.hip split_pair, kLoScale): lo = f16_rtz((x - hi) * 2^11), the cross products in a
    second accumulator multiplied by 2^-11 in the epilogue;
  * UNSCALED low part (attn.hip split_pair_unscaled, mixffn.hip mf_split_pair, heads.hip head_split_pair):
    lo = f16_rn(x - hi), one accumulator for all three products;
  * UNSCALED after x 2^4 staging (gemm_split3.hip, kActScale0): the unscaled form of
    x * 2^4, the result multiplied by 2^-4.
f16 subnormals are kept (the MFMA does not flush them), products of two f16 numbers are exact in float32, accumulation is
float32.  Weights may be NORMALISED (w * 2^-e with max |w| in [2^13, 2^14), gemm_split_weights) and activations may take
the SMALL-SIDE GUARD (an operand block whose max |x| is below SMALL_GUARD is split as x * 2^-e with max in [2^13, 2^14)); both scales
are exact powers of two multiplied back into the result.
"""
from __future__ import annotations

import numpy as np

GATE_FLOOR = 2.0 ** -20          # 4 x the 22-bit operand rounding
GATE_FACTOR = 4.0
# block maximum below which a kernel redoes a block with scaled activations, per form: the unscaled low part keeps its 11 bits
# while |x| >= 2^-3 (2^-7 after the x 2^4 staging); the scaled form's kernels share the 2^-7 bound of the staged one
SMALL_GUARD = {"scaled": 2.0 ** -7, "unscaled": 2.0 ** -3, "staged16": 2.0 ** -7}


# ------------------------------------------------------------------ (a) metric and gate
def denominator(ax, aw, *extra):
    """D = |x| @ |w|^T (+ |extra| terms, broadcast) in float64: x [M,K], w [N,K] -> [M,N]."""
    d = np.abs(np.asarray(ax, np.float64)) @ np.abs(np.asarray(aw, np.float64)).T
    for t in extra:
        if t is not None:
            d = d + np.abs(np.asarray(t, np.float64))
    return d


def componentwise_error(got, ref, den) -> float:
    """max |got - ref| / D over the elements.  D == 0 (an exactly zero reference with zero operands) demands got == 0."""
    got, ref, den = (np.asarray(a, np.float64) for a in (got, ref, den))
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float("inf")
    zero = den == 0
    if (err[zero] != 0).any():
        return float("inf")
    return float((err[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def gate_bound(e_f32: float) -> float:
    return max(GATE_FACTOR * e_f32, GATE_FLOOR)


def gate_ok(e_split: float, e_f32: float) -> bool:
    return e_split <= gate_bound(e_f32)


# ------------------------------------------------------------------ (b) the split forms
def f16_rtz(a) -> np.ndarray:
    """float32 -> f16 rounded toward zero (v_cvt_pkrtz_f16_f32), subnormals kept."""
    a = np.asarray(a, np.float32)
    h = a.astype(np.float16)                                        # round to nearest even
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h


def f16_rn(a) -> np.ndarray:
    return np.asarray(a, np.float32).astype(np.float16)


def _f32(a):
    return np.asarray(a, np.float32)


def split_scaled(a):
    """(hi, lo) with a ~= hi + lo * 2^-11 (split_pair: both conversions v_cvt_pkrtz)."""
    a = _f32(a)
    hi = f16_rtz(a)
    lo = f16_rtz((a - hi.astype(np.float32)) * np.float32(2048.0))
    return hi, lo


def split_unscaled(a):
    """(hi, lo) with a ~= hi + lo (split_pair_unscaled / mf_split_pair / head_split_pair: lo by v_fma_mix, round to nearest;
    a - hi is exact in float32 because hi is a truncation of a)."""
    a = _f32(a)
    hi = f16_rtz(a)
    lo = f16_rn(a - hi.astype(np.float32))
    return hi, lo


def pow2_exponent(maxabs: float) -> int:
    """e with maxabs * 2^-e in [2^13, 2^14) (norm_exponent of gemm_split.hip); 0 for a zero maximum."""
    if maxabs == 0 or not np.isfinite(maxabs):
        return 0
    return int(np.floor(np.log2(np.float64(maxabs)))) - 13


def split_dot(x, w, form: str, normalise_w: bool = True, small_guard: bool = False) -> np.ndarray:
    """float32 result of x [M,K] . w [N,K]^T as a split-operand kernel of `form` computes it:
    'scaled' | 'unscaled' | 'staged16'.  normalise_w: weights stored as w * 2^-ew (gemm_split_weights);
    small_guard: activations whose max |x| is below SMALL_GUARD[form] split as x * 2^-ex (the small-side second pass)."""
    x, w = _f32(x), _f32(w)
    ew = pow2_exponent(float(np.abs(w).max())) if normalise_w else 0
    ex = 0
    if small_guard:
        mx = float(np.abs(x).max())
        if 0 < mx < SMALL_GUARD[form]:
            ex = pow2_exponent(mx)
    ws = _f32(np.float64(w) * 2.0 ** -ew)
    xs = _f32(np.float64(x) * 2.0 ** -ex)
    if form == "scaled":
        xh, xl = split_scaled(xs)
        wh, wl = split_scaled(ws)
        f = lambda a: a.astype(np.float32)                                   # noqa: E731
        main = f(xh) @ f(wh).T
        corr = np.concatenate([f(xh), f(xl)], 1) @ np.concatenate([f(wl), f(wh)], 1).T
        acc = main + corr * np.float32(2.0 ** -11)
        post = 0
    elif form in ("unscaled", "staged16"):
        pre = 4 if (form == "staged16" and ex == 0) else 0                    # the optimistic pass stages x * 2^4
        xh, xl = split_unscaled(xs * np.float32(2.0 ** pre))
        wh, wl = split_unscaled(ws)
        f = lambda a: a.astype(np.float32)                                   # noqa: E731
        acc = np.concatenate([f(xh), f(xh), f(xl)], 1) @ np.concatenate([f(wh), f(wl), f(wh)], 1).T
        post = -pre
    else:
        raise ValueError(form)
    return _f32(np.float64(acc) * 2.0 ** (ew + ex + post))
