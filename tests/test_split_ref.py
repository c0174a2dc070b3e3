"""The componentwise gate of tests/split_ref.py, checked without a GPU on the bit-level model of the split forms: it accepts the
healthy forms at every point of the magnitude sweep the GPU tests run and rejects the known-degraded ones, so the gate constant is
pinned and the metric can see the failure tests/test_gpu_split_magnitudes.py looks for."""
import numpy as np
import pytest

from tests import split_ref as S

M, K, N = 256, 256, 128
SCALES = (0, -4, -8, -12, -16, -20)


def _weights(kind, rng):
    w = rng.standard_normal((N, K))
    if kind == "inv_sqrt_k":
        w = w / K ** 0.5
    elif kind == "2^-10":
        w = w * 2.0 ** -10
    else:
        w = w * 0.02
        if kind == "0.02_per_channel":
            w = w * np.exp2(rng.uniform(-8, 0, (N, 1)))
    return w.astype(np.float32)


def _errors(x, w, **form):
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    den = S.denominator(x, w)
    e_f32 = S.componentwise_error(x @ w.T, ref, den)
    return S.componentwise_error(S.split_dot(x, w, **form), ref, den), e_f32


def test_split_forms_are_bit_exact_models():
    """the emulated parts reconstruct x as the kernels' parts do: hi a truncation, x - hi exact, low parts rounded once"""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(4096) * np.exp2(rng.uniform(-24, 14, 4096))).astype(np.float32)
    hi, lo = S.split_unscaled(x)
    assert (np.abs(hi.astype(np.float32)) <= np.abs(x)).all()
    assert np.array_equal(S.f16_rtz(np.float32(1.0 + 2.0 ** -11 * 1.5)), np.float16(1.0))          # RN would round up
    r = x.astype(np.float64) - hi.astype(np.float64)
    assert (np.abs(lo.astype(np.float64) - r) <= 2.0 ** -25 + np.abs(r) * 2.0 ** -11).all()          # one rounding, subnormal floor 2^-25
    hs, ls = S.split_scaled(x)
    assert np.array_equal(hs, hi)
    assert S.pow2_exponent(0.02) == -6 - 13 and S.pow2_exponent(1.0) == -13


@pytest.mark.parametrize("wkind", ["inv_sqrt_k", "0.02", "2^-10", "0.02_per_channel"])
@pytest.mark.parametrize("s", SCALES)
def test_gate_accepts_healthy_forms(wkind, s):
    """scaled low parts, and normalised weights with the small-side guard, at every scale and weight setting"""
    rng = np.random.default_rng(abs(s) * 7 + len(wkind))
    w = _weights(wkind, rng)
    x = (rng.standard_normal((M, K)) * 2.0 ** s).astype(np.float32)
    for form in ("scaled", "unscaled", "staged16"):
        e_s, e_f = _errors(x, w, form=form, normalise_w=True, small_guard=True)
        assert S.gate_ok(e_s, e_f), (form, e_s / 2 ** -22, e_f / 2 ** -22)
        assert e_f < 2 * 2.0 ** -22                                       # the float32 twin sits at the float32 rounding


def test_gate_rejects_unnormalised_small_weights():
    """unscaled low parts of weights at std 2^-9 without normalisation (the Mix-FFN split before this gate existed)"""
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((N, K)) * 2.0 ** -9).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    e_s, e_f = _errors(x, w, form="unscaled", normalise_w=False)
    assert not S.gate_ok(e_s, e_f), e_s / 2 ** -22
    e_s, e_f = _errors(x, w, form="unscaled", normalise_w=True)
    assert S.gate_ok(e_s, e_f)


@pytest.mark.parametrize("form", ["unscaled", "staged16"])
def test_gate_rejects_small_activations_without_guard(form):
    """unscaled low parts of activations at 2^-12 without the small-side guard (and also the x 2^4 staged form)"""
    rng = np.random.default_rng(4)
    w = _weights("0.02", rng)
    x = (rng.standard_normal((M, K)) * 2.0 ** -12).astype(np.float32)
    e_s, e_f = _errors(x, w, form=form, normalise_w=True, small_guard=False)
    assert not S.gate_ok(e_s, e_f), e_s / 2 ** -22
    e_s, e_f = _errors(x, w, form=form, normalise_w=True, small_guard=True)
    assert S.gate_ok(e_s, e_f)


def test_gate_rejects_subnormal_high_parts_without_guard():
    """scaled low parts do not rescue activations at 2^-20: the f16 high parts are subnormal"""
    rng = np.random.default_rng(5)
    w = _weights("inv_sqrt_k", rng)
    x = (rng.standard_normal((M, K)) * 2.0 ** -20).astype(np.float32)
    e_s, e_f = _errors(x, w, form="scaled", normalise_w=True, small_guard=False)
    assert not S.gate_ok(e_s, e_f), e_s / 2 ** -22


def test_metric_has_no_floor():
    """a kernel that returned 0 for tiny products would pass an absolute floor; the componentwise metric sees it"""
    x = np.full((2, 4), 1e-30, np.float32); w = np.ones((3, 4), np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    assert S.componentwise_error(np.zeros_like(ref), ref, S.denominator(x, w)) == pytest.approx(1.0)
    assert S.componentwise_error(np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1))) == 0.0
    assert S.componentwise_error(np.ones((1, 1)), np.zeros((1, 1)), np.zeros((1, 1))) == float("inf")
