"""CPU tests (-m "not gpu") of the streamed temperature calibration: the float64 model against torch's float64 cross
entropy and the reference's ECE expressions, the host math that turns the device counters into result keys, the grid's
host validation and the ABI declarations."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import calib_ref as CR

ROOT = Path(__file__).resolve().parent.parent


def _logits(seed, b=2, c=7, h=9, w=11, scale=2.0, ignore=0.05):
    g = torch.Generator().manual_seed(seed)
    r = (torch.randn(b, c, h, w, generator=g) * scale).float()
    y = torch.randint(0, c, (b, h, w), generator=g)
    y[torch.rand(b, h, w, generator=g) < ignore] = 255
    return r, y


def _ece_reference(conf, correct, edges):
    """PKG/evaluation/metrics.py:179-194 in float64."""
    ece = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        inb = (conf > lo) & (conf <= hi)
        prop = inb.double().mean()
        if prop > 0:
            ece += abs(conf[inb].mean() - correct[inb].double().mean()) * prop
    return float(ece)


@pytest.mark.parametrize("scale", [0.1, 2.0, 30.0, 200.0])
def test_f64_model_matches_torch_cross_entropy_and_reference_ece(scale):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import ConfidenceCalibration
    r, y = _logits(1, scale=scale)
    temps = np.array([0.1, 0.5, 1.0, 3.0], np.float32)
    edges = torch.linspace(0, 1, 16)
    ref = CR.grid_stats_f64(r.numpy(), y.numpy(), temps, edges.numpy())
    for k, t in enumerate(temps):
        z = r.double() / float(t)
        want = F.cross_entropy(z, y, ignore_index=255).item()
        assert ref["nll_exact"][0, k] / ref["count"][0, k] == pytest.approx(want, rel=1e-12, abs=1e-12)
        p = F.softmax(z, dim=1)
        conf, pred = p.max(dim=1)[0].reshape(-1), r.argmax(dim=1).reshape(-1)
        keep = y.reshape(-1) != 255
        e_ref = _ece_reference(conf[keep], (pred == y.reshape(-1))[keep], edges.double())
        b = np.zeros(15, dtype=[("count", "<i8"), ("sum_conf", "<f8"), ("sum_correct", "<i8")])
        b["count"], b["sum_conf"], b["sum_correct"] = ref["bin_count"][0, k], ref["bin_conf"][0, k], ref["bin_correct"][0, k]
        assert ConfidenceCalibration.ece_from_bins(b) == pytest.approx(e_ref, abs=1e-12)
        assert CR.ece_f64(ref, 0, k) == pytest.approx(e_ref, abs=1e-12)
    if scale == 200.0:
        assert ref["saturated"][0, 0] > 0                       # t = 0.1 at logit scale 200 clamps some pixels
        assert ref["nll_sum"][0, 0] < ref["nll_exact"][0, 0]


def _stats(count, nll_mean, n_bins=2, conf=0.5, correct_frac=0.5, saturated=None):
    """Synthetic decoded counters [slots, K]: the NLL sums in fixed point, one populated ECE bin."""
    count = np.asarray(count, np.int64)
    nll_q = np.round(np.asarray(nll_mean, np.float64) / CR.NLL_UNIT).astype(np.int64) * count
    bins = np.zeros(count.shape + (n_bins,), dtype=[("count", "<i8"), ("sum_conf", "<f8"), ("sum_correct", "<i8")])
    bins["count"][..., 1] = count
    bins["sum_conf"][..., 1] = count * conf
    bins["sum_correct"][..., 1] = np.round(count * correct_frac).astype(np.int64)
    return {"count": count, "nll_q": nll_q, "saturated": np.zeros_like(count) if saturated is None else np.asarray(saturated),
            "nonfinite": np.zeros_like(count), "bins": bins, "out_of_range": np.zeros(count.shape[0], np.int64)}


def test_calibration_from_stats_picks_the_first_minimum_and_reports_at_it():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import calibration_from_stats
    temps = [0.5, 1.0, 2.0, 4.0]
    conds = ["clean", "fog"]
    # slot 0 overall, 1 clean (minimum at k = 1 and a tie at k = 2: the first wins), 2 fog (own minimum at k = 3)
    s = _stats([[10, 10, 10, 10], [4, 4, 4, 4], [6, 6, 6, 6]],
               [[2.0, 1.5, 1.5, 1.7], [2.0, 1.0, 1.0, 3.0], [3.0, 2.0, 1.8, 1.1]])
    s["bins"]["sum_correct"][0, 1, 1] = 10                         # overall ECE at k = 1: |0.5 - 1.0| = 0.5
    s["bins"]["sum_correct"][2, 1, 1] = 0                          # fog ECE at k = 1: |0.5 - 0| = 0.5
    s["bins"]["sum_correct"][1, 1, 1] = 2                          # clean ECE at k = 1: 0
    res = calibration_from_stats(s, temps, conds, "clean")
    assert res["calibration_temperature"] == 1.0
    assert res["nll_calibrated"] == pytest.approx(1.5, abs=1e-6)
    assert res["ece_calibrated"] == pytest.approx(0.5)
    assert res["ece_calibrated_clean"] == pytest.approx(0.0)
    assert res["ece_calibrated_fog"] == pytest.approx(0.5)
    assert res["nll_calibrated_fog"] == pytest.approx(2.0, abs=1e-6)
    assert res["calibration_temperature_clean"] == 1.0
    assert res["calibration_temperature_fog"] == 4.0
    assert "calibration_saturated_pixels" not in res
    assert all(isinstance(v, float) for v in res.values())


def test_calibration_from_stats_falls_back_to_slot0_and_omits_absent_conditions():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import calibration_from_stats
    temps = [0.5, 1.0, 2.0]
    s = _stats([[8, 8, 8], [0, 0, 0], [8, 8, 8]], [[2.0, 1.9, 1.2], [0, 0, 0], [2.0, 1.9, 1.2]], saturated=[[3, 2, 0], [0, 0, 0], [3, 2, 0]])
    res = calibration_from_stats(s, temps, ["clean", "snow"], "clean")          # no clean pixel: fit on slot 0
    assert res["calibration_temperature"] == 2.0
    assert not any(k.endswith("_clean") for k in res)
    assert "ece_calibrated_snow" in res and res["calibration_temperature_snow"] == 2.0
    assert res["calibration_saturated_pixels"] == 3.0           # pixels at the worst grid point, not (pixel, t) pairs (5)
    assert calibration_from_stats(s, temps, ["clean", "snow"], "night")["calibration_temperature"] == 2.0   # not a condition
    empty = _stats([[0, 0, 0]], [[0, 0, 0]])
    assert calibration_from_stats(empty, temps, [], "clean") == {}


def test_first_minimum_compares_exact_integer_sums():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import first_min_index
    # means 7/3 and 14/6 are equal: the first wins; 2**62-scale sums must not lose precision to float64
    assert first_min_index([7, 14, 15], [3, 6, 6]) == 0
    big = 1 << 62
    assert first_min_index([big + 1, big], [1 << 31, 1 << 31]) == 1
    assert first_min_index([5, 3], [0, 0]) is None


def test_default_grid_is_the_reference_linspace_and_has_no_exact_one():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    want = torch.linspace(0.1, 10.0, 100)
    assert ops.DEFAULT_TEMPERATURE_GRID.dtype == np.float32
    assert np.array_equal(ops.DEFAULT_TEMPERATURE_GRID, want.numpy())
    assert 1.0 not in ops.DEFAULT_TEMPERATURE_GRID.tolist() and ops.DEFAULT_TEMPERATURE_GRID[9] == np.float32(0.99999994)


@pytest.mark.parametrize("temps", [[0.5, 0.0], [1.0, -2.0], [float("nan")], [float("inf")], list(np.linspace(0.1, 10, 129)), []])
def test_host_validation_raises_before_any_launch(temps):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    logits, label = torch.zeros(1, 19, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8)         # host tensors: a launch would raise otherwise
    stats = torch.zeros(1, max(len(temps), 1) + 1, 4 + 3 * 15, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.temperature_grid_stats(logits, label, stats, temps, torch.linspace(0, 1, 16))
    with pytest.raises(ValueError):
        ops.ensemble_temperature_grid_stats(logits, logits, 0, None, None, label, stats, temps, torch.linspace(0, 1, 16))
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.harness import EvalState, temperature_grid
    with pytest.raises(ValueError):
        temperature_grid(temps)


def test_header_declares_the_calibration_entry_points_with_their_contract():
    text = (ROOT / "include" / "awseg.h").read_text()
    for name in ("awseg_temperature_grid_stats", "awseg_ensemble_temperature_grid_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    for macro, value in (("AWSEG_CALIB_MAX_TEMPS", "128"), ("AWSEG_CALIB_NLL_FRAC_BITS", "20"), ("AWSEG_CALIB_NLL_CAP", "2048"),
                         ("AWSEG_CALIB_PIXEL_BUDGET", "((1LL << 32) - 1)")):
        assert re.search(rf"#define\s+{macro}\s+{re.escape(value)}", text), macro
    assert "metrics.py:266-321" in text and "evaluate.py:230-238" in text
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native, ops
    assert {"awseg_temperature_grid_stats", "awseg_ensemble_temperature_grid_stats"} <= set(_native.SIGNATURES)
    assert ops.CALIB_MAX_TEMPS == 128 and ops.CALIB_NLL_UNIT == 2.0 ** -20 and ops.CALIB_PIXEL_BUDGET == (1 << 32) - 1
    assert ops.CALIB_PIXEL_BUDGET * int(ops.CALIB_NLL_CAP / ops.CALIB_NLL_UNIT) <= (1 << 63) - 1   # the int64 NLL sum cannot wrap


def test_temperature_grid_config_forms():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.harness import temperature_grid
    assert temperature_grid(None) is None
    assert np.array_equal(temperature_grid({"min": 0.1, "max": 10.0, "steps": 100}), torch.linspace(0.1, 10.0, 100).numpy())
    assert temperature_grid([0.5, 1, 2]).tolist() == [0.5, 1.0, 2.0]


def test_decoder_layout():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    K, nb, S = 3, 2, 2
    raw = np.arange(S * (K + 1) * (4 + 3 * nb), dtype=np.int64).reshape(S, K + 1, 4 + 3 * nb)
    d = ops.temperature_grid_stats_to_numpy(raw)
    assert d["count"].shape == (S, K) and d["bins"].shape == (S, K, nb)
    assert d["nll_q"][1, 2] == raw[1, 2, 1] and d["saturated"][0, 1] == raw[0, 1, 2] and d["nonfinite"][1, 0] == raw[1, 0, 3]
    assert d["bins"]["count"][1, 2, 1] == raw[1, 2, 7] and d["bins"]["sum_correct"][0, 0, 0] == raw[0, 0, 6]
    assert d["bins"]["sum_conf"][0, 1, 1] == raw[0, 1, 8] * 2.0 ** -30
    assert d["out_of_range"].tolist() == [raw[0, K, 0], raw[1, K, 0]]


def test_calibration_budget_is_checked_on_the_summed_counters(monkeypatch):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import RobustnessMetrics
    harness.check_calibration_budget(ops.CALIB_PIXEL_BUDGET)
    with pytest.raises(OverflowError):
        harness.check_calibration_budget(ops.CALIB_PIXEL_BUDGET + 1)
    st = harness.EvalState(RobustnessMetrics(4, ["clean"]), ["clean"], "cpu", 3, temperature_grid=[0.5, 1.0])
    st.calib["pixels"] = ops.CALIB_PIXEL_BUDGET // 2 + 1          # a rank whose own count fits, summed with another that does too

    def two_ranks(ts):                                           # stands in for the SUM all-reduce over two equal ranks
        for t in ts:
            t.mul_(2)
    monkeypatch.setattr(harness.parallel, "all_reduce_sum_", two_ranks)
    with pytest.raises(OverflowError):
        st.all_reduce()

