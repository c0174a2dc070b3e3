"""CPU tests of the failure-detection counters: the layout constants and the bit rule of the bins, the host math
of evaluation.metrics.failure_metrics_from_hist against scikit-learn and an exact running-risk mean, the result keys, the report
section, the switch, and the monotone sandwich the GPU tests gate on, checked on the model itself."""
import importlib.util
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics, report
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import failure_metrics_from_hist
from tests import failure_ref as FR

ROOT = Path(__file__).resolve().parent.parent
NEW_STATS = ops.new_failure_stats


def _cases():
    """(name, scores64, scores32, label) of the two generators, flag ties already relabelled."""
    out = []
    for name, gen in (("random", lambda: FR.random_case(3, 2, 19, 96, 192)), ("trained-like", lambda: FR.trained_like_case(4, 2, 19, 96, 192))):
        s1, s2, label = gen()
        r = FR.combine(s1, s2, "mean")
        sc = FR.ensemble_scores(s1, s2, r)
        label, share = FR.drop_flag_ties(label, sc)
        out.append((name, sc, FR.ensemble_scores(s1, s2, r, FR.torch.float32), label, share))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


# ----------------------------------------------------------------------------- 1. layout and bins
def test_layout_constants_equal_the_header_and_the_bit_rule_holds():
    text = (ROOT / "include" / "awseg.h").read_text()
    macro = {k: v for k, v in re.findall(r"#define\s+(AWSEG_FAIL_[A-Z_]+)\s+(.+)", text)}
    scores, bins = int(macro["AWSEG_FAIL_SCORES"]), int(macro["AWSEG_FAIL_BINS"])
    assert (scores, bins) == (len(ops.FAIL_SCORES), ops.FAIL_BINS) == (4, 3072)
    assert macro["AWSEG_FAIL_ROW"].strip() == "(AWSEG_FAIL_SCORES * 2 * AWSEG_FAIL_BINS + 4)" and ops.FAIL_ROW == scores * 2 * bins + 4
    assert [int(macro[f"AWSEG_FAIL_{s.upper()}"]) for s in ops.FAIL_SCORES] == [0, 1, 2, 3]
    assert ops.FAIL_SCORES == FR.SCORES and ops.FAIL_BINS == FR.BINS
    f32 = np.float32
    lo, step = f32(2.0 ** -22), f32(2.0 ** -22 * (1 + 1 / 128))
    vals = np.array([-1e-7, 0.0, lo, np.nextafter(step, f32(0)), 1.0, np.nextafter(f32(4), f32(0)), 4.0, np.inf, -0.0, -np.inf, step], f32)
    want = [0, 0, 0, 0, 22 * 128, 3071, 3071, 3071, 0, 0, 1]
    assert ops.failure_bin(vals).tolist() == want
    assert FR.bin_index(vals.astype(np.float64)).tolist() == want              # the arithmetic rule of the model agrees
    edges = ops.failure_bin_edges()
    assert edges.dtype == np.float32 and edges.shape == (ops.FAIL_BINS,) and (np.diff(edges.astype(np.float64)) > 0).all()
    assert np.array_equal(ops.failure_bin(edges), np.arange(ops.FAIL_BINS))
    assert np.array_equal(edges.astype(np.float64), FR.EDGES) and edges[0] == lo
    below = np.nextafter(edges[1:], f32(0))
    assert np.array_equal(ops.failure_bin(below), np.arange(ops.FAIL_BINS - 1))
    rs = np.random.RandomState(0)
    x = np.exp(rs.uniform(np.log(1e-9), np.log(8.0), 100000)).astype(f32)
    assert np.array_equal(ops.failure_bin(x), FR.bin_index(x.astype(np.float64)))
    st = ops.failure_stats_to_numpy(np.arange(2 * ops.FAIL_ROW, dtype=np.int64).reshape(2, -1))
    assert st["hist"].shape == (2, 4, 2, 3072) and st["hist"][1, 3, 1, 5] == ops.FAIL_ROW + (3 * 2 + 1) * 3072 + 5
    assert st["pixels"].tolist() == [ops.FAIL_ROW - 4, 2 * ops.FAIL_ROW - 4] and st["out_of_range"][0] == ops.FAIL_ROW - 2
    assert tuple(NEW_STATS("cpu", 3).shape) == (3, ops.FAIL_ROW)


# ----------------------------------------------------------------------------- 2. host math
def test_host_math_against_sklearn_and_the_exact_running_risk(cases):
    from sklearn.metrics import roc_auc_score
    for name, sc, _, label, _ in cases:
        ok = label != 255
        e_mean, e_r = FR.flags(sc, label)
        for score in FR.SCORES:
            s, wrong = sc[score][ok], (e_r if score == "msp" else e_mean)[ok]
            b = FR.bin_index(s)
            m = failure_metrics_from_hist(*FR.hist_of(s, wrong))
            assert all(isinstance(v, float) for v in m.values())
            assert abs(m["auroc"] - roc_auc_score(wrong, b)) <= 1e-12, (name, score)
            exact = roc_auc_score(wrong, s)
            assert abs(exact - m["auroc"]) <= m["auroc_halfwidth"] + 1e-15, (name, score, exact, m)
            gap = abs(m["aurc"] - FR.exact_aurc(s, wrong))
            print(f"failure host math [{name} {score}]: auroc {m['auroc']:.6f} +- {m['auroc_halfwidth']:.2e} (exact {exact:.6f}), "
                  f"aurc {m['aurc']:.6f} (gap to the running-risk mean {gap:.2e}), eaurc {m['eaurc']:.6f}, error rate {m['error_rate']:.4f}")
            assert gap <= 1e-4, (name, score, gap)
            assert m["error_rate"] == wrong.mean() and -1e-12 <= m["eaurc"] <= m["aurc"]


def test_host_math_on_hand_made_histograms():
    f = failure_metrics_from_hist
    perfect = f([5, 3, 0, 0], [0, 0, 2, 6])
    assert perfect["auroc"] == 1.0 and perfect["auroc_halfwidth"] == 0.0 and abs(perfect["eaurc"]) <= 1e-12
    assert perfect["error_rate"] == 0.5
    one = f([0, 30, 0], [0, 10, 0])
    assert one["auroc"] == 0.5 and one["auroc_halfwidth"] == 0.5 and one["aurc"] == pytest.approx(0.25, abs=1e-15) == one["error_rate"]
    clean = f([4, 4], [0, 0])
    assert (clean["auroc"], clean["auroc_halfwidth"], clean["aurc"], clean["eaurc"], clean["error_rate"]) == (0.5, 0.0, 0.0, 0.0, 0.0)
    allwrong = f([0, 0], [3, 5])
    assert allwrong["auroc"] == 0.5 and allwrong["aurc"] == pytest.approx(1.0) and allwrong["eaurc"] == pytest.approx(0.0)
    assert f([0, 0], [0, 0]) == {"auroc": 0.5, "auroc_halfwidth": 0.0, "aurc": 0.0, "eaurc": 0.0, "error_rate": 0.0}
    worst = f([0, 6], [2, 0])                                                  # every error ranked most certain
    assert worst["auroc"] == 0.0 and worst["aurc"] == pytest.approx((2 + 2 * np.log(4.0)) / 8)
    # two singletons per bin: the integral by hand, (w + (a - w T / n) ln((T + n) / T)) / N
    h = f([1, 1], [1, 1])
    assert h["aurc"] == pytest.approx((1 + 1 + (1 - 1 * 2 / 2) * np.log(2.0)) / 4) and h["auroc"] == 0.5 and h["auroc_halfwidth"] == 0.25
    with pytest.raises(ValueError):
        f([1, 2], [1])


# ----------------------------------------------------------------------------- 3. keys, report, switch, CLI
def _stats(slots):
    raw = np.zeros((slots, ops.FAIL_ROW), np.int64)
    return raw, raw[:, :-4].reshape(slots, 4, 2, ops.FAIL_BINS)


def test_result_keys_slots_kinds_and_single_model():
    conds = ["clean", "fog", "night"]
    raw, hist = _stats(4)
    for slot, (r, w) in ((1, (90, 10)), (2, (60, 40))):
        for i in range(4):
            hist[slot, i, 0, 10 + i] = r
            hist[slot, i, 1, 500] = w - 1
            hist[slot, i, 1, 10 + i] = 1
        raw[slot, -4] = r + w
    hist[2, 3, 0, 13] -= 5
    hist[2, 3, 1, 500] += 5                                                    # the combined logits err more often than the mean probability
    raw[0] = raw[1:].sum(0)
    raw[0, -3], raw[0, -2] = 7, 0
    res = metrics.failure_metrics_from_stats(raw, conds)
    assert all(isinstance(v, float) for v in res.values())
    for sfx in ("", "_clean", "_fog"):
        for s in ops.FAIL_SCORES:
            for k in ("auroc", "auroc_halfwidth", "aurc", "eaurc"):
                assert f"failure_{k}_{s}{sfx}" in res
        assert f"failure_error_rate{sfx}" in res and f"failure_error_rate_mean_probability{sfx}" in res
    assert not any(k.endswith("_night") for k in res)                          # empty slot: no keys
    assert res["failure_error_rate_fog"] == 0.45 and res["failure_error_rate_mean_probability_fog"] == 0.4
    assert res["failure_error_rate_clean"] == 0.1 and res["failure_error_rate"] == 55 / 200
    want = failure_metrics_from_hist(hist[2, 0, 0], hist[2, 0, 1])
    assert res["failure_auroc_mi_fog"] == want["auroc"] and res["failure_eaurc_mi_fog"] == want["eaurc"]
    assert res["failure_nonfinite_pixels"] == 7.0 and "failure_out_of_range_labels" not in res
    raw[0, -3], raw[0, -2] = 0, 3
    res2 = metrics.failure_metrics_from_stats(raw, conds)
    assert res2["failure_out_of_range_labels"] == 3.0 and "failure_nonfinite_pixels" not in res2
    single = metrics.failure_metrics_from_stats(raw, conds, single=True)
    assert "failure_auroc_entropy_fog" in single and "failure_aurc_msp" in single and "failure_error_rate_clean" in single
    assert not any("_mi" in k or "_variance" in k or "mean_probability" in k for k in single)
    assert metrics.failure_metrics_from_stats(np.zeros((4, ops.FAIL_ROW), np.int64), conds) == {}
    with pytest.raises(ValueError):
        metrics.failure_metrics_from_stats(raw[:3], conds)
    # severity sweep: every kind also from its slots summed
    slots = ["clean", "fog_s1", "fog_s2"]
    sweep = metrics.failure_metrics_from_stats(raw, slots, kinds=["fog"], levels=2)
    summed = failure_metrics_from_hist(*(hist[2] + hist[3])[1])
    assert sweep["failure_auroc_entropy_fog"] == summed["auroc"] and sweep["failure_aurc_entropy_fog"] == summed["aurc"]
    assert "failure_auroc_mi_fog_s1" in sweep and "failure_auroc_mi_fog_s2" not in sweep and "failure_error_rate_fog" in sweep


def test_report_has_a_failure_section_only_with_failure_keys():
    base = {"overall_miou": 0.5, "miou_clean": 0.6, "expected_calibration_error": 0.1}
    assert "## Failure Detection" not in report.report_markdown(base, None)
    res = dict(base)
    for sfx, v in (("", 0.8), ("_fog", 0.7)):
        for s in ("entropy", "msp"):
            res.update({f"failure_auroc_{s}{sfx}": v, f"failure_auroc_halfwidth_{s}{sfx}": 0.002, f"failure_aurc_{s}{sfx}": 0.1,
                        f"failure_eaurc_{s}{sfx}": 0.05})
        res[f"failure_error_rate{sfx}"] = 0.25
    res["failure_nonfinite_pixels"] = 4.0
    text = report.report_markdown(res, None)
    assert "## Failure Detection" in text and "| Condition | entropy | msp | Error rate |" in text
    assert "| fog | 0.700 ± 0.002 / 0.050 | 0.700 ± 0.002 / 0.050 | 0.250 |" in text and "| all | 0.800" in text
    assert "Non-finite pixels**: 4" in text and "Out-of-range" not in text


def test_switch_rejects_non_booleans_and_the_cli_flag_sets_it(monkeypatch, tmp_path):
    opt = harness.failure_option
    assert opt({}) is False and opt({"evaluation.failure_detection": False}) is False and opt({"evaluation.failure_detection": True}) is True
    for bad in ("yes", 1, 0, 1.0, [True]):
        with pytest.raises(ValueError, match="failure_detection"):
            opt({"evaluation.failure_detection": bad})
    spec = importlib.util.spec_from_file_location("evaluate_script", ROOT / "scripts" / "evaluate.py")
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    seen = []

    class DS:
        def __init__(self, **kw):
            pass
    monkeypatch.setattr(ev, "load_model", lambda config, ckpt, device: None)
    monkeypatch.setattr(ev, "CityscapesKITTIDataset", DS)
    monkeypatch.setattr(ev, "create_dataloader", lambda ds, **kw: [])
    monkeypatch.setattr(ev, "setup_logging", lambda config: None)
    monkeypatch.setattr(ev.parallel, "init_from_env", lambda *a, **k: (0, 0, 1))
    monkeypatch.setattr(ev, "evaluate_model", lambda model, loader, m, device, config: seen.append(config.get("evaluation.failure_detection")) or {})
    monkeypatch.setattr(ev, "generate_evaluation_report", lambda res, out: None)
    for argv, want in ((["none", "--device", "cpu"], None), (["none", "--device", "cpu", "--failure-detection"], True)):
        monkeypatch.setattr(sys, "argv", ["evaluate.py"] + argv)
        ev.main()
        assert seen[-1] is True if want else not seen[-1]
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "default.yaml").read_text())
    assert cfg["evaluation"]["failure_detection"] is False


def test_eval_state_allocates_the_counters_only_when_asked():
    m = metrics.RobustnessMetrics(19, ["clean", "fog"])
    assert harness.EvalState(m, ["clean", "fog"], "cpu", 15, True).failure is None
    st = harness.EvalState(m, ["clean", "fog"], "cpu", 15, True, failure=True)
    assert tuple(st.failure["stats"].shape) == (3, ops.FAIL_ROW) and st.failure["conditions"] == ["clean", "fog"]
    assert st.failure["single"] is False and harness.EvalState(m, ["clean"], "cpu", 15, False, failure=True).failure["single"] is True


# ----------------------------------------------------------------------------- 4. the sandwich, on the model
def test_sandwich_holds_under_perturbations_of_the_model_scores(cases):
    rs = np.random.RandomState(9)
    for name, sc, sc32, label, share in cases:
        ok = label != 255
        delta = FR.deltas(sc, sc32, label, 19)
        e_mean, e_r = FR.flags(sc, label)
        for score in FR.SCORES:
            s, wrong, d = sc[score][ok], (e_r if score == "msp" else e_mean)[ok], delta[score]
            assert 0 < d < 1e-4, (name, score, d)
            sw = FR.sandwich(s, wrong, d, failure_metrics_from_hist)
            base = failure_metrics_from_hist(*FR.hist_of(s, wrong))
            width = max(sw["auroc"][1] - sw["auroc"][0], sw["aurc"][1] - sw["aurc"][0])
            print(f"failure sandwich [{name} {score}]: delta {d:.2e}, width {width:.2e}, halfwidth {base['auroc_halfwidth']:.2e}, "
                  f"flag ties removed {share:.4%}")
            assert width + base["auroc_halfwidth"] < 0.01, (name, score, width, base["auroc_halfwidth"])
            for trial in range(4):
                noise = rs.uniform(-d, d, s.shape) if trial < 2 else d * rs.choice([-1.0, 1.0], s.shape)
                m = failure_metrics_from_hist(*FR.hist_of(s + noise, wrong))
                for k in ("auroc", "aurc"):
                    assert sw[k][0] - FR.HOST_EPS <= m[k] <= sw[k][1] + FR.HOST_EPS, (name, score, trial, k, sw[k], m[k])
