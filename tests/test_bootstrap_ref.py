"""CPU checks of the frame bootstrap: the numpy model (tests/bootstrap_ref.py) against itself, against independently built
confusion matrices and against closed forms; the host math (bootstrap_metrics_from_replicates), the option parser, the resampling
set, the report lines and the command line.  No GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import bootstrap_ref as BR

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def M():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import metrics
    return metrics


@pytest.fixture(scope="module")
def H():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness
    return harness


def random_frames(seed, n, V, c, hw=40, absent=0.0, n_slots=None):
    """n x V frames of hw pixels: predictions that agree with the label more often in low variants; a few ignored pixels.
    -> (pred [n, V, hw], label [n, V, hw], slots int32 [n, V]) with slot 1 + v for variant v, 0 where the frame is absent."""
    rng = np.random.default_rng(seed)
    label = np.repeat(rng.integers(0, c, (n, 1, hw)), V, axis=1)
    flip = rng.random((n, V, hw)) < (0.15 + 0.5 * np.arange(V)[None, :, None] / max(V, 1))
    pred = np.where(flip, rng.integers(0, c, (n, V, hw)), label)
    label = np.where(rng.random((n, V, hw)) < 0.05, 255, label)
    slots = np.tile(1 + np.arange(V, dtype=np.int32), (n, 1))
    slots[rng.random((n, V)) < absent] = 0
    return pred.astype(np.uint8), label.astype(np.uint8), slots


def table_of(pred, label, c):
    n, V = pred.shape[:2]
    rows = np.arange(n * V)
    t, oob = BR.frame_counts(pred.reshape(n * V, -1), label.reshape(n * V, -1), c, rows, n * V)
    assert oob == 0
    return t.reshape(n, V, 3 * c)


# ----------------------------------------------------------------------------- the model against itself
def test_draws_are_indices_spread_over_the_sources():
    for n in (1, 2, 3, 5, 64, 1000):
        d = BR.draws(7, 11, n)
        assert d.shape == (n,) and d.min() >= 0 and d.max() < n
    hits = np.bincount(np.concatenate([BR.draws(3, q, 8) for q in range(4000)]), minlength=8)
    assert np.abs(hits / hits.sum() - 0.125).max() < 4 * np.sqrt(0.125 * 0.875 / hits.sum())
    assert not np.array_equal(BR.draws(1, 0, 64), BR.draws(2, 0, 64)) and not np.array_equal(BR.draws(1, 0, 64), BR.draws(1, 1, 64))
    assert np.array_equal(BR.draws(2 ** 40 + 5, 9, 64), BR.draws(2 ** 40 + 5, 9, 64))
    assert not np.array_equal(BR.draws(2 ** 40 + 5, 9, 64), BR.draws(5, 9, 64))          # the high key word is used


@pytest.mark.parametrize("n,V", [(1, 1), (2, 3), (3, 1), (5, 13), (64, 2)], ids=str)
def test_loop_and_multiplicity_formulations_agree(n, V):
    c = 4
    pred, label, slots = random_frames(n * 31 + V, n, V, c, absent=0.2)
    slots[0, 0] = V + 5                                              # out of range: skipped
    if n > 1:
        slots[1, V - 1] = -2
    table = table_of(pred, label, c)
    a = BR.replicate_sums_loop(table, slots, 1 + V, 9, 2, 6)
    b = BR.replicate_sums(table, slots, 1 + V, 9, 2, 6)
    assert np.array_equal(a, b) and BR.slot_oob(slots, 1 + V) == (2 if n > 1 else 1)
    # chunking: (2, 6) = (2, 2) joined with (4, 4)
    assert np.array_equal(b, np.concatenate([BR.replicate_sums(table, slots, 1 + V, 9, 2, 2), BR.replicate_sums(table, slots, 1 + V, 9, 4, 4)]))
    assert np.array_equal(b[:, 0], b[:, 1:].sum(1))                  # every counted frame sits in slot 0 and in one other slot


def test_frame_rows_are_the_marginals_of_a_confusion_matrix():
    c = 5
    pred, label, slots = random_frames(4, 6, 3, c, hw=57)
    label = label.astype(np.int64)
    label[0, 0, :3] = c + 1                                          # outside [0, C): not a labelled pixel
    label[1, 1, 0] = -1
    pred[2, 2, 5], label[2, 2, 5] = 200, 0                           # a prediction no argmax gives: not counted
    rows = np.arange(18)
    table, oob = BR.frame_counts(pred.reshape(18, -1), label.reshape(18, -1), c, rows, 18)
    assert oob == 3 + 1 + 1
    table = table.reshape(6, 3, 3 * c)
    for v in range(3):
        cm = sum(BR.confusion(pred[i, v], label[i, v], c) for i in range(6))
        got = table[:, v].sum(0)
        assert np.array_equal(got[:c], np.diag(cm)) and np.array_equal(got[c:2 * c], cm.sum(1)) and np.array_equal(got[2 * c:], cm.sum(0))
    # rows: -1 skips, >= n_rows adds the frame's pixels to oob, two frames into one row add up, a second call accumulates
    t2, oob2 = BR.frame_counts(pred[:, 0], label[:, 0], c, [0, 0, -1, 7, 1, 1], 2)
    assert oob2 == 57 + 3 and np.array_equal(t2[0], table[0, 0] + table[1, 0]) and np.array_equal(t2[1], table[4, 0] + table[5, 0])
    t3, _ = BR.frame_counts(pred[:2, 1], label[:2, 1], c, [1, 0], 2, table=t2)
    assert np.array_equal(t3[0], t2[0] + table[1, 1]) and np.array_equal(t3[1], t2[1] + table[0, 1])


def test_replicate_miou_equals_iou_from_counts_on_the_resampled_confusion_matrix(M):
    c, n, V = 7, 9, 3
    pred, label, slots = random_frames(12, n, V, c, hw=90, absent=0.15)
    table = table_of(pred, label, c)
    cms = np.stack([[BR.confusion(pred[i, v], label[i, v], c).reshape(-1) for v in range(V)] for i in range(n)])
    rep = BR.replicate_sums(table, slots, 1 + V, 5, 0, 40)
    rep_cm = BR.replicate_sums(cms, slots, 1 + V, 5, 0, 40)          # the same draws on whole confusion matrices
    miou, present = M.replicate_miou(rep, c)
    assert present.all()
    for r in range(40):
        for s in range(1 + V):
            want = M.iou_from_counts(torch.from_numpy(rep_cm[r, s].copy()), c)["mean_iou"]
            assert abs(miou[r, s] - want) <= 1e-6, (r, s)
    miou0, present0 = M.replicate_miou(np.zeros((2, 3 * c), np.int64), c)
    assert not present0.any() and np.isnan(miou0).all()


# ----------------------------------------------------------------------------- closed forms
def point_of(M, table, slots, names, c, kinds=(), levels=0):
    """The pooled point estimates the harness would have reported, from the summed rows."""
    tot = BR.replicate_sums(table, slots, 1 + len(names), 0, 0, 1) * 0
    for i in range(table.shape[0]):
        for v in range(table.shape[1]):
            s = int(slots[i, v])
            if 1 <= s <= len(names):
                tot[0, 0] += table[i, v]
                tot[0, s] += table[i, v]
    miou, present = M.replicate_miou(tot[0], c)
    deg = M.RobustnessMetrics().compute_robustness_degradation_ratio
    point = {"overall_miou": float(miou[0])}
    for k, name in enumerate(names):
        if present[1 + k]:
            point[f"miou_{name}"] = float(miou[1 + k])
    for kind in kinds:
        idx = [1 + names.index(f"{kind}_s{j}") for j in range(1, levels + 1)]
        m, p = M.replicate_miou(tot[0, idx].sum(0), c)
        if p:
            point[f"miou_{kind}"] = float(m)
    for name in list(point):
        n = name[len("miou_"):]
        if name.startswith("miou_") and n != "clean" and "miou_clean" in point:
            point[f"robustness_degradation_{n}"] = deg(point["miou_clean"], point[name])
    degs = [point[f"robustness_degradation_{w}"] for w in M.ADVERSE_KINDS if f"robustness_degradation_{w}" in point]
    if degs:
        point["robustness_degradation_ratio"] = float(np.mean(degs))
    return point


def test_one_source_every_replicate_is_the_total(M):
    c = 3
    pred, label, slots = random_frames(2, 1, 2, c)
    table = table_of(pred, label, c)
    rep = BR.replicate_sums(table, slots, 3, 77, 0, 16)
    assert (rep[:, 1] == table[0, 0]).all() and (rep[:, 2] == table[0, 1]).all() and (rep[:, 0] == table[0].sum(0)).all()
    names = ["clean", "fog"]
    res = M.bootstrap_metrics_from_replicates(rep, names, c, point_of(M, table, slots, names, c), 0.9, 77)
    assert res["miou_clean_ci_low"] == res["miou_clean_ci_high"] and res["miou_fog_se"] == 0.0


@pytest.mark.parametrize("better", ["clean", "fog"])
def test_identical_sources_give_zero_width_intervals(M, better):
    c, n = 4, 6
    pred, label, slots = random_frames(8, 1, 2, c, hw=200)
    if better == "fog":
        pred = pred[:, ::-1].copy()                                  # variant 1 (fog) now agrees more often than clean
    table = np.repeat(table_of(pred, label, c), n, axis=0)
    slots = np.repeat(slots, n, axis=0)
    names = ["clean", "fog"]
    point = point_of(M, table, slots, names, c)
    res = M.bootstrap_metrics_from_replicates(BR.replicate_sums(table, slots, 3, 1, 0, 50), names, c, point, seed=1)
    for q in ("overall_miou", "miou_clean", "miou_fog", "robustness_degradation_fog", "robustness_degradation_ratio", "miou_drop_fog"):
        assert res[f"{q}_ci_low"] == res[f"{q}_ci_high"] and res[f"{q}_se"] == 0.0, q
        assert abs(res[f"{q}_ci_low"] - (res[q] if q.startswith("miou_drop") else point[q])) < 1e-6, q
    assert res["miou_drop_fog"] == point["miou_clean"] - point["miou_fog"] and res["miou_drop_fog"] != 0
    assert res["miou_drop_fog_p_nonpositive"] == (1.0 if better == "fog" else 0.0)
    if better == "fog":
        assert res["robustness_degradation_fog_ci_high"] == 0.0      # the reference's clamp at 0 holds per replicate
    assert res["bootstrap_replicates"] == 50.0 and res["bootstrap_confidence"] == 0.95 and res["bootstrap_seed"] == 1.0


def test_two_class_accuracy_has_the_binomial_spread():
    """64 sources of equal size, half of them all right and half all wrong: a replicate's accuracy is Binomial(64, 1/2) / 64, standard
    deviation sqrt(0.25 / 64).  The spread of R = 4096 replicates estimates it to about 1 / sqrt(2 R) = 1.1 % (relative); the gate of
    5 % is about 4.5 sigma of that."""
    n, R, px = 64, 4096, 10
    label = np.tile(np.array([0, 1] * (px // 2), np.uint8), (n, 1, 1))
    pred = label.copy()
    pred[n // 2:] = 1 - pred[n // 2:]
    table = table_of(pred, label, 2)
    slots = np.ones((n, 1), np.int32)
    rep = BR.replicate_sums(table, slots, 2, 0, 0, R)
    acc = rep[:, 0, :2].sum(1) / rep[:, 0, 2:4].sum(1)
    assert (rep[:, 0, 2:4].sum(1) == n * px).all()
    want = np.sqrt(0.25 / n)
    assert abs(acc.std(ddof=1) / want - 1) < 0.05, acc.std(ddof=1) / want
    assert abs(acc.mean() - 0.5) < 4 * want / np.sqrt(R)


# ----------------------------------------------------------------------------- host side
def test_metrics_keys_quantiles_and_empty_replicates(M):
    c, R = 5, 300
    pred, label, slots = random_frames(21, 3, 3, c, hw=120)
    slots[1:, 1] = 0                                                  # fog on one source of three
    names = ["clean", "fog", "night"]
    table = table_of(pred, label, c)
    rep = BR.replicate_sums(table, slots, 4, 4, 0, R)
    point = point_of(M, table, slots, names, c)
    res = M.bootstrap_metrics_from_replicates(rep, names, c, point, 0.8, 4)
    miou, present = M.replicate_miou(rep, c)
    drawn = np.array([(BR.draws(4, q, 3) == 0).any() for q in range(R)])
    assert np.array_equal(present[:, 2], drawn) and 0 < drawn.sum() < R and present[:, [0, 1, 3]].all()
    assert res["bootstrap_empty_replicates_fog"] == float(R - drawn.sum())
    assert not any(k.startswith("bootstrap_empty_replicates_") and not k.endswith("_fog") for k in res)
    lo, hi = np.quantile(miou[drawn, 2], [0.1, 0.9], method="linear")
    assert res["miou_fog_ci_low"] == lo and res["miou_fog_ci_high"] == hi and res["miou_fog_se"] == np.std(miou[drawn, 2], ddof=1)
    lo, hi = np.quantile(miou[:, 3], [0.1, 0.9], method="linear")
    assert res["miou_night_ci_low"] == lo and res["miou_night_ci_high"] == hi
    deg = M.RobustnessMetrics().compute_robustness_degradation_ratio
    d = np.array([deg(float(a), float(b)) for a, b in zip(miou[drawn, 1], miou[drawn, 2])])
    assert res["robustness_degradation_fog_ci_low"] == np.quantile(d, 0.1) and res["robustness_degradation_fog_se"] == np.std(d, ddof=1)
    drop = miou[drawn, 1] - miou[drawn, 2]
    assert res["miou_drop_fog_p_nonpositive"] == float(np.mean(drop <= 0)) and res["miou_drop_fog"] == point["miou_clean"] - point["miou_fog"]
    ratio = np.mean([d, [deg(float(a), float(b)) for a, b in zip(miou[drawn, 1], miou[drawn, 3])]], axis=0)
    assert res["robustness_degradation_ratio_ci_high"] == np.quantile(ratio, 0.9)
    assert all(isinstance(v, float) for v in res.values()) and "miou_drop_clean" not in res
    # a quantity without a point estimate gets no interval; fewer than two valid replicates: no standard error
    del point["miou_night"], point["robustness_degradation_night"]
    res2 = M.bootstrap_metrics_from_replicates(rep, names, c, point, 0.8, 4)
    assert "miou_night_ci_low" not in res2 and "robustness_degradation_night_se" not in res2 and "miou_fog_ci_low" in res2
    one = M.bootstrap_metrics_from_replicates(rep[:1], names, c, point)
    assert np.isnan(one["miou_clean_se"]) and one["miou_clean_ci_low"] == one["miou_clean_ci_high"]
    for bad in (dict(confidence=0.0), dict(confidence=1.0)):
        with pytest.raises(ValueError):
            M.bootstrap_metrics_from_replicates(rep, names, c, point, **bad)
    with pytest.raises(ValueError):
        M.bootstrap_metrics_from_replicates(rep[:, :3], names, c, point)


def test_metrics_sweep_kinds_sum_their_levels(M):
    c, R = 4, 64
    names = ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2"]
    pred, label, slots = random_frames(33, 4, 5, c, hw=150)
    table = table_of(pred, label, c)
    rep = BR.replicate_sums(table, slots, 6, 2, 0, R)
    point = point_of(M, table, slots, names, c, kinds=("fog", "night"), levels=2)
    res = M.bootstrap_metrics_from_replicates(rep, names, c, point, 0.95, 2, kinds=("fog", "night"), levels=2)
    fog, _ = M.replicate_miou(rep[:, 2:4].sum(1), c)
    clean, _ = M.replicate_miou(rep[:, 1], c)
    assert res["miou_fog_ci_low"] == np.quantile(fog, 0.025) and res["miou_drop_fog_ci_high"] == np.quantile(clean - fog, 0.975)
    for k in ("miou_fog_s2_ci_low", "robustness_degradation_night_s1_se", "robustness_degradation_night_ci_high", "miou_drop_night_s2",
              "miou_drop_fog_s1_p_nonpositive", "robustness_degradation_ratio_ci_low", "miou_drop_fog_p_nonpositive"):
        assert k in res, k
    assert res["miou_drop_fog_s2_p_nonpositive"] <= 0.05             # the frames of level 2 flip far more pixels than the clean ones


def test_option_parser(H):
    assert H.bootstrap_options({}) is None and H.bootstrap_options({"evaluation.bootstrap_replicates": None}) is None
    assert H.bootstrap_options({"evaluation.bootstrap_replicates": 1000}) == {"replicates": 1000, "confidence": 0.95, "seed": 0, "sources": None}
    got = H.bootstrap_options({"evaluation.bootstrap_replicates": np.int64(65536), "evaluation.bootstrap_confidence": 0.5,
                               "evaluation.bootstrap_seed": 2 ** 63 - 1}, 20)
    assert got == {"replicates": 65536, "confidence": 0.5, "seed": 2 ** 63 - 1, "sources": 20}
    for key, bad in (("replicates", [0, -1, 65537, True, "100", 10.0]), ("confidence", [0, 1, 0.0, 1.0, -0.5, True, "0.9", float("nan")]),
                     ("seed", [-1, 2 ** 63, True, "3", 1.5])):
        for v in bad:
            with pytest.raises(ValueError, match=f"evaluation.bootstrap_{key}"):
                H.bootstrap_options({"evaluation.bootstrap_replicates": 10, f"evaluation.bootstrap_{key}": v})
    with pytest.raises(ValueError, match="bootstrap_seed"):          # checked even while the option is off, as depth_min is
        H.bootstrap_options({"evaluation.bootstrap_seed": -1})
    for n in (0, -3, True, 2.0):
        with pytest.raises(ValueError, match="sized dataset"):
            H.bootstrap_options({"evaluation.bootstrap_replicates": 10}, n)


def test_evaluate_model_needs_a_sized_dataset(H, M):
    class Loader:
        def __iter__(self):
            return iter(())
    with pytest.raises(ValueError, match="sized dataset"):
        H.evaluate_model(torch.nn.Identity(), Loader(), M.RobustnessMetrics(3, ["clean"]), "cpu", {"evaluation.bootstrap_replicates": 5})


def test_resampling_set_drops_missing_sources_and_refuses_duplicates(H):
    table = torch.arange(5 * 2 * 6, dtype=torch.int64).view(5, 2, 6)
    seen = torch.tensor([[1, 1], [0, 0], [1, 0], [0, 0], [0, 1]])
    slot = torch.tensor([[1, 2], [0, 0], [1, 0], [0, 0], [0, 2]])
    oob = torch.zeros(1, dtype=torch.int64)
    t, s, keep = H.bootstrap_resampling_set(table, seen, slot, oob)
    assert keep.tolist() == [0, 2, 4] and torch.equal(t, table[[0, 2, 4]]) and s.dtype == torch.int32 and s.tolist() == [[1, 2], [1, 0], [0, 2]]
    twice = seen.clone()
    twice[2, 0] = 2
    with pytest.raises(ValueError, match="source 2"):
        H.bootstrap_resampling_set(table, twice, slot, oob)
    with pytest.raises(IndexError):
        H.bootstrap_resampling_set(table, seen, slot, oob + 3)
    with pytest.raises(ValueError, match="no frame"):
        H.bootstrap_resampling_set(table, seen * 0, slot, oob)


def test_report_lines(M):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    base = {"overall_miou": 0.5, "miou_clean": 0.6, "miou_fog": 0.4, "robustness_degradation_fog": 1 / 3, "robustness_degradation_ratio": 1 / 3}
    plain = report_markdown(base)
    assert "- **Clean**: mIoU = 0.600\n" in plain and "[" not in plain and "## Bootstrap Intervals" not in plain
    on = dict(base, **{"miou_clean_ci_low": 0.55, "miou_clean_ci_high": 0.65, "miou_clean_se": 0.02, "miou_fog_ci_low": 0.3,
                       "miou_fog_ci_high": 0.5, "miou_fog_se": 0.05, "robustness_degradation_fog_ci_low": 0.0,
                       "robustness_degradation_fog_ci_high": 0.5, "robustness_degradation_fog_se": 0.1, "miou_drop_fog": 0.2,
                       "miou_drop_fog_ci_low": -0.1, "miou_drop_fog_ci_high": 0.3, "miou_drop_fog_se": 0.1, "miou_drop_fog_p_nonpositive": 0.125,
                       "bootstrap_replicates": 1000.0, "bootstrap_confidence": 0.9, "bootstrap_seed": 3.0, "bootstrap_sources": 20.0,
                       "bootstrap_empty_replicates_fog": 7.0})
    text = report_markdown(on)
    assert "- **Clean**: mIoU = 0.600 [0.550, 0.650]" in text and "- **Fog Degradation**: 0.333 [0.000, 0.500]" in text
    assert "- **Overall Degradation Ratio**: 0.333\n" in text        # no interval keys for it: the line stays as it was
    assert "## Bootstrap Intervals" in text and "1000 paired bootstrap replicates over 20 source frames" in text and "90 %" in text
    assert "| miou_drop_fog | 0.200 | -0.100 | 0.300 | 0.100 | 0.125 |" in text and "| miou_clean | 0.600 | 0.550 | 0.650 | 0.020 | - |" in text
    assert "labelled pixel of fog**: 7" in text
    sweep = dict(on, **{"severity_levels": 1.0, "severity_intensity_fog_s1": 0.3, "miou_fog_s1": 0.41, "miou_fog_s1_ci_low": 0.31,
                        "miou_fog_s1_ci_high": 0.51, "robustness_degradation_fog_s1": 0.2})
    assert "| 1 | 0.300 | 0.410 [0.310, 0.510] | 0.200 |" in report_markdown(sweep)


def test_command_line():
    spec = importlib.util.spec_from_file_location("awseg_evaluate_script", ROOT / "scripts" / "evaluate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()

    class Config(dict):
        set = dict.__setitem__
    args = ap.parse_args(["ckpt.pt"])
    assert args.bootstrap is None and args.bootstrap_confidence is None and args.bootstrap_seed is None
    cfg = Config()
    mod.apply_bootstrap_options(args, cfg)
    assert cfg == {}
    args = ap.parse_args(["ckpt.pt", "--severities", "reference", "--bootstrap", "1000", "--bootstrap-confidence", "0.9", "--bootstrap-seed", "7"])
    mod.apply_bootstrap_options(args, cfg)
    assert cfg == {"evaluation.bootstrap_replicates": 1000, "evaluation.bootstrap_confidence": 0.9, "evaluation.bootstrap_seed": 7}
    with pytest.raises(SystemExit):
        ap.parse_args(["ckpt.pt", "--bootstrap", "many"])
