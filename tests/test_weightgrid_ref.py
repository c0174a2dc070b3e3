"""The numpy model of the ensemble weight sweep (tests/weightgrid_ref.py) against hand-made 2 x 2-pixel cases, the host math of
evaluation.metrics.weight_grid_metrics_from_stats on hand-filled counters, and the option evaluation.ensemble_weight_grid.  No GPU.

The first three tests check the MODEL alone (the oracle the GPU tests compare with): they use no code of the package and so do not
depend on the feature; every test from the host math on does."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import weightgrid_ref as WR

from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics

INF, NAN = np.inf, np.nan


def _members(p1, p2):
    """Per-pixel class vectors of a 2 x 2 frame -> members float32 [1, C, 2, 2]."""
    a = np.asarray(p1, np.float32).T.reshape(1, -1, 2, 2)
    b = np.asarray(p2, np.float32).T.reshape(1, -1, 2, 2)
    return a, b


# ----------------------------------------------------------------------------- the model on hand-made frames
def test_argmax_rule_first_maximum_and_nan():
    v = np.array([[1, 3, 3, 0], [NAN, 5, 0, 0], [0, NAN, 9, NAN], [2, 2, 2, 2], [-INF, -INF, -INF, -INF], [0, INF, INF, 1]], np.float32)
    assert WR.argmax_rule(v).tolist() == [1, 0, 1, 0, 0, 1]
    assert WR.argmax_rule(v).tolist() == torch.from_numpy(v).argmax(dim=1).tolist()


def test_hand_made_frame_ties_nan_and_inf():
    # pixel 0: both members tie classes 0 and 1 -> the first maximum, class 0, at every weight
    # pixel 1: SegFormer says class 0 (3 against 0), DeepLab class 1 (1 against 0): 0.25 * 3 == 0.75 * 1 ties at (0.25, 0.75) and the
    #          first class keeps it; at (0.125, 0.875) 0.375 < 0.875 -> class 1; at (0.5, 0.5) 1.5 > 0.5 -> class 0
    # pixel 2: a NaN in SegFormer's class 0: it wins SegFormer's own argmax and every combined argmax (0 * NaN is NaN too)
    # pixel 3: +inf in SegFormer's class 1: at the end (0, 1) 0 * inf is NaN and wins, although DeepLab alone says class 2
    p1 = [[1, 1, 0], [3, 0, 0], [NAN, 5, 0], [0, INF, 0]]
    p2 = [[1, 1, 0], [0, 1, 0], [0, 0, 9], [0, 0, 4]]
    s1, s2 = _members(p1, p2)
    w = np.array([[0, 1], [0.125, 0.875], [0.25, 0.75], [0.5, 0.5], [1, 0]], np.float32)
    label = np.array([[[0, 1], [2, 2]]], np.uint8)
    st = WR.counters(s1, s2, w, label)
    C, G = 3, 5
    assert st.shape == (1, G + 3, 2 * C)
    preds = {0: [0, 1, 0, 1], 1: [0, 1, 0, 1], 2: [0, 0, 0, 1], 3: [0, 0, 0, 1], 4: [0, 0, 0, 1]}     # per grid point, pixels 0 .. 3
    lab = [0, 1, 2, 2]
    for g, pr in preds.items():
        hits = [sum(1 for p, t in zip(pr, lab) if p == t == c) for c in range(C)]
        cnt = [pr.count(c) for c in range(C)]
        assert st[0, g].tolist() == hits + cnt, g
    # members alone: m1 = [0, 0, 0 (NaN), 1 (inf)], m2 = [0, 1, 2, 2]
    assert st[0, G].tolist() == [1, 1, 2] + [1, 0, 0]                 # labelled per class | both right (pixel 0)
    assert st[0, G + 1].tolist() == [0, 0, 0] + [0, 1, 2]             # only SegFormer | only DeepLab (pixels 1, 2, 3)
    assert st[0, G + 2].tolist() == [0, 1, 3, 0, 0, 0]                # out of range, NaN pixels, m1 != m2
    # the end (0, 1) is NOT DeepLab alone: pixel 3 is predicted 1 there, DeepLab's own argmax is 2 and counted right
    assert st[0, 0, 2] == 0 and st[0, G + 1, C + 2] == 2


def test_labels_slots_and_ignore_index():
    s1, s2 = _members([[2, 0, 0], [0, 2, 0], [0, 0, 2], [2, 0, 0]], [[2, 0, 0], [0, 2, 0], [0, 2, 0], [0, 0, 2]])
    s1, s2 = np.concatenate([s1, s1, s1]), np.concatenate([s2, s2, s2])
    label = np.array([[0, 1, 2, 255], [0, 7, 2, 0], [-1, 1, 1, 200]], np.int64)
    w = np.array([[0.5, 0.5]], np.float32)
    st = WR.counters(s1, s2, w, label, cond=[1, -1, 5], n_slots=3)
    assert st[0, 1, :3].tolist() == [3, 3, 2] and st[0, 3, 0] == 3           # labelled per class; 7, -1 and 200 are out of range
    assert st[1].sum() == 0                                                  # no frame has condition 0
    assert st[2, 1, :3].tolist() == [1, 1, 1] and st[2, 3, 0] == 0           # frame 0 only; frames 1 (-1) and 2 (5 >= 2) go to slot 0 alone
    # with ignore_index 0 the class-0 labels leave the labelled pixels and 255 becomes an out-of-range value
    st0 = WR.counters(s1, s2, w, label, ignore_index=0)
    assert st0[0, 1, :3].tolist() == [0, 3, 2] and st0[0, 3, 0] == 4


# ----------------------------------------------------------------------------- host math on hand-filled counters
C = 19
GRID = np.array([[0, 1], [0.25, 0.75], [0.5, 0.5], [0.75, 0.25], [1, 0], [0.625, 0.375]], np.float32)      # the last one: configured
G = len(GRID)


def _slot(ious, both=0, only1=0, only2=0, disagree=0, n=8):
    """One slot with classes 0 and 1 labelled n pixels each; ious[g] = (hits of class 0, hits of class 1): the misses of a class are
    predicted as the other one, so IoU_c = hits_c / (2 n - hits_other)."""
    s = np.zeros((G + 3, 2 * C), np.int64)
    for g, (h0, h1) in enumerate(ious):
        s[g, 0], s[g, 1] = h0, h1
        s[g, C + 0], s[g, C + 1] = h0 + (n - h1), h1 + (n - h0)
    s[G, 0] = s[G, 1] = n
    s[G, C + 0], s[G + 1, 0], s[G + 1, C + 1] = both, only1, only2
    s[G + 2, 2] = disagree
    return s


def _expect(h0, h1, n=8):
    return WR.miou([h0, h1], [n, n], [h0 + n - h1, h1 + n - h0])


def test_host_math_best_fitted_regret_and_gain():
    conds = ["clean", "fog", "night"]
    clean = _slot([(0, 8), (4, 8), (8, 8), (8, 8), (8, 4), (8, 8)], both=10, only1=3, only2=2, disagree=5)      # 1.0 at shares 0.5, 0.75, 0.625
    fog = _slot([(8, 8), (8, 4), (8, 0), (4, 0), (0, 0), (8, 0)], both=4, only1=0, only2=8, disagree=9)         # best at share 0
    night = _slot([(0, 0)] * G)
    stats = np.stack([clean + fog + night, clean, fog, night])
    res = metrics.weight_grid_metrics_from_stats(stats, conds, C, GRID, G - 1)
    assert res["ensemble_weight_grid"] == [0.0, 0.25, 0.5, 0.75, 1.0, 0.625]
    # clean: three points tie at mIoU 1; the one nearest the configured share 0.625 is the configured point itself
    assert res["ensemble_weight_best_clean"] == 0.625 and res["miou_best_weight_clean"] == 1.0
    assert res["ensemble_weight_fitted"] == 0.625
    assert res["miou_weight_gain_clean"] == 0.0 and res["miou_weight_regret_clean"] == 0.0
    assert res["miou_configured_weight_clean"] == 1.0 and res["miou_configured_weight_fog"] == _expect(8, 0)
    assert res["ensemble_weight_miou_curve_clean"] == [_expect(0, 8), _expect(4, 8), 1.0, 1.0, _expect(8, 4), 1.0]
    assert res["segformer_miou_clean"] == _expect(8, 4) and res["deeplabv3plus_miou_clean"] == _expect(0, 8)
    # fog: its own best is DeepLab alone; the clean-fitted weighting loses the difference there
    assert res["ensemble_weight_best_fog"] == 0.0 and res["miou_best_weight_fog"] == 1.0
    assert res["miou_fitted_weight_fog"] == _expect(8, 0)
    assert res["miou_weight_regret_fog"] == 1.0 - _expect(8, 0)
    assert res["miou_weight_gain_fog"] == 0.0                                # the fitted point is the configured one
    assert res["member_both_right_fog"] == 4 / 16 and res["member_only_segformer_fog"] == 0.0
    assert res["member_only_deeplabv3plus_fog"] == 8 / 16 and res["member_neither_right_fog"] == 4 / 16
    assert res["member_oracle_accuracy_fog"] == 0.75 and res["member_disagreement_fog"] == 9 / 16
    # night: every point has mIoU 0 -> a tie over the whole grid, broken towards the configured share
    assert res["ensemble_weight_best_night"] == 0.625 and res["miou_best_weight_night"] == 0.0
    # slot 0 carries no regret key; the unnamed keys describe every frame
    assert "miou_weight_regret" not in res and "ensemble_weight_best" in res and "member_oracle_accuracy" in res
    assert "weight_grid_out_of_range_labels" not in res and "weight_grid_nan_pixels" not in res


def test_host_math_ties_go_to_the_nearest_share_then_the_lower_index():
    grid = np.array([[0, 1], [0.25, 0.75], [0.75, 0.25], [1, 0], [0.5, 0.5]], np.float32)
    g = len(grid)

    def slot(rows):
        s = np.zeros((g + 3, 2 * C), np.int64)
        for k, h in enumerate(rows):
            s[k, 0], s[k, C] = h, 8
        s[g, 0] = 8
        return s
    # shares 0.25 and 0.75 are equally far from the configured 0.5: the lower index wins
    res = metrics.weight_grid_metrics_from_stats(np.stack([slot([0, 6, 6, 0, 2])] * 2), ["clean"], C, grid, g - 1)
    assert res["ensemble_weight_best_clean"] == 0.25 and res["ensemble_weight_fitted"] == 0.25
    assert res["miou_weight_gain_clean"] == WR.miou([6], [8], [8]) - WR.miou([2], [8], [8])
    # shares 0 and 0.75 tie: 0.75 is nearer the configured 0.5
    res = metrics.weight_grid_metrics_from_stats(np.stack([slot([6, 1, 6, 0, 2])] * 2), ["clean"], C, grid, g - 1)
    assert res["ensemble_weight_best_clean"] == 0.75
    # a fitting condition that was not seen: no fitted point, hence no gain or regret
    res = metrics.weight_grid_metrics_from_stats(np.stack([slot([6, 1, 6, 0, 2])] * 2), ["fog"], C, grid, g - 1)
    assert "ensemble_weight_fitted" not in res and "miou_weight_gain_fog" not in res and res["ensemble_weight_best_fog"] == 0.75
    assert res["miou_configured_weight_fog"] == WR.miou([2], [8], [8])
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    assert "| fog | 0.143 | - | 0.600 | 0.750 |" in report_markdown(res)         # no fitted point: the configured mIoU is still printed


def test_host_math_kind_pooling_counts_and_empty():
    slots = ["clean", "fog_s1", "fog_s2"]
    clean = _slot([(0, 8), (4, 8), (8, 8), (8, 8), (8, 4), (8, 8)])
    f1 = _slot([(8, 8), (8, 4), (8, 0), (4, 0), (0, 0), (8, 0)])
    f2 = _slot([(0, 0), (0, 4), (0, 8), (8, 8), (8, 8), (0, 8)])
    stats = np.stack([clean + f1 + f2, clean, f1, f2])
    stats[0, G + 2, 0], stats[0, G + 2, 1] = 3, 2
    res = metrics.weight_grid_metrics_from_stats(stats, slots, C, GRID, G - 1, kinds=["fog"], levels=2)
    pooled = f1 + f2                                                         # summed BEFORE the ratio
    curve = [WR.miou(pooled[g, :C], pooled[G, :C], pooled[g, C:]) for g in range(G)]
    best = max(range(G), key=lambda g: curve[g])
    assert res["ensemble_weight_best_fog"] == float(GRID[best, 0])
    assert res["miou_weight_regret_fog"] == curve[best] - curve[G - 1]
    assert res["ensemble_weight_best_fog_s1"] == 0.0 and res["ensemble_weight_best_fog_s2"] == 0.75
    assert res["weight_grid_out_of_range_labels"] == 3.0 and res["weight_grid_nan_pixels"] == 2.0
    assert metrics.weight_grid_metrics_from_stats(np.zeros_like(stats), slots, C, GRID, G - 1, kinds=["fog"], levels=2) == {}
    assert metrics.weight_grid_metrics_from_stats(torch.zeros(4, G + 3, 2 * C, dtype=torch.int64), slots, C, GRID, G - 1) == {}
    for bad in (dict(stats=stats[:3]), dict(stats=stats[:, :-1]), dict(grid=GRID[:-1]), dict(idx=G), dict(idx=-1), dict(idx=True)):
        with pytest.raises(ValueError):
            metrics.weight_grid_metrics_from_stats(bad.get("stats", stats), slots, C, bad.get("grid", GRID), bad.get("idx", G - 1))


def test_row_miou_is_the_confusion_matrix_rule():
    rs = np.random.RandomState(3)
    cm = rs.randint(0, 1000, (C, C)).astype(np.int64)
    cm[5] = 0
    cm[:, 5] = 0                                                             # a class without a union
    want = metrics.iou_from_counts(torch.from_numpy(cm.reshape(-1)), C)["mean_iou"]
    assert metrics.weight_grid_row_miou(np.diag(cm), cm.sum(1), cm.sum(0)) == want
    assert metrics.weight_grid_row_miou(np.zeros(C), np.zeros(C), np.zeros(C)) is None


# ----------------------------------------------------------------------------- the option
def _ensemble(weights=(0.3, -0.2), strategy="weighted_average"):
    return SimpleNamespace(segformer=object(), deeplabv3plus=object(), ensemble_weights=torch.tensor(weights), ensemble_strategy=strategy)


def test_option_is_off_by_default():
    assert harness.weight_grid_option({}) is None
    assert harness.weight_grid_option({"evaluation.ensemble_weight_grid": None}, _ensemble()) is None
    assert harness.weight_grid_option({"evaluation.weight_grid_condition": "fog"}) is None


def test_option_integer_list_and_the_appended_configured_point():
    base = {"data.weather_conditions": ["clean", "fog"]}
    opt = harness.weight_grid_option(dict(base, **{"evaluation.ensemble_weight_grid": 5}))
    assert opt == {"shares": [0.0, 0.25, 0.5, 0.75, 1.0], "condition": "clean"}
    own = torch.softmax(torch.tensor([0.3, -0.2]), 0).numpy()
    opt = harness.weight_grid_option(dict(base, **{"evaluation.ensemble_weight_grid": 4}), _ensemble())
    a = np.array([0, 1 / 3, 2 / 3, 1], np.float32)
    assert opt["pairs"].dtype == np.float32 and opt["pairs"].shape == (5, 2) and opt["configured_index"] == 4
    assert np.array_equal(opt["pairs"][:4], np.stack([a, np.float32(1) - a], 1)) and np.array_equal(opt["pairs"][4], own)
    # a list: 0 and 1 are added when missing, and only then
    for spec, want in (([0.3], [0.0, 0.3, 1.0]), ([0, 0.5], [0.0, 0.5, 1.0]), ((0.25, 1), [0.0, 0.25, 1.0]), ([0.0, 1.0], [0.0, 1.0]),
                       (np.array([0.5]), [0.0, 0.5, 1.0])):
        assert harness.weight_grid_option(dict(base, **{"evaluation.ensemble_weight_grid": spec}))["shares"] == want
    top = harness.weight_grid_option(dict(base, **{"evaluation.ensemble_weight_grid": 63}), _ensemble())
    assert top["pairs"].shape == (64, 2) and top["configured_index"] == 63
    inner = [k / 62 for k in range(1, 62)]                                  # 61 shares + both ends = 63
    assert len(harness.weight_grid_option(dict(base, **{"evaluation.ensemble_weight_grid": inner}))["shares"]) == 63
    opt = harness.weight_grid_option(dict(base, **{"evaluation.ensemble_weight_grid": 2, "evaluation.weight_grid_condition": "fog"}))
    assert opt["condition"] == "fog"
    # under a severity sweep the slots are known to the evaluation state only: any name passes here
    assert harness.weight_grid_option({"evaluation.ensemble_weight_grid": 2, "evaluation.severities": [0.5],
                                       "evaluation.weight_grid_condition": "fog_s1"})["condition"] == "fog_s1"


@pytest.mark.parametrize("spec", [True, False, 1, 64, -3, 0, 0.5, "11", "0.2,0.4", {"n": 5}, [], [0.5, 0.5], [0.6, 0.4], [-0.1, 0.5],
                                  [0.5, 1.5], [float("nan")], [0.5, float("inf")], [True], ["0.5"], [None], [0.5, [0.6]],
                                  [k / 64 for k in range(1, 64)], [k / 63 for k in range(64)], np.float32(3), b"5"])
def test_option_rejects(spec):
    with pytest.raises(ValueError, match="evaluation.ensemble_weight_grid"):
        harness.weight_grid_option({"data.weather_conditions": ["clean"], "evaluation.ensemble_weight_grid": spec})


def test_option_rejects_conditions_and_models():
    on = {"data.weather_conditions": ["clean", "fog"], "evaluation.ensemble_weight_grid": 3}
    for cond in ("night", "", 3, True, ["clean"]):
        with pytest.raises(ValueError, match="weight_grid_condition"):
            harness.weight_grid_option(dict(on, **{"evaluation.weight_grid_condition": cond}))
    with pytest.raises(ValueError, match="weight_grid_condition"):               # checked also when the option is off
        harness.weight_grid_option({"evaluation.weight_grid_condition": 3})
    with pytest.raises(ValueError, match="no two members"):
        harness.weight_grid_option(on, SimpleNamespace(backbone=object()))
    with pytest.raises(ValueError, match="no two members"):
        harness.weight_grid_option(on, torch.nn.Linear(2, 2))
    for strategy in ("mean", "max_confidence"):
        with pytest.raises(ValueError, match="weighted_average"):
            harness.weight_grid_option(on, _ensemble(strategy=strategy))


def test_report_section():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    conds = ["clean", "fog"]
    clean = _slot([(0, 8), (4, 8), (8, 8), (8, 8), (8, 4), (8, 8)], both=10, only1=3, only2=2)
    fog = _slot([(8, 8), (8, 4), (8, 0), (4, 0), (0, 0), (8, 0)], both=4, only2=8)
    res = metrics.weight_grid_metrics_from_stats(np.stack([clean + fog, clean, fog]), conds, C, GRID, G - 1)
    text = report_markdown(res)
    assert "## Ensemble Weights" in text and "| fog | 0.250 | 0.250 | 1.000 | 0.000 | 0.000 | 1.000 | 0.750 |" in text
    assert "## Ensemble Weights" not in report_markdown({"overall_miou": 0.5})
