"""CPU tests (-m "not gpu") of the paired severity sweep: the schedule, the configuration check, the host math on hand-made
counters, the report section and the numpy model of tests/paired_ref.py."""
import math

import numpy as np
import pytest
import torch

from tests import paired_ref as PR
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import (REFERENCE_SEVERITIES, _Loader, paired_plan,
                                                                                     resolve_severities)
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import severity_sweep_results
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown

CONDS = ["clean", "fog", "rain", "snow", "night"]


@pytest.mark.parametrize("n,bs,world", [(20, 8, 1), (20, 8, 2), (20, 3, 3), (7, 4, 2), (5, 8, 4), (1, 2, 1)])
def test_paired_plan_covers_every_source_in_order(n, bs, world):
    kinds, sev = ("fog", "night"), [0.3, 0.6, 0.9]
    seen_clean, seen_var, owner = {}, {}, {}
    total = 0
    for rank in range(world):
        plan = paired_plan(n, bs, kinds, sev, rank, world)
        total += len(plan)
        per = (n + world - 1) // world
        assert all(rank * per <= it.start and it.start + it.n <= min((rank + 1) * per, n) for it in plan)
        for pos, it in enumerate(plan):
            assert 1 <= it.n <= bs
            for s in range(it.start, it.start + it.n):
                assert owner.setdefault(s, rank) == rank                 # every variant of a source on the rank that owns it
                if it.level == 0:
                    assert it.kind == "clean" and it.intensity is None and s not in seen_clean
                    seen_clean[s] = pos
                else:
                    assert s in seen_clean and seen_clean[s] < pos       # clean first
                    assert it.intensity == sev[it.level - 1]
                    seen_var.setdefault(s, []).append((it.kind, it.level))
        # the loader's length is the plan's batch count
        ds = type("D", (), {"weather_schedule": "paired", "plan": lambda self, b, d, r, w: paired_plan(n, b, kinds, sev, r, w, d),
                            "__len__": lambda self: n})()
        assert len(_Loader(ds, bs, False, rank, world)) == len(plan)
    assert sorted(seen_clean) == list(range(n))
    for s in range(n):
        assert sorted(seen_var[s]) == sorted((k, j) for k in kinds for j in (1, 2, 3))
    per = (n + world - 1) // world
    groups = sum(-(-len(range(min(r * per, n), min((r + 1) * per, n))) // bs) for r in range(world))
    assert total == groups * (1 + len(kinds) * len(sev))


def test_paired_plan_partial_last_group_and_drop_last():
    plan = paired_plan(5, 2, ["fog"], {"fog": [0.5]}, 0, 1)
    assert [(it.start, it.n, it.kind, it.level) for it in plan] == [(0, 2, "clean", 0), (0, 2, "fog", 1), (2, 2, "clean", 0), (2, 2, "fog", 1),
                                                                     (4, 1, "clean", 0), (4, 1, "fog", 1)]
    assert len(paired_plan(5, 2, ["fog"], [0.5], 0, 1, drop_last=True)) == 4


def test_reference_preset_and_forms():
    sw = resolve_severities("reference", CONDS)
    assert sw.kinds == ("fog", "rain", "snow", "night") and sw.levels == 3
    assert sw.intensities == {"fog": (0.3, 0.6, 0.9), "rain": (0.2, 0.5, 0.8), "snow": (0.2, 0.45, 0.7), "night": (0.4, 0.6, 0.8)}
    assert {k: tuple(v) for k, v in REFERENCE_SEVERITIES.items()} == sw.intensities
    sw = resolve_severities([0.1, 1.0], ["clean", "night", "fog"])
    assert sw.kinds == ("night", "fog") and sw.intensities == {"night": (0.1, 1.0), "fog": (0.1, 1.0)}
    assert sw.slots() == ["clean", "night_s1", "night_s2", "fog_s1", "fog_s2"]
    sw = resolve_severities({"fog": [0.2], "rain": [0.4]}, ["clean", "fog", "rain"])
    assert sw.intensities == {"fog": (0.2,), "rain": (0.4,)}


@pytest.mark.parametrize("spec,conds,rng,match", [
    ([0.3, 1.2], CONDS, "philox", "in \\[0, 1\\]"),
    ([-0.1], CONDS, "philox", "in \\[0, 1\\]"),
    ([float("nan")], CONDS, "philox", "in \\[0, 1\\]"),
    ([math.inf], CONDS, "philox", "in \\[0, 1\\]"),
    ({"fog": [0.3, 0.5], "rain": [0.3]}, ["clean", "fog", "rain"], "philox", "same number"),
    ({"fog": [0.3], "hail": [0.3]}, ["clean", "fog"], "philox", "not adverse kinds"),
    ([0.3], ["clean"], "philox", "at least one adverse kind"),
    ([0.3], ["fog", "night"], "philox", "must contain 'clean'"),
    ([0.3], CONDS, "numpy", "philox"),
    ([], CONDS, "philox", "empty"),
    ("strong", CONDS, "philox", "unknown preset"),
])
def test_severities_rejected(spec, conds, rng, match):
    with pytest.raises(ValueError, match=match):
        resolve_severities(spec, conds, rng)


def _cons(slots, rows):
    """decoded consistency counters from per-slot (A, T); slot 0 is their sum."""
    C = rows[0][0].shape[0]
    A = np.zeros((1 + len(slots), C, C), np.int64)
    T = np.zeros((1 + len(slots), 4), np.int64)
    for k, (a, t) in enumerate(rows):
        A[2 + k], T[2 + k] = a, t                           # slot 1 is 'clean': never counted
    A[0], T[0] = A.sum(0), T.sum(0)
    return {"agreement": A, "transitions": T}


def test_host_math_on_hand_made_counters():
    C = 3
    slots = ["clean", "fog_s1", "fog_s2"]
    same = np.diag([5, 3, 2]).astype(np.int64)                 # perfect agreement
    perm = np.array([[0, 4, 0], [0, 0, 6], [2, 0, 0]], np.int64)   # every pixel moved to another class
    cons = _cons(slots, [(same, np.array([7, 0, 0, 3])), (perm, np.array([0, 6, 0, 4]))])
    r = severity_sweep_results(cons, slots, ["fog"], 2, {"fog": (0.3, 0.9)}, 4, {"clean": 0.5, "fog_s1": 0.5, "fog_s2": 0.25})
    assert r["consistency_fog_s1"] == 1.0 and r["corruption_error_rate_fog_s1"] == 0.0 and r["consistency_miou_fog_s1"] == 1.0
    assert r["consistency_fog_s2"] == 0.0 and r["corruption_error_rate_fog_s2"] == 1.0 and r["consistency_miou_fog_s2"] == 0.0
    # pooled keys are ratios of the summed counters
    assert r["consistency_fog"] == (10 + 0) / (10 + 12)
    assert r["mean_consistency"] == r["consistency_fog"]
    assert r["mean_corruption_error_rate"] == 6 / (7 + 6)
    assert r["robustness_degradation_fog_s1"] == 0.0 and r["robustness_degradation_fog_s2"] == 0.5
    assert r["severity_intensity_fog_s2"] == 0.9 and r["paired_sources"] == 4.0 and r["severity_levels"] == 2.0
    assert all(isinstance(v, float) for v in r.values())


def test_host_math_pools_two_kinds():
    C = 2
    slots = ["clean", "fog_s1", "night_s1"]
    a1, a2 = np.array([[3, 1], [0, 4]], np.int64), np.array([[1, 1], [1, 1]], np.int64)
    cons = _cons(slots, [(a1, np.array([2, 1, 0, 1])), (a2, np.array([1, 1, 1, 1]))])
    r = severity_sweep_results(cons, slots, ["fog", "night"], 1, {"fog": (0.5,), "night": (0.5,)}, 2, {})
    assert r["consistency_fog"] == 7 / 8 and r["consistency_night"] == 0.5
    assert r["mean_consistency"] == (7 + 2) / (8 + 4)
    assert r["mean_corruption_error_rate"] == (1 + 1) / (3 + 2)
    assert "robustness_degradation_fog_s1" not in r                  # no mIoU given


def test_report_section_present_only_with_the_sweep():
    base = {"overall_miou": 0.5, "miou_clean": 0.6, "miou_fog": 0.4, "robustness_degradation_fog": 0.33, "robustness_degradation_ratio": 0.33,
            "expected_calibration_error": 0.1}
    plain = report_markdown(dict(base))
    assert "Severity Sweep" not in plain
    sweep = dict(base, paired_sources=4.0, severity_levels=2.0, severity_intensity_fog_s1=0.3, severity_intensity_fog_s2=0.9,
                 miou_fog_s1=0.5, miou_fog_s2=0.3, consistency_fog_s1=0.9, consistency_fog_s2=0.7, corruption_error_rate_fog_s1=0.05,
                 corruption_error_rate_fog_s2=0.2, robustness_degradation_fog_s1=0.16, robustness_degradation_fog_s2=0.5,
                 mean_consistency=0.8, mean_corruption_error_rate=0.12)
    md = report_markdown(sweep)
    assert md.startswith(plain)                                    # the report without the sweep keys is unchanged
    assert "## Severity Sweep" in md and "### Fog" in md
    assert "| 2 | 0.900 | 0.300 | 0.500 | 0.700 | 0.200 |" in md


def test_numpy_model_counts():
    ref = np.array([0, 1, 2, 2, 3, 1], np.uint8)
    var = np.array([0, 2, 2, 1, 1, 7], np.uint8)
    lab = np.array([0, 1, 1, 255, 2, 1], np.uint8)
    row, oob = PR.consistency_counts(var, ref, lab, 4)
    A = row[:16].reshape(4, 4)
    assert oob == 1 and A.sum() == 5 and A[0, 0] == 1 and A[1, 2] == 1 and A[2, 2] == 1 and A[2, 1] == 1 and A[3, 1] == 1
    # labelled: px0 both correct, px1 ref correct var wrong, px2 ref wrong var wrong(2 vs 1), px4 both wrong
    assert row[16:].tolist() == [1, 1, 0, 2]
