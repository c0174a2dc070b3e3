"""The rain and snow removal front-end without a GPU (-m "not gpu"): properties of the numpy model (tests/deocclude_ref.py), the cap
on the fixtures of the GPU comparisons, the option and host math of the harness, the report and the command line, the bindings of
include/awseg_restore.h and the launcher's argument checks on host pointers."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import deocclude_ref as D

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "awseg_restore.h"
MEAN, STD = D.IMAGENET_MEAN, D.IMAGENET_STD
H, W = 64, 96


def frame_of(v, **kw):
    return D.deocclude_frame(D.normalise(v), MEAN, STD, **kw)


def within_the_window(J, clean, mask, r):
    """The distance the fills are held to: a filled value is a mean of unmasked pixels of its window, so it lies between the window
    minimum and maximum of the occluder-free scene, up to the 2^-16 grid of q (half a unit per term, one more for the normalising
    round trip of the scene)."""
    v = D.unit(D.normalise(clean), MEAN, STD)
    lo, hi = D.window(v, r, np.minimum, np.float32(np.inf)), D.window(v, r, np.maximum, np.float32(-np.inf))
    m = mask != 0
    slack = 2.0 ** -15
    return bool((J[:, m] >= lo[:, m] - slack).all() and (J[:, m] <= hi[:, m] + slack).all())


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("r", [1, 2, 9, 15])
def test_the_opening_never_exceeds_the_frame(r):
    rng = np.random.default_rng(r)
    for shape in ((3, 5, 7), (3, 33, 65)):
        v = rng.random(shape).astype(np.float32)
        o = D.opening(v, r)
        assert (o <= v).all() and np.isfinite(o).all()
        e = D.window(v, r, np.minimum, np.float32(np.inf))
        assert (e <= v).all() and (e <= o).all()
    # every window larger than the frame: the minimum and the opening are the frame's minimum
    small = rng.random((3, 5, 7)).astype(np.float32)
    if r >= 7:
        assert (D.opening(small, r) == small.min(axis=(1, 2), keepdims=True)).all()


def test_a_frame_without_seeds_comes_back_as_it_came():
    bg = D.background(H, W, 1)
    f = frame_of(bg)
    assert not f["seed"].any() and not f["mask"].any() and f["row"][D.SEEDS:D.CHANGE + 1].tolist() == [0, 0, 0, 0]
    assert f["J"].tobytes() == f["v"].tobytes() and f["row"][D.PIXELS] == H * W and f["row"][D.FRAMES] == 1
    # bright but wide, and thin but coloured: neither is a seed
    wide = bg.copy()
    wide[:, 10:50, 20:70] = 0.95
    pole = bg.copy()
    pole[0, :, 40:43] = 1.0                                             # a thin red pole lifts one channel only
    dim = bg.copy()
    dim[:, :, 40] = np.minimum(bg[:, :, 40] + 0.2, 0.45)                # a thin line that is lifted but stays darker than bright_min
    for v in (wide, pole, dim):
        assert not frame_of(v)["mask"].any()


@pytest.mark.parametrize("thick", [1, 3])
def test_bright_lines_are_masked_and_filled_from_the_background(thick):
    bg = D.background(H, W, 2)
    v = bg.copy()
    v[:, :, 40:40 + thick] = 1.0
    f = frame_of(v)
    assert f["mask"][:, 40:40 + thick].all() and f["mask"][:, 39].all() and f["mask"][:, 40 + thick].all()    # with the rim of d = 1
    assert not f["mask"][:, :38].any() and not f["mask"][:, 42 + thick:].any()
    assert f["row"][D.SEEDS] == H * thick and f["row"][D.MASKED] == H * (thick + 2) and f["row"][D.UNFILLED] == 0
    assert within_the_window(f["J"], bg, f["mask"], 9) and f["row"][D.CHANGE] > 0
    assert np.abs(f["J"] - v)[:, f["mask"] == 0].max() < 2.0 ** -20     # the round trip through the normalisation, nothing else


@pytest.mark.parametrize("radius", [2, 8])
def test_discs_are_masked_at_r9_and_the_large_one_is_not_at_r2(radius):
    bg = D.background(H, W, 3)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (yy - 32) ** 2 + (xx - 48) ** 2 <= radius * radius
    v = bg.copy()
    v[:, disc] = 1.0
    f = frame_of(v)
    assert f["mask"][disc].all() and f["seed"][disc].all() and f["row"][D.SEEDS] == disc.sum() and f["row"][D.UNFILLED] == 0
    assert within_the_window(f["J"], bg, f["mask"], 9)
    small = frame_of(v, radius=2)
    if radius == 8:
        # the window (5 x 5) is smaller than the flake: the opening keeps it but for the narrow parts of its round rim
        assert not small["mask"][32 - 4:32 + 5, 48 - 4:48 + 5].any() and small["mask"][disc].mean() < 0.25
    else:
        assert small["mask"][disc].all()


def test_filled_square_is_kept():
    """A filled square of side 2 r + 2 d + 3 is wider than the window: the opening returns it whole, its top-hat is 0 and nothing
    is masked.  (It cannot leave pixels unfilled: what does is the ruled square of unfilled_frame.)"""
    bg = D.background(H, W, 4)
    f = frame_of(D.draw_square(bg, 2 * 9 + 2 * 1 + 3))
    assert not f["mask"].any() and f["row"][D.UNFILLED] == 0


@pytest.mark.parametrize("r,d", [(9, 1), (4, 2), (15, 2)])
def test_a_ruled_square_leaves_its_middle_unfilled_and_as_it_was(r, d):
    x = D.unfilled_frame(80, 112, r, d)
    f = D.deocclude_frame(x[0], MEAN, STD, radius=r, dilate=d)
    assert f["row"][D.UNFILLED] > 0 and f["row"][D.UNFILLED] == f["unfilled"].sum() and (f["N"][f["unfilled"]] == 0).all()
    assert (f["mask"][f["unfilled"]] == 1).all() and f["J"][:, f["unfilled"]].tobytes() == f["v"][:, f["unfilled"]].tobytes()
    assert f["restored"][:, f["unfilled"]].tobytes() == np.stack([(f["v"][c] - MEAN[c]) / STD[c] for c in range(3)])[:, f["unfilled"]].tobytes()
    filled = (f["mask"] != 0) & ~f["unfilled"]
    assert filled.any() and (f["N"][filled] > 0).all()


def test_counters_add_up_over_a_split_batch_and_follow_the_slot_rule():
    x = D.occluder_batch((3, 3, 33, 65), 5)
    whole = D.deocclude(x)[2]
    parts = D.deocclude(x[:1])[2] + D.deocclude(x[1:])[2]
    assert whole.tolist() == parts.tolist() and whole[0, D.FRAMES] == 3 and whole[0, D.PIXELS] == 3 * 33 * 65
    restored, mask, stats = D.deocclude(x, cond=[1, -1, 1], n_slots=3)
    rows = [D.deocclude_frame(x[b], MEAN, STD)["row"] for b in range(3)]
    assert (stats[0] == rows[0] + rows[1] + rows[2]).all() and not stats[1].any() and (stats[2] == rows[0] + rows[2]).all()
    assert restored.shape == x.shape and mask.shape == (3, 33, 65) and mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    lone = D.deocclude(x, cond=[5, 1, -3], n_slots=2)[2]               # a condition that is no slot reaches slot 0 only
    assert lone[0].tolist() == whole[0].tolist() and not lone[1].any()


def test_values_that_are_not_finite_are_counted_and_act_as_zero_or_one():
    x = D.nonfinite_frame(40, 72, 8)
    f = D.deocclude_frame(x[0], MEAN, STD)
    assert f["row"][D.NONFINITE] == 3 and np.isfinite(f["restored"]).all()
    assert f["v"][0, 20, 36] == 0 and f["v"][1, 1, 2] == 1 and f["v"][2, 39, 71] == 0
    clean = x.copy()
    clean[0, 0, 20, 36], clean[0, 1, 1, 2], clean[0, 2, 39, 71] = D.normalise(np.array([0.0, 1.0, 0.0], np.float32).reshape(3, 1, 1)).reshape(3)
    g = D.deocclude_frame(clean[0], MEAN, STD)
    assert g["row"][D.NONFINITE] == 0 and g["mask"].tobytes() == f["mask"].tobytes() and g["restored"].tobytes() == f["restored"].tobytes()


def test_the_float32_fill_stays_within_its_stated_bound_of_the_float64_one():
    worst = 0.0
    for _, x, kw, _ in D.gpu_cases():
        for b in range(x.shape[0]):
            v = D.unit(x[b], MEAN, STD)
            mask = D.detect(v, kw["radius"], 0.06, 0.5, kw["dilate"])["mask"]
            j32, j64 = D.fill(v, mask, kw["radius"])["J"], D.fill(v, mask, kw["radius"], float64=True)["J"]
            assert j32.dtype == np.float32 and j64.dtype == np.float64
            worst = max(worst, float(np.abs(j32.astype(np.float64) - j64).max()))
    assert 0.0 < worst <= D.FILL_F32_BOUND                              # and not vacuous: some fill is no float32 number
    # the extremes of the quotient: all ones, one unit in 961
    for s, n in ((961 * 65536, 961), (1, 961), (65535, 1), (2 ** 26 - 1, 960)):
        q = np.float64(s) / (np.float64(n) * 65536.0)
        assert abs(float(np.float32(q)) - float(q)) <= D.FILL_F32_BOUND


def test_the_fixtures_of_the_gpu_comparisons_are_not_vacuous():
    """Every occluder fixture used on the GPU masks between 2 % and 50 % of its pixels, and at least one leaves pixels unfilled."""
    unfilled = 0
    for name, x, kw, shift in D.gpu_cases():
        stats = D.deocclude(x, **kw)[2][0]
        share = stats[D.MASKED] / stats[D.PIXELS]
        assert 0.02 <= share <= 0.50, (name, share)
        assert stats[D.SEEDS] > 0 and stats[D.CHANGE] > 0 and shift in (0, 1)
        unfilled += int(stats[D.UNFILLED])
    assert unfilled > 0
    shapes = {(x.shape, kw["radius"], kw["dilate"]) for _, x, kw, _ in D.gpu_cases()}
    assert {((1, 3, 33, 65), 9, 1), ((2, 3, 40, 72), 9, 1), ((1, 3, 5, 7), 9, 1), ((3, 3, 37, 70), 15, 2), ((1, 3, 64, 128), 1, 0)} <= shapes


def test_rendered_rain_and_snow_gain_fidelity():
    """Occluders drawn as the renderer draws them (streaks and discs under a blur) come back closer to the scene than they went: a
    masked value sat more than the threshold above its opened surroundings and is replaced by a mean of them.  How much closer is
    the benchmark's question, not this test's: a one-pixel streak under the 3 x 3 blur keeps a third of its height and mostly
    stays below bright_min."""
    bg = D.background(96, 128, 9)
    psnr = lambda a: -10.0 * np.log10(np.mean((a.astype(np.float64) - bg) ** 2))           # noqa: E731
    for v in (D.draw_streaks(bg, 30, 30, 1, 1), D.draw_streaks(bg, 12, 30, 3, 2), D.draw_discs(bg, 25, 2, 3, 3, lift=0.0)):
        f = frame_of(v)
        assert f["row"][D.MASKED] > 0 and psnr(f["J"]) > psnr(v), (psnr(f["J"]), psnr(v))


# ---------------------------------------------------------------------------------------------------------------- the harness
def test_restoration_option_accepts_tophat_and_refuses_what_is_not_its_own():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness
    opt = harness.restoration_option
    f32 = lambda v: float(np.float32(v))                                                    # noqa: E731
    dark = {"radius": 7, "omega": f32(0.95), "t_min": f32(0.1), "airlight_min": f32(0.1), "refine": 1, "conditions": None}
    clahe = {"method": "clahe", "grid": (8, 8), "clip_limit": 2.0, "max_gain": 8.0, "white_balance": True, "conditions": None}
    default = {"method": "tophat", "radius": 9, "threshold": f32(0.06), "bright_min": 0.5, "dilate": 1, "conditions": None}
    assert harness.RESTORATION_METHODS == ("dark_channel", "clahe", "tophat")
    # every spec accepted before returns what it returned
    assert opt({}) is None
    assert opt({"evaluation.restoration": "dark_channel"}) == dark == opt({"evaluation.restoration": {"method": "dark_channel"}})
    assert opt({"evaluation.restoration": {"radius": 3, "refine": "none"}}) == dict(dark, radius=3, refine=0)
    assert opt({"evaluation.restoration": {"method": "dark_channel", "radius": 15}}) == dict(dark, radius=15)
    guided = opt({"evaluation.restoration": {"refine": "guided", "radius": 5}})
    assert guided == {"radius": 5, "omega": f32(0.95), "t_min": f32(0.1), "airlight_min": f32(0.1), "guided_radius": 20,
                      "guided_eps": f32(1e-3), "refine": "guided", "conditions": None}
    assert opt({"evaluation.restoration": "clahe"}) == clahe
    assert opt({"evaluation.restoration": {"method": "clahe", "grid": [4, 6]}, "evaluation.restoration_conditions": ["night"]}) \
        == dict(clahe, grid=(4, 6), conditions=["night"])
    # the new method
    assert opt({"evaluation.restoration": "tophat"}) == default == opt({"evaluation.restoration": {"method": "tophat"}})
    got = opt({"evaluation.restoration": {"method": "tophat", "radius": 15, "threshold": 1, "bright_min": 0, "dilate": 0},
               "evaluation.restoration_conditions": ["rain", "snow"]})
    assert got == {"method": "tophat", "radius": 15, "threshold": 1.0, "bright_min": 0.0, "dilate": 0, "conditions": ["rain", "snow"]}
    assert opt({"evaluation.restoration": {"method": "tophat", "radius": 2, "dilate": 2}}) == dict(default, radius=2, dilate=2)
    tophat = lambda **kw: {"evaluation.restoration": {"method": "tophat", **kw}}            # noqa: E731
    for bad in ({"radius": 0}, {"radius": 16}, {"radius": 9.0}, {"radius": True}, {"radius": "9"}, {"threshold": 0}, {"threshold": 1.5},
                {"threshold": float("nan")}, {"threshold": "0.06"}, {"threshold": None}, {"bright_min": -0.1}, {"bright_min": 1.01},
                {"bright_min": float("nan")}, {"bright_min": True}, {"dilate": -1}, {"dilate": 3}, {"dilate": 1.0}, {"window": 7},
                {"omega": 0.9}, {"t_min": 0.1}, {"airlight_min": 0.1}, {"refine": "none"}, {"refine": "guided"}, {"guided_radius": 8},
                {"guided_eps": 0.01}, {"grid": 8}, {"clip_limit": 2.0}, {"max_gain": 8}, {"white_balance": "none"}):
        with pytest.raises(ValueError, match="evaluation.restoration"):
            opt(tophat(**bad))
    # its keys under the other methods, with or without their name (radius belongs to the dark channel there)
    for bad in ({"threshold": 0.06}, {"bright_min": 0.5}, {"dilate": 1}, {"method": "dark_channel", "dilate": 1},
                {"method": "clahe", "threshold": 0.06}, {"method": "clahe", "dilate": 1}, {"method": "clahe", "radius": 9},
                {"method": "top_hat"}, {"method": "TOPHAT"}, "top-hat", "white_tophat"):
        with pytest.raises(ValueError, match="evaluation.restoration"):
            opt({"evaluation.restoration": bad})
    for bad in ("rain", [], [3]):
        with pytest.raises(ValueError, match="restoration_conditions"):
            opt({"evaluation.restoration": "tophat", "evaluation.restoration_conditions": bad})
    assert opt({"evaluation.restoration": "tophat"}, images=torch.zeros(2, 3, 4, 5)) == default
    with pytest.raises(ValueError, match="float32"):
        opt({"evaluation.restoration": "tophat"}, images=torch.zeros(2, 1, 4, 5))


def test_deocclude_parameters_are_checked_and_float32():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    f32 = lambda v: float(np.float32(v))                                                    # noqa: E731
    assert ops.deocclude_parameters() == {"radius": 9, "threshold": f32(0.06), "bright_min": 0.5, "dilate": 1}
    assert ops.deocclude_parameters() == ops.deocclude_parameters(**ops.DEOCCLUDE_DEFAULTS) and ops.DEOCCLUDE_DEFAULTS == D.DEFAULTS
    p = ops.deocclude_parameters(radius=np.int64(3), threshold=np.float32(0.1), bright_min=0, dilate=np.int32(2))
    assert p == {"radius": 3, "threshold": f32(0.1), "bright_min": 0.0, "dilate": 2}
    for kw in ({"radius": 0}, {"radius": 16}, {"radius": 2.0}, {"threshold": 0.0}, {"threshold": 1.0001}, {"threshold": float("nan")},
               {"bright_min": -1e-9}, {"bright_min": 1.5}, {"bright_min": "0.5"}, {"dilate": 3}, {"dilate": -1}, {"dilate": True}):
        with pytest.raises(ValueError, match="deocclude"):
            ops.deocclude_parameters(**kw)
    assert ops.DEOCCLUDE_ROW == len(ops.DEOCCLUDE_FIELDS) == D.ROW == 7 and ops.DEOCCLUDE_MAX_DILATE == D.MAX_DILATE
    assert ops.new_deocclude_stats("cpu", 3).shape == (3, 7) and ops.new_deocclude_stats("cpu", 3).dtype == torch.int64
    with pytest.raises(ValueError):
        ops.new_deocclude_stats("cpu", 0)
    dec = ops.deocclude_stats_to_numpy(np.arange(14).reshape(2, 7))
    assert list(dec) == list(ops.DEOCCLUDE_FIELDS) and dec["unfilled_pixels"].tolist() == [4, 11]
    assert list(ops.DEOCCLUDE_FIELDS).index("sum_change") == D.CHANGE and list(ops.DEOCCLUDE_FIELDS).index("nonfinite_values") == D.NONFINITE
    with pytest.raises(ValueError):
        ops.deocclude_stats_to_numpy(np.zeros((2, 8), np.int64))


def _rows():
    """Hand-made counters for ['clean', 'rain', 'snow', 'fog']: fog was not selected, clean has pixels but no occluder."""
    stats = np.zeros((5, 7), np.int64)
    stats[1] = [2, 1000, 0, 0, 0, 0, 0]
    stats[2] = [1, 500, 20, 50, 0, 150 * 6554, 4]
    stats[3] = [1, 500, 40, 100, 25, 300 * 32768, 0]
    stats[0] = stats[1:].sum(0)
    return stats


def test_deocclude_metrics_from_hand_made_counters():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import deocclude_metrics_from_stats
    stats, names = _rows(), ["clean", "rain", "snow", "fog"]
    res = deocclude_metrics_from_stats(stats, names)
    assert res.pop("restoration_method") == "tophat" and all(isinstance(v, float) for v in res.values())
    assert res["occluder_fraction_rain"] == 0.1 and res["occluder_seed_fraction_rain"] == 0.04
    assert res["occluder_unfilled_fraction_rain"] == 0.0 and res["occluder_change_rain"] == 6554 / 65536
    assert res["occluder_fraction_snow"] == 0.2 and res["occluder_unfilled_fraction_snow"] == 0.25 and res["occluder_change_snow"] == 0.5
    assert res["occluder_fraction_clean"] == 0.0 and res["occluder_seed_fraction_clean"] == 0.0
    assert res["mean_occluder_fraction"] == 150 / 2000 and res["mean_occluder_seed_fraction"] == 60 / 2000
    assert res["mean_occluder_unfilled_fraction"] == 25 / 150
    assert res["mean_occluder_change"] == (150 * 6554 + 300 * 32768) / 65536 / 450
    assert res["restoration_nonfinite_values"] == 4.0
    # absent denominators: no key, never a 0
    for key in ("occluder_unfilled_fraction_clean", "occluder_change_clean", "occluder_fraction_fog", "occluder_seed_fraction_fog",
                "occluder_unfilled_fraction_fog", "occluder_change_fog"):
        assert key not in res
    assert deocclude_metrics_from_stats(np.zeros_like(stats), names) == {"restoration_method": "tophat"}
    with pytest.raises(ValueError):
        deocclude_metrics_from_stats(stats[:, :6], names)
    with pytest.raises(ValueError):
        deocclude_metrics_from_stats(stats, names[:3])


def test_deocclude_metrics_pool_the_levels_of_a_kind_under_a_sweep():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import deocclude_metrics_from_stats
    slots = ["clean", "rain_s1", "rain_s2"]
    stats = np.zeros((4, 7), np.int64)
    stats[1] = [1, 100, 0, 0, 0, 0, 0]
    stats[2] = [1, 100, 4, 10, 0, 30 * 16384, 0]
    stats[3] = [1, 100, 12, 30, 10, 90 * 49152, 0]
    stats[0] = stats[1:].sum(0)
    res = deocclude_metrics_from_stats(stats, slots, kinds=["rain"], levels=2)
    assert res["occluder_fraction_rain_s1"] == 0.1 and res["occluder_fraction_rain_s2"] == 0.3 and res["occluder_fraction_rain"] == 0.2
    assert res["occluder_unfilled_fraction_rain"] == 0.25 and res["occluder_change_rain"] == (30 * 16384 + 90 * 49152) / 65536 / 120
    assert res["occluder_seed_fraction_rain"] == 16 / 200 and "occluder_change_clean" not in res


def test_report_names_the_method_and_prints_the_occluder_columns():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    results = {"miou_clean": 0.8, "miou_rain": 0.5, "miou_clean_restored": 0.79, "miou_rain_restored": 0.6, "overall_miou_restored": 0.7,
               "restoration_gain_clean": -0.01, "restoration_gain_rain": 0.1, "occluder_fraction_clean": 0.03, "occluder_fraction_rain": 0.12,
               "occluder_change_clean": 0.2, "occluder_change_rain": 0.45, "mean_occluder_fraction": 0.075, "mean_occluder_change": 0.4,
               "mean_occluder_unfilled_fraction": 0.015, "restoration_clean_cost": 0.01, "mean_restoration_gain": 0.045,
               "restoration_method": "tophat", "restoration_nonfinite_values": 3.0}
    text = report_markdown(results)
    assert "## Input Restoration" in text and "Method: tophat" in text and "| Occluders | Change |" in text
    assert "Mean t" not in text and "Luma gain" not in text and "Airlight" not in text
    assert "| clean | 0.800 | 0.790 | -0.010 | 0.030 | 0.200 |" in text and "| rain | 0.500 | 0.600 | 0.100 | 0.120 | 0.450 |" in text
    assert "| all | - | 0.700 | 0.045 | 0.075 | 0.400 |" in text
    assert "left unfilled** (no unmasked pixel in their window): 0.015" in text and "Clean cost" in text and "not finite**: 3" in text
    # the other two methods print what they printed
    dark = {k: v for k, v in results.items() if "occluder" not in k and k != "restoration_method"}
    dark.update({"transmission_mean_clean": 0.9, "transmission_mean_rain": 0.4})
    text = report_markdown(dark)
    assert "Method: dark_channel" in text and "Mean t" in text and "Occluders" not in text and "| clean | 0.800 | 0.790 | -0.010 | 0.900 |" in text
    relit = dict(dark, restoration_method="clahe", relight_gain_clean=1.1, mean_relight_gain=1.4, mean_relight_capped_fraction=0.125)
    text = report_markdown(relit)
    assert "Method: clahe" in text and "Luma gain" in text and "Occluders" not in text and "| all | - | 0.700 | 0.045 | 1.400 | 0.125 |" in text


def test_command_line_sets_the_tophat_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_cli_deocclude", ROOT / "scripts" / "evaluate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness

    class Config(dict):
        set = dict.__setitem__
    ap = mod.build_parser()
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "tophat"]), cfg)
    assert cfg == {"evaluation.restoration": "tophat"} and harness.restoration_option(cfg)["radius"] == 9
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "tophat", "--restoration-radius", "5", "--restoration-threshold",
                                                 "0.125", "--restoration-bright-min", "0.25", "--restoration-dilate", "2",
                                                 "--restoration-conditions", "rain,snow"]), cfg)
    assert harness.restoration_option(cfg) == {"method": "tophat", "radius": 5, "threshold": 0.125, "bright_min": 0.25, "dilate": 2,
                                               "conditions": ["rain", "snow"]}
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "tophat", "--restoration-dilate", "0"]), cfg)
    assert cfg == {"evaluation.restoration": {"method": "tophat", "dilate": 0}}
    # the flags of one method are refused with another; the new ones without tophat
    for flags in (["--restoration", "tophat", "--restoration-refine", "none"], ["--restoration", "tophat", "--restoration-guided-radius", "8"],
                  ["--restoration", "tophat", "--restoration-guided-eps", "0.01"], ["--restoration", "tophat", "--restoration-grid", "8"],
                  ["--restoration", "tophat", "--restoration-clip-limit", "2"], ["--restoration", "tophat", "--restoration-max-gain", "4"],
                  ["--restoration", "tophat", "--restoration-white-balance", "none"], ["--restoration-threshold", "0.1"],
                  ["--restoration-radius", "9"], ["--restoration", "dark_channel", "--restoration-dilate", "1"],
                  ["--restoration", "clahe", "--restoration-bright-min", "0.5"], ["--restoration", "clahe", "--restoration-radius", "9"]):
        with pytest.raises(ValueError, match="--restoration"):
            mod.apply_restoration_options(ap.parse_args(["ckpt.pt", *flags]), Config())
    # the harness has the last word on the ranges
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "tophat", "--restoration-dilate", "3"]), cfg)
    with pytest.raises(ValueError, match="evaluation.restoration"):
        harness.restoration_option(cfg)
    # the other methods as before; the radius reaches the dark channel under its own name
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "dark_channel", "--restoration-refine", "none"]), cfg)
    assert cfg == {"evaluation.restoration": {"refine": "none"}}
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "dark_channel"]), cfg)
    assert cfg == {"evaluation.restoration": "dark_channel"}
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "clahe", "--restoration-grid", "8"]), cfg)
    assert cfg == {"evaluation.restoration": {"method": "clahe", "grid": 8}}
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "dark_channel", "--restoration-radius", "3"]), cfg)
    assert harness.restoration_option(cfg)["radius"] == 3 and "method" not in harness.restoration_option(cfg)


# --------------------------------------------------------------------------------------------------------------- the bindings
def test_bindings_declare_export_and_size_the_deocclude_entry_points():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc import build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(awseg_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(N.EXTENSION_SIGNATURES) and {"awseg_deocclude", "awseg_deocclude_workspace"} <= set(names)
    for name in names:                                                  # every prototype, with its argument count
        args = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(N.EXTENSION_SIGNATURES[name][1]), name
    assert len(N.EXTENSION_SIGNATURES["awseg_deocclude"][1]) == 18 and "deocclude.hip" in build.SOURCES
    raw = ctypes.CDLL(str(build.build()))
    assert hasattr(raw, "awseg_deocclude") and hasattr(raw, "awseg_deocclude_workspace")
    lib = N.lib()
    assert lib.awseg_abi_version() == 1 and lib.awseg_restore_header_hash() == build.header_hash(build.RESTORE_HEADER) != 0
    defines = dict(re.findall(r"#define\s+(AWSEG_DEOCCLUDE_\w+)\s+(\d+)", HEADER.read_text()))
    assert ops.DEOCCLUDE_ROW == int(defines["AWSEG_DEOCCLUDE_ROW"]) and ops.DEOCCLUDE_MAX_DILATE == int(defines["AWSEG_DEOCCLUDE_MAX_DILATE"])
    for b, h, w in ((1, 1, 1), (2, 5, 7), (8, 1024, 2048), (65535, 16, 1), (0, 0, 0)):
        assert lib.awseg_deocclude_workspace(b, h, w) == ops.deocclude_workspace_bytes(b, h, w) == 0


def test_the_deocclude_launcher_refuses_every_invalid_argument_before_any_launch():
    """Host-side only: the buffers are host memory of the right sizes, so each refusal below has exactly one reason and has to come
    before anything is launched."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N
    lib = N.lib()
    b, h, w = 2, 5, 7
    image, restored = np.zeros((b, 3, h, w), np.float32), np.full((b, 3, h, w), 7.0, np.float32)
    mask, stats = np.full((b, h, w), 7, np.uint8), np.zeros((2, 7), np.int64)
    ws = np.zeros(2, np.int64)
    cond = np.zeros(b, np.int32)
    mean, std = MEAN.copy(), STD.copy()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
    good = {"image": ptr(image), "batch": b, "channels": 3, "height": h, "width": w, "mean": ptr(mean), "std": ptr(std), "radius": 9,
            "threshold": 0.06, "bright_min": 0.5, "dilate": 1, "cond": ptr(cond), "restored": ptr(restored), "mask": ptr(mask),
            "stats": ptr(stats), "n_slots": 2, "workspace": ptr(ws), "stream": None}
    bad_std, bad_mean = np.array([0.2, 0.0, 0.2], np.float32), np.array([0.4, np.inf, 0.4], np.float32)
    nan_std = np.array([0.2, np.nan, 0.2], np.float32)
    einval = [("image", None), ("mean", None), ("std", None), ("restored", None), ("mask", None), ("stats", None),
              ("channels", 1), ("channels", 4), ("batch", -1), ("height", 0), ("width", 0), ("height", -3), ("n_slots", 0),
              ("radius", 0), ("radius", -1), ("radius", 16), ("threshold", 0.0), ("threshold", -0.5), ("threshold", 1.001),
              ("threshold", float("nan")), ("threshold", float("inf")), ("bright_min", -0.001), ("bright_min", 1.001),
              ("bright_min", float("nan")), ("dilate", -1), ("dilate", 3), ("std", ptr(bad_std)), ("std", ptr(nan_std)), ("mean", ptr(bad_mean))]
    for name, value in einval:
        args = dict(good, **{name: value})
        assert lib.awseg_deocclude(*args.values()) == -1, (name, value)
    assert lib.awseg_deocclude(*dict(good, batch=65536).values()) == -2
    assert lib.awseg_deocclude(*dict(good, height=1 << 16, width=1 << 15).values()) == -2
    odd = ctypes.c_void_p(ws.ctypes.data + 4)
    assert lib.awseg_deocclude(*dict(good, workspace=odd).values()) == -3
    assert lib.awseg_deocclude(*dict(good, batch=0).values()) == 0                          # nothing to do, nothing launched
    assert lib.awseg_deocclude(*dict(good, batch=0, cond=None, workspace=None).values()) == 0      # a workspace of no bytes may be NULL
    assert lib.awseg_deocclude(*dict(good, batch=0, radius=15, threshold=1.0, bright_min=0.0, dilate=0).values()) == 0
    assert lib.awseg_deocclude(*dict(good, batch=0, radius=1, bright_min=1.0, dilate=2).values()) == 0
    assert (restored == 7.0).all() and (mask == 7).all() and not stats.any() and not ws.any()


def test_ops_deocclude_checks_its_arguments_and_has_no_cpu_path():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    x = torch.zeros(1, 3, 4, 5)
    with pytest.raises(N.AwsegError, match="no CPU fallback"):
        ops.deocclude(x)
    for bad in (torch.zeros(1, 1, 4, 5), torch.zeros(1, 3, 4, 5, dtype=torch.float64), torch.zeros(3, 4, 5)):
        with pytest.raises(ValueError, match="float32"):
            ops.deocclude(bad)
    for kw in ({"radius": 0}, {"radius": 16}, {"threshold": 0}, {"bright_min": 2}, {"dilate": 3}, {"mean": [0.5] * 3},
               {"mean": [0.5] * 3, "std": [0.2, 0.0, 0.2]}, {"stats": torch.zeros(2, 8, dtype=torch.int64)},
               {"stats": torch.zeros(2, 10, dtype=torch.int64)}, {"cond": torch.zeros(2, dtype=torch.int32)},
               {"out": torch.zeros(1, 3, 4, 6)}, {"out": x}, {"mask": torch.zeros(1, 4, 5)}, {"mask": torch.zeros(1, 4, 6, dtype=torch.uint8)},
               {"mask": torch.zeros(1, 3, 4, 5, dtype=torch.uint8)}):
        with pytest.raises(ValueError):
            ops.deocclude(x, **kw)
    with pytest.raises(ValueError, match="new_deocclude_stats"):
        ops.deocclude(x, stats=torch.zeros(2, 8, dtype=torch.int64))
    out, mask = ops.deocclude(torch.zeros(0, 3, 4, 5))                  # nothing to do: no launch, so no device either
    assert tuple(out.shape) == (0, 3, 4, 5) and tuple(mask.shape) == (0, 4, 5) and mask.dtype == torch.uint8
