"""Test-time augmentation without a GPU (-m "not gpu"): structural facts of the numpy model (tests/tta_ref.py), the float32 model
against its float64 twin, the option, the host math, the report table and the command line of the harness, the bindings of the
two launchers and their argument checks on host pointers."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import tta_ref as T

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "awseg_restore.h"
EINVAL, ERANGE, EALIGN = -1, -2, -3
RESAMPLED = [((3, 5), (6, 10)), ((5, 7), (8, 12)), ((2, 3), (8, 12)), ((8, 12), (5, 7)), ((9, 16), (3, 4)), ((5, 7), (5, 12)),
             ((64, 96), (128, 192)), ((192, 288), (128, 192)), ((1, 1), (4, 6)), ((7, 1), (3, 5))]


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("hw", [(1, 1), (1, 4), (3, 5), (3, 8), (6, 7)])
def test_equal_size_is_the_identity_and_with_flip_an_exact_mirror(hw):
    x = T.maps(1, (2, 3) + hw)
    x[0, 0, 0, 0] = np.float32(-0.0)
    assert T.view(x, hw, False).tobytes() == x.tobytes()
    assert T.view(x, hw, True).tobytes() == np.ascontiguousarray(x[..., ::-1]).tobytes()
    zero = np.zeros_like(x)
    assert T.accumulate(x, zero, False, 1.0, T.SET).tobytes() == x.tobytes()
    assert T.accumulate(x, zero, True, 1.0, T.SET).tobytes() == np.ascontiguousarray(x[..., ::-1]).tobytes()
    # mirrored twice: the view's un-view is the frame
    assert T.accumulate(T.view(x, hw, True), zero, True, 1.0, T.SET).tobytes() == x.tobytes()


@pytest.mark.parametrize("flip", [False, True])
def test_one_inf_at_equal_size_gives_exactly_one_inf(flip):
    x = T.maps(2, (1, 2, 4, 8))
    x[0, 1, 2, 3] = np.inf
    for out in (T.view(x, (4, 8), flip), T.accumulate(x, np.zeros_like(x), flip, 0.25, T.SET)):
        assert np.isinf(out).sum() == 1 and not np.isnan(out).any()
        assert np.isinf(out[0, 1, 2, 4 if flip else 3])


def test_a_neighbour_of_weight_zero_does_not_poison_a_pixel():
    """Going up from 2 x 3, the first row and column sample at f = 0 exactly: their second taps weigh nothing.  A NaN or inf there
    reaches only the pixels it has a share in."""
    x = T.maps(3, (1, 1, 2, 3))
    x[0, 0, 1, 1] = np.inf
    out = T.view(x, (8, 12), False)
    y0, y1, ly0, ly1 = T.axis_taps(2, 8)
    x0, x1, lx0, lx1 = T.axis_taps(3, 12)
    touched = ((y0 == 1) | ((y1 == 1) & (ly1 != 0)))[:, None] & ((x0 == 1) | ((x1 == 1) & (lx1 != 0)))[None, :]
    assert (ly1[:2] == 0).all() and (lx1[:2] == 0).all() and not touched[:2].any() and not touched[:, :2].any()
    assert np.array_equal(~np.isfinite(out[0, 0]), touched) and np.isfinite(out[0, 0, :2]).all() and np.isfinite(out[0, 0, :, :2]).all()


@pytest.mark.parametrize("src,dst", RESAMPLED[:6])
@pytest.mark.parametrize("flip", [False, True])
def test_a_view_and_its_un_view_of_a_constant_map_is_that_constant(src, dst, flip):
    """The weights of an axis are l and 1 - l in float32, and their float32 sum is 1 (1 - l rounds by at most 2^-25, which the sum
    rounds away again).  For c a power of two the products with them are exact, so (1 - l) c + l c is c; a general c may come
    back an ulp off, which is the arithmetic of the header and no fault of the kernel."""
    for c in (0.0, 1.0, -2.0, 64.0, 2.0 ** -20):
        x = np.full((2, 3) + src, c, np.float32)
        v = T.view(x, dst, flip)
        assert (v == np.float32(c)).all()
        back = T.accumulate(v, np.zeros_like(x), flip, 1.0, T.SET)
        assert (back == np.float32(c)).all()


def test_the_accumulator_mirrors_first_and_resamples_then():
    """interpolate(flip(L)) is the contract; flip(interpolate(L)) differs in bits where the ratio is ragged."""
    x = T.maps(4, (1, 2, 5, 7))
    first = T.accumulate(x, np.zeros((1, 2, 8, 12), np.float32), True, 1.0, T.SET)
    assert first.tobytes() == T.sample(np.ascontiguousarray(x[..., ::-1]), (8, 12)).tobytes()
    other = np.ascontiguousarray(T.sample(x, (8, 12))[..., ::-1])
    assert first.tobytes() != other.tobytes() and np.allclose(first, other, atol=1e-5)
    # the view mirrors last
    assert T.view(x, (8, 12), True).tobytes() == other.tobytes()


def test_the_three_modes_round_each_product_and_each_sum():
    x, acc = T.maps(5, (2, 3, 5, 7)), T.maps(6, (2, 3, 8, 12))
    w = np.float32(1) / np.float32(3)
    u = T.sample(x, (8, 12))
    assert T.accumulate(x, acc, False, w, T.SET).tobytes() == (w * u).tobytes()
    assert T.accumulate(x, acc, False, w, T.ADD).tobytes() == (acc + w * u).tobytes()
    assert T.accumulate(x, acc, False, w, T.SCALE_ADD).tobytes() == (w * acc + w * u).tobytes()
    assert (w * acc + w * u).tobytes() != (w * (acc + u)).tobytes()
    with pytest.raises(ValueError):
        T.accumulate(x, acc, False, w, 3)


def test_taps_follow_the_header():
    y0, y1, l0, l1 = T.axis_taps(5, 8)
    f = np.maximum(np.float32(5 / 8) * (np.arange(8, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), 0)
    assert y0.tolist() == [0, 0, 1, 1, 2, 2, 3, 4] and y1.tolist() == [1, 1, 2, 2, 3, 3, 4, 4]
    assert l1.tobytes() == (f - y0.astype(np.float32)).tobytes() and l0.tobytes() == (np.float32(1) - l1).tobytes()
    down = T.axis_taps(9, 3)
    assert down[0].tolist() == [1, 4, 7] and down[1].tolist() == [2, 5, 8] and (down[3] == 0).all()      # cells are skipped


@pytest.mark.parametrize("src,dst", RESAMPLED)
@pytest.mark.parametrize("flip", [False, True])
def test_float32_model_against_its_float64_twin(src, dst, flip):
    """|U32 - U64| <= 2^-21 (S + 1) D + 2^-22 M, with S the larger source extent, D the largest difference between adjacent source
    values and M the largest magnitude.

    The coordinate: sy = float32(h / H) carries a relative error of 2^-24; (float) y + 0.5 is exact below 2^23; the product rounds
    once more (2^-24 relative) and the subtraction of 0.5 a third time, so |f32 - f64| <= 3 * 2^-24 * S per axis, f being at most
    S.  The taps may differ between the two models where f sits at a whole number, but bilinear interpolation is continuous
    there and Lipschitz in each coordinate with the constant D, so the two axes together move U by at most 6 * 2^-24 S D
    < 2^-21 S D.  ly1 = f - y0 is exact (both lie in one binade or f < 1), ly0 = 1 - ly1 rounds by at most 2^-24, which moves a
    blend of two values no more than D apart by 2^-24 D per axis: the "+ 1".  The blend itself rounds four times on the path of
    any one value (a product and a sum for the row pair, a product and a sum for the column pair), each by at most 2^-24 of a
    magnitude no larger than M: 4 * 2^-24 M = 2^-22 M."""
    x = T.maps(7, (2, 3) + src, lo=-30.0, hi=30.0)
    dx = np.abs(np.diff(x, axis=-1)).max() if src[1] > 1 else 0.0
    dy = np.abs(np.diff(x, axis=-2)).max() if src[0] > 1 else 0.0
    S, D, M = max(src), float(max(dx, dy)), float(np.abs(x).max())
    bound = 2.0 ** -21 * (S + 1) * D + 2.0 ** -22 * M
    lo, hi = T.view(x, dst, flip), T.view(x, dst, flip, dtype=np.float64)
    assert lo.dtype == np.float32 and hi.dtype == np.float64
    assert float(np.abs(lo.astype(np.float64) - hi).max()) <= bound
    zero = np.zeros((2, 3) + dst, np.float32)
    lo, hi = T.accumulate(x, zero, flip, 1.0, T.SET), T.accumulate(x, zero, flip, 1.0, T.SET, dtype=np.float64)
    assert float(np.abs(lo.astype(np.float64) - hi).max()) <= bound
    assert float(np.abs(hi).max()) <= M * (1 + 1e-12)                  # a convex combination


# ----------------------------------------------------------------------------------------------------------------- the option
def test_option_presets_added_scale_and_view_order():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness as H
    assert H.tta_option({}) is None and H.tta_option({"evaluation.tta": None}) is None
    flip = H.tta_option({"evaluation.tta": "flip"})
    assert flip == {"scales": [1.0], "flip": True} and H.tta_views(flip) == [(1.0, True)]
    ms = H.tta_option({"evaluation.tta": "ms_flip"})
    assert ms == {"scales": [0.5, 0.75, 1.0, 1.25, 1.5], "flip": True}
    assert H.tta_views(ms) == [(0.5, False), (0.5, True), (0.75, False), (0.75, True), (1.0, True), (1.25, False), (1.25, True),
                               (1.5, False), (1.5, True)]
    added = H.tta_option({"evaluation.tta": {"scales": [0.5, 1.5], "flip": False}})
    assert added == {"scales": [0.5, 1.0, 1.5], "flip": False} and H.tta_views(added) == [(0.5, False), (1.5, False)]
    assert H.tta_option({"evaluation.tta": {"scales": [0.5, 1.0]}}) == {"scales": [0.5, 1.0], "flip": True}      # flip defaults to true
    assert H.tta_option({"evaluation.tta": {"scales": (0.25, 2)}})["scales"] == [0.25, 1.0, 2.0]
    eight = [0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    assert H.tta_option({"evaluation.tta": {"scales": eight}})["scales"] == eight
    assert H.tta_option({"evaluation.tta": {}}) == flip


def test_option_size_rule():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness as H
    assert H.tta_view_size(128, 192, 1.0) == (128, 192) and H.tta_view_size(100, 50, 1.0) == (100, 50)      # the frame's own size
    assert H.tta_view_size(128, 192, 0.5) == (64, 96) and H.tta_view_size(1024, 2048, 0.75) == (768, 1536)
    assert H.tta_view_size(1024, 2048, 1.25) == (1280, 2560) and H.tta_view_size(1024, 2048, 1.5) == (1536, 3072)
    assert H.tta_view_size(100, 200, 0.5) == (64, 96)                   # floor(50 / 32 + 0.5) = 2, floor(100 / 32 + 0.5) = 3
    assert H.tta_view_size(64, 64, 0.25) == (64, 64)                    # never below two cells of 32
    assert H.tta_view_size(80, 112, 1.5) == (128, 160)                  # floor(3.75 + 0.5) = 4, floor(5.25 + 0.5) = 5
    opt = H.tta_option({"evaluation.tta": {"scales": [0.5, 1.0], "flip": True}})
    assert H.tta_view_sizes(opt, 128, 192) == [(0.5, False, (64, 96)), (0.5, True, (64, 96)), (1.0, True, (128, 192))]
    with pytest.raises(ValueError, match=r"evaluation\.tta: scales 0\.5 and 0\.6 both give views of 64 x 64"):
        H.tta_view_sizes(H.tta_option({"evaluation.tta": {"scales": [0.5, 0.6]}}), 128, 128)
    with pytest.raises(ValueError, match=r"evaluation\.tta"):           # 0.9 of 64 x 64 is the frame's own size
        H.tta_view_sizes(H.tta_option({"evaluation.tta": {"scales": [0.9]}}), 64, 64)


@pytest.mark.parametrize("spec,match", [
    ("hflip", "evaluation.tta is"), (3, "evaluation.tta is"), ([0.5, 1.0], "evaluation.tta is"), (True, "evaluation.tta is"),
    ({"scale": [0.5]}, "unknown key 'scale'"), ({"scales": [0.5], "vflip": True, "crop": 2}, "unknown keys 'crop', 'vflip'"),
    ({"flip": 1}, "evaluation.tta.flip"), ({"flip": "yes"}, "evaluation.tta.flip"),
    ({"scales": 0.5}, "evaluation.tta.scales"), ({"scales": "0.5,1"}, "evaluation.tta.scales"), ({"scales": []}, "evaluation.tta.scales"),
    ({"scales": [0.5, 0.5]}, "evaluation.tta.scales"), ({"scales": [1.0, 0.5]}, "evaluation.tta.scales"),
    ({"scales": [0.2]}, "evaluation.tta.scales"), ({"scales": [2.5]}, "evaluation.tta.scales"),
    ({"scales": [float("nan")]}, "evaluation.tta.scales"), ({"scales": [True]}, "evaluation.tta.scales"),
    ({"scales": ["0.5"]}, "evaluation.tta.scales"), ({"scales": [0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1]}, "evaluation.tta.scales"),
    ({"scales": [1.0], "flip": False}, "nothing to average"), ({"flip": False}, "nothing to average")])
def test_option_refusals(spec, match):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness as H
    with pytest.raises(ValueError, match=match):
        H.tta_option({"evaluation.tta": spec})


# ------------------------------------------------------------------------------------------------------------------ host math
def _counts(C, right, wrong):
    """A C x C confusion matrix with `right` on every diagonal cell and `wrong` on every other."""
    m = np.full((C, C), wrong, np.int64)
    np.fill_diagonal(m, right)
    return m.reshape(-1)


def _consistency(C, same, moved, transitions):
    return np.concatenate([_counts(C, same, moved), np.asarray(transitions, np.int64)])


def test_tta_metrics_on_hand_made_counters():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import iou_from_counts, tta_metrics_from_stats
    C, conditions = 2, ["clean", "fog", "rain"]
    miou = lambda c: float(iou_from_counts(torch.from_numpy(c.copy()), C)["mean_iou"])     # noqa: E731
    plain = np.stack([_counts(C, 0, 0), _counts(C, 90, 10), _counts(C, 60, 40), _counts(C, 50, 50)])
    tta = np.stack([_counts(C, 0, 0), _counts(C, 92, 8), _counts(C, 70, 30), _counts(C, 0, 0)])       # rain: no TTA frame
    plain[0], tta[0] = plain[1:].sum(0), tta[1:].sum(0)
    cons = np.stack([_consistency(C, 0, 0, [0, 0, 0, 0]), _consistency(C, 97, 3, [170, 6, 10, 4]), _consistency(C, 80, 20, [100, 12, 36, 32]),
                     _consistency(C, 0, 0, [0, 0, 0, 0])])
    cons[0] = cons[1:].sum(0)
    deg = lambda a, b: max(0.0, (a - b) / a)                                               # noqa: E731
    res = tta_metrics_from_stats(tta, plain, cons, conditions, C, degradation=deg, views=4, scales=[0.5, 1.0], flip=True)
    assert res["miou_clean_tta"] == miou(tta[1]) and res["miou_fog_tta"] == miou(tta[2]) and res["overall_miou_tta"] == miou(tta[0])
    assert res["tta_gain_clean"] == miou(tta[1]) - miou(plain[1]) and res["tta_gain_fog"] == miou(tta[2]) - miou(plain[2])
    assert res["mean_tta_gain"] == miou(tta[0]) - miou(plain[1] + plain[2])                 # the same frames: rain's are left out
    assert res["robustness_degradation_fog_tta"] == deg(miou(tta[1]), miou(tta[2]))
    assert res["tta_changed_fraction_clean"] == 1.0 - (2 * 97) / (2 * 97 + 2 * 3) and res["tta_changed_fraction_fog"] == 1.0 - 160 / 200
    assert res["mean_tta_changed_fraction"] == 1.0 - (2 * 97 + 2 * 80) / 400
    assert res["tta_fixed_fraction_clean"] == 10 / 190 and res["tta_broken_fraction_clean"] == 6 / 190
    assert res["tta_fixed_fraction_fog"] == 36 / 180 and res["tta_broken_fraction_fog"] == 12 / 180
    assert res["tta_views"] == 4.0 and res["tta_scales"] == [0.5, 1.0] and res["tta_flip"] == 1.0
    # absent denominators: no key, never a 0
    for key in ("miou_rain_tta", "tta_gain_rain", "robustness_degradation_rain_tta", "tta_changed_fraction_rain", "tta_fixed_fraction_rain",
                "tta_broken_fraction_rain", "robustness_degradation_clean_tta"):
        assert key not in res
    assert tta_metrics_from_stats(np.zeros_like(tta), plain, np.zeros_like(cons), conditions, C) == {}
    unlabelled = cons.copy()
    unlabelled[:, C * C:] = 0                                            # pixels, none of them labelled
    quiet = tta_metrics_from_stats(tta, plain, unlabelled, conditions, C)
    assert "tta_changed_fraction_fog" in quiet and "tta_fixed_fraction_fog" not in quiet and "tta_broken_fraction_fog" not in quiet
    assert "tta_views" not in quiet
    no_clean = tta_metrics_from_stats(tta[[0, 2, 3]], plain[[0, 2, 3]], cons[[0, 2, 3]], ["fog", "rain"], C)
    assert "robustness_degradation_fog_tta" not in no_clean and no_clean["tta_gain_fog"] == res["tta_gain_fog"]
    for bad in ((tta[:3], plain, cons), (tta, plain[:, :3], cons), (tta, plain, cons[:, :C * C])):
        with pytest.raises(ValueError):
            tta_metrics_from_stats(*bad, conditions, C)


def test_tta_metrics_pool_the_levels_of_a_kind_under_a_sweep():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import iou_from_counts, tta_metrics_from_stats
    C, slots = 2, ["clean", "fog_s1", "fog_s2"]
    miou = lambda c: float(iou_from_counts(torch.from_numpy(c.copy()), C)["mean_iou"])     # noqa: E731
    plain = np.stack([_counts(C, 0, 0), _counts(C, 90, 5), _counts(C, 70, 15), _counts(C, 40, 30)])
    tta = np.stack([_counts(C, 0, 0), _counts(C, 91, 4), _counts(C, 75, 10), _counts(C, 50, 20)])
    plain[0], tta[0] = plain[1:].sum(0), tta[1:].sum(0)
    cons = np.stack([_consistency(C, 0, 0, [0] * 4), _consistency(C, 95, 0, [180, 1, 3, 6]), _consistency(C, 80, 5, [140, 4, 14, 12]),
                     _consistency(C, 60, 10, [80, 6, 26, 28])])
    cons[0] = cons[1:].sum(0)
    res = tta_metrics_from_stats(tta, plain, cons, slots, C, kinds=["fog"], levels=2)
    assert res["miou_fog_tta"] == miou(tta[2] + tta[3]) and res["tta_gain_fog"] == miou(tta[2] + tta[3]) - miou(plain[2] + plain[3])
    assert res["tta_gain_fog_s2"] == miou(tta[3]) - miou(plain[3]) and res["mean_tta_gain"] == miou(tta[0]) - miou(plain[0])
    assert res["tta_fixed_fraction_fog"] == (14 + 26) / (170 + 140) and res["tta_broken_fraction_fog_s1"] == 4 / 170
    assert res["tta_changed_fraction_fog"] == 1.0 - 280 / 310
    assert "robustness_degradation_fog_tta" in res and "robustness_degradation_fog_s1_tta" in res


def test_report_prints_the_table():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    results = {"overall_miou": 0.65, "miou_clean": 0.8, "miou_fog": 0.5, "miou_clean_tta": 0.81, "miou_fog_tta": 0.56, "overall_miou_tta": 0.7,
               "tta_gain_clean": 0.01, "tta_gain_fog": 0.06, "mean_tta_gain": 0.05, "tta_changed_fraction_clean": 0.02,
               "tta_changed_fraction_fog": 0.1, "mean_tta_changed_fraction": 0.06, "tta_fixed_fraction_clean": 0.015,
               "tta_broken_fraction_clean": 0.005, "tta_fixed_fraction_fog": 0.08, "tta_views": 4.0, "tta_scales": [0.5, 1.0], "tta_flip": 1.0}
    text = report_markdown(results)
    assert "## Test-Time Augmentation" in text and "4 views (scales 0.5, 1, each also mirrored left to right)" in text
    assert "| Condition | Plain mIoU | TTA mIoU | Gain | Changed | Fixed | Broken |" in text
    assert "| clean | 0.800 | 0.810 | 0.010 | 0.020 | 0.015 | 0.005 |" in text and "| fog | 0.500 | 0.560 | 0.060 | 0.100 | 0.080 | - |" in text
    assert "| all | 0.650 | 0.700 | 0.050 | 0.060 | - | - |" in text
    assert "## Test-Time Augmentation" not in report_markdown({"miou_clean": 0.8})


def test_command_line_sets_the_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_cli_tta", ROOT / "scripts" / "evaluate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness

    class Config(dict):
        set = dict.__setitem__

    def parsed(*flags):
        cfg = Config()
        mod.apply_tta_options(mod.build_parser().parse_args(["ckpt.pt", *flags]), cfg)
        return cfg
    assert parsed() == {} and harness.tta_option(parsed()) is None
    assert parsed("--tta", "flip") == {"evaluation.tta": "flip"} and parsed("--tta", "ms_flip") == {"evaluation.tta": "ms_flip"}
    assert harness.tta_option(parsed("--tta", "ms_flip"))["scales"] == [0.5, 0.75, 1.0, 1.25, 1.5]
    assert harness.tta_option(parsed("--tta-scales", "0.5,1.5")) == {"scales": [0.5, 1.0, 1.5], "flip": True}
    assert harness.tta_option(parsed("--tta-scales", "0.5, 1", "--tta-no-flip")) == {"scales": [0.5, 1.0], "flip": False}
    assert harness.tta_option(parsed("--tta", "ms_flip", "--tta-no-flip")) == {"scales": [0.5, 0.75, 1.0, 1.25, 1.5], "flip": False}
    assert harness.tta_option(parsed("--tta", "flip", "--tta-scales", "0.75")) == {"scales": [0.75, 1.0], "flip": True}
    for flags, match in ((("--tta-no-flip",), "--tta-no-flip"), (("--tta", "flip", "--tta-no-flip"), "nothing is averaged"),
                         (("--tta-scales", "a,b"), "--tta-scales")):
        with pytest.raises(ValueError, match=match):
            parsed(*flags)
    with pytest.raises(ValueError, match="evaluation.tta.scales"):
        harness.tta_option(parsed("--tta-scales", "3"))
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(["ckpt.pt", "--tta", "vflip"])


# --------------------------------------------------------------------------------------------------------------- the bindings
def test_bindings_cover_the_two_launchers_and_their_constants():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc import build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(awseg_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(N.EXTENSION_SIGNATURES) and {"awseg_tta_view", "awseg_tta_accumulate"} <= set(names)
    assert not {"awseg_tta_view", "awseg_tta_accumulate"} & set(N.SIGNATURES) and "tta.hip" in build.SOURCES
    for name in ("awseg_tta_view", "awseg_tta_accumulate"):            # one ctypes argument per parameter of the prototype
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", text).group(1).split(",")
        assert len(params) == len(N.EXTENSION_SIGNATURES[name][1]) and N.EXTENSION_SIGNATURES[name][0] is ctypes.c_int
        for raw, ctype in zip(params, N.EXTENSION_SIGNATURES[name][1]):
            raw = " ".join(raw.split())
            want = (ctypes.c_void_p if "*" in raw or raw.startswith("awseg_stream_t") else ctypes.c_int64 if raw.startswith("int64_t")
                    else ctypes.c_float if raw.startswith("float") else ctypes.c_int)
            assert ctype is want, (name, raw)
    raw = ctypes.CDLL(str(build.build()))
    assert hasattr(raw, "awseg_tta_view") and hasattr(raw, "awseg_tta_accumulate")
    N.lib()                                                           # binds both tables; raises on drift
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(AWSEG_TTA_\w+)\s+(\d+)", HEADER.read_text())}
    assert (ops.TTA_SET, ops.TTA_ADD, ops.TTA_SCALE_ADD) == (defines["AWSEG_TTA_SET"], defines["AWSEG_TTA_ADD"], defines["AWSEG_TTA_SCALE_ADD"])
    assert (T.SET, T.ADD, T.SCALE_ADD) == (ops.TTA_SET, ops.TTA_ADD, ops.TTA_SCALE_ADD)
    assert ops.TTA_VIEW_MAX_CHANNELS == defines["AWSEG_TTA_VIEW_MAX_CHANNELS"] == 4
    assert "-ffp-contract=off" in build._flags() and "tta.hip" not in build.EXTRA_FLAGS      # the arithmetic depends on it


def test_the_launchers_refuse_every_invalid_argument_before_any_launch():
    """Host-side only: the buffers are host memory of the right sizes, so each refusal below has exactly one reason and has to come
    before anything is launched."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N
    lib = N.lib()
    b, c, h, w, H, W = 2, 3, 5, 7, 8, 12
    src, dst = np.full((b, c, h, w), 3.0, np.float32), np.full((b, c, H, W), 7.0, np.float32)
    ptr = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)                             # noqa: E731
    view = {"src": ptr(src), "batch": b, "channels": c, "src_height": h, "src_width": w, "dst": ptr(dst), "height": H, "width": W,
            "flip": 1, "stream": None}
    acc = {"src": ptr(src), "batch": b, "channels": c, "src_height": h, "src_width": w, "acc": ptr(dst), "height": H, "width": W,
           "flip": 1, "weight": 0.25, "mode": 1, "stream": None}
    sizes = [(k, v) for k in ("batch", "channels", "src_height", "src_width", "height", "width") for v in (0, -3)]
    shared = [("src", None), *sizes, ("flip", 2), ("flip", -1)]
    for name, value in shared + [("dst", None), ("dst", ptr(src)), ("channels", 5), ("channels", 19)]:
        assert lib.awseg_tta_view(*dict(view, **{name: value}).values()) == EINVAL, (name, value)
    for name, value in shared + [("acc", None), ("acc", ptr(src)), ("mode", 3), ("mode", -1), ("weight", float("nan")),
                                 ("weight", float("inf")), ("weight", float("-inf"))]:
        assert lib.awseg_tta_accumulate(*dict(acc, **{name: value}).values()) == EINVAL, (name, value)
    for name in ("src", "dst"):                                       # a float32 sits on 4 bytes; 16-byte accesses are only taken where they fit
        assert lib.awseg_tta_view(*dict(view, **{name: ptr(src if name == "src" else dst, 2)}).values()) == EALIGN
    for name in ("src", "acc"):
        assert lib.awseg_tta_accumulate(*dict(acc, **{name: ptr(src if name == "src" else dst, 2)}).values()) == EALIGN
    big = {"src_height": 1 << 16, "src_width": 1 << 15}               # a plane of 2^31 pixels
    assert lib.awseg_tta_view(*dict(view, **big).values()) == ERANGE and lib.awseg_tta_accumulate(*dict(acc, **big).values()) == ERANGE
    big = {"height": 1 << 16, "width": 1 << 15}
    assert lib.awseg_tta_view(*dict(view, **big).values()) == ERANGE and lib.awseg_tta_accumulate(*dict(acc, **big).values()) == ERANGE
    many = {"batch": 1 << 12, "channels": 19, "height": 1 << 10, "width": 1 << 11}       # 2^12 * 19 * 2^10 * 2^9 groups
    assert lib.awseg_tta_accumulate(*dict(acc, **many).values()) == ERANGE
    assert (src == 3.0).all() and (dst == 7.0).all()


def test_ops_check_their_arguments_and_have_no_cpu_path():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    x, acc = torch.zeros(1, 3, 4, 5), torch.zeros(1, 3, 8, 10)
    with pytest.raises(N.AwsegError, match="no CPU fallback"):
        ops.tta_view(x, (8, 10), True)
    with pytest.raises(N.AwsegError, match="no CPU fallback"):
        ops.tta_accumulate(x, acc, False, 0.5, "add")
    for bad in (torch.zeros(1, 5, 4, 5), torch.zeros(1, 3, 4, 5, dtype=torch.float64), torch.zeros(3, 4, 5), torch.zeros(1, 3, 4, 6)[..., :5],
                torch.zeros(0, 3, 4, 5)):
        with pytest.raises(ValueError, match="tta_view"):
            ops.tta_view(bad, (8, 10), False)
    for kw in ({"size": (0, 4)}, {"size": 8}, {"size": (8, 10, 2)}, {"flip": 1}, {"out": torch.zeros(1, 3, 8, 11)}, {"out": x},
               {"out": torch.zeros(1, 3, 4, 5, dtype=torch.float64)}):
        with pytest.raises(ValueError, match="tta_view"):
            ops.tta_view(x, **{"size": (4, 5), "flip": False, **kw})
    for args in ((x, torch.zeros(1, 4, 8, 10), False, 0.5), (x, torch.zeros(2, 3, 8, 10), False, 0.5), (x, x, False, 0.5),
                 (x, acc.double(), False, 0.5), (x, acc, 0, 0.5), (x, acc, False, float("nan")), (x, acc, False, 1e39), (x, acc, False, "1"),
                 (x, acc, False, 0.5, "mean"), (x, acc, False, 0.5, 3), (x, acc, False, 0.5, True), (x, acc[..., ::2], False, 0.5)):
        with pytest.raises(ValueError, match="tta_accumulate"):
            ops.tta_accumulate(*args)
