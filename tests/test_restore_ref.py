"""The dehazing front-end without a GPU (-m "not gpu"): identities of the numpy model (tests/restore_ref.py), the recovery property
the feature is for, the option and host math of the harness, the bindings of include/awseg_restore.h and the launcher's argument
checks on host pointers."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import restore_ref as R

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "awseg_restore.h"
IDENTITY = (np.zeros(3, np.float32), np.ones(3, np.float32))


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("r", [1, 3, 7])
def test_opening_lies_between_the_erosion_and_the_map(r):
    n = np.random.default_rng(r).random((2, 19, 23)).astype(np.float32)
    e, o = R.erode(n, r), R.opening(n, r)
    assert (o >= e).all() and (o <= n).all()
    assert (e <= n).all() and not np.array_equal(o, e)
    # clipped windows: a corner's minimum is that of the (r+1)^2 positions inside the frame
    assert e[0, 0, 0] == n[0, :r + 1, :r + 1].min() and e[1, -1, -1] == n[1, -r - 1:, -r - 1:].min()


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("value", [(0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (0.1015625, 0.25, 0.75), (0.1, 0.1, 0.1)])
def test_a_constant_frame_restores_to_itself_bit_for_bit(value, refine):
    """v_c = c everywhere, c >= airlight_min and a multiple of 2^-16 as float32 (so the fixed-point airlight is c): A = c, n = 1,
    t = t_min, J = (c - c) / t + c = c.  mean 0 / std 1: the frame is its own de-normalised value."""
    frame = np.broadcast_to(np.asarray(value, np.float32)[:, None, None], (3, 9, 13)).copy()
    f = R.dehaze_frame(frame, *IDENTITY, radius=2, refine=refine)
    assert f["airlight"].tobytes() == np.fmax(np.rint(frame[:, 0, 0] * 65536) / 65536, 0.1).astype(np.float32).tobytes()
    assert (f["t"] == np.float32(0.1)).all()
    if all(float(np.float32(c)) * 65536 % 1 == 0 for c in value):     # (0.1 is not such a multiple: its airlight is 6554 / 65536)
        assert f["restored"].tobytes() == frame.tobytes()
    else:
        assert f["airlight"][0] == np.float32(6554 / 65536) and not np.array_equal(f["restored"], frame)
    assert f["row"].tolist()[R.PIXELS:] == [9 * 13, 9 * 13 * int(np.rint(np.float32(0.1) * 65536)), 0, 0]
    assert f["selected"] == 9 * 13                                   # every pixel ties: all of them are the top fraction


def test_the_top_fraction_and_its_bin_under_ties():
    assert [R.n_top(hw) for hw in (1, 35, 999, 1000, 1001, 32 * 64, 1024 * 2048)] == [1, 1, 1, 1, 2, 3, 2098]
    hist = np.zeros(256, np.int64)
    hist[[255, 200, 10]] = 1, 5, 2042
    assert R.b_star(hist, 1) == 255 and R.b_star(hist, 2) == 200 and R.b_star(hist, 6) == 200 and R.b_star(hist, 7) == 10
    assert R.b_star([7] + [0] * 255, 3) == 0
    # in the model: 32 x 64, n_top = 3; one brightest pixel and a tie of five behind it -> all six are averaged, the rest are not
    frame = np.full((3, 32, 64), 0.25, np.float32)
    for k, (y, x) in enumerate([(3, 3), (3, 20), (20, 3), (20, 40), (28, 60), (10, 30)]):
        frame[:, y - 1:y + 2, x - 1:x + 2] = 0.5 if k else 0.75     # a 3 x 3 patch: its centre survives the r = 1 minimum
    f = R.dehaze_frame(frame, *IDENTITY, radius=1)
    assert f["selected"] == 6 and f["b_star"] == int(np.float32(0.5) * np.float32(255))
    want = np.float32((0.75 + 5 * 0.5) / 6)
    assert np.allclose(f["airlight"], want, atol=2.0 ** -16) and f["row"][R.FLOORED] == 0


def test_the_floor_engages_on_a_dark_frame_and_non_finite_values_are_counted():
    rng = np.random.default_rng(5)
    frame = (0.05 * rng.random((3, 12, 17))).astype(np.float32)
    frame[0, 2, 3], frame[1, 4, 5], frame[2, 6, 7] = np.nan, np.inf, -np.inf
    f = R.dehaze_frame(frame, *IDENTITY, radius=2)
    assert (f["airlight"] == np.float32(0.1)).all() and f["row"][R.FLOORED] == 1 and f["row"][R.NONFINITE] == 3
    assert np.isfinite(f["restored"]).all() and f["v"][0, 2, 3] == 0 and f["v"][1, 4, 5] == 1 and f["v"][2, 6, 7] == 0


@pytest.mark.parametrize("refine", [0, 1])
def test_the_restored_frame_is_closer_to_the_scene_than_the_hazy_one(refine):
    """What the front-end is for.  The scene obeys the prior (a black pixel in every window), the haze is smooth, the airlight is
    visible at the dense end: restoring must bring the frame strictly closer to the scene, with either transmission estimate."""
    I, J, t, A = R.hazy_scene()
    f = R.dehaze_frame(R.normalise(I), R.IMAGENET_MEAN, R.IMAGENET_STD, radius=7, refine=refine)
    before, after = float(np.mean((I - J) ** 2)), float(np.mean((f["J"] - J) ** 2))
    assert after < before, (before, after)
    assert after < 0.5 * before, (before, after)                     # and not by a hair
    # the brightest dark-channel pixels sit where t = 0.25: they are J t + A (1 - t) with 0 <= J <= A, so the estimate is below A by
    # at most t A
    assert ((f["airlight"] <= A) & (A - f["airlight"] <= 0.25 * A + 1e-6)).all()


def test_batches_route_frames_into_slots():
    rng = np.random.default_rng(2)
    image = R.normalise(rng.random((3, 3, 6, 9)))
    restored, airlight, stats = R.dehaze(image, cond=[1, -1, 1], n_slots=3, radius=1)
    rows = [R.dehaze_frame(image[b], R.IMAGENET_MEAN, R.IMAGENET_STD, radius=1)["row"] for b in range(3)]
    assert (stats[0] == rows[0] + rows[1] + rows[2]).all() and not stats[1].any() and (stats[2] == rows[0] + rows[2]).all()
    assert restored.shape == image.shape and airlight.shape == (3, 3)


# ---------------------------------------------------------------------------------------------------------------- the harness
def test_restoration_option_accepts_and_refuses():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness
    default = {"radius": 7, "omega": float(np.float32(0.95)), "t_min": float(np.float32(0.1)), "airlight_min": float(np.float32(0.1)),
               "refine": 1, "conditions": None}
    assert harness.restoration_option({}) is None
    assert harness.restoration_option({"evaluation.restoration_conditions": ["fog"]}) is None
    assert harness.restoration_option({"evaluation.restoration": "dark_channel"}) == default
    assert harness.restoration_option({"evaluation.restoration": {}}) == default
    got = harness.restoration_option({"evaluation.restoration": {"radius": 15, "omega": 1, "t_min": 0.25, "airlight_min": 1.0,
                                                                 "refine": "none"},
                                      "evaluation.restoration_conditions": ("fog", "clean")})
    assert got == {"radius": 15, "omega": 1.0, "t_min": 0.25, "airlight_min": 1.0, "refine": 0, "conditions": ["fog", "clean"]}
    for bad in ("guided_filter", True, 7, ["dark_channel"], {"window": 7}, {"radius": 0}, {"radius": 16}, {"radius": 7.0}, {"radius": True},
                {"omega": 0}, {"omega": 1.5}, {"omega": float("nan")}, {"omega": "0.9"}, {"t_min": 0.0}, {"t_min": -0.1},
                {"airlight_min": 0}, {"airlight_min": 2}, {"airlight_min": 1e-60}, {"refine": "matting"}, {"refine": 1}, {"refine": None}):
        with pytest.raises(ValueError, match="evaluation.restoration"):
            harness.restoration_option({"evaluation.restoration": bad})
    for bad in ("fog", [], [3], [""], {"fog": 1}, ["fog", None]):
        for spec in ("dark_channel", None):                          # checked also when the option is off
            with pytest.raises(ValueError, match="restoration_conditions"):
                harness.restoration_option({"evaluation.restoration": spec, "evaluation.restoration_conditions": bad})
    on = {"evaluation.restoration": "dark_channel"}
    assert harness.restoration_option(on, images=torch.zeros(2, 3, 4, 5)) == default
    for frames in (torch.zeros(2, 3, 4, 5, dtype=torch.float64), torch.zeros(2, 1, 4, 5), torch.zeros(3, 4, 5),
                   torch.zeros(2, 3, 4, 5, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="float32"):
            harness.restoration_option(on, images=frames)
    assert harness.restoration_option({}, images=torch.zeros(2, 1, 4, 5)) is None


def _counts(C, right, wrong):
    """Confusion counters [C * C] with `right` pixels on every diagonal cell and `wrong` in every other one."""
    return (np.full((C, C), wrong, np.int64) + np.eye(C, dtype=np.int64) * (right - wrong)).reshape(-1)


def test_restoration_metrics_from_hand_made_counters():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import (iou_from_counts,
                                                                                                  restoration_metrics_from_stats)
    C, conditions = 3, ["clean", "fog", "rain"]
    miou = lambda c: float(iou_from_counts(torch.from_numpy(c.copy()), C)["mean_iou"])     # noqa: E731
    plain = np.stack([_counts(C, 0, 0), _counts(C, 90, 5), _counts(C, 50, 25), _counts(C, 70, 15)])
    plain[0] = plain[1:].sum(0)
    restored = np.stack([_counts(C, 0, 0), _counts(C, 86, 7), _counts(C, 70, 15), _counts(C, 0, 0)])      # rain was not selected
    restored[0] = restored[1:].sum(0)
    stats = np.zeros((4, 8), np.int64)
    stats[1] = [2, 2 * 52429, 2 * 45875, 2 * 39322, 600, 600 * 58982, 0, 0]
    stats[2] = [1, 60293, 60293, 58982, 300, 300 * 26214, 4, 1]
    stats[0] = stats[1:].sum(0)
    res = restoration_metrics_from_stats(restored, plain, stats, conditions, C)
    assert all(isinstance(v, float) for v in res.values())
    assert res["miou_clean_restored"] == miou(restored[1]) and res["miou_fog_restored"] == miou(restored[2])
    assert res["overall_miou_restored"] == miou(restored[0])
    assert res["restoration_gain_fog"] == miou(restored[2]) - miou(plain[2]) > 0
    assert res["restoration_gain_clean"] == miou(restored[1]) - miou(plain[1]) < 0          # unclamped
    assert res["restoration_clean_cost"] == miou(plain[1]) - miou(restored[1]) == -res["restoration_gain_clean"]
    assert res["mean_restoration_gain"] == miou(restored[0]) - miou(plain[1] + plain[2])    # the same frames: rain's are left out
    m_clean = miou(plain[1])
    assert res["robustness_degradation_fog_restored"] == max(0.0, (m_clean - miou(restored[2])) / m_clean)
    assert res["airlight_clean"] == pytest.approx((0.8 + 0.7 + 0.6) / 3, abs=1e-5)
    assert res["airlight_fog"] == (60293 + 60293 + 58982) / 65536 / 3
    assert res["transmission_mean_clean"] == 58982 / 65536 and res["transmission_mean_fog"] == 26214 / 65536
    assert res["mean_transmission"] == (600 * 58982 + 300 * 26214) / 65536 / 900
    assert res["restoration_nonfinite_values"] == 4.0 and res["restoration_airlight_floored_frames"] == 1.0
    # absent denominators: no key, never a 0
    for key in ("miou_rain_restored", "restoration_gain_rain", "robustness_degradation_rain_restored", "airlight_rain",
                "transmission_mean_rain", "robustness_degradation_clean_restored"):
        assert key not in res
    quiet = restoration_metrics_from_stats(np.zeros_like(restored), plain, np.zeros_like(stats), conditions, C)
    assert quiet == {}
    no_clean = restoration_metrics_from_stats(restored[[0, 2, 3]], plain[[0, 2, 3]], stats[[0, 2, 3]], ["fog", "rain"], C)
    assert "restoration_clean_cost" not in no_clean and "robustness_degradation_fog_restored" not in no_clean
    assert no_clean["restoration_gain_fog"] == res["restoration_gain_fog"]
    with pytest.raises(ValueError):
        restoration_metrics_from_stats(restored[:3], plain, stats, conditions, C)
    with pytest.raises(ValueError):
        restoration_metrics_from_stats(restored, plain, stats[:, :7], conditions, C)


def test_restoration_metrics_pool_the_levels_of_a_kind_under_a_sweep():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import (iou_from_counts,
                                                                                                  restoration_metrics_from_stats)
    C, slots = 2, ["clean", "fog_s1", "fog_s2"]
    miou = lambda c: float(iou_from_counts(torch.from_numpy(c.copy()), C)["mean_iou"])     # noqa: E731
    plain = np.stack([_counts(C, 0, 0), _counts(C, 90, 5), _counts(C, 70, 15), _counts(C, 40, 30)])
    restored = np.stack([_counts(C, 0, 0), _counts(C, 88, 6), _counts(C, 80, 10), _counts(C, 60, 20)])
    plain[0], restored[0] = plain[1:].sum(0), restored[1:].sum(0)
    stats = np.zeros((4, 8), np.int64)
    stats[1:, 0], stats[1:, 4], stats[1:, 5] = 1, 100, [100 * 60000, 100 * 40000, 100 * 20000]
    stats[0] = stats[1:].sum(0)
    res = restoration_metrics_from_stats(restored, plain, stats, slots, C, kinds=["fog"], levels=2)
    assert res["miou_fog_restored"] == miou(restored[2] + restored[3])
    assert res["restoration_gain_fog"] == miou(restored[2] + restored[3]) - miou(plain[2] + plain[3])
    assert res["restoration_gain_fog_s2"] == miou(restored[3]) - miou(plain[3])
    assert res["transmission_mean_fog"] == 30000 / 65536 and res["mean_restoration_gain"] == miou(restored[0]) - miou(plain[0])
    assert "robustness_degradation_fog_restored" in res and "robustness_degradation_fog_s1_restored" in res


def test_report_prints_one_line_per_condition():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    results = {"miou_clean": 0.8, "miou_fog": 0.5, "miou_clean_restored": 0.79, "miou_fog_restored": 0.6, "overall_miou_restored": 0.7,
               "restoration_gain_clean": -0.01, "restoration_gain_fog": 0.1, "transmission_mean_clean": 0.9, "transmission_mean_fog": 0.4,
               "restoration_clean_cost": 0.01, "mean_restoration_gain": 0.045, "restoration_airlight_floored_frames": 2.0}
    text = report_markdown(results)
    assert "## Input Restoration" in text
    assert "| clean | 0.800 | 0.790 | -0.010 | 0.900 |" in text and "| fog | 0.500 | 0.600 | 0.100 | 0.400 |" in text
    assert "Clean cost" in text and "hit the floor**: 2" in text
    assert "## Input Restoration" not in report_markdown({"miou_clean": 0.8})


def test_command_line_sets_the_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_cli_restoration", ROOT / "scripts" / "evaluate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness

    class Config(dict):
        set = dict.__setitem__
    ap = mod.build_parser()
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt"]), cfg)
    assert cfg == {} and harness.restoration_option(cfg) is None
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "dark_channel"]), cfg)
    assert cfg == {"evaluation.restoration": "dark_channel"} and harness.restoration_option(cfg)["refine"] == 1
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "dark_channel", "--restoration-conditions", "fog, night",
                                                 "--restoration-refine", "none"]), cfg)
    opt = harness.restoration_option(cfg)
    assert opt["refine"] == 0 and opt["conditions"] == ["fog", "night"] and opt["radius"] == 7
    with pytest.raises(ValueError, match="--restoration-refine"):
        mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration-refine", "none"]), Config())
    with pytest.raises(SystemExit):
        ap.parse_args(["ckpt.pt", "--restoration", "guided_filter"])


# --------------------------------------------------------------------------------------------------------------- the bindings
def header_symbols():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(awseg_[a-z0-9_]+)\s*\(", text)))


def test_extension_bindings_cover_the_extension_header_and_the_library_exports_them():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc import build
    names = header_symbols()
    assert names == sorted(N.EXTENSION_SIGNATURES) and "awseg_dehaze" in names and "awseg_dehaze_workspace" in names
    assert not set(names) & set(N.SIGNATURES)
    raw = ctypes.CDLL(str(build.build()))
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/awseg_restore.h but not exported"
    lib = N.lib()                                                   # binds both tables; raises on drift
    assert lib.awseg_abi_version() == 1
    assert lib.awseg_restore_header_hash() == build.header_hash(build.RESTORE_HEADER) != 0
    assert "dehaze.hip" in build.SOURCES
    defines = dict(re.findall(r"#define\s+(AWSEG_DEHAZE_\w+)\s+(\d+)", HEADER.read_text()))
    assert (ops.DEHAZE_TILE_H, ops.DEHAZE_TILE_W) == (int(defines["AWSEG_DEHAZE_TILE_H"]), int(defines["AWSEG_DEHAZE_TILE_W"]))
    assert ops.DEHAZE_ROW == int(defines["AWSEG_DEHAZE_ROW"]) == R.ROW
    assert ops.DEHAZE_MAX_RADIUS == int(defines["AWSEG_DEHAZE_MAX_RADIUS"])
    assert ops.DEHAZE_FRAME_RECORD == int(defines["AWSEG_DEHAZE_FRAME_RECORD"])
    for b, h, w in ((1, 1, 1), (2, 5, 7), (8, 1024, 2048), (3, 31, 53)):
        assert lib.awseg_dehaze_workspace(b, h, w) == b * (ops.DEHAZE_FRAME_RECORD + h * w)


def test_a_library_built_from_another_extension_header_is_refused(monkeypatch):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc import build
    N.lib()
    real = build.header_hash
    monkeypatch.setattr(build, "header_hash", lambda path=build.HEADER: 12345 if path == build.RESTORE_HEADER else real(path))
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.AwsegError, match="awseg_restore.h"):
        N.lib()
    monkeypatch.undo()
    N.lib()


def test_the_launcher_refuses_every_invalid_argument_before_any_launch():
    """Host-side only: the buffers are host memory of the right sizes, so each refusal below has exactly one reason and has to come
    before anything is launched (the pattern of test_rain_and_snow_refuse_a_missing_workspace)."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N
    lib = N.lib()
    b, h, w = 2, 5, 7
    image, restored = np.zeros((b, 3, h, w), np.float32), np.full((b, 3, h, w), 7.0, np.float32)
    airlight, stats = np.full((b, 3), 7.0, np.float32), np.zeros((2, 8), np.int64)
    ws = np.zeros(lib.awseg_dehaze_workspace(b, h, w) // 8 + 1, np.int64)
    cond = np.zeros(b, np.int32)
    mean, std = R.IMAGENET_MEAN.copy(), R.IMAGENET_STD.copy()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
    good = {"image": ptr(image), "batch": b, "channels": 3, "height": h, "width": w, "mean": ptr(mean), "std": ptr(std), "radius": 7,
            "omega": 0.95, "t_min": 0.1, "airlight_min": 0.1, "refine": 1, "cond": ptr(cond), "restored": ptr(restored),
            "airlight": ptr(airlight), "stats": ptr(stats), "n_slots": 2, "workspace": ptr(ws), "stream": None}
    bad_std, bad_mean = np.array([0.2, 0.0, 0.2], np.float32), np.array([0.4, np.inf, 0.4], np.float32)
    einval = [("image", None), ("mean", None), ("std", None), ("restored", None), ("airlight", None), ("stats", None), ("workspace", None),
              ("channels", 1), ("channels", 4), ("batch", -1), ("height", 0), ("width", 0), ("n_slots", 0),
              ("radius", 0), ("radius", 16), ("radius", -7), ("refine", 2), ("refine", -1),
              ("omega", 0.0), ("omega", 1.5), ("omega", float("nan")), ("t_min", 0.0), ("t_min", 1.0001), ("t_min", float("nan")),
              ("airlight_min", 0.0), ("airlight_min", -0.1), ("airlight_min", 2.0), ("airlight_min", float("inf")),
              ("std", ptr(bad_std)), ("mean", ptr(bad_mean))]
    for name, value in einval:
        args = dict(good, **{name: value})
        assert lib.awseg_dehaze(*args.values()) == -1, (name, value)
    assert lib.awseg_dehaze(*dict(good, batch=65536).values()) == -2
    assert lib.awseg_dehaze(*dict(good, height=1 << 16, width=1 << 15).values()) == -2
    odd = ctypes.c_void_p(ws.ctypes.data + 4)
    assert lib.awseg_dehaze(*dict(good, workspace=odd).values()) == -3
    assert lib.awseg_dehaze(*dict(good, batch=0).values()) == 0                             # nothing to do, nothing launched
    assert (restored == 7.0).all() and (airlight == 7.0).all() and not stats.any() and not ws.any()


def test_ops_dehaze_checks_its_arguments_and_has_no_cpu_path():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    x = torch.zeros(1, 3, 4, 5)
    with pytest.raises(N.AwsegError, match="no CPU fallback"):
        ops.dehaze(x)
    for bad in (torch.zeros(1, 1, 4, 5), torch.zeros(1, 3, 4, 5, dtype=torch.float64), torch.zeros(3, 4, 5)):
        with pytest.raises(ValueError, match="float32"):
            ops.dehaze(bad)
    for kw in ({"radius": 0}, {"radius": 16}, {"omega": 0.0}, {"t_min": 1.5}, {"airlight_min": 0}, {"refine": 2}, {"mean": [0.5] * 3},
               {"mean": [0.5] * 3, "std": [0.2, 0.0, 0.2]}, {"stats": torch.zeros(2, 7, dtype=torch.int64)},
               {"cond": torch.zeros(2, dtype=torch.int32)}, {"out": torch.zeros(1, 3, 4, 6)}, {"out": x}):
        with pytest.raises(ValueError):
            ops.dehaze(x, **kw)
    assert ops.new_dehaze_stats("cpu", 3).shape == (3, ops.DEHAZE_ROW)
    with pytest.raises(ValueError):
        ops.new_dehaze_stats("cpu", 0)
