"""The guided-filter refinement of the dehazing front-end without a GPU (-m "not gpu"): what the numpy model of
tests/guided_ref.py does on a depth-step scene, its float32 against its float64 version, its identities; the option, the host math
and the command line of the harness; the bindings of include/awseg_restore.h and the launcher's argument checks on host pointers."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import guided_ref as G
from tests import quality_ref as Q
from tests import restore_ref as R

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "awseg_restore.h"
IDENTITY = (np.zeros(3, np.float32), np.ones(3, np.float32))
NORM = (R.IMAGENET_MEAN, R.IMAGENET_STD)
SETTINGS = [(8, 1e-3), (16, 1e-3), (28, 1e-3), (32, 1e-3), (16, 1e-4), (16, 1e-2)]      # (R, eps) of the depth-step scene


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def scene():
    """The depth-step scene (64 x 96, t_true 0.85 | 0.3, A = (0.86, 0.88, 0.9), seed 0), its ideal transmission, the band of 7
    columns either side of the step, and the model's frames at every setting in float32 and float64 (computed once)."""
    I, J, t_true, A = G.depth_step_scene()
    x = R.normalise(I)
    t_star = np.maximum(1.0 - 0.95 * (1.0 - t_true.astype(np.float64)), 0.1)
    band = np.zeros(t_true.shape, bool)
    band[:, t_true.shape[1] // 2 - 7:t_true.shape[1] // 2 + 7] = True
    frames = {(r, eps, dt): G.dehaze_guided_frame(x, *NORM, radius=7, omega=0.95, guided_radius=r, guided_eps=eps, dtype=dt)
              for r, eps in SETTINGS for dt in (np.float32, np.float64)}
    patch = R.dehaze_frame(x, *NORM, radius=7, omega=0.95, refine=0)["t"]
    return {"x": x, "t_star": t_star, "band": band, "frames": frames, "patch": patch}


@pytest.fixture(scope="module")
def rendered():
    x = Q.rendered_frames(11, 2, 3, 43, 140)[0]
    return [{dt: G.dehaze_guided_frame(x[b], *NORM, guided_radius=28, dtype=dt) for dt in (np.float32, np.float64)} for b in range(2)]


@pytest.mark.parametrize("r,eps", SETTINGS)
def test_guided_is_closer_to_the_ideal_transmission_than_the_patch_minimum(scene, r, eps):
    """Mean |t - t*| inside the band around the depth step and outside it.  (Nothing is claimed against the opening: on this
    textured scene the opening is tighter inside the band, 0.111 against 0.134 at R = 28.)"""
    t, band, t_star = scene["frames"][(r, eps, np.float32)]["t"], scene["band"], scene["t_star"]
    err = lambda m: (float(np.abs(m - t_star)[band].mean()), float(np.abs(m - t_star)[~band].mean()))     # noqa: E731
    (g_in, g_out), (p_in, p_out) = err(t), err(scene["patch"])
    print(f"R={r} eps={eps}: guided {g_in:.4f} / {g_out:.4f}, patch minimum {p_in:.4f} / {p_out:.4f}")
    assert g_in < p_in and g_out < p_out


def test_the_variance_stays_usable(scene, rendered):
    low = []
    for (r, eps, dt), f in scene["frames"].items():
        if dt is np.float32:
            assert (f["var"] > -eps / 10).all(), (r, eps, float(f["var"].min()))
            low.append(float(f["var"].min()))
    for f in rendered:
        assert (f[np.float32]["var"] > -1e-3 / 10).all()
        low.append(float(f[np.float32]["var"].min()))
    print("smallest float32 var:", min(low))


def test_float32_model_against_float64_model(scene, rendered):
    """|dt| <= 2e-5: five times the 3.7e-6 a prototype of this arithmetic measured, for a model whose order may differ in nothing."""
    worst = 0.0
    for r, eps in SETTINGS:
        worst = max(worst, float(np.abs(scene["frames"][(r, eps, np.float32)]["t"] - scene["frames"][(r, eps, np.float64)]["t"]).max()))
    worst_rendered = max(float(np.abs(f[np.float32]["t"] - f[np.float64]["t"]).max()) for f in rendered)
    print(f"float32 against float64: depth-step scene {worst:.3g}, rendered frames {worst_rendered:.3g}")
    assert worst <= 2e-5 and worst_rendered <= 2e-5
    for f in list(scene["frames"].values()) + [g[np.float32] for g in rendered]:
        assert f["t"].dtype == f["p"].dtype == f["a"].dtype == f["restored"].dtype


def test_a_constant_frame_has_no_slope():
    frame = np.broadcast_to(np.asarray((0.1015625, 0.25, 0.75), np.float32)[:, None, None], (3, 9, 13)).copy()
    f = G.dehaze_guided_frame(frame, *IDENTITY, radius=2, guided_radius=3)
    # (the guide's constant is no dyadic number: the rounding of the window sums leaves a cov of an ulp here and there)
    flat = f["cov"] == 0
    assert flat.any() and (f["a"][flat] == 0).all() and f["a"].dtype == np.float32
    assert float(np.abs(f["a"]).max()) < 1e-5 and (f["p"] == f["p"][0, 0]).all()
    # a guide that is constant without rounding (0: every sum is exact) under any p: cov = 0 and a = 0 everywhere, b = M(p), and
    # t is the mean of the means
    p = np.random.default_rng(4).random((9, 13)).astype(np.float32)
    f = G.guided_transmission(np.zeros((3, 9, 13), np.float32), p, 3, 1e-3, 0.1)
    assert (f["cov"] == 0).all() and (f["a"] == 0).all() and f["b"].tobytes() == G.box_mean(p, 3).tobytes()
    want = np.fmax(np.fmin(G.box_mean(G.box_mean(p, 3), 3), np.float32(1)), np.float32(0.1))
    assert f["t"].tobytes() == want.tobytes()
    # a texture with a constant p: cov is not exactly 0 everywhere, but where it is, a is
    rng = np.random.default_rng(1)
    tex = rng.random((3, 12, 17)).astype(np.float32)
    g = G.guided_transmission(tex, np.full((12, 17), 0.5, np.float32), 2, 1e-3, 0.1)
    assert (g["a"][g["cov"] == 0] == 0).all()


def test_a_radius_larger_than_the_frame_takes_the_whole_frame_everywhere():
    rng = np.random.default_rng(3)
    x = rng.random((5, 7)).astype(np.float32)
    for r in (7, 28, 32):
        assert (G.window_count(5, 7, r, np.float32) == 35).all()
        m = G.box_mean(x, r)
        assert (m == m[0, 0]).all()
    f = G.dehaze_guided_frame(R.normalise(rng.random((3, 5, 7))), *NORM, radius=7, guided_radius=28)
    for name in ("var", "cov", "a", "b"):
        assert (f[name] == f[name][0, 0]).all(), name
    # and a window clipped at a corner counts only what is inside
    assert G.window_count(9, 13, 2, np.float32)[0, 0] == 9 and G.window_count(9, 13, 2, np.float32)[4, 6] == 25
    assert G.box_sum(np.ones((9, 13), np.float32), 2).tobytes() == G.window_count(9, 13, 2, np.float32).tobytes()


def test_batches_route_frames_into_slots_of_both_counter_tensors():
    rng = np.random.default_rng(2)
    image = R.normalise(rng.random((3, 3, 6, 9)))
    restored, airlight, t, stats, guided = G.dehaze_guided(image, cond=[1, -1, 1], n_slots=3, radius=1, guided_radius=2)
    rows = [G.dehaze_guided_frame(image[b], *NORM, radius=1, guided_radius=2) for b in range(3)]
    assert (guided[0] == sum(r["guided_row"] for r in rows)).all() and not guided[1].any()
    assert (guided[2] == rows[0]["guided_row"] + rows[2]["guided_row"]).all() and (stats[2] == rows[0]["row"] + rows[2]["row"]).all()
    assert guided[0, G.PIXELS] == 3 * 54 and t.shape == (3, 6, 9) and restored.dtype == np.float32
    assert stats[0, R.SUM_T] == int(np.rint(t * np.float32(65536)).astype(np.int64).sum())


# ---------------------------------------------------------------------------------------------------------------- the harness
def test_restoration_option_accepts_guided_and_leaves_the_other_refinements_as_they_were():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness
    f32 = lambda v: float(np.float32(v))                                                     # noqa: E731
    default = {"radius": 7, "omega": f32(0.95), "t_min": f32(0.1), "airlight_min": f32(0.1), "refine": 1, "conditions": None}
    opt = lambda spec: harness.restoration_option({"evaluation.restoration": spec})         # noqa: E731
    assert opt("dark_channel") == default and opt({}) == default and opt({"refine": "opening"}) == default
    assert opt({"refine": "none"}) == dict(default, refine=0)
    guided = {"radius": 7, "omega": f32(0.95), "t_min": f32(0.1), "airlight_min": f32(0.1), "guided_radius": 28, "guided_eps": f32(1e-3),
              "refine": "guided", "conditions": None}
    assert opt({"refine": "guided"}) == guided
    assert opt({"refine": "guided", "radius": 3})["guided_radius"] == 12 and opt({"refine": "guided", "radius": 15})["guided_radius"] == 32
    got = opt({"refine": "guided", "guided_radius": 1, "guided_eps": 1, "omega": 0.8})
    assert (got["guided_radius"], got["guided_eps"], got["omega"]) == (1, 1.0, f32(0.8))
    assert opt({"refine": "guided", "guided_radius": 32, "guided_eps": 1e-4})["guided_eps"] == f32(1e-4)
    bad = [{"guided_radius": v} for v in (0, 33, 7.0, True)] + [{"guided_eps": v} for v in (0, 5e-5, 2, float("nan"), "1e-3")]
    for extra in bad:
        with pytest.raises(ValueError, match="evaluation.restoration"):
            opt(dict(extra, refine="guided"))
    for refine in ({"refine": "none"}, {"refine": "opening"}, {}):
        for extra in ({"guided_radius": 8}, {"guided_eps": 1e-3}):
            with pytest.raises(ValueError, match="evaluation.restoration"):
                opt(dict(refine, **extra))
    for spec in ("guided_filter", "guided", {"refine": "matting"}, {"refine": 2}, {"refine": "guided", "window": 3}):
        with pytest.raises(ValueError, match="evaluation.restoration"):
            opt(spec)


def test_guided_metrics_from_hand_made_counters():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import guided_metrics_from_stats
    conditions = ["clean", "fog", "rain"]
    stats = np.zeros((4, 4), np.int64)
    stats[1] = [10, 0, 600 * 655, 600]
    stats[2] = [0, 30, 300 * 6554, 300]
    stats[0] = stats[1:].sum(0)
    res = guided_metrics_from_stats(stats, conditions)
    assert all(isinstance(v, float) for v in res.values())
    assert res["transmission_refinement_clean"] == 655 / 65536 and res["transmission_refinement_fog"] == 6554 / 65536
    assert res["transmission_clamped_fraction_clean"] == 10 / 600 and res["transmission_clamped_fraction_fog"] == 30 / 300
    assert res["mean_transmission_refinement"] == (600 * 655 + 300 * 6554) / 65536 / 900
    assert res["mean_transmission_clamped_fraction"] == 40 / 900
    assert not any(k.endswith("_rain") for k in res)
    assert guided_metrics_from_stats(np.zeros_like(stats), conditions) == {}
    sweep = guided_metrics_from_stats(stats, ["clean", "fog_s1", "fog_s2"], kinds=["fog"], levels=2)
    assert sweep["transmission_refinement_fog"] == sweep["transmission_refinement_fog_s1"] == 6554 / 65536
    with pytest.raises(ValueError):
        guided_metrics_from_stats(stats[:, :3], conditions)


def _iq_row(frames, terms, sum_abs, sum_sq, windows, lum, con, ssim):
    return [frames, terms, sum_abs, sum_sq, 0, windows, lum, con, ssim, 0]


def test_restored_quality_keys_from_two_hand_made_tensors():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import (
        IQ_PLAIN_STEMS, quality_metrics_from_stats, restored_quality_metrics_from_stats)
    U = 1 << 24
    slots, kinds, levels = ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2"], ["fog", "night"], 2
    plain = np.zeros((6, 10), np.int64)
    plain[2] = _iq_row(2, 600, 30 * U, 3 * U, 100, 90 * U, 80 * U, 72 * U)
    plain[3] = _iq_row(2, 600, 90 * U, 20 * U, 100, 70 * U, 60 * U, 42 * U)
    plain[4] = _iq_row(2, 600, 120 * U, 40 * U, 100, 40 * U, 90 * U, 36 * U)
    plain[5] = _iq_row(2, 600, 200 * U, 90 * U, 100, 20 * U, 80 * U, 16 * U)
    plain[0] = plain[1:].sum(0)
    restored = np.zeros((6, 10), np.int64)
    restored[1] = _iq_row(2, 600, 6 * U, U // 4, 100, 99 * U, 98 * U, 97 * U)          # the clean frames, restored, against themselves
    restored[2] = _iq_row(2, 600, 20 * U, 2 * U, 100, 95 * U, 82 * U, 78 * U)
    restored[3] = _iq_row(2, 600, 60 * U, 10 * U, 100, 85 * U, 65 * U, 55 * U)
    restored[4] = _iq_row(2, 600, 130 * U, 50 * U, 100, 50 * U, 60 * U, 30 * U)        # worse than before: the gain is negative
    restored[5] = _iq_row(2, 600, 210 * U, 95 * U, 100, 30 * U, 50 * U, 15 * U)
    restored[0] = restored[1:].sum(0)
    res = restored_quality_metrics_from_stats(restored, plain, slots, kinds, levels)
    assert all(isinstance(v, float) for v in res.values())
    pooled = restored.copy()
    pooled[0] = restored[2:].sum(0)                                                    # the clean frames leave the pooled row
    after, before = quality_metrics_from_stats(pooled, slots, kinds, levels, {}), quality_metrics_from_stats(plain, slots, kinds, levels, {})
    names = ["fog_s1", "fog_s2", "night_s1", "night_s2", "fog", "night"]
    for stem in IQ_PLAIN_STEMS:
        for n in names:
            assert res[f"{stem}_{n}_restored"] == after[f"{stem}_{n}"]
        assert res[f"mean_{stem}_restored"] == after[f"mean_{stem}"]
    for stem in ("psnr", "ssim"):
        for n in names:
            assert res[f"restoration_{stem}_gain_{n}"] == after[f"{stem}_{n}"] - before[f"{stem}_{n}"]
        assert res[f"mean_restoration_{stem}_gain"] == after[f"mean_{stem}"] - before[f"mean_{stem}"]
    assert res["restoration_psnr_gain_fog_s1"] > 0 > res["restoration_psnr_gain_night_s2"]
    assert res["psnr_clean_restored"] == 10.0 * np.log10(1.0 / ((U // 4) / U / 600)) and res["ssim_clean_restored"] == 0.97
    assert not any("miou_at_ssim" in k or "not_monotonic" in k or "drop_per_ssim" in k for k in res)
    # only fog restored: the pooled gain is over fog's frames, night has no key
    part = restored.copy()
    part[[1, 4, 5]] = 0
    part[0] = part[1:].sum(0)
    res = restored_quality_metrics_from_stats(part, plain, slots, kinds, levels)
    fog_plain = plain.copy()
    fog_plain[0] = plain[2:4].sum(0)
    assert res["mean_restoration_ssim_gain"] == after["ssim_fog"] - quality_metrics_from_stats(fog_plain, slots, kinds, levels, {})["mean_ssim"]
    assert "psnr_night_restored" not in res and "restoration_psnr_gain_night_s1" not in res and "psnr_clean_restored" not in res
    assert restored_quality_metrics_from_stats(np.zeros_like(plain), plain, slots, kinds, levels) == {}
    with pytest.raises(ValueError):
        restored_quality_metrics_from_stats(restored[:5], plain, slots, kinds, levels)


def test_report_names_the_refinement_and_gains_its_columns():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    base = {"miou_clean": 0.8, "miou_fog_s1": 0.5, "miou_clean_restored": 0.79, "miou_fog_s1_restored": 0.6, "overall_miou_restored": 0.7,
            "restoration_gain_clean": -0.01, "restoration_gain_fog_s1": 0.1, "transmission_mean_clean": 0.9, "transmission_mean_fog_s1": 0.4}
    plain = report_markdown(base)
    assert "| fog_s1 | 0.500 | 0.600 | 0.100 | 0.400 | - | - |\n" in plain + "\n" and "Transmission refinement" not in plain
    assert "| Condition | Plain mIoU | Restored mIoU | Gain | Mean t | Airlight | Degradation restored |\n|---|---|---|---|---|---|---|" in plain
    full = dict(base, restoration_refine="guided", transmission_refinement_fog_s1=0.0312, transmission_clamped_fraction_fog_s1=0.25,
                mean_transmission_refinement=0.02, psnr_fog_s1_restored=21.5, restoration_psnr_gain_fog_s1=1.25, ssim_fog_s1_restored=0.81,
                restoration_ssim_gain_fog_s1=-0.02, psnr_clean_restored=30.0, ssim_clean_restored=0.97)
    text = report_markdown(full)
    assert "Transmission refinement: guided filter" in text
    assert "| Refinement | Clamped | PSNR restored (gain) | SSIM restored (gain) |" in text
    assert "| fog_s1 | 0.500 | 0.600 | 0.100 | 0.400 | - | - | 0.031 | 0.250 | 21.50 (+1.25) | 0.810 (-0.020) |" in text
    assert "| clean | 0.800 | 0.790 | -0.010 | 0.900 | - | - | - | - | 30.00 | 0.970 |" in text


def test_command_line_sets_the_guided_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_cli_guided", ROOT / "scripts" / "evaluate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness

    class Config(dict):
        set = dict.__setitem__
    ap = mod.build_parser()
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "dark_channel", "--restoration-refine", "guided"]), cfg)
    assert cfg == {"evaluation.restoration": {"refine": "guided"}}
    opt = harness.restoration_option(cfg)
    assert opt["refine"] == "guided" and opt["guided_radius"] == 28 and opt["guided_eps"] == float(np.float32(1e-3))
    cfg = Config()
    mod.apply_restoration_options(ap.parse_args(["ckpt.pt", "--restoration", "dark_channel", "--restoration-refine", "guided",
                                                 "--restoration-guided-radius", "16", "--restoration-guided-eps", "0.01"]), cfg)
    opt = harness.restoration_option(cfg)
    assert opt["guided_radius"] == 16 and opt["guided_eps"] == float(np.float32(0.01))
    for argv in (["--restoration", "dark_channel", "--restoration-guided-radius", "16"],
                 ["--restoration", "dark_channel", "--restoration-refine", "none", "--restoration-guided-eps", "0.01"]):
        with pytest.raises(ValueError, match="--restoration-refine guided"):
            mod.apply_restoration_options(ap.parse_args(["ckpt.pt"] + argv), Config())


# --------------------------------------------------------------------------------------------------------------- the bindings
def test_bindings_constants_and_the_workspace_closed_form():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.csrc import build
    assert "awseg_dehaze_guided" in N.EXTENSION_SIGNATURES and "awseg_dehaze_guided_workspace" in N.EXTENSION_SIGNATURES
    assert "awseg_dehaze_guided" not in (ROOT / "include" / "awseg.h").read_text()
    assert "dehaze_guided.hip" in build.SOURCES
    lib = N.lib()
    defines = dict(re.findall(r"#define\s+(AWSEG_GUIDED_\w+)\s+(\d+)", HEADER.read_text()))
    assert ops.GUIDED_ROW == int(defines["AWSEG_GUIDED_ROW"]) == G.ROW == len(ops.GUIDED_FIELDS)
    assert ops.GUIDED_MAX_RADIUS == int(defines["AWSEG_GUIDED_MAX_RADIUS"]) == G.MAX_RADIUS
    ceil8 = lambda v: (v + 7) // 8 * 8                                                        # noqa: E731
    for b, h, w in ((1, 1, 1), (2, 5, 7), (8, 1024, 2048), (3, 31, 53), (1, 43, 140), (0, 0, 0)):
        bb, hh, ww = max(b, 1), max(h, 1), max(w, 1)
        want = ceil8(bb * (ops.DEHAZE_FRAME_RECORD + hh * ww)) + 3 * ceil8(4 * bb * hh * ww)
        assert lib.awseg_dehaze_guided_workspace(b, h, w) == want == ops.dehaze_guided_workspace_bytes(b, h, w)
    assert ops.default_guided_radius(7) == G.default_guided_radius(7) == 28 and ops.default_guided_radius(9) == 32


def test_the_guided_launcher_refuses_every_invalid_argument_before_any_launch():
    """Host-side only (the pattern of test_restore_ref's launcher test): the buffers are host memory of the right sizes, so each
    refusal has exactly one reason and has to come before anything is launched."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N
    lib = N.lib()
    b, h, w = 2, 5, 7
    image, restored = np.zeros((b, 3, h, w), np.float32), np.full((b, 3, h, w), 7.0, np.float32)
    airlight, t = np.full((b, 3), 7.0, np.float32), np.full((b, h, w), 7.0, np.float32)
    stats, guided = np.zeros((2, 8), np.int64), np.zeros((2, 4), np.int64)
    ws = np.zeros(lib.awseg_dehaze_guided_workspace(b, h, w) // 8 + 1, np.int64)
    cond = np.zeros(b, np.int32)
    mean, std = R.IMAGENET_MEAN.copy(), R.IMAGENET_STD.copy()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
    good = {"image": ptr(image), "batch": b, "channels": 3, "height": h, "width": w, "mean": ptr(mean), "std": ptr(std), "radius": 7,
            "omega": 0.95, "t_min": 0.1, "airlight_min": 0.1, "guided_radius": 28, "guided_eps": 1e-3, "cond": ptr(cond),
            "restored": ptr(restored), "airlight": ptr(airlight), "transmission": ptr(t), "stats": ptr(stats),
            "guided_stats": ptr(guided), "n_slots": 2, "workspace": ptr(ws), "stream": None}
    bad_std, bad_mean = np.array([0.2, 0.0, 0.2], np.float32), np.array([0.4, np.inf, 0.4], np.float32)
    einval = [("image", None), ("mean", None), ("std", None), ("restored", None), ("airlight", None), ("stats", None), ("guided_stats", None),
              ("workspace", None), ("channels", 1), ("channels", 4), ("batch", -1), ("height", 0), ("width", 0), ("n_slots", 0),
              ("radius", 0), ("radius", 16), ("radius", -7),
              ("guided_radius", 0), ("guided_radius", 33), ("guided_radius", -28),
              ("guided_eps", 0.0), ("guided_eps", 5e-5), ("guided_eps", 1.0001), ("guided_eps", -1e-3), ("guided_eps", float("nan")),
              ("guided_eps", float("inf")),
              ("omega", 0.0), ("omega", 1.5), ("omega", float("nan")), ("t_min", 0.0), ("t_min", 1.0001), ("t_min", float("nan")),
              ("airlight_min", 0.0), ("airlight_min", -0.1), ("airlight_min", 2.0), ("airlight_min", float("inf")),
              ("std", ptr(bad_std)), ("mean", ptr(bad_mean))]
    for name, value in einval:
        args = dict(good, **{name: value})
        assert lib.awseg_dehaze_guided(*args.values()) == -1, (name, value)
    assert lib.awseg_dehaze_guided(*dict(good, batch=65536).values()) == -2
    assert lib.awseg_dehaze_guided(*dict(good, height=1 << 16, width=1 << 15).values()) == -2
    odd = ctypes.c_void_p(ws.ctypes.data + 4)
    assert lib.awseg_dehaze_guided(*dict(good, workspace=odd).values()) == -3
    for kw in ({}, {"transmission": None}, {"cond": None}, {"guided_radius": 1, "guided_eps": 1.0}, {"guided_radius": 32, "guided_eps": 1e-4}):
        assert lib.awseg_dehaze_guided(*dict(good, batch=0, **kw).values()) == 0            # nothing to do, nothing launched
    assert (restored == 7.0).all() and (airlight == 7.0).all() and (t == 7.0).all()
    assert not stats.any() and not guided.any() and not ws.any()


def test_ops_dehaze_guided_checks_its_arguments_and_has_no_cpu_path():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N, ops
    x = torch.zeros(1, 3, 4, 5)
    with pytest.raises(N.AwsegError, match="no CPU fallback"):
        ops.dehaze_guided(x)
    for bad in (torch.zeros(1, 1, 4, 5), torch.zeros(1, 3, 4, 5, dtype=torch.float64), torch.zeros(3, 4, 5)):
        with pytest.raises(ValueError, match="float32"):
            ops.dehaze_guided(bad)
    for kw in ({"radius": 0}, {"radius": 16}, {"omega": 0.0}, {"t_min": 1.5}, {"airlight_min": 0}, {"guided_radius": 0}, {"guided_radius": 33},
               {"guided_radius": 7.0}, {"guided_radius": True}, {"guided_eps": 0}, {"guided_eps": 5e-5}, {"guided_eps": 2},
               {"guided_eps": float("nan")}, {"guided_eps": "1e-3"}, {"mean": [0.5] * 3}, {"mean": [0.5] * 3, "std": [0.2, 0.0, 0.2]},
               {"stats": torch.zeros(2, 7, dtype=torch.int64)}, {"guided_stats": torch.zeros(1, 3, dtype=torch.int64)},
               {"stats": torch.zeros(2, 8, dtype=torch.int64), "guided_stats": torch.zeros(3, 4, dtype=torch.int64)},
               {"guided_stats": torch.zeros(1, 4, dtype=torch.int32)}, {"cond": torch.zeros(2, dtype=torch.int32)},
               {"out": torch.zeros(1, 3, 4, 6)}, {"out": x}):
        with pytest.raises(ValueError):
            ops.dehaze_guided(x, **kw)
    with pytest.raises(TypeError):
        ops.dehaze_guided(x, refine=1)
    p = ops.dehaze_guided_parameters()
    assert p == {"radius": 7, "omega": float(np.float32(0.95)), "t_min": float(np.float32(0.1)), "airlight_min": float(np.float32(0.1)),
                 "guided_radius": 28, "guided_eps": float(np.float32(1e-3))}
    assert ops.dehaze_guided_parameters(radius=3)["guided_radius"] == 12
    assert ops.new_guided_stats("cpu", 3).shape == (3, ops.GUIDED_ROW) and ops.new_guided_stats("cpu", 3).dtype == torch.int64
    with pytest.raises(ValueError):
        ops.new_guided_stats("cpu", 0)
    empty = ops.dehaze_guided(torch.zeros(0, 3, 4, 5), transmission=True)
    assert [tuple(v.shape) for v in empty] == [(0, 3, 4, 5), (0, 3), (0, 4, 5)]
