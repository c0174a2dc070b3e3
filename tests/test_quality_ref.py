"""CPU checks of the image-quality feature: the two numpy models (tests/quality_ref.py) against each other and against closed
forms, the host math of the counters (quality_metrics_from_stats), the option parser, the report section, the command line and the
harness with the native call replaced by the float32 model.  No GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import paired_ref as PR
from tests import quality_ref as QR
from tests.test_strata_ref import TinyModel, _sweep_batches

ROOT = Path(__file__).resolve().parent.parent
TAPS = QR.taps11()
# The float32 taps sum to 1 only within rounding, so a window mean of a constant k is S k with S = (sum of the taps)^2, and the
# window variance of a constant is k^2 S (1 - S) instead of 0: the closed forms below hold within that.
S2 = float(TAPS.astype(np.float64).sum()) ** 2
TAP_SLACK = abs(S2 * (1.0 - S2))
# The float32 separable model against the float64 direct one, on the frame means of l, cs and s: the worst deviation measured over
# the inputs of tests/test_gpu_quality.py's equality test (every shape, rendered and random frames) was 1.41e-6; the bound is 4 x
# that.  It is float32 cancellation in mxx - mx * mx, and it is the accuracy of the reported ssim_* numbers.
FRAME_MEAN_TOLERANCE = 4 * 1.41e-6
# single windows of smooth frames deviate far more (same cancellation, no averaging)
SHAPES = [(2, 3, 11, 11), (3, 3, 31, 53), (2, 3, 67, 131), (1, 3, 41, 73), (1, 3, 42, 74), (1, 3, 43, 75), (2, 3, 43, 140),
          (3, 1, 31, 53), (3, 4, 31, 53), (2, 1, 43, 76), (2, 4, 43, 76)]


def _pkg():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics, report
    return ops, harness, metrics, report


# ----------------------------------------------------------------------------- the two formulations
@pytest.mark.parametrize("maker", [QR.rendered_frames, QR.random_frames], ids=["rendered", "random"])
def test_the_two_formulations_agree_on_frame_means(maker):
    worst = 0.0
    for b, ch, h, w in SHAPES:
        var, clean, fr, mean, std = maker(11 + h + w + ch, b, ch, h, w)
        for i in range(b):
            row = QR.frame_terms(var[i], clean[fr[i]], mean, std, TAPS, QR.C1, QR.C2)
            assert row[QR.BAD_WIN] == 0 and row[QR.N_WIN] == ch * (h - 10) * (w - 10)
            for idx, v in zip((QR.SUM_L, QR.SUM_CS, QR.SUM_S), QR.ssim_float64(var[i], clean[fr[i]], mean, std, TAPS)):
                worst = max(worst, abs(row[idx] * QR.UNIT / row[QR.N_WIN] - float(v.mean())))
    print(f"worst frame-mean deviation float32 separable vs float64 direct: {worst:.3e}")
    assert worst <= FRAME_MEAN_TOLERANCE


def test_layout_constants_mirror_the_header_and_the_taps_are_the_ssim_window():
    import re
    ops, _, _, _ = _pkg()
    text = (ROOT / "include" / "awseg.h").read_text()
    get = lambda n: re.search(r"#define\s+%s\s+(.+)" % n, text).group(1).strip()   # noqa: E731
    assert int(get("AWSEG_IQ_ROW")) == ops.IQ_ROW == QR.IQ_ROW == len(ops.IQ_FIELDS)
    assert (int(get("AWSEG_IQ_TILE_H")), int(get("AWSEG_IQ_TILE_W"))) == (ops.IQ_TILE_H, ops.IQ_TILE_W)
    assert get("AWSEG_IQ_TERM_BUDGET") == "(1LL << 36)" and ops.IQ_TERM_BUDGET == 1 << 36 and ops.IQ_UNIT == QR.UNIT == 2.0 ** -24
    assert ops.IQ_TERM_BUDGET * (1 << 26) < 1 << 63                   # a term is at most 4.0 * 2^24
    taps = ops.ssim_taps()
    assert taps.dtype == np.float32 and taps.shape == (11,) and np.array_equal(taps, TAPS) and np.array_equal(taps, taps[::-1])
    assert abs(float(taps.astype(np.float64).sum()) - 1.0) < 1e-7 and abs(taps[5] / taps[4] - np.exp(0.5 / 2.25)) < 1e-6
    assert [ops.IQ_FIELDS.index(f) for f in ("frames", "sum_sq", "windows", "sum_ssim", "windows_unmeasured")] == [0, 3, 5, 8, 9]


# ----------------------------------------------------------------------------- closed forms
def test_identical_frames_give_one_exactly_at_every_window():
    for maker in (QR.rendered_frames, QR.random_frames):
        _, clean, _, mean, std = maker(7, 1, 3, 29, 37)
        st, oob = QR.counters(clean, clean, np.arange(clean.shape[0]), mean, std)
        n = clean.shape[0] * 3 * 19 * 27
        assert oob == 0 and st[0, QR.N_WIN] == n and st[0, QR.BAD_WIN] == 0
        assert st[0, QR.SUM_L] == st[0, QR.SUM_CS] == st[0, QR.SUM_S] == n << 24
        assert st[0, QR.SUM_ABS] == st[0, QR.SUM_SQ] == 0 and st[0, QR.N_ERR] == clean.size


def test_constant_frames_against_the_analytic_luminance():
    mean, std = np.zeros(1, np.float32), np.ones(1, np.float32)
    for a, b in ((0.2, 0.7), (0.5, 0.5), (0.0, 1.0), (0.9, 0.1)):
        x, y = np.full((1, 14, 15), a, np.float32), np.full((1, 14, 15), b, np.float32)
        a, b = float(np.float32(a)), float(np.float32(b))
        row = QR.frame_terms(x, y, mean, std, TAPS, QR.C1, QR.C2)
        lum = (2 * a * b + QR.C1) / (a * a + b * b + QR.C1)
        assert row[QR.N_WIN] == 4 * 5
        assert abs(row[QR.SUM_L] * QR.UNIT / 20 - lum) < 2e-6        # a handful of float32 roundings of numbers <= 1
        l64, cs64, _ = QR.ssim_float64(x, y, mean, std, TAPS)
        # 2 cxy - vx - vy = -(a - b)^2 S (1 - S) over a denominator of at least c2
        assert np.allclose(l64, lum, rtol=0, atol=1e-9) and np.allclose(cs64, 1.0, rtol=0, atol=(a - b) ** 2 * TAP_SLACK / QR.C2 + 1e-12)


def test_an_added_constant_leaves_the_contrast_factor_at_one():
    rng = np.random.default_rng(5)
    x = rng.random((2, 20, 23)) * 0.6
    mean, std = np.zeros(2), np.ones(2)
    lum, cs, s = QR.ssim_float64(x + 0.3, x, mean, std, TAPS)
    assert np.abs(cs - 1.0).max() <= 0.3 ** 2 * TAP_SLACK / QR.C2 + 1e-12 and TAP_SLACK < 1e-6 and lum.max() < 1.0 and np.allclose(s, lum * cs)


def test_a_single_changed_pixel_gives_the_analytic_mse():
    _, clean, _, mean, std = QR.rendered_frames(2, 1, 3, 16, 18, refs=1)
    var = clean.copy()
    var[0, 1, 7, 9] = clean[0, 1, 7, 9] + np.float32(64.0 / 255.0) / std[1]
    st, _ = QR.counters(var, clean, [0], mean, std)
    d = float((var[0, 1, 7, 9] - clean[0, 1, 7, 9]) * std[1])
    assert st[0, QR.N_ERR] == 3 * 16 * 18 and st[0, QR.BAD_ERR] == 0
    assert st[0, QR.SUM_SQ] == int(np.rint(np.float32(d) * np.float32(d) * QR.SCALE)) and st[0, QR.SUM_ABS] == int(np.rint(np.float32(d) * QR.SCALE))
    _, _, metrics, _ = _pkg()
    full = np.zeros((3, QR.IQ_ROW), np.int64)
    full[0] = full[2] = st[0]
    res = metrics.quality_metrics_from_stats(full, ["clean", "fog_s1"], ["fog"], 1, {})
    want = (64.0 / 255.0) ** 2 / (3 * 16 * 18)
    assert abs(res["mse_fog_s1"] - want) < want * 1e-5 and abs(res["psnr_fog_s1"] - 10 * np.log10(1 / want)) < 1e-4
    assert abs(res["mean_abs_change_fog_s1"] - 64.0 / (3 * 16 * 18)) < 1e-4 and res["mse_fog"] == res["mse_fog_s1"] == res["mean_mse"]


def test_frame_routing_of_the_model():
    var, clean, _, mean, std = QR.rendered_frames(9, 4, 3, 12, 13, refs=2)
    st, oob = QR.counters(var, clean, [0, -1, 2, 1], mean, std, cond=[0, 0, 0, 7], n_slots=3)
    assert oob == 12 * 13 and st[0, QR.FRAMES] == 2 and st[1, QR.FRAMES] == 1 and not st[2].any()
    short, _ = QR.counters(var[:, :, :10], clean[:, :, :10], [0, 1, 0, 1], mean, std)
    assert short[0, QR.N_WIN] == short[0, QR.BAD_WIN] == 0 and short[0, QR.N_ERR] == 4 * 3 * 10 * 13    # no window, the error terms stay


# ----------------------------------------------------------------------------- host math
def _stats(slots, ssim, mse=None, windows=1000):
    """Counters that give the named slots the SSIM values asked for (and, when given, the MSE)."""
    raw = np.zeros((1 + len(slots), QR.IQ_ROW), np.int64)
    for name, q in ssim.items():
        r = raw[1 + slots.index(name)]
        r[QR.FRAMES], r[QR.N_WIN], r[QR.N_ERR] = 1, windows, windows
        r[QR.SUM_S] = int(round(q * windows * 2 ** 24))
        r[QR.SUM_L], r[QR.SUM_CS] = int(0.9 * windows * 2 ** 24), int(0.8 * windows * 2 ** 24)
        r[QR.SUM_SQ] = int((0.01 if mse is None else mse[name]) * windows * 2 ** 24)
        r[QR.SUM_ABS] = int(0.05 * windows * 2 ** 24)
    raw[0] = raw[1:].sum(0)
    return raw


def test_matched_damage_interpolation_end_points_and_refusals_to_extrapolate():
    _, _, metrics, _ = _pkg()
    slots = ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2"]
    ssim = {"fog_s1": 0.875, "fog_s2": 0.5, "night_s1": 0.75, "night_s2": 0.625}
    res0 = {"miou_clean": 0.8, "miou_fog_s1": 0.7, "miou_fog_s2": 0.4, "miou_night_s1": 0.6, "miou_night_s2": 0.5}
    deg = lambda c, a: max(0.0, (c - a) / c)                          # noqa: E731
    res = metrics.quality_metrics_from_stats(_stats(slots, ssim), slots, ["fog", "night"], 2, res0, [0.9375, 0.75, 0.5, 0.625, 1 - 2 ** -20],
                                             degradation=deg)
    assert all(isinstance(v, float) for v in res.values()) and not any(k.endswith("_clean") for k in res)
    assert res["ssim_fog_s1"] == 0.875 and res["ssim_luminance_fog_s1"] == pytest.approx(0.9, abs=1e-6)
    assert res["ssim_fog"] == pytest.approx((0.875 + 0.5) / 2) and res["mean_ssim"] == pytest.approx(sum(ssim.values()) / 4)
    # first segment (1, 0.8) .. (0.875, 0.7): halfway; second segment (0.875, 0.7) .. (0.5, 0.4): a third of the way; the end point
    assert res["miou_at_ssim94_fog"] == pytest.approx(0.75) and res["miou_at_ssim75_fog"] == pytest.approx(0.6)
    assert res["miou_at_ssim50_fog"] == pytest.approx(0.4) and res["robustness_degradation_at_ssim50_fog"] == pytest.approx(0.5)
    assert res["miou_at_ssim75_night"] == pytest.approx(0.6) and res["miou_at_ssim62_night"] == pytest.approx(0.5)
    assert res["miou_at_ssim100_fog"] == pytest.approx(0.8, abs=1e-6)
    assert "miou_at_ssim50_night" not in res                         # below night's last level: no extrapolation
    assert res["mean_miou_at_ssim75"] == pytest.approx(0.6) and "mean_miou_at_ssim50" not in res
    assert res["miou_drop_per_ssim_fog_s2"] == pytest.approx(0.4 / 0.5) and res["miou_drop_per_ssim_night_s1"] == pytest.approx(0.2 / 0.25)
    assert not any(k.startswith("ssim_not_monotonic") for k in res) and "quality_unmeasured_terms" not in res


def test_non_monotonic_ssim_missing_slots_and_zero_mse():
    _, _, metrics, _ = _pkg()
    slots = ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2", "rain_s1", "rain_s2"]
    ssim = {"fog_s1": 0.6, "fog_s2": 0.7, "night_s1": 1.0, "night_s2": 0.5, "rain_s1": 0.9}
    mse = {"fog_s1": 0.01, "fog_s2": 0.02, "night_s1": 0.0, "night_s2": 0.1, "rain_s1": 0.001}
    res0 = {"miou_clean": 0.8, "miou_fog_s1": 0.7, "miou_fog_s2": 0.4, "miou_night_s1": 0.8, "miou_night_s2": 0.5, "miou_rain_s1": 0.7}
    raw = _stats(slots, ssim, mse)
    raw[0, QR.BAD_ERR], raw[0, QR.BAD_WIN] = 3, 5
    res = metrics.quality_metrics_from_stats(raw, slots, ["fog", "night", "rain"], 2, res0)
    for kind in ("fog", "night", "rain"):                             # rising, flat at 1 (an identical variant), a level without frames
        assert res[f"ssim_not_monotonic_{kind}"] == 1.0 and not any(k.startswith("miou_at_ssim") and k.endswith(kind) for k in res)
    assert not any(k.startswith("mean_miou_at_ssim") for k in res)
    assert res["mse_night_s1"] == 0.0 and "psnr_night_s1" not in res and "psnr_night_s2" in res and "psnr_night" in res
    assert "miou_drop_per_ssim_night_s1" not in res and "miou_drop_per_ssim_night_s2" in res      # 1 - ssim below 1e-6
    assert "ssim_rain_s2" not in res and "mse_rain_s2" not in res and "ssim_rain" in res
    assert res["quality_unmeasured_terms"] == 3.0 and res["quality_unmeasured_windows"] == 5.0
    assert res["psnr_fog_s1"] == pytest.approx(20.0, abs=1e-5)
    no_clean = metrics.quality_metrics_from_stats(raw, slots, ["fog"], 2, {"miou_fog_s1": 0.7})
    assert no_clean["ssim_not_monotonic_fog"] == 1.0 and not any(k.startswith("miou_drop") for k in no_clean)
    with pytest.raises(ValueError, match="image-quality stats"):
        metrics.quality_metrics_from_stats(raw[:-1], slots, ["fog"], 2, res0)


def test_option_parser():
    _, harness, _, _ = _pkg()
    sweep = {"evaluation.severities": [0.3, 0.8]}
    assert harness.quality_options({}) is None and harness.quality_options(dict(sweep, **{"evaluation.image_quality": False})) is None
    assert harness.quality_options(dict(sweep, **{"evaluation.image_quality": True})) == {"targets": [0.9, 0.75, 0.5]}
    assert harness.quality_options(dict(sweep, **{"evaluation.image_quality": True, "evaluation.image_quality_targets": (0.25,)})) == {"targets": [0.25]}
    with pytest.raises(ValueError, match="severity sweep"):
        harness.quality_options({"evaluation.image_quality": True})
    for on in (1, "yes", [True]):
        with pytest.raises(ValueError, match="true or false"):
            harness.quality_options(dict(sweep, **{"evaluation.image_quality": on}))
    for bad in ([], [0.5] * 9, [0.0], [1.0], [0.5, -0.1], [float("nan")], ["0.5"], [True], 0.5, "0.5,0.6", {"a": 0.5}, [[0.5]]):
        for on in (True, False):                                      # checked also when the option is off
            with pytest.raises(ValueError, match="image_quality_targets"):
                harness.quality_options(dict(sweep, **{"evaluation.image_quality": on, "evaluation.image_quality_targets": bad}))
    with pytest.raises(ValueError, match="float32"):
        harness.quality_options(dict(sweep, **{"evaluation.image_quality": True}), images=torch.zeros(1, 3, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        harness.quality_options(dict(sweep, **{"evaluation.image_quality": True}), images=torch.zeros(1, 1, 4, 4))
    harness.check_quality_budget(1 << 36)
    with pytest.raises(OverflowError, match="image-quality"):
        harness.check_quality_budget((1 << 36) + 1)


def test_ops_refuses_bad_arguments_before_any_launch():
    """Every refusal comes before the library is touched: host tensors never reach a launch here."""
    ops, _, _, _ = _pkg()
    img, ref = torch.zeros(2, 3, 12, 16), torch.zeros(3, 3, 12, 16)
    fr, stats = torch.zeros(2, dtype=torch.int32), torch.zeros(2, 10, dtype=torch.int64)
    for kw in (dict(image=img.double()), dict(image=img[0]), dict(ref_images=ref[:, :, :11]), dict(ref_images=ref[:, :2]),
               dict(ref_images=ref.reshape(3, 3, -1)), dict(frame_ref=fr.long()), dict(stats=stats[:, :9]), dict(stats=stats.int()),
               dict(cond=torch.zeros(3, dtype=torch.int32)), dict(oob=torch.zeros(2, dtype=torch.int64)), dict(c1=0.0),
               dict(c2=float("nan")), dict(mean=[0.5] * 3), dict(mean=[0.5] * 3, std=[0.2, 0.0, 0.2]), dict(taps=[0.1] * 10)):
        with pytest.raises(ValueError):
            ops.image_quality(**dict(dict(image=img, ref_images=ref, frame_ref=fr, stats=stats), **kw))
    with pytest.raises(ValueError, match="n_slots"):
        ops.new_image_quality_stats("cpu", 0)
    assert ops.new_image_quality_stats("cpu", 3).shape == (3, 10)
    dec = ops.image_quality_to_numpy(np.arange(20).reshape(2, 10))
    assert list(dec) == list(ops.IQ_FIELDS) and dec["sum_ssim"].tolist() == [8, 18]
    with pytest.raises(ValueError, match="10 counters"):
        ops.image_quality_to_numpy(np.zeros((2, 9), np.int64))


def test_report_section():
    _, _, metrics, report = _pkg()
    slots = ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2"]
    ssim = {"fog_s1": 0.875, "fog_s2": 0.5, "night_s1": 0.75, "night_s2": 0.8}
    res0 = {"miou_clean": 0.8, "miou_fog_s1": 0.7, "miou_fog_s2": 0.4, "miou_night_s1": 0.6, "miou_night_s2": 0.5}
    res = dict(res0, **metrics.quality_metrics_from_stats(_stats(slots, ssim), slots, ["fog", "night"], 2, res0))
    text = report.report_markdown(res)
    assert "## Image Quality" in text and "## Image Quality" not in report.report_markdown(res0)
    assert "| fog | 2 | 20.00 | 0.500 | 0.900 | 0.800 | 0.400 | 0.800 |" in text
    assert "| Kind | SSIM 0.9 | SSIM 0.75 | SSIM 0.5 |" in text and "| fog | 0.720 / 0.100 | 0.600 / 0.250 | 0.400 / 0.500 |" in text
    assert "SSIM does not decrease with the level for night" in text and "| night | - / - | - / - | - / - |" in text


def test_command_line():
    spec = importlib.util.spec_from_file_location("evaluate_cli_quality", ROOT / "scripts" / "evaluate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    args = ap.parse_args(["ckpt.pt"])
    assert args.image_quality is False and args.image_quality_targets is None
    args = ap.parse_args(["ckpt.pt", "--image-quality", "--image-quality-targets", "0.9,0.75,0.5"])
    assert args.image_quality is True and mod.parse_image_quality_targets(args.image_quality_targets) == [0.9, 0.75, 0.5]
    with pytest.raises(ValueError, match="--image-quality-targets"):
        mod.parse_image_quality_targets("a,b")


# ----------------------------------------------------------------------------- the harness with the native calls replaced
def _patch_native(monkeypatch, ops, C, seen):
    def combine_argmax_confusion(logits, seg2, mode, want_logits=False, label=None, counts=None, oob=None, cond=None, pred_out=None, **k):
        pred = logits.argmax(1).to(torch.uint8)
        if pred_out is not None:
            pred_out.copy_(pred.view(pred_out.shape))
        for b in range(pred.shape[0]):
            row = torch.from_numpy(PR.confusion(pred[b].numpy(), label[b].numpy(), C))
            counts[0] += row
            if cond[b] >= 0:
                counts[1 + int(cond[b])] += row

    def prediction_consistency(pred, ref_maps, frame_ref, label, c, stats, oob, cond=None, **k):
        refs = [ref_maps[int(r)].numpy() for r in frame_ref]
        st, bad = PR.consistency_stats(pred.numpy(), refs, label.numpy(), c, cond=cond.tolist(), n_slots=stats.shape[0])
        stats += torch.from_numpy(st)
        oob += bad

    def image_quality(image, ref_images, frame_ref, stats, cond=None, oob=None, **k):
        assert not k and ref_images.dim() == 4 and ref_images.shape[1:] == image.shape[1:]
        st, bad = QR.counters(image.numpy(), ref_images.numpy(), frame_ref.numpy(), cond=cond.tolist(), n_slots=stats.shape[0])
        stats += torch.from_numpy(st)
        oob += bad
        seen.append((image.clone(), ref_images[frame_ref.long()].clone()))
    for name, fn in (("combine_argmax_confusion", combine_argmax_confusion), ("prediction_consistency", prediction_consistency),
                     ("image_quality", image_quality)):
        monkeypatch.setattr(ops, name, fn)


def _run(harness, metrics_mod, C, batches, sweep, quality):
    conds = ["clean", *sweep.kinds]
    m = metrics_mod.RobustnessMetrics(C, conds)
    st = harness.EvalState(m, conds, "cpu", 15, False, sweep=sweep, quality=quality)
    model = TinyModel(C)
    for b in batches:
        harness.eval_batch(model, st, b["image"], b["label"], b["weather_condition"], m, with_stats=False, sources=b["source"],
                           severity=b["severity"])
    return st, harness.finalize(st, m)


def test_harness_on_the_cpu_with_the_model_in_place_of_the_native_call(monkeypatch):
    ops, harness, metrics, report = _pkg()
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import resolve_severities
    C, kinds, levels = 5, ("fog", "night"), 2
    seen = []
    _patch_native(monkeypatch, ops, C, seen)
    sweep = resolve_severities([0.3, 0.8], ["clean", *kinds])
    batches = _sweep_batches(8, 4, 12, 13, C, kinds, levels)
    st_off, off = _run(harness, metrics, C, batches, sweep, None)
    assert st_off.quality is None and st_off.clean_frames is None and not seen      # off: nothing allocated, nothing called
    st, on = _run(harness, metrics, C, batches, sweep, {"targets": [0.9, 0.5]})
    assert len(seen) == 8                                             # every variant batch, no clean batch
    by_source = {s: b["image"][i] for b in batches if b["severity"] == 0 for i, s in enumerate(b["source"])}
    variants = [b for b in batches if b["severity"]]
    for (image, twins), b in zip(seen, variants):
        assert torch.equal(image, b["image"]) and torch.equal(twins, torch.stack([by_source[s] for s in b["source"]]))
    # with the option on, the old keys keep their values bit for bit
    assert list(off) == [k for k in on if k in off]
    assert repr([off[k] for k in off]) == repr([on[k] for k in off])
    new = {k: v for k, v in on.items() if k not in off}
    want = metrics.quality_metrics_from_stats(st.quality["stats"].numpy(), sweep.slots(), kinds, levels, off, [0.9, 0.5],
                                              metrics.RobustnessMetrics(C).compute_robustness_degradation_ratio)
    assert new == want and st.quality["terms"] == 8 * 2 * 3 * 12 * 13
    names = ["fog_s1", "fog_s2", "fog", "night_s2", "night"]
    assert {f"{m}_{n}" for n in names for m in ("mse", "psnr", "mean_abs_change", "ssim", "ssim_luminance", "ssim_contrast")} <= set(new)
    # night_s1 is an identical variant: no error, SSIM exactly 1, so night's SSIM does not strictly decrease from the clean point
    assert new["mse_night_s1"] == 0.0 and "psnr_night_s1" not in new and new["ssim_night_s1"] == 1.0
    assert new["ssim_not_monotonic_night"] == 1.0 and 1.0 > new["ssim_fog_s1"] > new["ssim_fog_s2"]
    # fog adds 6 and 12 grey levels to every pixel: the mean absolute change says so, and only the luminance factor moves
    assert new["mean_abs_change_fog_s1"] == pytest.approx(6.0, abs=1e-3) and new["mean_abs_change_fog_s2"] == pytest.approx(12.0, abs=1e-3)
    assert new["ssim_contrast_fog_s2"] == pytest.approx(1.0, abs=1e-4) and new["ssim_luminance_fog_s2"] < 0.999
    assert not any(k.endswith("_clean") for k in new) and not st.quality["stats"][1].any()
    assert "## Image Quality" in report.report_markdown(on) and "## Image Quality" not in report.report_markdown(off)


def test_one_clean_frame_buffer_serves_both_options(monkeypatch):
    ops, harness, metrics, _ = _pkg()
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import resolve_severities
    from tests import test_strata_ref as TS
    C, kinds = 5, ("fog", "night")
    seen, seen_q = [], []
    TS._patch_native(monkeypatch, ops, C, seen)
    _patch_native(monkeypatch, ops, C, seen_q)
    sweep = resolve_severities([0.3, 0.8], ["clean", *kinds])
    batches = _sweep_batches(8, 4, 12, 13, C, kinds, 2)
    conds = ["clean", *kinds]
    m = metrics.RobustnessMetrics(C, conds)
    st = harness.EvalState(m, conds, "cpu", 15, False, sweep=sweep, change=[0.5, 4.5], quality={"targets": [0.5]})
    for b in batches:
        harness.eval_batch(TinyModel(C), st, b["image"], b["label"], b["weather_condition"], m, with_stats=False, sources=b["source"],
                           severity=b["severity"])
    assert st.change["rows"] is st.clean_frames["rows"] and st.change["rows"].shape == (st.paired["rows"].shape[0], 3 * 12 * 13)
    assert len(seen_q) == 8 and [s[0] for s in seen] == ["change", "stats"] * 8
    res = harness.finalize(st, m)
    assert "ssim_fog_s1" in res and "change_fraction_fog_s1_chg0" in res
