"""CPU checks of the change-strata feature: the numpy model (tests/strata_ref.py) against itself and against closed forms, the host
math of the counters (change_metrics_from_stats), the option parser, the report section, the command line and the harness with the
native calls replaced by the model.  No GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import paired_ref as PR
from tests import strata_ref as SR

ROOT = Path(__file__).resolve().parent.parent
DEFAULT = [0.5, 4.5, 16.5, 64.5]


def _pkg():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics, report
    return ops, harness, metrics, report


def frames(seed, b, ch, hw, refs=None):
    """Normalised float32 frames rendered from 8-bit data: `refs` clean frames and b variants that change a part of the pixels."""
    rng = np.random.default_rng(seed)
    refs = b if refs is None else refs
    std = SR.IMAGENET_STD[:ch] if ch <= 3 else np.full(ch, 0.25, np.float32)
    u8 = rng.integers(0, 256, (refs, ch, hw))
    clean = ((u8 / 255.0).astype(np.float32) - np.float32(0.45)) / std[:, None]
    delta = rng.choice([0, 0, 0, 1, 3, 5, 17, 40, 65, 200], (b, ch, hw))
    fr = rng.integers(0, refs, b)
    var = ((np.clip(u8[fr] + delta, 0, 255) / 255.0).astype(np.float32) - np.float32(0.45)) / std[:, None]
    return var.astype(np.float32), clean.astype(np.float32), fr.astype(np.int32), (255.0 * std).astype(np.float32)


def maps(seed, b, c, hw, K, oob=True):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, c, (b, hw)).astype(np.uint8)
    pred = np.where(rng.random((b, hw)) < 0.3, rng.integers(0, c, (b, hw)), ref).astype(np.uint8)
    label = np.where(rng.random((b, hw)) < 0.5, ref, rng.integers(0, c, (b, hw))).astype(np.int64)
    label[:, :3] = 255
    label[:, 3:5] = c + 2
    label[:, 5] = -1
    stratum = rng.integers(0, K, (b, hw)).astype(np.uint8)
    stratum[:, 6] = 255
    stratum[:, 7] = K
    if oob:
        pred[0, 8], ref[-1, 9] = c, 250
    return pred, label, stratum, ref


# ----------------------------------------------------------------------------- the model against itself
@pytest.mark.parametrize("shape", [(2, 3, 40), (3, 1, 7), (1, 4, 5), (2, 2, 1)], ids=str)
@pytest.mark.parametrize("edges", [[0.5], DEFAULT, [0.0, 1.0, 2.5, 3.0, 17.0, 64.5, 199.5]], ids=str)
def test_change_strata_loop_and_vector_formulations_agree(shape, edges):
    b, ch, hw = shape
    var, clean, fr, scale = frames(1, b, ch, hw, refs=3)
    var[0, 0, 0] = np.nan
    clean[int(fr[0]), ch - 1, hw - 1] = np.inf
    fr[-1] = -1 if b > 1 else fr[-1]
    fr2 = fr.copy()
    fr2[0] = 3                                                       # a row the clean frames do not have
    for f in (fr, fr2):
        a, oob_a = SR.change_strata(var, clean, f, edges, scale)
        l, oob_l = SR.change_strata_loop(var, clean, f, edges, scale)
        assert np.array_equal(a, l) and oob_a == oob_l == (hw if f is fr2 else 0)
        assert a.dtype == np.uint8 and set(np.unique(a)) <= set(range(len(edges) + 1)) | {255}


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "unpaired"])
@pytest.mark.parametrize("c,K", [(5, 2), (7, 8), (19, 5)], ids=str)
def test_stratified_loop_and_vector_formulations_agree(c, K, paired):
    pred, label, stratum, ref = maps(2, 3, c, 90, K)
    kw = dict(refs=ref, frame_ref=[2, -1, 0]) if paired else {}
    a, oob_a = SR.stratified_stats(pred, label, stratum, K, c, cond=[0, 1, 5], n_slots=3, **kw)
    l, oob_l = SR.stratified_stats(pred, label, stratum, K, c, cond=[0, 1, 5], n_slots=3, counts=SR.stratified_counts_loop, **kw)
    assert np.array_equal(a, l) and oob_a == oob_l and oob_a > 0
    assert a.shape == (3, K + 1, c * c + 6) and a[0, K, c * c + 5] > 0     # 255 and K went to the unmeasured row
    if not paired:
        assert not a[..., c * c:c * c + 5].any()
    # summed over the strata: the consistency counters of the paired sweep
    if paired:
        want, bad = PR.consistency_stats(pred, [ref[2], None, ref[0]], label, c, cond=[0, 1, 5], n_slots=3, skip={1})
        assert np.array_equal(a[..., c * c:c * c + 4].sum(1), want[:, c * c:]) and bad == oob_a
        agree = want[:, :c * c].reshape(3, c, c)
        assert np.array_equal(a[..., c * c + 4].sum(1), np.trace(agree, axis1=1, axis2=2))
        assert np.array_equal(a[..., c * c + 5].sum(1), agree.sum((1, 2)))


# ----------------------------------------------------------------------------- planted closed forms
def _results(metrics, stats, edges, C):
    return metrics.change_metrics_from_stats(stats, edges, ["clean", "fog_s1"], ["fog"], 1, C)


def test_identical_twin_is_all_stratum_zero():
    ops, harness, metrics, report = _pkg()
    var, clean, fr, scale = frames(3, 2, 3, 50)
    fr = np.arange(2, dtype=np.int32)
    s, oob = SR.change_strata(clean.copy(), clean, fr, DEFAULT)
    assert oob == 0 and not s.any()
    pred, label, _, _ = maps(4, 2, 5, 50, 5, oob=False)
    stats, _ = SR.stratified_stats(pred, label, s, 5, 5, refs=pred, frame_ref=fr, cond=[1, 1], n_slots=3)
    res = _results(metrics, stats, DEFAULT, 5)
    assert res["change_fraction_fog_s1_chg0"] == 1.0 and res["consistency_fog_s1_chg0"] == 1.0 and res["mean_consistency_chg0"] == 1.0
    assert all(res[f"change_fraction_fog_chg{k}"] == 0.0 for k in range(1, 5))
    assert res["corruption_error_rate_fog_chg0"] == 0.0
    assert not any("corruption_error_share" in k for k in res) and "change_unmeasured_pixels" not in res
    assert not any(k.endswith(("_chg1", "_chg2", "_chg3", "_chg4")) and not k.startswith(("change_fraction", "mean_change_fraction")) for k in res)


def test_planted_square_edge_equality_nan_and_inf():
    ops, harness, metrics, report = _pkg()
    H, W = 20, 30
    clean = np.zeros((1, 3, H * W), np.float32)
    var = clean.copy().reshape(1, 3, H, W)
    var[0, 1, 4:10, 5:15] = 10.0                                     # 60 pixels, change 10 in channel 1
    var[0, 0, 0, 0] = 4.5                                            # exactly on an edge: the upper stratum
    var[0, 2, 0, 1] = np.nextafter(np.float32(4.5), np.float32(0))   # just below it
    var[0, 2, 19, 29] = np.inf
    var[0, 0, 19, 28] = -np.inf
    var[0, 1, 19, 27] = np.nan
    var[0, 0, 19, 27] = 100.0                                        # another channel's large change does not rescue a NaN
    s, oob = SR.change_strata(var.reshape(1, 3, -1), clean, [0], DEFAULT, scale=[1.0, 1.0, 1.0])
    s = s.reshape(H, W)
    assert oob == 0 and (s[4:10, 5:15] == 2).all() and s[0, 0] == 2 and s[0, 1] == 1
    assert s[19, 29] == 4 and s[19, 28] == 4 and s[19, 27] == 255
    assert np.bincount(s.reshape(-1), minlength=256)[[0, 1, 2, 3, 4, 255]].tolist() == [H * W - 65, 1, 61, 0, 2, 1]
    # the loop formulation plants the same
    assert np.array_equal(SR.change_strata_loop(var.reshape(1, 3, -1), clean, [0], DEFAULT, scale=[1.0, 1.0, 1.0])[0].reshape(H, W), s)
    # counters: the clean prediction is right everywhere, the variant wrong exactly on the square
    label = np.ones((1, H * W), np.int64)
    ref = np.ones((1, H * W), np.uint8)
    pred = ref.copy().reshape(H, W)
    pred[4:10, 5:15] = 0
    stats, bad = SR.stratified_stats(pred.reshape(1, -1), label, s.reshape(1, -1), 5, 3, refs=ref, frame_ref=[0], cond=[1], n_slots=3)
    res = _results(metrics, stats, DEFAULT, 3)
    n = H * W
    assert bad == 0 and res["change_unmeasured_pixels"] == 1.0
    assert res["change_fraction_fog_s1_chg2"] == 61 / n and res["change_fraction_fog_chg0"] == (n - 65) / n
    assert res["mean_change_fraction_chg4"] == 2 / n and res["change_fraction_fog_chg3"] == 0.0
    assert res["corruption_error_share_fog_chg2"] == 1.0 and res["corruption_error_share_fog_chg0"] == 0.0
    assert res["corruption_error_rate_fog_chg2"] == 60 / 61 and res["consistency_fog_chg2"] == 1 / 61
    assert res["accuracy_fog_chg2"] == 1 / 61 and res["accuracy_fog_chg0"] == 1.0 and res["miou_fog_chg0"] == 1.0
    assert "miou_fog_chg3" not in res and "consistency_fog_chg3" not in res
    assert [res[f"change_edge_{k}"] for k in range(4)] == DEFAULT and "change_edge_4" not in res


def test_uint8_frames_sit_far_from_half_integer_edges():
    """The reason for half-integer default edges: with the default scale, the float32 change of a frame rendered from 8-bit data is
    within 3.1e-5 of an integer number of grey levels."""
    u = np.arange(256, dtype=np.int64)
    a, b = np.meshgrid(u, u, indexing="ij")
    worst = 0.0
    for c in range(3):
        mean, std = np.float32([0.485, 0.456, 0.406][c]), SR.IMAGENET_STD[c]
        norm = (u.astype(np.float32) / np.float32(255.0) - mean) / std   # the loader's float32 expression, one rounding per step
        change = np.abs(norm[a] - norm[b]) * SR.DEFAULT_SCALE[c]
        assert change.dtype == np.float32
        worst = max(worst, float(np.abs(change.astype(np.float64) - np.abs(a - b)).max()))
    assert worst < 3.1e-5, worst


# ----------------------------------------------------------------------------- host math
def test_metrics_from_stats_equal_metrics_from_masks():
    ops, harness, metrics, report = _pkg()
    C, K = 5, 5
    pred, label, stratum, ref = maps(6, 4, C, 300, K, oob=False)
    slots = ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2"]
    cond = [1, 2, 2, 3]                                              # night_s2 stays empty
    stats, bad = SR.stratified_stats(pred, label, stratum, K, C, refs=ref, frame_ref=[0, 1, 2, 3], cond=cond, n_slots=6)
    assert bad == 0
    got = metrics.change_metrics_from_stats(stats, DEFAULT, slots, ["fog", "night"], 2, C)
    groups = {"_fog_s1": [0], "_fog_s2": [1, 2], "_fog": [0, 1, 2], "_night_s1": [3], "_night": [3], None: [0, 1, 2, 3]}
    checked = 0
    for name, sel in groups.items():
        want = SR.metrics_from_masks(pred[sel], label[sel], stratum[sel], ref[sel], K, C)
        for metric, per in want.items():
            for k in range(K):
                key = f"mean_{metric}_chg{k}" if name is None else f"{metric}{name}_chg{k}"
                assert (key in got) == (k in per), key
                if k in per:
                    # float64 ratios of integers below 2^53; iou_from_counts divides in float32 (the reference's own expressions)
                    tol = dict(rel=1e-12) if metric != "miou" else dict(abs=2e-7)
                    assert got[key] == pytest.approx(per[k], **tol), key
                    checked += 1
    assert checked > 100 and not any("night_s2" in k for k in got)
    assert all(isinstance(v, float) for v in got.values())
    assert sum(got[f"corruption_error_share_fog_chg{k}"] for k in range(K)) <= 1.0 + 1e-12  # the rest sits in the unmeasured row
    assert got["change_unmeasured_pixels"] == 8.0
    with pytest.raises(ValueError):
        metrics.change_metrics_from_stats(stats[:, :3], DEFAULT, slots, ["fog", "night"], 2, C)
    dec = ops.strata_stats_to_numpy(stats, C)
    assert dec["conf"].shape == (6, K + 1, C, C) and dec["transitions"].shape == (6, K + 1, 4) and dec["pixels"].shape == (6, K + 1)
    assert np.array_equal(dec["pixels"][0], dec["pixels"][1:].sum(0))


# ----------------------------------------------------------------------------- option parser, report, command line
class Cfg(dict):
    def get(self, key, default=None):
        return dict.get(self, key, default)


def test_option_parser():
    ops, harness, metrics, report = _pkg()
    sev = {"evaluation.severities": [0.3, 0.8]}
    assert ops.MAX_STRATA == 8 and ops.STRATUM_NONE == 255
    assert harness.change_option(Cfg()) is None and harness.change_option(Cfg(sev)) is None
    assert harness.change_option(Cfg(sev, **{"evaluation.change_strata": "default"})) == DEFAULT
    assert harness.change_option(Cfg(sev, **{"evaluation.change_strata": [0, 2.5]})) == [0.0, 2.5]
    assert harness.change_option(Cfg(sev, **{"evaluation.change_strata": (1, 2, 3, 4, 5, 6, 7)})) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    with pytest.raises(ValueError, match="severity sweep"):
        harness.change_option(Cfg({"evaluation.change_strata": "default"}))
    for bad in ([], [2.0, 1.0], [1.0, 1.0], [-0.5, 1.0], [1, 2, 3, 4, 5, 6, 7, 8], [1.0, float("inf")], [float("nan")], [1e39], "fine", "1,2",
                True, 3, 2.5, [True], ["1"], {"a": 1}, [[1.0]]):
        with pytest.raises(ValueError, match="evaluation.change_strata"):
            harness.change_option(Cfg(sev, **{"evaluation.change_strata": bad}))
    good = Cfg(sev, **{"evaluation.change_strata": "default"})
    assert harness.change_option(good, torch.zeros(2, 3, 4, 5)) == DEFAULT
    for images in (torch.zeros(2, 1, 4, 5), torch.zeros(2, 3, 20), torch.zeros(2, 3, 4, 5, dtype=torch.float64),
                   torch.zeros(2, 3, 4, 5, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="float32"):
            harness.change_option(good, images)
    assert np.array_equal(ops.change_edges("default"), np.float32(DEFAULT)) and ops.change_edges([1]).dtype == np.float32
    m = metrics.RobustnessMetrics(5, ["clean", "fog"])
    with pytest.raises(ValueError, match="severity sweep"):
        harness.EvalState(m, ["clean", "fog"], "cpu", 15, False, change=DEFAULT)


def test_report_section():
    ops, harness, metrics, report = _pkg()
    C, K = 5, 5
    pred, label, stratum, ref = maps(6, 2, C, 300, K, oob=False)
    stats, _ = SR.stratified_stats(pred, label, stratum, K, C, refs=ref, frame_ref=[0, 1], cond=[1, 2], n_slots=4)
    res = metrics.change_metrics_from_stats(stats, DEFAULT, ["clean", "fog_s1", "night_s1"], ["fog", "night"], 1, C)
    base = {"overall_miou": 0.5}
    assert "Change Strata" not in report.report_markdown(base)
    text = report.report_markdown(dict(base, **res))
    assert "## Change Strata" in text and "Pixels without a measured change" in text
    rows = [ln for ln in text.splitlines() if ln.startswith(("| fog |", "| night |", "| all |"))]
    assert len(rows) == 3 * K                                        # one line per kind and stratum, and the pooled lines
    row = [ln for ln in rows if ln.startswith("| night | [4.5, 16.5) |")][0]
    for key in ("change_fraction_night_chg2", "miou_night_chg2", "consistency_night_chg2", "corruption_error_share_night_chg2"):
        assert f"{res[key]:.3f}" in row
    assert [ln for ln in rows if ln.startswith("| all | >= 64.5 |")] and not [ln for ln in text.splitlines() if ln.startswith("| fog_s1 |")]


def test_command_line():
    spec = importlib.util.spec_from_file_location("awseg_evaluate_script_change", ROOT / "scripts" / "evaluate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args(["ckpt.pt"]).change_strata is None
    assert mod.parse_change_strata(ap.parse_args(["ckpt.pt", "--change-strata", "default"]).change_strata) == "default"
    assert mod.parse_change_strata(ap.parse_args(["ckpt.pt", "--change-strata", "0.5,4.5,16.5"]).change_strata) == [0.5, 4.5, 16.5]
    with pytest.raises(ValueError, match="--change-strata"):
        mod.parse_change_strata("a,b")


# ----------------------------------------------------------------------------- the harness with the native calls replaced
class TinyModel:
    """A pixelwise linear classifier: enough of a model for the single-model branch of eval_batch."""

    def __init__(self, C):
        g = torch.Generator().manual_seed(0)
        self.w = torch.randn(C, 3, generator=g)

    def __call__(self, images):
        return {"segmentation": torch.einsum("kc,bchw->bkhw", self.w, images)}


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

    def change_strata(image, ref_images, frame_ref, edges, out=None, scale=None, oob=None):
        b = image.shape[0]
        s, bad = SR.change_strata(image.reshape(b, 3, -1).numpy(), ref_images.reshape(ref_images.shape[0], 3, -1).numpy(),
                                  frame_ref.numpy(), edges, scale)
        out.copy_(torch.from_numpy(s).view(out.shape))
        oob += bad
        seen.append(("change", image.clone(), ref_images[frame_ref.long()].clone()))
        return out

    def stratified_stats(pred, label, stratum, K, c, stats, oob, ref_maps=None, frame_ref=None, cond=None, **k):
        b = pred.shape[0]
        st, bad = SR.stratified_stats(pred.reshape(b, -1).numpy(), label.reshape(b, -1).numpy(), stratum.reshape(b, -1).numpy(), K, c,
                                      refs=ref_maps.numpy(), frame_ref=frame_ref.numpy(), cond=cond.tolist(), n_slots=stats.shape[0])
        stats += torch.from_numpy(st)
        oob += bad
        seen.append(("stats", K))
    for name, fn in (("combine_argmax_confusion", combine_argmax_confusion), ("prediction_consistency", prediction_consistency),
                     ("change_strata", change_strata), ("stratified_stats", stratified_stats)):
        monkeypatch.setattr(ops, name, fn)


def _sweep_batches(seed, n_src, H, W, C, kinds, levels):
    """Paired batches of two sources: the clean frames first, then every (kind, level); rendered from 8-bit data."""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 200, (n_src, 3, H, W))
    norm = lambda x: torch.from_numpy((((x / 255.0).astype(np.float32) - np.float32(0.45)) / SR.IMAGENET_STD[:, None, None]).astype(np.float32))  # noqa: E731
    label = torch.from_numpy(rng.integers(0, C, (n_src, H, W)).astype(np.uint8))
    label[:, 0, :2] = 255
    out = []
    for g in range(0, n_src, 2):
        src = list(range(g, g + 2))
        out.append(dict(image=norm(u8[src]), label=label[src], weather_condition=["clean"] * 2, source=src, severity=0))
        for i, kind in enumerate(kinds):
            for j in range(1, levels + 1):
                x = u8[src].copy()
                if kind == "fog":
                    x = x + 6 * j                                     # every pixel changes a little
                elif (i, j) != (1, 1):
                    x[:, :, 1:4, 2:7] += 50                           # a local occluder
                # (night_s1: an identical variant, intensity 0)
                out.append(dict(image=norm(x), label=label[src], weather_condition=[kind] * 2, source=src, severity=j))
    return out


def _run(harness, metrics_mod, C, batches, sweep, change):
    conds = ["clean", *sweep.kinds]
    m = metrics_mod.RobustnessMetrics(C, conds)
    st = harness.EvalState(m, conds, "cpu", 15, False, sweep=sweep, change=change)
    model = TinyModel(C)
    for b in batches:
        harness.eval_batch(model, st, b["image"], b["label"], b["weather_condition"], m, with_stats=False, sources=b["source"],
                           severity=b["severity"])
    return st, harness.finalize(st, m)


def test_harness_on_the_cpu_with_the_model_in_place_of_the_native_calls(monkeypatch):
    ops, harness, metrics, report = _pkg()
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import resolve_severities
    C, kinds, levels = 5, ("fog", "night"), 2
    seen = []
    _patch_native(monkeypatch, ops, C, seen)
    sweep = resolve_severities([0.3, 0.8], ["clean", *kinds])
    batches = _sweep_batches(8, 4, 6, 9, C, kinds, levels)
    st_off, off = _run(harness, metrics, C, batches, sweep, None)
    assert st_off.change is None and not seen                        # off: nothing allocated, nothing called
    st, on = _run(harness, metrics, C, batches, sweep, DEFAULT)
    assert [s[0] for s in seen] == ["change", "stats"] * 8           # every variant batch, no clean batch
    for tag, image, twin in (s for s in seen if s[0] == "change"):
        assert image.shape == (2, 3, 6, 9) and twin.shape == (2, 3 * 6 * 9)
    # with the option on, the old keys keep their values bit for bit
    assert list(off) == [k for k in on if k in off]
    assert repr([off[k] for k in off]) == repr([on[k] for k in off])
    new = {k: v for k, v in on.items() if k not in off}
    want = metrics.change_metrics_from_stats(st.change["stats"].numpy(), DEFAULT, sweep.slots(), kinds, levels, C)
    assert new == want
    names = ["fog_s1", "fog_s2", "fog", "night_s1", "night_s2", "night"]
    expect = {f"change_edge_{k}" for k in range(4)}
    expect |= {f"change_fraction_{n}_chg{k}" for n in names for k in range(5)} | {f"mean_change_fraction_chg{k}" for k in range(5)}
    assert expect <= set(new) and not any("clean" in k for k in new)
    assert all(k.startswith(("change_", "mean_")) or "_chg" in k for k in new)
    # fog adds 6 / 12 grey levels to every pixel; the identical night_s1 is all stratum 0; night_s2 changes the 3 x 5 patch by 50
    assert new["change_fraction_fog_s1_chg2"] == 1.0 and new["change_fraction_fog_s2_chg2"] == 1.0
    assert new["change_fraction_night_s1_chg0"] == 1.0 and new["consistency_night_s1_chg0"] == 1.0
    assert new["change_fraction_night_s2_chg3"] == 15 / 54 and new["change_fraction_night_s2_chg0"] == 39 / 54
    assert "miou_fog_chg2" in new and "consistency_night_chg3" in new and "accuracy_night_s2_chg0" in new
    # the counters, summed over the strata, are the consistency counters the sweep already keeps
    c2 = C * C
    assert torch.equal(st.change["stats"][..., c2:c2 + 4].sum(1), st.paired["stats"][:, c2:])
    assert st.change["rows"].shape[1] == 3 * 6 * 9 and st.change["rows"].shape[0] == st.paired["rows"].shape[0]
    assert "## Change Strata" in report.report_markdown(on) and "## Change Strata" not in report.report_markdown(off)


def test_harness_refuses_frames_that_are_not_float32_rgb(monkeypatch):
    ops, harness, metrics, report = _pkg()
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import resolve_severities
    _patch_native(monkeypatch, ops, 5, [])
    sweep = resolve_severities([0.5], ["clean", "fog"])
    m = metrics.RobustnessMetrics(5, ["clean", "fog"])
    st = harness.EvalState(m, ["clean", "fog"], "cpu", 15, False, sweep=sweep, change=[1.5])
    b = _sweep_batches(1, 2, 4, 4, 5, ("fog",), 1)[0]
    with pytest.raises(ValueError, match="float32"):
        harness.eval_batch(TinyModel(5), st, b["image"].double(), b["label"], b["weather_condition"], m, with_stats=False,
                           sources=b["source"], severity=0)
