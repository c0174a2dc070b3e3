"""awseg_image_quality on the device against the float32 numpy model of tests/quality_ref.py (exact: every term is a float32 value
numpy reproduces bit for bit, every counter an integer sum), and the harness option evaluation.image_quality end to end.

csrc/quality.hip: a block owns IQ_TILE_H x IQ_TILE_W window centres, so a frame of (IQ_TILE_H + 10) x (IQ_TILE_W + 10) pixels is
exactly one tile; one row or column more opens a second tile, whose last tile also owns the error terms of the apron.  16-byte loads
need W % 4 == 0 and 16-byte aligned bases."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import quality_ref as QR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import loader
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    return SimpleNamespace(ops=ops, N=native, loader=loader, harness=harness, metrics=metrics, RobustnessMetrics=pkg.RobustnessMetrics,
                           pkg=pkg)


def _dev(a, offset=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if offset:                                                        # the same data one element behind a 16-byte boundary
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:].copy_(t.reshape(-1))
        t = buf[1:].view(t.shape)
        assert t.data_ptr() % 16 == 4
    return t


def _run(P, var, clean, fr, mean, std, cond=None, n_slots=1, offset=False, stats=None, oob=None, **kw):
    stats = P.ops.new_image_quality_stats("cuda", n_slots) if stats is None else stats
    oob = torch.zeros(1, dtype=torch.int64, device="cuda") if oob is None else oob
    P.ops.image_quality(_dev(var, offset), _dev(clean, offset), _dev(np.asarray(fr, np.int32)), stats,
                        cond=None if cond is None else _dev(np.asarray(cond, np.int32)), oob=oob, mean=mean, std=std, **kw)
    return stats.cpu().numpy(), int(oob.item())


TH, TW = 32, 64                                                       # asserted against ops.IQ_TILE_H / IQ_TILE_W below
SHAPES = [(2, 3, 11, 11), (1, 3, 10, 40), (3, 3, 31, 53), (2, 3, 67, 131),
          (1, 3, TH + 9, TW + 9), (1, 3, TH + 10, TW + 10), (1, 3, TH + 11, TW + 11),      # tile - 1, tile, tile + 1 window centres
          (2, 3, TH + 11, 2 * TW + 12),                               # W % 4 == 0 across three tile columns and two tile rows
          (3, 1, 31, 53), (3, 4, 31, 53), (2, 1, TH + 11, TW + 12), (2, 4, TH + 11, TW + 12)]


def test_tile_constants_mirror_the_header(P):
    text = (ROOT / "include" / "awseg.h").read_text()
    import re
    get = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, text).group(1))   # noqa: E731
    assert (P.ops.IQ_TILE_H, P.ops.IQ_TILE_W, P.ops.IQ_ROW) == (get("AWSEG_IQ_TILE_H"), get("AWSEG_IQ_TILE_W"), get("AWSEG_IQ_ROW"))
    assert (TH, TW) == (P.ops.IQ_TILE_H, P.ops.IQ_TILE_W) and QR.IQ_ROW == P.ops.IQ_ROW
    assert np.array_equal(P.ops.ssim_taps(), QR.taps11())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("maker", [QR.rendered_frames, QR.random_frames], ids=["rendered", "random"])
def test_counters_equal_the_float32_model(P, shape, maker):
    b, ch, h, w = shape
    var, clean, fr, mean, std = maker(11 + h + w + ch, b, ch, h, w)
    cond = [i % 3 for i in range(b)]
    want, bad = QR.counters(var, clean, fr, mean, std, cond=cond, n_slots=4)
    got, oob = _run(P, var, clean, fr, mean, std, cond=cond, n_slots=4)
    assert bad == oob == 0
    assert want[0, QR.FRAMES] == b and want[0, QR.N_ERR] + want[0, QR.BAD_ERR] == b * ch * h * w
    assert want[0, QR.N_WIN] + want[0, QR.BAD_WIN] == b * ch * max(h - 10, 0) * max(w - 10, 0)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("shape", [(1, 3, 10, 40), (2, 3, TH + 11, 2 * TW + 12)], ids=lambda s: "x".join(map(str, s)))
def test_a_base_pointer_off_16_byte_alignment_takes_the_scalar_path(P, shape):
    b, ch, h, w = shape
    assert w % 4 == 0
    var, clean, fr, mean, std = QR.rendered_frames(5, b, ch, h, w)
    want, _ = QR.counters(var, clean, fr, mean, std)
    assert np.array_equal(_run(P, var, clean, fr, mean, std, offset=True)[0], want)
    assert np.array_equal(_run(P, var, clean, fr, mean, std)[0], want)


def test_planted_values_land_in_the_unmeasured_counters(P):
    b, ch, h, w = 2, 3, 40, 48
    var, clean, fr, _, _ = QR.random_frames(3, b, ch, h, w)
    mean, std = np.zeros(3, np.float32), np.ones(3, np.float32)       # d is the plain difference
    fr[:] = [0, 1]
    var[0, 0, 3, 3], var[0, 1, 20, 30], var[0, 2, 39, 47] = np.nan, np.inf, -np.inf
    clean[0, 0, 12, 12], clean[0, 1, 5, 40] = np.nan, np.inf
    var[0, 1, 5, 40] = np.inf                                         # inf - inf
    var[1, 0, 30, 7], clean[1, 0, 30, 7] = 2.0, 0.0                   # |d| exactly 2: measured
    var[1, 0, 30, 8], clean[1, 0, 30, 8] = np.nextafter(np.float32(2.0), np.float32(3.0)), 0.0    # just above: not
    var[1, 1, 0, 0], clean[1, 1, 0, 0] = -1.0, 1.0
    want, _ = QR.counters(var, clean, fr, mean, std)
    one = QR.frame_terms(var[1, :1, 30:31, 7:9], clean[1, :1, 30:31, 7:9], mean, std, QR.taps11(), QR.C1, QR.C2)
    assert one[QR.N_ERR] == 1 and one[QR.BAD_ERR] == 1 and one[QR.SUM_ABS] == 2 << 24 and one[QR.SUM_SQ] == 4 << 24
    assert want[0, QR.BAD_ERR] >= 6 and want[0, QR.BAD_WIN] >= 250
    got, _ = _run(P, var, clean, fr, mean, std)
    assert np.array_equal(got, want), (got, want)


def test_a_twin_outside_the_unit_range_drives_a_denominator_to_zero(P):
    """Constant frames far outside [0, 1]: float32 cancellation makes the window variance mxx - mx * mx a non-zero constant; with
    c2 = -(vx + vy) the contrast denominator is exactly 0 in every window of the frame (0 / 0: unmeasured)."""
    taps, h, w = QR.taps11(), 13, 14
    f = lambda v: float(QR._filter(QR._filter(np.full((11, 11), v, np.float32), taps, 1), taps, 0)[0, 0])   # noqa: E731
    found = None
    for a in np.arange(100.25, 140.0, 0.37, dtype=np.float32):
        mx, mxx = np.float32(f(a)), np.float32(f(np.float32(a * a)))
        vx = np.float32(mxx - mx * mx)
        if vx < 0:
            found = (np.float32(a), np.float32(-(vx + vx)))
            break
    assert found is not None
    a, c2 = found
    mean, std = np.zeros(1, np.float32), np.ones(1, np.float32)
    var = np.stack([np.full((1, h, w), a, np.float32), QR.random_frames(1, 1, 1, h, w)[0][0]])
    clean = var.copy()
    want, _ = QR.counters(var, clean, [0, 1], mean, std, c2=float(c2))
    assert want[0, QR.BAD_WIN] == 3 * 4 and want[0, QR.N_WIN] == 3 * 4      # every window of the constant frame, none of the other
    got, _ = _run(P, var, clean, [0, 1], mean, std, c2=float(c2))
    assert np.array_equal(got, want), (got, want)


def test_frame_routing_additivity_and_streams(P):
    b, ch, h, w = 5, 3, 23, 36
    var, clean, _, mean, std = QR.rendered_frames(9, b, ch, h, w, refs=2)
    fr = [1, -1, 2, 0, 7]                                             # -1: skipped; 2, 7: outside the two twins
    cond = [0, 1, 2, 5, -3]                                           # 5 and -3: slot 0 only (frame 3); frames 2, 4 are not counted
    want, bad = QR.counters(var, clean, fr, mean, std, cond=cond, n_slots=4)
    assert bad == 2 * h * w and want[0, QR.FRAMES] == 2 and want[1, QR.FRAMES] == 1 and not want[2:].any()
    got, oob = _run(P, var, clean, fr, mean, std, cond=cond, n_slots=4)
    assert oob == bad and np.array_equal(got, want)
    none, _ = _run(P, var, clean, fr, mean, std, cond=None, n_slots=4)                      # NULL cond: slot 0 only
    assert np.array_equal(none[0], want[0]) and not none[1:].any()
    # two launches add up; a batch split equals one batch; a side stream
    stats, o = P.ops.new_image_quality_stats("cuda", 4), torch.zeros(1, dtype=torch.int64, device="cuda")
    _run(P, var, clean, fr, mean, std, cond=cond, n_slots=4, stats=stats, oob=o)
    twice, oob2 = _run(P, var, clean, fr, mean, std, cond=cond, n_slots=4, stats=stats, oob=o)
    assert oob2 == 2 * bad and np.array_equal(twice, 2 * want)
    stats, o = P.ops.new_image_quality_stats("cuda", 4), torch.zeros(1, dtype=torch.int64, device="cuda")
    _run(P, var[:2], clean, fr[:2], mean, std, cond=cond[:2], n_slots=4, stats=stats, oob=o)
    split, oob3 = _run(P, var[2:], clean, fr[2:], mean, std, cond=cond[2:], n_slots=4, stats=stats, oob=o)
    assert oob3 == bad and np.array_equal(split, want)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got_side, oob4 = _run(P, var, clean, fr, mean, std, cond=cond, n_slots=4)
    side.synchronize()
    assert oob4 == bad and np.array_equal(got_side, want)


def test_refusals_of_the_abi_and_of_ops(P):
    N, ops = P.N, P.ops
    b, ch, h, w = 2, 3, 12, 16
    var, clean, fr, mean, std = QR.rendered_frames(2, b, ch, h, w)
    img, ref, frt = _dev(var), _dev(clean), _dev(fr)
    stats, oob = ops.new_image_quality_stats("cuda", 2), torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    taps = ops.ssim_taps()

    def call(**kw):
        a = dict(image=N.ptr(img), ref=N.ptr(ref), n_refs=3, batch=b, ch=ch, h=h, w=w, fr=N.ptr(frt), mean=mean.copy(), std=std.copy(),
                 taps=taps.copy(), c1=1e-4, c2=9e-4, cond=None, stats=N.ptr(stats), n_slots=2, oob=N.ptr(oob), ws=N.ptr(ws))
        a.update(kw)
        host = lambda v: None if v is None else N.host(v)             # noqa: E731
        N.call("awseg_image_quality", a["image"], a["ref"], a["n_refs"], a["batch"], a["ch"], a["h"], a["w"], a["fr"], host(a["mean"]),
               host(a["std"]), host(a["taps"]), a["c1"], a["c2"], a["cond"], a["stats"], a["n_slots"], a["oob"], a["ws"], N.stream())

    def arr(base, i, v):
        out = base.copy()
        out[i] = v
        return out
    inval = [dict(image=None), dict(ref=None), dict(fr=None), dict(mean=None), dict(std=None), dict(taps=None), dict(stats=None),
             dict(oob=None), dict(ws=None), dict(n_refs=0), dict(batch=-1), dict(ch=0), dict(ch=5), dict(h=0), dict(w=0), dict(n_slots=0),
             dict(std=arr(std, 1, 0.0)), dict(std=arr(std, 0, -1.0)), dict(std=arr(std, 2, np.inf)), dict(std=arr(std, 2, np.nan)),
             dict(mean=arr(mean, 0, np.nan)), dict(mean=arr(mean, 1, -np.inf)), dict(taps=arr(taps, 10, np.nan)),
             dict(taps=arr(taps, 0, np.inf)), dict(c1=0.0), dict(c1=-1e-4), dict(c1=float("nan")), dict(c1=float("inf")),
             dict(c2=0.0), dict(c2=-9e-4), dict(c2=float("nan")), dict(c2=float("inf"))]
    for kw in inval:
        with pytest.raises(N.AwsegError, match="code -1"):
            call(**kw)
    for kw in (dict(batch=65536), dict(h=1 << 16, w=1 << 15), dict(h=1, w=1 << 31)):
        with pytest.raises(N.AwsegError, match="code -2"):
            call(**kw)
    call(batch=0)
    torch.cuda.synchronize()
    assert not stats.any() and not oob.any()                          # nothing was launched
    assert N.lib().awseg_image_quality_workspace(b, ch, h, w) == b * 1 * 1 * 10 * 8
    assert N.lib().awseg_image_quality_workspace(3, 3, TH + 11, 2 * TW + 11) == 3 * 2 * 3 * 10 * 8
    call()
    torch.cuda.synchronize()
    assert int(stats[0, 0]) == b and int(stats[0, 1]) == b * ch * h * w
    good = dict(image=img, ref_images=ref, frame_ref=frt, stats=stats, oob=oob)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    for kw in (dict(image=img.double()), dict(image=img[0]), dict(image=img[:, :0]), dict(image=torch.cat([img, img[:, :2]], 1)),
               dict(ref_images=ref.double()), dict(ref_images=ref[:0]), dict(ref_images=ref[:, :, :11].contiguous()),
               dict(ref_images=ref[:, :2].contiguous()), dict(ref_images=ref.reshape(3, ch, w, h)), dict(ref_images=ref.reshape(3, ch, -1)),
               dict(frame_ref=frt.long()), dict(frame_ref=i32(3)), dict(stats=stats.int()), dict(stats=stats[:, :9]), dict(stats=stats[0]),
               dict(oob=torch.zeros(2, dtype=torch.int64, device="cuda")), dict(oob=oob.int()), dict(cond=i32(3)), dict(cond=i32(2).long()),
               dict(mean=[0.5, 0.5]), dict(mean=[0.5] * 3), dict(std=[0.2] * 3), dict(mean=[0.5] * 3, std=[0.2, 0.0, 0.2]),
               dict(mean=[0.5, np.nan, 0.5], std=[0.2] * 3), dict(mean=[0.5] * 3, std=[0.2, np.inf, 0.2]), dict(c1=0.0), dict(c2=-1.0),
               dict(c1=float("nan")), dict(c2=float("inf")), dict(c1=1e-60), dict(c1="1e-4"), dict(taps=[0.1] * 10),
               dict(taps=[np.nan] + [0.1] * 10), dict(image=img[:, :1].contiguous(), ref_images=ref[:, :1].contiguous())):
        with pytest.raises(ValueError):
            ops.image_quality(**dict(good, **kw))
    with pytest.raises(N.AwsegError):
        ops.image_quality(img.cpu(), ref, frt, stats, oob=oob)
    torch.cuda.synchronize()
    assert int(stats[0, 0]) == b                                      # refused before any launch


# ----------------------------------------------------------------------------- the harness end to end
def _dataset(P, n=4, hw=(128, 256), kinds=("fog", "night"), sev=(0.3, 0.8)):
    return P.loader.CityscapesKITTIDataset(split="test", image_size=hw, weather_conditions=["clean", *kinds], include_depth=False,
                                           device="cuda", num_samples=n, weather_schedule="paired", severities=list(sev))


def _sweep_run(P, monkeypatch, model, ds, quality, ensemble, identical=None):
    """eval_batch over the paired batches.  identical = (kind, level): that variant is replaced by its clean frames.
    -> (state, results, what the entry point was handed in call order, the variant batches, the clean frames)."""
    seen = []
    real = P.ops.image_quality

    def spy(image, ref_images, frame_ref, stats, cond=None, oob=None, **k):
        seen.append(dict(image=image.cpu().numpy(), twins=ref_images[frame_ref.long()].cpu().numpy(), cond=cond.cpu().numpy(), kw=k))
        return real(image, ref_images, frame_ref, stats, cond=cond, oob=oob, **k)
    monkeypatch.setattr(P.ops, "image_quality", spy)
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    st = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, ensemble, sweep=ds.sweep, quality=quality)
    clean, order = {}, []
    for batch in ds.batches(2):
        image = batch["image"]
        if batch["severity"] == 0:
            clean.update({s: image[i].clone() for i, s in enumerate(batch["source"])})
        elif identical == (batch["weather_condition"][0], batch["severity"]):
            image = torch.stack([clean[s] for s in batch["source"]])
        if batch["severity"]:
            order.append((batch["weather_condition"][0], batch["severity"], list(batch["source"])))
        P.harness.eval_batch(model, st, image, batch["label"], batch["weather_condition"], metrics, sources=batch["source"],
                             severity=batch["severity"])
    res = P.harness.finalize(st, metrics)
    monkeypatch.undo()
    return st, res, seen, order, clean


@pytest.mark.parametrize("ensemble", [True, False], ids=["ensemble", "single model"])
def test_harness_counters_equal_the_model_on_the_kept_tensors(P, monkeypatch, ensemble):
    from tests.test_gpu_paired import _model
    from tests.test_gpu_strata import _single_model
    model = _model() if ensemble else _single_model(P)
    ds = _dataset(P, hw=(64, 128))
    slots = ds.sweep.slots()
    st_off, off, none, _, _ = _sweep_run(P, monkeypatch, model, ds, None, ensemble, identical=("night", 1))
    assert not none and st_off.quality is None and st_off.clean_frames is None      # off: nothing allocated, nothing called
    st, on, seen, order, clean = _sweep_run(P, monkeypatch, model, ds, {"targets": [0.9, 0.75, 0.5]}, ensemble, identical=("night", 1))
    assert len(seen) == len(order) == 8                               # 2 source groups x 2 kinds x 2 levels; no clean batch
    total = np.zeros((1 + len(slots), QR.IQ_ROW), np.int64)
    for call, (kind, level, sources) in zip(seen, order):
        b = len(sources)
        assert np.array_equal(call["twins"], torch.stack([clean[s] for s in sources]).cpu().numpy())
        slot = slots.index(f"{kind}_s{level}")
        assert call["cond"].tolist() == [slot] * b and not call["kw"]
        rows, bad = QR.counters(call["image"], call["twins"], np.arange(b), cond=call["cond"], n_slots=1 + len(slots))
        assert bad == 0
        if (kind, level) == ("night", 1):                            # the identical variant: no error, every window exactly 1
            assert rows[0, QR.SUM_SQ] == 0 and rows[0, QR.SUM_S] == rows[0, QR.N_WIN] << 24
        total += rows
    assert np.array_equal(st.quality["stats"].cpu().numpy(), total) and int(st.quality["oob"].item()) == 0
    assert st.quality["terms"] == 8 * 2 * 3 * 64 * 128 and not total[1 + slots.index("clean")].any()
    assert list(off) == [k for k in on if k in off]
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k
    new = {k: v for k, v in on.items() if k not in off}
    want = P.metrics.quality_metrics_from_stats(total, slots, ["fog", "night"], 2, off, [0.9, 0.75, 0.5],
                                                metrics_degradation(P))
    assert new == want and all(isinstance(v, float) for v in new.values())
    for n in ("fog_s1", "fog_s2", "fog", "night_s2", "night"):
        assert {f"mse_{n}", f"psnr_{n}", f"ssim_{n}", f"ssim_luminance_{n}", f"ssim_contrast_{n}", f"mean_abs_change_{n}"} <= set(new), n
    assert new["mse_night_s1"] == 0.0 and "psnr_night_s1" not in new and new["ssim_night_s1"] == 1.0
    assert new["ssim_not_monotonic_night"] == 1.0 and "miou_drop_per_ssim_night_s1" not in new
    assert "mean_ssim" in new and "mean_psnr" in new and not any(k.endswith("_clean") for k in new)
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    assert "## Image Quality" in report_markdown(on) and "## Image Quality" not in report_markdown(off)


def metrics_degradation(P):
    return P.RobustnessMetrics(19, ["clean", "fog", "night"]).compute_robustness_degradation_ratio


def test_harness_option_through_evaluate_model_and_its_refusals(P):
    from tests.test_gpu_paired import _model
    model = _model()
    ds = _dataset(P, hw=(64, 128))
    conds = list(ds.weather_conditions)
    loader = lambda: P.loader.create_dataloader(ds, batch_size=2, shuffle=False)      # noqa: E731
    cfg = {"data.weather_conditions": conds, "evaluation.severities": [0.3, 0.8]}
    off = P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda", cfg)
    on = P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda", dict(cfg, **{"evaluation.image_quality": True}))
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k
    assert "ssim_fog_s2" in on and "psnr_night_s1" in on and "mean_ssim" in on and not any(k.startswith(("ssim_", "psnr_")) for k in off)
    assert 0.0 < on["ssim_fog_s2"] < on["ssim_fog_s1"] < 1.0          # more fog, less structure
    both = P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda",
                                    dict(cfg, **{"evaluation.image_quality": True, "evaluation.change_strata": "default"}))
    for k, v in on.items():
        assert repr(both[k]) == repr(v), k                            # one buffer of clean frames serves both options
    with pytest.raises(ValueError, match="severity sweep"):
        P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda",
                                 {"data.weather_conditions": conds, "evaluation.image_quality": True})
    with pytest.raises(ValueError, match="image_quality_targets"):
        P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda", dict(cfg, **{"evaluation.image_quality_targets": [1.0]}))
    metrics = P.RobustnessMetrics(19, conds)
    st = P.harness.EvalState(metrics, conds, "cuda", 15, True, sweep=ds.sweep, quality={"targets": [0.5]})
    z = torch.zeros(1, 3, 12, 12, device="cuda")
    P.ops.image_quality(z, z, torch.ones(1, dtype=torch.int32, device="cuda"), st.quality["stats"], oob=st.quality["oob"])
    with pytest.raises(IndexError, match="image-quality"):
        P.harness.finalize(st, metrics)
    st = P.harness.EvalState(metrics, conds, "cuda", 15, True, sweep=ds.sweep, quality={"targets": [0.5]})
    st.quality["terms"] = P.ops.IQ_TERM_BUDGET - 5
    with pytest.raises(OverflowError, match="image-quality"):
        st.update_quality(z, [0], None)


_WORKER = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1])
import torch
from adverse_weather_semantic_segmentation_robustness_benchmark_amd import parallel
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import CityscapesKITTIDataset, create_dataloader
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.harness import evaluate_model
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import RobustnessMetrics
import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
from tests.test_gpu_models import calibrate_bn
rank, local, world = parallel.init_from_env(backend="gloo")
torch.manual_seed(2)
model = calibrate_bn(pkg.EnsembleModel(num_classes=19, include_depth=False, pretrained=False)).cuda().eval()
conds = ["clean", "fog", "night"]
ds = CityscapesKITTIDataset(split="test", image_size=(64, 128), weather_conditions=conds, include_depth=False, device="cuda",
                            num_samples=4, weather_schedule="paired", severities=[0.3, 0.8])
loader = create_dataloader(ds, batch_size=2, shuffle=False, rank=rank, world_size=world)
res = evaluate_model(model, loader, RobustnessMetrics(19, conds), "cuda",
                     {"data.weather_conditions": conds, "evaluation.severities": [0.3, 0.8], "evaluation.image_quality": True})
if rank == 0:
    open(sys.argv[2], "w").write(json.dumps({k: float(v) for k, v in res.items()}))
'''


def test_two_ranks_over_gloo_equal_one_process(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    one = subprocess.run([sys.executable, str(script), str(ROOT), str(tmp_path / "one.json")], env=base, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=300)
    assert one.returncode == 0, one.stdout.decode()[-2000:]
    procs = []
    for r in range(2):
        env = dict(base, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), str(ROOT), str(tmp_path / "two.json")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, out.decode()[-2000:]
    a, b = json.loads((tmp_path / "one.json").read_text()), json.loads((tmp_path / "two.json").read_text())
    for k in ("ssim_fog_s2", "psnr_night_s1", "mean_ssim", "ssim_luminance_night", "mse_fog"):
        assert k in a, k
    assert a == b


# ----------------------------------------------------------------------------- full size
def test_fullsize_frame_pair(P):
    h, w = 1024, 2048
    var, clean, fr, mean, std = QR.rendered_frames(4, 1, 3, h, w, refs=1)
    want, _ = QR.counters(var, clean, fr, mean, std, cond=[1], n_slots=3)
    got, oob = _run(P, var, clean, fr, mean, std, cond=[1], n_slots=3)
    assert oob == 0 and want[0, QR.N_ERR] == 3 * h * w and want[0, QR.N_WIN] == 3 * (h - 10) * (w - 10)
    assert np.array_equal(got, want), (got, want)
