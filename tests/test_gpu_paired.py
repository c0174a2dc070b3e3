"""-m gpu: the paired severity sweep.  awseg_combine_confusion_stats_pred against the two calls it fuses,
awseg_prediction_consistency against the numpy counts of tests/paired_ref.py, and the harness end to end: paired loader, clean
maps kept on the device, consistency counters, the single all-reduce and the result keys."""
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import paired_ref as PR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import loader
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    return SimpleNamespace(pkg=pkg, ops=ops, loader=loader, harness=harness, metrics=metrics, EnsembleModel=pkg.EnsembleModel,
                           RobustnessMetrics=pkg.RobustnessMetrics)


# ----------------------------------------------------------------------------- the one-pass statistics with the prediction map
def _members(seed, b, h, w, ldt):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s1 = torch.randn(b, 19, h, w, device="cuda", generator=g)
    s2 = torch.randn(b, 19, h, w, device="cuda", generator=g)
    s1[0, 3, 0, :5] = float("nan")                                   # NaN wins torch's argmax
    s2[1, :, 1, :8] = 0.5                                            # exact ties: the first class wins
    s1[1, :, 1, :8] = 0.5
    y = torch.randint(0, 19, (b, h, w), device="cuda", generator=g)
    y[:, 2, :16] = 255
    y[:, 3, :4] = 19                                                 # out of range: counted in oob, map still written
    return s1, s2, y.to(ldt).contiguous()


@pytest.mark.parametrize("ldt", [torch.uint8, torch.int64], ids=["u8 labels", "i64 labels"])
@pytest.mark.parametrize("with_t", [False, True], ids=["no T", "T"])
@pytest.mark.parametrize("mode", [0, 2], ids=["weighted", "mean"])
def test_stats_pred_map_and_counts_equal_the_unfused_calls(P, mode, with_t, ldt):
    ops = P.ops
    b, h, w = 2, 32, 64
    s1, s2, y = _members(5, b, h, w, ldt)
    wts = torch.softmax(torch.tensor([0.3, 0.7]), 0).cuda() if mode == 0 else None
    T = torch.tensor([1.7], device="cuda") if with_t else None
    cond = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    edges = torch.linspace(0, 1, 16).cuda()

    def run(pred_out):
        cnt, oob = ops.new_counts(19, "cuda", 4), torch.zeros(1, dtype=torch.int64, device="cuda")
        bins, hist = ops.new_ece_bins(15, "cuda", 4), torch.zeros(2, 1024, dtype=torch.int64, device="cuda")
        ops.combine_confusion_stats(s1, s2, mode, wts, T, y, cond, cnt, oob, edges, bins, hist, 0.0, 0.7, pred_out=pred_out)
        return cnt, oob, bins, hist

    pmap = torch.full((b, h, w), 77, dtype=torch.uint8, device="cuda")
    got = run(pmap)
    ref = run(None)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)                                     # confusion, oob, ECE bins, AUROC histogram bit-identical
    if ldt == torch.int64:                                           # (uint8 labels wrap 19 * 19 into range, as the reference does)
        assert int(got[1].item()) == b * 4                           # the label-19 pixels
    _, pred = ops.combine_argmax_confusion(s1, s2, mode, wts, T, want_logits=False, want_pred=True, pred_dtype=torch.uint8)
    assert torch.equal(pmap, pred)                                   # every pixel, labelled 255 / out of range included
    assert int(pmap[0, 0, 0]) == 3 and int(pmap[1, 1, 0]) == 0


# ----------------------------------------------------------------------------- awseg_prediction_consistency
CONS_CASES = [("C=19 hw%16==0 (16-byte loads) u8", 19, 32, 64, torch.uint8), ("C=19 hw%16==0 i64", 19, 32, 64, torch.int64),
              ("C=7 ragged 31x53 (byte loads) u8", 7, 31, 53, torch.uint8), ("C=7 ragged 31x53 i64", 7, 31, 53, torch.int64)]


def _maps(seed, b, c, h, w, ldt, coherent=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ref = torch.randint(0, c, (b, h, w), device="cuda", generator=g)
    if coherent:                                                     # blocks of one class, the variant flips some blocks
        ref = ref[:, ::8, ::8].repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :h, :w]
    var = torch.where(torch.rand(b, h, w, device="cuda", generator=g) < 0.3, torch.randint(0, c, (b, h, w), device="cuda", generator=g), ref)
    y = torch.randint(0, c, (b, h, w), device="cuda", generator=g)
    y = torch.where(torch.rand(b, h, w, device="cuda", generator=g) < 0.5, ref, y)
    y[:, 0, :7] = 255
    y[:, 1, :3] = c + 2                                              # outside [0, C): not a labelled pixel
    return ref.to(torch.uint8).contiguous(), var.to(torch.uint8).contiguous(), y.to(ldt).contiguous()


@pytest.mark.parametrize("case,c,h,w,ldt", CONS_CASES, ids=[x[0] for x in CONS_CASES])
@pytest.mark.parametrize("coherent", [True, False], ids=["coherent", "random"])
def test_consistency_counts_equal_numpy(P, case, c, h, w, ldt, coherent):
    ops = P.ops
    b = 4
    ref, var, y = _maps(11, b, c, h, w, ldt, coherent)
    var[2, 5, 9] = c                                                 # injected map values >= C go to oob, nowhere else
    ref[3, 6, 1] = 250
    rows = torch.flip(ref, [0]).contiguous()                         # frame b compares with row b' of the buffer
    fr = [3, -1, 1, 0]                                               # frame 1 skipped
    frame_ref = torch.tensor(fr, dtype=torch.int32, device="cuda")
    cond = torch.tensor([0, 0, 2, 1], dtype=torch.int32, device="cuda")
    st, oob = ops.new_consistency_stats(c, "cuda", 4), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.prediction_consistency(var, rows, frame_ref, y, c, st, oob, cond)
    rn = rows.cpu().numpy()
    refs = [rn[r] if r >= 0 else None for r in fr]
    want, want_oob = PR.consistency_stats(var.cpu().numpy(), refs, y.cpu().numpy(), c, cond=[0, 0, 2, 1], n_slots=4, skip={1})
    assert want_oob == 2 and int(oob.item()) == want_oob
    assert np.array_equal(st.cpu().numpy(), want), case
    # additive: two launches over a split batch equal one; permuting the frames changes nothing
    st2, oob2 = ops.new_consistency_stats(c, "cuda", 4), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.prediction_consistency(var[:2], rows, frame_ref[:2], y[:2], c, st2, oob2, cond[:2])
    ops.prediction_consistency(var[2:], rows, frame_ref[2:], y[2:], c, st2, oob2, cond[2:])
    assert torch.equal(st2, st) and torch.equal(oob2, oob)
    perm = torch.tensor([2, 0, 3, 1], device="cuda")
    st3, oob3 = ops.new_consistency_stats(c, "cuda", 4), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.prediction_consistency(var[perm].contiguous(), rows, frame_ref[perm].contiguous(), y[perm].contiguous(), c, st3, oob3,
                               cond[perm].contiguous())
    assert torch.equal(st3, st) and torch.equal(oob3, oob)


def test_consistency_row_outside_the_buffer_is_counted_not_read(P):
    ops = P.ops
    ref, var, y = _maps(3, 2, 19, 32, 64, torch.uint8)
    st, oob = ops.new_consistency_stats(19, "cuda", 1), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.prediction_consistency(var, ref, torch.tensor([0, 2], dtype=torch.int32, device="cuda"), y, 19, st, oob)
    want, _ = PR.consistency_stats(var[:1].cpu().numpy(), ref[:1].cpu().numpy(), y[:1].cpu().numpy(), 19)
    assert np.array_equal(st.cpu().numpy(), want) and int(oob.item()) == 32 * 64


# ----------------------------------------------------------------------------- the harness end to end
def _model(strategy="weighted_average", include_depth=False):
    from tests.test_gpu_models import calibrate_bn
    torch.manual_seed(2)
    return calibrate_bn(_pkg().EnsembleModel(num_classes=19, include_depth=include_depth, pretrained=False,
                                             ensemble_strategy=strategy)).cuda().eval()


def _pkg():
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    return pkg


def _dataset(P, n=4, hw=(256, 512), kinds=("fog", "night"), sev=(0.3, 0.8), schedule="paired"):
    extra = {"weather_schedule": schedule, "severities": list(sev)} if schedule == "paired" else {"weather_schedule": schedule}
    return P.loader.CityscapesKITTIDataset(split="test", image_size=hw, weather_conditions=["clean", *kinds], include_depth=False,
                                           device="cuda", num_samples=n, **extra)


def _sweep_run(P, model, ds, B=2, grid=None):
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    st = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, True, temperature_grid=grid, sweep=ds.sweep)
    for batch in ds.batches(B):
        P.harness.eval_batch(model, st, batch["image"], batch["label"], batch["weather_condition"], metrics,
                             sources=batch["source"], severity=batch["severity"])
    return st, P.harness.finalize(st, metrics)


@pytest.mark.parametrize("strategy", ["weighted_average", "max_confidence"], ids=["one-pass path", "max_confidence fallback"])
def test_harness_sweep_equals_direct_recount(P, strategy):
    ops = P.ops
    model = _model(strategy)
    ds = _dataset(P)
    st, res = _sweep_run(P, model, ds)
    slots = ds.sweep.slots()
    assert slots == ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2"]
    conf = np.zeros((1 + len(slots), 19 * 19), np.int64)
    cons = np.zeros((1 + len(slots), 19 * 19 + 4), np.int64)
    clean = {}
    with torch.no_grad():
        for batch in ds.batches(2):
            name = P.loader.slot_name(batch["weather_condition"][0], batch["severity"])
            res_b = model.forward_eval(batch["image"], want_logits=True, want_pred=False)     # materialised ensemble logits
            _, pred = ops.combine_argmax_confusion(res_b["segmentation"], None, 3, want_logits=False, want_pred=True,
                                                   pred_dtype=torch.uint8)
            pn, yn = pred.cpu().numpy(), batch["label"].cpu().numpy()
            k = 1 + slots.index(name)
            for i, s in enumerate(batch["source"]):
                c = PR.confusion(pn[i], yn[i], 19)
                conf[0] += c
                conf[k] += c
                if batch["severity"] == 0:
                    clean[s] = pn[i]
                else:
                    row, bad = PR.consistency_counts(pn[i], clean[s], yn[i], 19)
                    assert bad == 0
                    cons[0] += row
                    cons[k] += row
    assert np.array_equal(st.acc.counts.cpu().numpy(), conf)
    assert np.array_equal(st.paired["stats"].cpu().numpy(), cons)
    assert res["paired_sources"] == 4.0 and res["severity_levels"] == 2.0
    iou = P.metrics.iou_from_counts
    for j, name in enumerate(slots):
        assert res[f"miou_{name}"] == iou(torch.from_numpy(conf[1 + j]), 19)["mean_iou"], name
        if name == "clean":
            continue
        A, T = cons[1 + j, :361].reshape(19, 19), cons[1 + j, 361:]
        assert res[f"consistency_{name}"] == float(np.trace(A)) / A.sum()
        assert res[f"consistency_miou_{name}"] == iou(torch.from_numpy(A.reshape(-1).copy()), 19)["mean_iou"]
        assert res[f"corruption_error_rate_{name}"] == (T[1] / (T[0] + T[1]) if T[0] + T[1] else 0.0)
        assert res[f"robustness_degradation_{name}"] == max(0.0, (res["miou_clean"] - res[f"miou_{name}"]) / res["miou_clean"])
        assert isinstance(res[f"ece_{name}"], float)
    for kind in ("fog", "night"):
        idx = [1 + slots.index(f"{kind}_s{j}") for j in (1, 2)]
        assert res[f"miou_{kind}"] == iou(torch.from_numpy(conf[idx].sum(0)), 19)["mean_iou"]
        A = cons[idx, :361].sum(0)
        assert res[f"consistency_{kind}"] == float(A.reshape(19, 19).trace()) / A.sum()
        assert res[f"severity_intensity_{kind}_s2"] == 0.8
    assert res["mean_consistency"] == float(cons[0, :361].reshape(19, 19).trace()) / cons[0, :361].sum()
    # the clean slot equals today's path over the same clean frames; with the sweep off no new key appears
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    base = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, True)
    for item in ds.plan(2):
        if item.level == 0:
            b = ds.make_paired_batch(ds.synth_raw(item.start, item.n), item)
            P.harness.eval_batch(model, base, b["image"], b["label"], ["clean"] * item.n, metrics)
    off = P.harness.finalize(base, metrics)
    assert off["miou_clean"] == res["miou_clean"] and off["ece_clean"] == res["ece_clean"]
    new = ("paired_", "severity_", "consistency", "corruption_error", "mean_consistency", "mean_corruption")
    assert not any(k.startswith(new) or "_s1" in k for k in off)


def test_sweep_order_errors(P):
    model = _model()
    ds = _dataset(P, n=2)
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    items = ds.plan(2)
    raw = ds.synth_raw(0, 2)
    batches = [ds.make_paired_batch(raw, it) for it in items]

    def state():
        return P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, True, sweep=ds.sweep)

    def feed(st, b):
        P.harness.eval_batch(model, st, b["image"], b["label"], b["weather_condition"], metrics, sources=b["source"], severity=b["severity"])
    st = state()
    with pytest.raises(ValueError, match="before its clean frame"):
        feed(st, batches[1])
    st = state()
    feed(st, batches[0])
    with pytest.raises(ValueError, match="came twice"):
        feed(st, batches[0])
    st = state()
    for b in batches[:-1]:
        feed(st, b)
    with pytest.raises(ValueError, match="incomplete"):
        P.harness.finalize(st, metrics)


def test_temperature_grid_composes_with_the_sweep(P):
    grid = np.array([0.5, 1.0, 2.0], np.float32)
    model = _model()
    ds = _dataset(P)
    _, res = _sweep_run(P, model, ds, grid=grid)
    for k in ("ece_calibrated_fog_s1", "ece_calibrated_night_s2", "calibration_temperature_clean"):
        assert isinstance(res[k], float), k
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    base = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, True, temperature_grid=grid)
    for item in ds.plan(2):
        if item.level == 0:
            b = ds.make_paired_batch(ds.synth_raw(item.start, item.n), item)
            P.harness.eval_batch(model, base, b["image"], b["label"], ["clean"] * item.n, metrics)
    off = P.harness.finalize(base, metrics)
    for k in ("calibration_temperature", "calibration_temperature_clean", "nll_calibrated_clean", "ece_calibrated_clean"):
        assert off[k] == res[k], k


def _options_run(P, model, ds, ensemble, options):
    """eval_batch over ds with EvalState(**options) -> (state, results)."""
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    sweep = getattr(ds, "sweep", None)
    st = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, ensemble, sweep=sweep, **options)
    for batch in ds.batches(2):
        extra = {"severity": batch["severity"]} if sweep is not None else {}
        if "depth" in options:
            extra["depth"] = batch["depth"]
        P.harness.eval_batch(model, st, batch["image"], batch["label"], batch["weather_condition"], metrics, sources=batch["source"],
                             **extra)
    return st, P.harness.finalize(st, metrics)


@pytest.mark.parametrize("sweep", [True, False], ids=["ensemble, sweep, every option", "single model, no sweep, the three map readers"])
def test_every_option_in_one_state_equals_each_option_alone(P, sweep):
    """The options share the batch's prediction map, the clean-row stores and the row indices: with all of them on, every result
    key and every counter is what the option gives alone.  The counters are exact integers and the forward pass is a pure function
    of the frame (test_eval_forward_is_a_pure_function_of_the_frame), so the comparison is exact."""
    if sweep:
        sev = [0.3, 0.8]
        model = _model(include_depth=True)                           # (the depth metrics need the depth heads)
        ds = P.loader.CityscapesKITTIDataset(split="test", image_size=(64, 128), weather_conditions=["clean", "fog", "night"],
                                             include_depth=True, device="cuda", num_samples=4, weather_schedule="paired", severities=sev)
        cfg = {"data.weather_conditions": list(ds.weather_conditions), "evaluation.severities": sev, "evaluation.change_strata": "default",
               "evaluation.ensemble_weight_grid": 3}
        options = {"temperature_grid": np.array([0.5, 1.0, 2.0], np.float32), "depth": {"min": 1e-3, "target": "clean"}, "failure": True,
                   "boundary": [1, 2], "bootstrap": {"replicates": 16, "confidence": 0.95, "seed": 0, "sources": len(ds)},
                   "change": P.harness.change_option(cfg), "quality": {"targets": [0.9, 0.75, 0.5]},
                   "segments": {"threshold": 0.5, "min_area": 16}, "weight_grid": P.harness.weight_grid_option(cfg, model)}
    else:
        from tests.test_gpu_strata import _single_model
        model = _single_model(P)
        ds = _dataset(P, n=4, hw=(64, 128), kinds=("fog",), schedule="round_robin")
        options = {"boundary": [1, 2], "bootstrap": {"replicates": 16, "confidence": 0.95, "seed": 0, "sources": len(ds)},
                   "segments": {"threshold": 0.5, "min_area": 16}}
    st_all, all_on = _options_run(P, model, ds, sweep, options)
    for name, value in options.items():
        st, single = _options_run(P, model, ds, sweep, {name: value})
        assert set(single) <= set(all_on), name
        for k, v in single.items():
            assert repr(all_on[k]) == repr(v), (name, k)
        attr = "calib" if name == "temperature_grid" else name
        for t in (("table", "seen", "slot") if name == "bootstrap" else ("stats",)):
            assert torch.equal(getattr(st_all, attr)[t], getattr(st, attr)[t]), (name, t)
        assert torch.equal(st_all.acc.counts, st.acc.counts) and torch.equal(st_all.ece, st.ece), name
        if sweep:
            assert torch.equal(st_all.paired["stats"], st.paired["stats"]), name


def test_variant_distance_grows_with_severity(P):
    ds = _dataset(P, n=2, sev=(0.2, 0.5, 0.8))
    clean, dist = {}, {}
    for b in ds.batches(2):
        for i, s in enumerate(b["source"]):
            if b["severity"] == 0:
                clean[s] = b["image"][i].clone()
            else:
                dist.setdefault((b["weather_condition"][0], s), []).append((b["image"][i] - clean[s]).abs().mean().item())
    assert set(k for k, _ in dist) == {"fog", "night"}
    for key, d in dist.items():
        assert len(d) == 3 and d[0] < d[1] < d[2], (key, d)


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
ds = CityscapesKITTIDataset(split="test", image_size=(128, 256), weather_conditions=conds, include_depth=False, device="cuda",
                            num_samples=4, weather_schedule="paired", severities=[0.3, 0.8])
loader = create_dataloader(ds, batch_size=2, shuffle=False, rank=rank, world_size=world)
assert len(loader) == len(list(ds.plan(2, False, rank, world)))
res = evaluate_model(model, loader, RobustnessMetrics(19, conds), "cuda", {"data.weather_conditions": conds, "evaluation.severities": [0.3, 0.8]})
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
    assert a["paired_sources"] == 4.0 and "consistency_fog_s2" in a
    assert a == b


def test_fullsize_group_reference_preset(P):
    """One group of 8 sources at 1024 x 2048 under the 'reference' preset: 1 clean + 4 kinds x 3 levels = 13 batches."""
    model = _model()
    conds = ["clean", "fog", "rain", "snow", "night"]
    ds = P.loader.CityscapesKITTIDataset(split="test", image_size=(1024, 2048), weather_conditions=conds, include_depth=False,
                                         device="cuda", num_samples=8, weather_schedule="paired", severities="reference")
    metrics = P.RobustnessMetrics(19, conds)
    st = P.harness.EvalState(metrics, conds, "cuda", 15, True, sweep=ds.sweep)
    n = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for batch in ds.batches(8):
        P.harness.eval_batch(model, st, batch["image"], batch["label"], batch["weather_condition"], metrics,
                             sources=batch["source"], severity=batch["severity"])
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = P.harness.finalize(st, metrics)
    px = 1024 * 2048
    cons = st.paired["stats"].cpu().numpy()
    assert n == 13 and res["paired_sources"] == 8.0 and res["severity_levels"] == 3.0
    assert int(cons[0, :361].sum()) == 12 * 8 * px
    assert all(int(cons[1 + k, :361].sum()) == 8 * px for k in range(1, 13))
    assert int(cons[0, 361:].sum()) == 12 * 8 * px                    # every synthetic label is in [0, 19)
    counts = st.acc.counts.cpu().numpy()
    assert int(counts[0].sum()) == 13 * 8 * px and all(int(counts[1 + k].sum()) == 8 * px for k in range(13))
    print(f"reference-preset sweep, 8 sources at 1024x2048: {dt:.2f} s for 13 batches = {dt / 8:.3f} s per source frame")
