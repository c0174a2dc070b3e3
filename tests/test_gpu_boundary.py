"""awseg_boundary_stats on the device against the numpy model of tests/boundary_ref.py (exact: every number is an integer count), and
the harness option evaluation.boundary_widths end to end.

The kernel works on 32 x 64 tiles (csrc/boundary.hip kTH x kTW) with a halo of the widest band; SEAM below is a frame of 4 x 4
tiles whose 13-pixel class blocks are aligned to no tile edge, so bands straddle every seam, and whose last tiles are ragged."""
import ctypes
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import boundary_ref as BR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WIDTH_SETS = [(1,), (16,), (1, 2, 4, 8), (3, 5)]
SEAM = (19, 100, 200, 13)


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import loader
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    return SimpleNamespace(ops=ops, N=native, loader=loader, harness=harness, metrics=metrics, EnsembleModel=pkg.EnsembleModel,
                           RobustnessMetrics=pkg.RobustnessMetrics, pkg=pkg)


def _maps(seed, b, c, h, w, ldt, block=8):
    """test_gpu_paired._maps for this entry point: frame 0 in blocks of one class with a prediction that flips pixels, the last frame
    independent noise; a row of 255, unlabelled values, and one prediction value of 200 on a labelled pixel."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.randint(0, c, (b, h, w), device="cuda", generator=g)
    coarse = y[:, ::block, ::block].repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :h, :w]
    y[:max(1, b - 1)] = coarse[:max(1, b - 1)]
    pred = torch.where(torch.rand(b, h, w, device="cuda", generator=g) < 0.1, torch.randint(0, c, (b, h, w), device="cuda", generator=g), y)
    if h > 2:
        y[:, 2, :] = 255
    y[:, 0, :3] = c + 2                                              # outside [0, C): not a labelled pixel
    if ldt == torch.int64:
        y[:, h - 1, :2] = c
        y[:, h - 1, w - 1] = -1
    y[0, h // 2, w // 2] = 0
    pred[0, h // 2, w // 2] = 200                                    # oob == 1, and no neighbour of anything
    return pred.to(torch.uint8).contiguous(), y.to(ldt).contiguous()


def run(P, pred, label, widths, c, cond=None, n_slots=1, stats=None, oob=None):
    stats = P.ops.new_boundary_stats(c, len(widths), "cuda", n_slots) if stats is None else stats
    oob = torch.zeros(1, dtype=torch.int64, device="cuda") if oob is None else oob
    ct = None if cond is None else torch.tensor(list(cond), dtype=torch.int32, device="cuda")
    P.ops.boundary_stats(pred, label, list(widths), c, stats, oob, ct)
    return stats, oob


def model(pred, label, widths, c, cond=None, n_slots=1):
    return BR.boundary_counters(pred.cpu().numpy(), label.cpu().numpy(), widths, c, cond=cond, n_slots=n_slots)


CASES = [("C=19 64x96 u8", 19, 64, 96, torch.uint8, 8), ("C=19 64x96 i64", 19, 64, 96, torch.int64, 8),
         ("C=7 ragged 31x53 u8", 7, 31, 53, torch.uint8, 8), ("C=7 ragged 31x53 i64", 7, 31, 53, torch.int64, 8),
         ("C=7 5x7 (smaller than the band)", 7, 5, 7, torch.uint8, 2), ("C=7 1x70 (one row)", 7, 1, 70, torch.uint8, 4),
         ("C=7 70x1 (one column)", 7, 70, 1, torch.int64, 4), ("C=19 100x200 (4 x 4 tiles, blocks of 13)",) + SEAM[:3] + (torch.uint8, SEAM[3]),
         ("C=32 40x70 i64", 32, 40, 70, torch.int64, 8)]


@pytest.mark.parametrize("case,c,h,w,ldt,block", CASES, ids=[x[0] for x in CASES])
@pytest.mark.parametrize("widths", WIDTH_SETS, ids=str)
def test_counters_equal_the_model(P, widths, case, c, h, w, ldt, block):
    pred, label = _maps(7, 2, c, h, w, ldt, block)
    stats, oob = run(P, pred, label, widths, c, cond=[1, 0], n_slots=3)
    want, want_oob = model(pred, label, widths, c, cond=[1, 0], n_slots=3)
    assert want_oob == 1 and int(oob.item()) == 1
    got = stats.cpu().numpy()
    assert got.shape == want.shape == (3, len(widths) + 1, c * c + 2 * c)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{case} widths {widths}: {len(bad)} counters differ, first (slot, ring, cell) {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert want[0, :-1].sum() > 0 or h * w < 4                       # the case has a band


def band_counts(P, label, widths, c=19, pred=None):
    """Cumulative label-band pixel counts per width, and the interior count, from the device counters (pred defaults to the label)."""
    label = torch.from_numpy(label).cuda()
    pred = label.clone() if pred is None else torch.from_numpy(pred).cuda()
    stats, oob = run(P, pred.to(torch.uint8), label, widths, c)
    dec = P.ops.boundary_stats_to_numpy(stats, c)
    ring = dec["conf"][0].sum(axis=(1, 2))
    return np.cumsum(ring[:-1]).tolist(), int(ring[-1]), dec, int(oob.item())


def test_planted_vertical_split(P):
    h, w, widths = 40, 150, (1, 2, 5, 16)
    for x0 in (1, 63, 64, 65, 149):                                  # at, before and behind a tile seam; next to either border
        label = np.zeros((1, h, w), dtype=np.uint8)
        label[..., x0:] = 3
        band, interior, dec, oob = band_counts(P, label, widths)
        want = [h * (min(w, x0 + d) - max(0, x0 - d)) for d in widths]
        assert band == want and interior == h * w - want[-1] and oob == 0, (x0, band, want)
        assert np.array_equal(dec["pr"], dec["inter"]) and np.array_equal(dec["conf"][0].sum(1), dec["pr"][0])   # pred == label


def test_planted_single_pixel(P):
    h, w, widths = 70, 130, (1, 3, 8)
    for y, x in ((0, 0), (31, 63), (32, 64), (69, 129), (40, 2)):
        label = np.zeros((1, h, w), dtype=np.int64)
        label[0, y, x] = 2
        band, interior, dec, oob = band_counts(P, label, widths)
        want = [(min(h, y + d + 1) - max(0, y - d)) * (min(w, x + d + 1) - max(0, x - d)) for d in widths]
        assert band == want and interior == h * w - want[-1], ((y, x), band, want)
        assert dec["conf"][0, 0, 2, 2] == 1 and dec["conf"][0, :, 2, 2].sum() == 1                      # the pixel itself: ring 0


def test_planted_ignore_stripe(P):
    h, w, x0, widths = 35, 140, 60, (1, 2, 4, 8)                      # stripe = columns [x0, x0 + t): across the seam at 64 for t > 4
    for t in (1, 3, 6):
        label = np.zeros((1, h, w), dtype=np.uint8)
        label[..., x0:x0 + t] = 255
        label[..., x0 + t:] = 4
        pred = np.where(label == 255, 9, label).astype(np.uint8)     # the prediction has a class under the stripe
        band, interior, dec, oob = band_counts(P, label, widths, pred=pred)
        want = [2 * h * max(0, d - t) for d in widths]
        assert band == want and band[-1] + interior == h * (w - t) and oob == 0, (t, band, want)
        # the prediction's band: the stripe's class is an ordinary neighbour there, one pixel away on both sides
        pr_band = np.cumsum(dec["pr"][0].sum(1)[:-1]).tolist()
        assert pr_band == [2 * h * d for d in widths]


def test_constant_frames_have_no_band_and_do_not_see_each_other(P):
    for h, w in ((6, 9), (64, 128), (33, 65)):
        label = torch.stack([torch.full((h, w), 2, dtype=torch.uint8), torch.full((h, w), 5, dtype=torch.uint8)]).cuda()
        stats, oob = run(P, label.clone(), label, (1, 4, 16), 7)
        dec = P.ops.boundary_stats_to_numpy(stats, 7)
        assert not stats[0, :3].any() and int(oob.item()) == 0
        assert dec["conf"][0, 3, 2, 2] == h * w and dec["conf"][0, 3, 5, 5] == h * w and dec["conf"][0, 3].sum() == 2 * h * w


def test_identities(P):
    c, widths = 19, (1, 2, 4, 8)
    pred, label = _maps(9, 3, c, 64, 96, torch.int64)
    pred[0, 32, 48] = 3                                              # no oob here: IoUMetrics.confusion has no such notion
    stats, oob = run(P, pred, label, widths, c)
    dec = P.ops.boundary_stats_to_numpy(stats, c)
    assert int(oob.item()) == 0
    keep = (label >= 0) & (label < c)                                # in-range labels (255 is ignore_index there as well)
    ref = P.metrics.IoUMetrics(c, 255, wrap_uint8_labels=False).confusion(pred[keep].contiguous(), label[keep].contiguous())
    assert np.array_equal(dec["conf"][0].sum(0).reshape(-1), ref.reshape(-1).cpu().numpy())
    gt, pr, inter = (np.cumsum(a, axis=0) for a in (dec["conf"][0].sum(2), dec["pr"][0], dec["inter"][0]))
    assert (np.diff(gt, axis=0) >= 0).all() and (np.diff(pr, axis=0) >= 0).all() and (np.diff(inter, axis=0) >= 0).all()
    assert (inter <= np.minimum(gt, pr)).all() and inter[-1].sum() == np.trace(dec["conf"][0].sum(0))
    assert np.array_equal(pr[-1], dec["conf"][0].sum(0).sum(0)) and 0 < gt[0].sum() < gt[-1].sum()


def test_slots_additivity_and_stream(P):
    c, widths = 7, (2, 5)
    pred, label = _maps(13, 4, c, 31, 53, torch.uint8)
    pred[0, 15, 26] = 1                                              # no oob in this test
    cond = [2, -1, 0, 7]                                             # 7 and -1: out of range, slot 0 only
    stats, oob = run(P, pred, label, widths, c, cond=cond, n_slots=4)
    want, _ = model(pred, label, widths, c, cond=cond, n_slots=4)
    got = stats.cpu().numpy()
    assert np.array_equal(got, want) and not got[2].any() and got[1].any() and got[3].any()
    assert np.array_equal(got[1] + got[3], model(pred[[0, 2]], label[[0, 2]], widths, c)[0][0])
    none, _ = run(P, pred, label, widths, c, cond=None, n_slots=4)
    assert torch.equal(none[0], stats[0]) and not none[1:].any()
    # two launches accumulate; 4 = 2 + 2
    split = P.ops.new_boundary_stats(c, len(widths), "cuda", 4)
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    run(P, pred[:2].contiguous(), label[:2].contiguous(), widths, c, cond=cond[:2], n_slots=4, stats=split, oob=zero)
    run(P, pred[2:].contiguous(), label[2:].contiguous(), widths, c, cond=cond[2:], n_slots=4, stats=split, oob=zero)
    assert torch.equal(split, stats)
    run(P, pred, label, widths, c, cond=cond, n_slots=4, stats=split, oob=zero)
    assert torch.equal(split, 2 * stats) and int(zero.item()) == 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other, _ = run(P, pred, label, widths, c, cond=cond, n_slots=4)
    s.synchronize()
    assert torch.equal(other, stats)


def test_refusals(P):
    N = P.N
    c, h, w = 7, 8, 16
    pred = torch.zeros(1, h, w, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(1, h, w, dtype=torch.uint8, device="cuda")
    stats = P.ops.new_boundary_stats(c, 2, "cuda", 2)
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(int(N.lib().awseg_boundary_workspace(1, c, h, w, 4)), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())         # noqa: E731

    def call(pr=pred, label=lab, ldt=0, batch=1, hh=h, ww=w, cc=c, widths=(1, 2), nw=None, st=stats, slots=2, ob=oob, wk=ws):
        wd = None if widths is None else np.asarray(widths, dtype=np.int32)
        N.call("awseg_boundary_stats", p(pr), p(label), ldt, 255, batch, hh, ww, cc, None if wd is None else N.host(wd),
               len(widths) if nw is None else nw, None, p(st), slots, p(ob), p(wk), None)
    einval = [dict(pr=None), dict(label=None), dict(st=None), dict(ob=None), dict(wk=None), dict(widths=None, nw=2), dict(batch=0),
              dict(hh=0), dict(ww=0), dict(cc=0), dict(cc=33), dict(slots=0), dict(ldt=2), dict(widths=(), nw=0),
              dict(widths=(1, 2, 3, 4, 5)), dict(widths=(2, 2)), dict(widths=(4, 2)), dict(widths=(0, 1)), dict(widths=(1, 17)),
              dict(widths=(-3,))]
    for kw in einval:
        with pytest.raises(N.AwsegError, match="code -1"):
            call(**kw)
    for kw in (dict(batch=65536), dict(hh=65536, ww=32768)):
        with pytest.raises(N.AwsegError, match="code -2"):
            call(**kw)
    torch.cuda.synchronize()
    assert not stats.any() and not oob.any()                         # nothing was launched
    call()
    torch.cuda.synchronize()
    assert int(stats[0, 2, 0]) == h * w
    ops = P.ops
    good = dict(pred=pred, label=lab, widths=[1, 2], num_classes=c, stats=stats, oob=oob)
    for kw in (dict(pred=pred.long()), dict(pred=pred[0]), dict(label=lab.int()), dict(label=lab[:, :4].contiguous()),
               dict(label=torch.zeros(2, h, w, dtype=torch.uint8, device="cuda")), dict(widths=[2, 1]), dict(widths=[]), dict(widths=[1.0]),
               dict(widths=[1, 2, 3]), dict(stats=stats[:, :2]), dict(stats=stats.int()), dict(num_classes=33),
               dict(oob=torch.zeros(2, dtype=torch.int64, device="cuda")), dict(cond=torch.zeros(1, dtype=torch.int64, device="cuda")),
               dict(cond=torch.zeros(2, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            ops.boundary_stats(**dict(good, **kw))
    torch.cuda.synchronize()
    assert int(stats[0, 2, 0]) == h * w                               # refused before any launch


# ----------------------------------------------------------------------------- the harness end to end
class Spy:
    """Counts the calls of the new entry points and keeps the prediction map every forward wrote with the labels it saw."""

    def __init__(self, P, monkeypatch, model):
        self.calls, self.batches = [], []
        for name in ("boundary_stats", "new_boundary_stats"):
            real = getattr(P.ops, name)
            monkeypatch.setattr(P.ops, name, lambda *a, _n=name, _r=real, **k: (self.calls.append(_n), _r(*a, **k))[1])
        fe = model.forward_eval

        def wrapped(images, labels, counts, oob, cond, **k):
            out = fe(images, labels, counts, oob, cond, **k)
            self.kw = sorted(k)
            if k.get("pred_out") is not None:
                self.batches.append((k["pred_out"].clone().cpu().numpy(), labels.clone().cpu().numpy(), cond.clone().cpu().numpy()))
            return out
        monkeypatch.setattr(model, "forward_eval", wrapped, raising=False)


def _recount(spy, widths, n_slots):
    total = None
    for pred, label, cond in spy.batches:
        st, oob = BR.boundary_counters(pred.reshape(label.shape), label, widths, 19, cond=cond, n_slots=n_slots)
        assert oob == 0
        total = st if total is None else total + st
    return total


def test_harness_option_off_changes_nothing_and_on_equals_the_model(P, monkeypatch):
    from tests.test_gpu_failure import _dataset, _evaluate, _model
    model = _model(P)
    ds = _dataset(P)
    conds = list(ds.weather_conditions)
    base = {"data.weather_conditions": conds}
    spy = Spy(P, monkeypatch, model)
    absent = _evaluate(P, model, ds, base)
    kw_off = spy.kw
    off = _evaluate(P, model, ds, dict(base, **{"evaluation.boundary_widths": None}))
    assert not spy.calls and not spy.batches and "pred_out" in kw_off           # the argument is there today, as None
    assert not any("boundary" in k or "interior" in k for k in off)
    assert list(absent) == list(off) and repr([absent[k] for k in absent]) == repr([off[k] for k in off])
    widths = [1, 2, 4, 8]
    on = _evaluate(P, model, ds, dict(base, **{"evaluation.boundary_widths": widths}))
    assert spy.calls.count("new_boundary_stats") == 1 and spy.calls.count("boundary_stats") == 3 and len(spy.batches) == 3
    assert spy.kw == kw_off                                          # the forward takes the same arguments
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k                             # every old key keeps its value, bit for bit
    want = P.metrics.boundary_metrics_from_stats(_recount(spy, widths, 1 + len(conds)), widths, conds, 19)
    new = {k: v for k, v in on.items() if k not in off}
    # (the synthetic set labels every pixel independently: each labelled pixel is within 1 of a boundary, so no interior keys here;
    # tests/test_boundary_ref.py checks those)
    assert new == want and "boundary_iou_w8_fog" in want and "boundary_degradation_w8_night" in want
    assert "boundary_miou_w1" in want and "boundary_fraction_w4_clean" in want and all(isinstance(v, float) for v in want.values())
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    assert "## Boundary Bands" in report_markdown(on) and "## Boundary Bands" not in report_markdown(off)


def test_harness_sweep_slots_and_kinds(P, monkeypatch):
    from tests.test_gpu_failure import _dataset, _evaluate, _model
    model = _model(P)
    ds = _dataset(P, n=4, sev=(0.3, 0.8))
    slots = ds.sweep.slots()
    cfg = {"data.weather_conditions": list(ds.weather_conditions), "evaluation.severities": [0.3, 0.8]}
    off = _evaluate(P, model, ds, cfg)
    spy = Spy(P, monkeypatch, model)
    widths = [2, 5]
    on = _evaluate(P, model, ds, dict(cfg, **{"evaluation.boundary_widths": widths}))
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k
    assert len(spy.batches) == 10                                    # 2 source groups x (clean + 2 kinds x 2 levels)
    want = P.metrics.boundary_metrics_from_stats(_recount(spy, widths, 1 + len(slots)), widths, slots, 19, kinds=["fog", "night"], levels=2)
    assert {k: v for k, v in on.items() if k not in off} == want
    for k in ("boundary_iou_w2_fog_s1", "boundary_iou_w5_night_s2", "boundary_iou_w5_fog", "boundary_degradation_w5_night",
              "boundary_fraction_w2_clean", "boundary_miou_w2_night"):
        assert k in want, k


def _run_direct(P, monkeypatch, model, ds, widths, ensemble, relabel=None):
    """eval_batch over the dataset with the counters on (labels replaced by `relabel(label)` when given); -> (results, counters of the
    numpy model on the very maps and labels ops.boundary_stats was handed)."""
    seen = []
    real = P.ops.boundary_stats

    def spy(pred, label, w, c, stats, oob, cond=None, **k):
        seen.append((pred.clone().cpu().numpy(), label.clone().cpu().numpy(), cond.clone().cpu().numpy()))
        return real(pred, label, w, c, stats, oob, cond, **k)
    monkeypatch.setattr(P.ops, "boundary_stats", spy)
    conds = list(ds.weather_conditions)
    metrics = P.RobustnessMetrics(19, conds)
    st = P.harness.EvalState(metrics, conds, "cuda", 15, ensemble, boundary=widths)
    for batch in ds.batches(2):
        label = batch["label"] if relabel is None else relabel(batch["label"])
        P.harness.eval_batch(model, st, batch["image"], label, batch["weather_condition"], metrics)
    res = P.harness.finalize(st, metrics)
    total = sum(BR.boundary_counters(p, l, widths, 19, cond=c, n_slots=1 + len(conds))[0] for p, l, c in seen)
    assert len(seen) == 3 and torch.equal(st.boundary["stats"].cpu(), torch.from_numpy(total))
    return res, total, conds


def test_harness_with_coherent_labels_reports_the_interior(P, monkeypatch):
    """The synthetic set labels every pixel independently; with labels in 32 x 32 blocks of one class (a stripe of 255 across them)
    the label band is a part of the frame and the interior keys appear."""
    from tests.test_gpu_failure import _dataset, _model

    def blocky(label):
        out = label[:, ::32, ::32].repeat_interleave(32, 1).repeat_interleave(32, 2).clone()
        out[:, 40:43, :] = 255
        return out.contiguous()
    widths = [1, 2, 4, 8]
    res, total, conds = _run_direct(P, monkeypatch, _model(P), _dataset(P), widths, True, relabel=blocky)
    want = P.metrics.boundary_metrics_from_stats(total, widths, conds, 19)
    assert {k: v for k, v in res.items() if "boundary_" in k or "interior_" in k} == want
    for k in ("interior_miou", "interior_miou_clean", "interior_miou_fog", "interior_degradation_fog", "interior_degradation_night",
              "boundary_degradation_w8_fog", "boundary_iou_w1_night"):
        assert k in want, k
    fr = [want[f"boundary_fraction_w{d}"] for d in widths]
    assert 0 < fr[0] < fr[1] < fr[2] < fr[3] < 1                     # 32-pixel blocks: the 8-pixel band leaves an interior
    assert total[0, -1, :19 * 19].sum() > 0 and total[0, 0, :19 * 19].sum() > 0


def test_harness_single_model_branch(P, monkeypatch):
    """A model without forward_eval: the scratch prediction map goes through combine_argmax_confusion."""
    from tests.test_gpu_failure import _dataset, _evaluate
    from tests.test_gpu_models import calibrate_bn
    torch.manual_seed(3)
    model = calibrate_bn(P.pkg.DeepLabV3PlusModel(num_classes=19, include_depth=True, pretrained=False)).cuda().eval()
    ds = _dataset(P)
    widths = [2, 5]
    off = _evaluate(P, model, ds, {"data.weather_conditions": list(ds.weather_conditions)})
    res, total, conds = _run_direct(P, monkeypatch, model, ds, widths, False)
    want = P.metrics.boundary_metrics_from_stats(total, widths, conds, 19)
    assert want and {k: v for k, v in res.items() if k not in off} == want and "boundary_iou_w5_fog" in want
    for k, v in off.items():
        assert repr(res[k]) == repr(v), k                            # every old key keeps its value
    with torch.no_grad():                                            # the map is the model's argmax
        batch = next(iter(ds.batches(2)))
        ref = model(batch["image"])["segmentation"].float().argmax(1)
    st = P.harness.EvalState(P.RobustnessMetrics(19, conds), conds, "cuda", 15, False, boundary=widths)
    P.harness.eval_batch(model, st, batch["image"], batch["label"], batch["weather_condition"], P.RobustnessMetrics(19, conds))
    assert torch.equal(st.pred_scratch.view(ref.shape).long(), ref)


def test_harness_raises_on_an_out_of_range_prediction(P):
    metrics = P.RobustnessMetrics(19, ["clean"])
    st = P.harness.EvalState(metrics, ["clean"], "cuda", 15, False, boundary=[1, 2])
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    pred = lab.clone()
    pred[0, 3, 3] = 19
    P.ops.boundary_stats(pred, lab, st.boundary["widths"], 19, st.boundary["stats"], st.boundary["oob"])
    with pytest.raises(IndexError, match="boundary"):
        P.harness.finalize(st, metrics)


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
model = calibrate_bn(pkg.EnsembleModel(num_classes=19, include_depth=True, pretrained=False)).cuda().eval()
conds = ["clean", "fog", "night"]
ds = CityscapesKITTIDataset(split="test", image_size=(128, 256), weather_conditions=conds, include_depth=True, device="cuda",
                            num_samples=4, weather_schedule="paired", severities=[0.3, 0.8])
loader = create_dataloader(ds, batch_size=2, shuffle=False, rank=rank, world_size=world)
res = evaluate_model(model, loader, RobustnessMetrics(19, conds), "cuda",
                     {"data.weather_conditions": conds, "evaluation.severities": [0.3, 0.8], "evaluation.boundary_widths": [1, 2, 4, 8]})
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
    for k in ("boundary_iou_w8_fog_s2", "boundary_miou_w1_night", "boundary_degradation_w4_fog", "boundary_fraction_w2_clean"):
        assert k in a, k
    assert a == b


# ----------------------------------------------------------------------------- full size
def test_fullsize_batch_against_the_separable_model(P):
    c, widths = 19, (1, 2, 4, 8)
    pred, label = _maps(21, 2, c, 1024, 2048, torch.uint8, block=16)  # 1024 tiles per frame: every block walks two tiles
    stats, oob = run(P, pred, label, widths, c, cond=[0, 1], n_slots=3)
    want, want_oob = model(pred, label, widths, c, cond=[0, 1], n_slots=3)
    assert int(oob.item()) == want_oob == 1
    assert np.array_equal(stats.cpu().numpy(), want) and want[0, 0].sum() > 0 and want[0, -1].sum() > 0
