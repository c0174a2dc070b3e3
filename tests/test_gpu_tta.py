"""-m gpu: awseg_tta_view and awseg_tta_accumulate against the numpy float32 model of tests/tta_ref.py, bit for bit (the header
states every operation, so there is no tolerance); one launch of each replayed inside the fenced arena of tests/fenced.py with the
prototypes of include/awseg_restore.h; and the harness option `evaluation.tta` end to end."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import fenced
from tests import launch_geometry as G
from tests import tta_ref as T
from tests.test_gpu_relight import on_device, same_bits

pytestmark = pytest.mark.gpu
RESTORE_HEADER = Path(__file__).resolve().parents[1] / "include" / "awseg_restore.h"
MODES = (T.SET, T.ADD, T.SCALE_ADD)
THIRD = np.float32(1) / np.float32(3)
# W = 1: the mirror of one column; 4: one group; 5: a ragged tail; 8: two groups; odd widths keep their middle column
EQUAL = [((h, w), (h, w)) for h in (1, 3) for w in (1, 4, 5, 8)]
# up by 2; a ragged ratio; more than 3x up; down with source cells skipped, ragged and whole
RESAMPLED = [((3, 5), (6, 10)), ((5, 7), (8, 12)), ((2, 3), (8, 12)), ((8, 12), (5, 7)), ((9, 16), (3, 4))]


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import loader
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    return SimpleNamespace(pkg=pkg, ops=ops, N=native, loader=loader, harness=harness, metrics=metrics, RobustnessMetrics=pkg.RobustnessMetrics)


def first_difference(got: torch.Tensor, want: np.ndarray) -> str:
    diff = np.nonzero(got.cpu().numpy().view(np.int32) != np.ascontiguousarray(want).view(np.int32))
    return f"{diff[0].size} of {want.size} values differ, first at {[int(d[0]) for d in diff] if diff[0].size else None}"


# ------------------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("channels", [3, 19])
@pytest.mark.parametrize("src,dst", EQUAL + RESAMPLED, ids=lambda s: "x".join(map(str, s)))
def test_accumulate_equals_the_numpy_model_bit_for_bit(P, src, dst, channels):
    """Both flips, the three modes, and a base on a 16-byte boundary and 4 bytes past it: the same bits."""
    x = T.maps(11, (2, channels) + src)
    held = T.maps(12, (2, channels) + dst)
    for flip in (False, True):
        for mode in MODES:
            want = T.accumulate(x, held, flip, THIRD, mode)
            for shift in (0, 1):
                acc = on_device(held, shift)
                got = P.ops.tta_accumulate(on_device(x, shift), acc, flip, THIRD, mode)
                assert got.data_ptr() == acc.data_ptr()
                assert same_bits(got, want), (flip, mode, shift, first_difference(got, want))
            if mode != T.SET:                                        # what the accumulator held is still in it
                assert want.tobytes() != T.accumulate(x, np.zeros_like(held), flip, THIRD, mode).tobytes()


@pytest.mark.parametrize("src,dst", EQUAL + [((5, 7), (8, 12)), ((8, 12), (5, 7))], ids=lambda s: "x".join(map(str, s)))
def test_view_equals_the_numpy_model_bit_for_bit(P, src, dst):
    for channels in (1, 3, 4):
        x = T.maps(13, (2, channels) + src)
        for flip in (False, True):
            want = T.view(x, dst, flip)
            for shift in (0, 1):
                out = on_device(np.full((2, channels) + dst, 7.0, np.float32), shift)
                got = P.ops.tta_view(on_device(x, shift), dst, flip, out=out)
                assert got.data_ptr() == out.data_ptr()
                assert same_bits(got, want), (channels, flip, shift, first_difference(got, want))
    if src == dst:                                                    # a copy and an exact mirror
        assert same_bits(P.ops.tta_view(on_device(x), dst, False), x) and same_bits(P.ops.tta_view(on_device(x), dst, True), x[..., ::-1])


@pytest.mark.parametrize("src,dst", [((5, 7), (8, 12)), ((8, 12), (5, 7)), ((2, 3), (8, 12)), ((3, 8), (3, 8))], ids=lambda s: "x".join(map(str, s)))
def test_nan_and_inf_reach_only_the_pixels_they_have_a_share_in(P, src, dst):
    x = T.maps(14, (2, 3) + src)
    x[0, 1, 0, 0], x[1, 2, src[0] - 1, src[1] // 2], x[1, 0, src[0] // 2, src[1] - 1] = np.nan, np.inf, -np.inf
    held = T.maps(15, (2, 3) + dst)
    for flip in (False, True):
        want = T.accumulate(x, held, flip, THIRD, T.ADD)
        got = P.ops.tta_accumulate(on_device(x), on_device(held), flip, THIRD, T.ADD)
        finite = np.isfinite(want)
        assert np.array_equal(torch.isfinite(got).cpu().numpy(), finite) and 0 < (~finite).sum() < finite.size
        assert np.array_equal(got.cpu().numpy()[finite].view(np.int32), want[finite].view(np.int32))
        assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want))
        v = P.ops.tta_view(on_device(x), dst, flip)
        want_v = T.view(x, dst, flip)
        assert np.array_equal(np.isnan(v.cpu().numpy()), np.isnan(want_v))
        ok = ~np.isnan(want_v)
        assert np.array_equal(v.cpu().numpy()[ok].view(np.int32), want_v[ok].view(np.int32))
    if src == dst:                                                    # one in, one out
        assert int((~finite).sum()) == 3


def test_the_second_trip_of_the_grid_is_ragged_and_right(P):
    """2 x 19 x 192 x 324 floats are 590 976 groups of four: past the cap of awseg_grid_1d (AWSEG_CUS * 8 blocks of 256 lanes), so
    some lanes take a second item and most do not.  2 x 19 x 193 x 322 (the scalar path) also ends its second trip inside a wave."""
    for shape, half, ragged in (((2, 19, 192, 324), (96, 162), False), ((2, 19, 193, 322), (97, 161), True)):
        trip = G.capped_1d(int(np.prod(shape[:3])) * G.ceil_div(shape[3], 4), per_block=256)
        assert trip["blocks"] == G.MAX_BLOCKS and trip["trips"] == 2 and trip["tail"] < G.MAX_BLOCKS * 256 and trip["ragged"] == ragged
        held = T.maps(16, shape)
        for src, flip, mode in ((half, True, T.ADD), (shape[2:], True, T.SCALE_ADD)):
            x = T.maps(17, shape[:2] + src)
            want = T.accumulate(x, held, flip, THIRD, mode)
            got = P.ops.tta_accumulate(on_device(x), on_device(held), flip, THIRD, mode)
            assert same_bits(got, want), first_difference(got, want)
    frames = T.maps(18, (2, 4, 96, 162))                              # the view launcher walks the same loop
    want = T.view(frames, (418, 650), True)
    trip = G.capped_1d(2 * 4 * 418 * G.ceil_div(650, 4), per_block=256)
    assert trip["trips"] == 2 and trip["ragged"]
    got = P.ops.tta_view(on_device(frames), (418, 650), True)
    assert same_bits(got, want), first_difference(got, want)


def test_frames_do_not_depend_on_their_batch_mates(P):
    x, held = T.maps(19, (3, 19, 10, 14)), T.maps(20, (3, 19, 16, 24))
    whole = P.ops.tta_accumulate(on_device(x), on_device(held), True, THIRD, T.SCALE_ADD)
    view = P.ops.tta_view(on_device(x[:, :3]), (16, 24), True)
    for b in range(3):
        one = P.ops.tta_accumulate(on_device(x[b:b + 1]), on_device(held[b:b + 1]), True, THIRD, T.SCALE_ADD)
        assert torch.equal(one[0], whole[b])
        assert torch.equal(P.ops.tta_view(on_device(x[b:b + 1, :3]), (16, 24), True)[0], view[b])


def test_the_views_average_is_the_sum_of_its_folds(P):
    """The harness's order: the plain logits scaled and the first view added in one launch, then ADD per view."""
    plain = T.maps(21, (2, 19, 8, 12))
    views = [(T.maps(22, (2, 19, 5, 7)), False), (T.maps(23, (2, 19, 5, 7)), True), (T.maps(24, (2, 19, 8, 12)), True)]
    w = np.float32(1) / np.float32(4)
    acc, want = on_device(plain), plain
    for i, (logits, flip) in enumerate(views):
        mode = T.SCALE_ADD if i == 0 else T.ADD
        want = T.accumulate(logits, want, flip, w, mode)
        P.ops.tta_accumulate(on_device(logits), acc, flip, w, mode)
    assert same_bits(acc, want)
    mean = (plain.astype(np.float64) + sum(T.accumulate(l, np.zeros_like(plain), f, 1.0, T.SET, dtype=np.float64) for l, f in views)) / 4
    assert np.abs(want - mean).max() < 1e-5


# --------------------------------------------------------------------------------------------------------------------- fences
@pytest.mark.parametrize("launcher", ["awseg_tta_view", "awseg_tta_accumulate"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "4 bytes off alignment"])
def test_fenced_replay_writes_nothing_outside_its_buffers(P, monkeypatch, launcher, shift):
    """One launch recorded and replayed by tests/fenced.py with the prototypes of both headers: 64 KiB of fence around source and
    destination, the destination poisoned with three bytes.  No fence byte changes, every output bit equals the plain run whatever
    the poison, no output element stays unwritten (the view; the accumulator under SET), the input is untouched."""
    protos = {**fenced.parse_header(), **fenced.parse_header(RESTORE_HEADER)}
    assert [p.name for p in protos[launcher]][-1] == "stream" and protos[launcher][0].const and not protos[launcher][5].const
    monkeypatch.setattr(fenced, "parse_header", lambda path=None: protos)         # record() asks it for the launchers' parameters
    src, dst = (5, 8), (7, 12)
    trace = fenced.Trace()
    if launcher == "awseg_tta_view":
        x = T.maps(25, (2, 3) + src)
        out = on_device(np.zeros((2, 3) + dst, np.float32), shift)
        with fenced.record(trace):
            got = P.ops.tta_view(on_device(x, shift), dst, True, out=out)
        want, written = T.view(x, dst, True), "dst"
    else:
        x = T.maps(26, (2, 19) + src)
        out = on_device(np.zeros((2, 19) + dst, np.float32), shift)
        with fenced.record(trace):
            got = P.ops.tta_accumulate(on_device(x, shift), out, True, THIRD, T.SET)
        want, written = T.accumulate(x, np.zeros((2, 19) + dst, np.float32), True, THIRD, T.SET), "acc"
    torch.cuda.synchronize()
    assert same_bits(got, want) and [l.name for l in trace.launches] == [launcher]
    slots = fenced.plan(trace, protos)
    assert {"/".join(sorted(s.params)): s.kind for s in slots} == {"src": "in", written: "out"}
    replay = fenced.Replay(trace, slots, "cuda", protos=protos)
    for s in slots:
        assert s.region.view.data_ptr() % 16 == 4 * shift
    after = {}
    for byte in (0x00, 0xFF, 0x7F):
        replay.run(byte)
        damage = replay.arena.check()
        assert not damage, f"poison {byte:#04x}: bytes outside a region changed: {damage}"
        for s in slots:
            if s.kind == "in":
                assert torch.equal(s.region.view, s.initial), f"input {s.region.name} was modified"
            else:
                assert torch.equal(s.region.view, s.final), f"poison {byte:#04x}: {s.region.name} differs from the plain run"
                after[byte] = s.region.view.clone()
    out_slot = next(s for s in slots if s.kind == "out")
    left = fenced.unwritten(after[0x00], after[0xFF], out_slot.elem)
    assert left.numel() == 0, f"{left.numel()} elements of {out_slot.region.name} were never written"


# ----------------------------------------------------------------------------------------------------------------- end to end
OPTION = {"evaluation.tta": {"scales": [0.5, 1.0], "flip": True}}
TTA_STEMS = ("tta_", "mean_tta_")


def _run(P, model, ds, ensemble, tta=None, **state):
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    st = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, ensemble, tta=tta, **state)
    for batch in ds.batches(2):
        P.harness.eval_batch(model, st, batch["image"], batch["label"], batch["weather_condition"], metrics)
    return st, P.harness.finalize(st, metrics)


def _members(model, images, ensemble):
    if ensemble:
        out = model.forward_eval(images, want_logits=False, want_pred=False, want_depth=False, combine=False)
        return [out["segformer_seg"].contiguous(), out["deeplabv3plus_seg"].contiguous()]
    return [model(images)["segmentation"].float().contiguous()]


def _by_hand(P, model, ds, ensemble, option, conditions):
    """The option's counters from ops.tta_view, the model, ops.tta_accumulate and combine_argmax_confusion over the same batches."""
    ops, n = P.ops, 1 + len(conditions)
    counts, plain_counts = ops.new_counts(19, "cuda", n), ops.new_counts(19, "cuda", n)
    stats = ops.new_consistency_stats(19, "cuda", n)
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    views = P.harness.tta_views(option)
    weight = np.float32(1) / np.float32(1 + len(views))
    sizes = []
    with torch.no_grad():
        for batch in ds.batches(2):
            images, labels = batch["image"].contiguous(), batch["label"].contiguous()
            if labels.dtype not in (torch.uint8, torch.int64):
                labels = labels.long()
            cond = torch.tensor([conditions.index(c) for c in batch["weather_condition"]], dtype=torch.int32, device="cuda")
            acc = _members(model, images, ensemble)
            mode, w, temperature = model.combine_arguments() if ensemble else (3, None, None)
            second = acc[1] if ensemble else None
            plain = torch.empty(labels.shape, dtype=torch.uint8, device="cuda")
            ops.combine_argmax_confusion(acc[0], second, mode, w, temperature, want_logits=False, label=labels, counts=plain_counts,
                                         oob=oob, cond=cond, pred_out=plain)
            for i, (scale, flip) in enumerate(views):
                size = P.harness.tta_view_size(images.shape[2], images.shape[3], scale)
                sizes.append(size)
                view = ops.tta_view(images, size, flip)
                assert tuple(view.shape[2:]) == size
                for logits, a in zip(_members(model, view, ensemble), acc):
                    ops.tta_accumulate(logits, a, flip, weight, ops.TTA_SCALE_ADD if i == 0 else ops.TTA_ADD)
            pred = torch.empty_like(plain)
            ops.combine_argmax_confusion(acc[0], second, mode, w, temperature, want_logits=False, label=labels, counts=counts, oob=oob,
                                         cond=cond, pred_out=pred)
            ops.prediction_consistency(pred, plain, torch.arange(len(images), dtype=torch.int32, device="cuda"), labels, 19, stats, oob, cond)
    assert int(oob.item()) == 0
    return counts, plain_counts, stats, sizes


@pytest.mark.parametrize("ensemble", [True, False], ids=["ensemble", "single model"])
def test_harness_scores_the_averaged_views_a_second_time(P, ensemble):
    from tests.test_gpu_paired import _dataset, _model
    from tests.test_gpu_strata import _single_model
    model = _model() if ensemble else _single_model(P)
    ds = _dataset(P, n=3, hw=(128, 192), kinds=("fog", "night"), schedule="round_robin")     # one frame per condition, batches of 2 and 1
    conditions = list(ds.weather_conditions)
    option = P.harness.tta_option(OPTION)
    st_on, on = _run(P, model, ds, ensemble, option)
    st_off, off = _run(P, model, ds, ensemble)

    # off: nothing allocated, and key for key, bit for bit what the on-run reports for everything that existed before
    assert st_off.tta is None
    new = set(on) - set(off)
    assert set(off) <= set(on) and all(repr(on[k]) == repr(off[k]) for k in off)
    assert torch.equal(st_on.acc.counts, st_off.acc.counts) and torch.equal(st_on.ece, st_off.ece)
    assert new and all(k.startswith(TTA_STEMS) or k.endswith("_tta") for k in new)
    assert on["tta_views"] == 4.0 and on["tta_scales"] == [0.5, 1.0] and on["tta_flip"] == 1.0

    # the second accumulator and the consistency counters are a recount by hand
    counts, plain_counts, stats, sizes = _by_hand(P, model, ds, ensemble, option, conditions)
    assert sizes[:3] == [(64, 96), (64, 96), (128, 192)]
    t = st_on.tta
    assert torch.equal(plain_counts, st_on.acc.counts)
    assert torch.equal(t["counts"], counts) and int(counts.sum()) > 0 and torch.equal(t["stats"], stats) and int(t["oob"].item()) == 0
    assert int(stats[0, :19 * 19].sum()) == len(ds) * 128 * 192
    assert not torch.equal(counts, plain_counts)                      # the views move the prediction

    # every key of the option
    want = P.metrics.tta_metrics_from_stats(counts.cpu().numpy(), plain_counts.cpu().numpy(), stats.cpu().numpy(), conditions, 19,
                                            degradation=P.RobustnessMetrics(19, conditions).compute_robustness_degradation_ratio,
                                            views=4, scales=[0.5, 1.0], flip=True)
    assert set(want) == new and {k: on[k] for k in want} == want
    for c in conditions:
        assert on[f"tta_gain_{c}"] == on[f"miou_{c}_tta"] - on[f"miou_{c}"]
        assert 0.0 < on[f"tta_changed_fraction_{c}"] < 1.0
        assert 0.0 <= on[f"tta_fixed_fraction_{c}"] <= 1.0 and 0.0 <= on[f"tta_broken_fraction_{c}"] <= 1.0
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    text = report_markdown({k: v if isinstance(v, (str, list)) else float(v) for k, v in on.items()})
    assert "## Test-Time Augmentation" in text and "4 views (scales 0.5, 1, each also mirrored left to right)" in text
    assert all(f"| {c} | {on[f'miou_{c}']:.3f} | {on[f'miou_{c}_tta']:.3f} | {on[f'tta_gain_{c}']:.3f} | "
               f"{on[f'tta_changed_fraction_{c}']:.3f} |" in text for c in conditions)
    st_on.all_reduce()                                                 # the table-driven reduce takes the state's tensors

    # two scales that collapse to one size are refused at the first batch, by the option's name
    collapsed = P.harness.tta_option({"evaluation.tta": {"scales": [0.5, 0.55]}})
    metrics = P.RobustnessMetrics(19, conditions)
    st = P.harness.EvalState(metrics, conditions, "cuda", 15, ensemble, tta=collapsed)
    batch = next(iter(ds.batches(2)))
    with pytest.raises(ValueError, match=r"evaluation\.tta"):
        P.harness.eval_batch(model, st, batch["image"], batch["label"], batch["weather_condition"], metrics)


def test_harness_under_a_two_level_sweep(P):
    from tests.test_gpu_dehaze_guided import _sweep_run
    from tests.test_gpu_paired import _model
    from tests.test_gpu_quality import _dataset
    model = _model()
    ds = _dataset(P, n=2, hw=(128, 192))
    slots = ds.sweep.slots()
    option = P.harness.tta_option({"evaluation.tta": "flip"})
    st, on, _ = _sweep_run(P, model, ds, True, tta=option)
    st_off, off, _ = _sweep_run(P, model, ds, True)
    assert st_off.tta is None and all(repr(on[k]) == repr(v) for k, v in off.items())
    assert torch.equal(st.acc.counts, st_off.acc.counts) and torch.equal(st.paired["stats"], st_off.paired["stats"])
    assert slots == ["clean", "fog_s1", "fog_s2", "night_s1", "night_s2"] and on["tta_views"] == 2.0
    t = st.tta
    for name in slots + ["fog", "night"]:
        for stem in ("miou_{}_tta", "tta_gain_{}", "tta_changed_fraction_{}", "tta_fixed_fraction_{}", "tta_broken_fraction_{}"):
            assert stem.format(name) in on, stem.format(name)
        assert on[f"tta_gain_{name}"] == on[f"miou_{name}_tta"] - on[f"miou_{name}"]
    for kind in ("fog", "night"):
        idx = [1 + slots.index(f"{kind}_s{j}") for j in (1, 2)]
        summed = t["counts"][idx].sum(0)
        assert int(summed.sum()) > 0
        assert on[f"miou_{kind}_tta"] == float(P.metrics.iou_from_counts(summed.cpu(), 19)["mean_iou"])
        assert f"robustness_degradation_{kind}_tta" in on and f"robustness_degradation_{kind}_s2_tta" in on
    assert torch.equal(t["counts"][1:].sum(0), t["counts"][0]) and torch.equal(t["stats"][1:].sum(0), t["stats"][0])
    want = P.metrics.tta_metrics_from_stats(t["counts"].cpu().numpy(), st.acc.counts.cpu().numpy(), t["stats"].cpu().numpy(), slots, 19,
                                            kinds=["fog", "night"], levels=2,
                                            degradation=P.RobustnessMetrics(19, ds.weather_conditions).compute_robustness_degradation_ratio,
                                            views=2, scales=[1.0], flip=True)
    assert {k: on[k] for k in want} == want
