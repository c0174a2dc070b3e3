"""awseg_segment_stats on the device against the numpy model of tests/segments_ref.py (exact: every counter is an integer count and
every id the raster-first pixel of its segment), and the harness option evaluation.segment_metrics end to end.

The tile pass works on 32 x 64 tiles (csrc/segments.hip kTH x kTW) and joins 8-pixel row runs first; the shapes below are the
smallest at which each path can go wrong: single tiles, ragged tiles, single rows and columns, 4 x 4 tiles whose 13-pixel class
blocks straddle every seam, and hand-made shapes at 70 x 130 (3 x 3 tiles, seams at rows 32 / 64 and columns 64 / 128) that only
a correct merge across seams turns into one segment."""
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

from tests import segments_ref as SR
from tests.test_gpu_boundary import _maps

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import loader
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    return SimpleNamespace(ops=ops, N=native, loader=loader, harness=harness, metrics=metrics, EnsembleModel=pkg.EnsembleModel,
                           RobustnessMetrics=pkg.RobustnessMetrics, pkg=pkg)


def run(P, pred, label, c, cond=None, n_slots=1, stats=None, oob=None, ref_maps=None, frame_ref=None, ids=True):
    pred, label = (torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a for a in (pred, label))
    stats = P.ops.new_segment_stats(c, "cuda", n_slots) if stats is None else stats
    oob = torch.zeros(1, dtype=torch.int64, device="cuda") if oob is None else oob
    ct = None if cond is None else torch.tensor(list(cond), dtype=torch.int32, device="cuda")
    ft = None if frame_ref is None else torch.tensor(list(frame_ref), dtype=torch.int32, device="cuda")
    if isinstance(ref_maps, np.ndarray):
        ref_maps = torch.from_numpy(ref_maps).cuda()
    lid = torch.full(pred.shape, -7, dtype=torch.int32, device="cuda") if ids else None
    pid = torch.full(pred.shape, -7, dtype=torch.int32, device="cuda") if ids else None
    P.ops.segment_stats(pred, label, c, stats, oob, ct, ref_maps=ref_maps, frame_ref=ft, label_ids=lid, pred_ids=pid)
    return stats, oob, lid, pid


def model(pred, label, c, cond=None, n_slots=1, ref_maps=None, frame_ref=None):
    to = lambda a: a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()       # noqa: E731
    return SR.segment_counters(to(pred), to(label), c, cond=cond, n_slots=n_slots, ref_maps=to(ref_maps), frame_ref=frame_ref)


def check(P, pred, label, c, what, **kw):
    """Every counter, oob and both id maps of one launch equal the model's; -> the model's (stats, oob, label ids, pred ids)."""
    stats, oob, lid, pid = run(P, pred, label, c, **kw)
    want, want_oob, want_lid, want_pid = model(pred, label, c, **kw)
    got = stats.cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} counters differ, first (slot, class, bucket, cell) {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert int(oob.item()) == want_oob, what
    for name, g, w in (("label", lid, want_lid), ("prediction", pid, want_pid)):
        g = g.cpu().numpy()
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: {len(bad)} {name} ids differ, first (frame, y, x) {bad[0]}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"
    return want, want_oob, want_lid, want_pid


CASES = [("C=19 64x96 u8", 19, 64, 96, torch.uint8, 8), ("C=19 64x96 i64", 19, 64, 96, torch.int64, 8),
         ("C=7 ragged 31x53 u8", 7, 31, 53, torch.uint8, 8), ("C=7 5x7", 7, 5, 7, torch.uint8, 2),
         ("C=7 1x70 (one row)", 7, 1, 70, torch.uint8, 4), ("C=7 70x1 (one column)", 7, 70, 1, torch.int64, 4),
         ("C=19 100x200 (4 x 4 tiles, blocks of 13)", 19, 100, 200, torch.uint8, 13), ("C=32 40x70 i64", 32, 40, 70, torch.int64, 8)]


@pytest.mark.parametrize("case,c,h,w,ldt,block", CASES, ids=[x[0] for x in CASES])
def test_counters_and_ids_equal_the_model(P, case, c, h, w, ldt, block):
    pred, label = _maps(7, 2, c, h, w, ldt, block)
    want, want_oob, lid, pid = check(P, pred, label, c, case, cond=[1, 0], n_slots=3)
    assert want_oob == 1
    assert want[0, :, :, :42].sum() == sum(len(np.unique(a[a >= 0])) for a in lid)           # one cell per label segment
    assert want[0, :, :, 42:].sum() == sum(len(np.unique(a[a >= 0])) for a in pid)
    assert np.array_equal(want[0], want[1] + want[2]) and want[1].any() and want[2].any()


# ----------------------------------------------------------------------------- shapes built to break the merge (70 x 130)
H, W = 70, 130


def _serpentine():
    """One-pixel-wide path of class 1 on class 0 that crosses the seam at column 64 on every other row."""
    m = np.zeros((H, W), dtype=np.uint8)
    for k, y in enumerate(range(0, H, 2)):
        m[y, 50:80] = 1
        if y + 1 < H:
            m[y + 1, 79 if k % 2 == 0 else 50] = 1
    return m


def _spiral(cy=32, cx=64):
    """A square spiral of class 1 around the corner where four tiles meet, arms two pixels apart."""
    m = np.zeros((H, W), dtype=np.uint8)
    y, x, dy, dx, run = cy, cx, 0, 1, 2
    m[y, x] = 1
    while True:
        for _ in range(2):
            for _ in range(run):
                y, x = y + dy, x + dx
                if not (0 <= y < H and 0 <= x < W):
                    return m
                m[y, x] = 1
            dy, dx = dx, -dy
        run += 2


def _diagonal_touch():
    """Two squares of class 2 that touch only diagonally across the corner (32, 64) where four tiles meet."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[22:32, 54:64] = 2
    m[32:42, 64:74] = 2
    return m


def _u_shape():
    """A U whose arms lie in the tile left of column 64 and whose base lies right of it: two tile-local components of one segment."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[5, 40:70] = 3
    m[20, 40:70] = 3
    m[5:21, 69] = 3
    return m


def _checkerboard():
    yy, xx = np.mgrid[:H, :W]
    return ((yy + xx) & 1).astype(np.uint8)


# name -> (map, the class whose pixels must come out as ONE segment)
PLANTED = {"serpentine": (_serpentine, 1), "spiral": (_spiral, 1), "diagonal touch": (_diagonal_touch, 2), "U": (_u_shape, 3),
           "one class": (lambda: np.full((H, W), 4, dtype=np.uint8), 4), "checkerboard": (_checkerboard, 1)}


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_shapes_merge_across_seams(P, name):
    make, one = PLANTED[name]
    label = make()[None]
    rng = np.random.default_rng(3)
    pred = np.where(rng.random(label.shape) < 0.3, 0, label).astype(np.uint8)                # some of every segment is found
    want, _, lid, _ = check(P, pred, label, 7, name)
    assert (label == one).sum() > 60 and len(np.unique(lid[label == one])) == 1, name
    if name == "one class":
        assert want[0, 4, 6, :42].sum() == 1 and lid.max() == 0                              # one segment of 9100 pixels: bucket 6
    if name == "checkerboard":
        assert len(np.unique(lid)) == 2                                                      # two segments under 8-connectivity
    # the same map as the prediction of a one-class label: the prediction side merges the same way
    check(P, label[0][None].copy(), np.zeros_like(label), 7, name + " (prediction side)")


def test_frames_do_not_leak_and_an_ignored_stripe_splits(P):
    label = np.zeros((2, 40, 70), dtype=np.uint8)
    label[0, -1, :] = 5                                              # the last row of frame 0 and the first of frame 1: one class
    label[1, 0, :] = 5
    label[1, 10:30, 33] = 255                                        # a stripe of ignored pixels that does not split class 0 ...
    label[1, 1:, 50] = 255                                           # ... and one that does
    want, _, lid, _ = check(P, label.copy(), label, 7, "frames")
    assert lid[0, -1, 0] == 39 * 70 and lid[1, 0, 0] == 0            # ids are positions within the frame
    assert want[0, 5].sum() == 4 and want[0, 0].sum() == 6           # per side: 2 segments of class 5; 1 + 2 of class 0
    assert len(np.unique(lid[1][label[1] == 0])) == 2


def test_reference_maps(P):
    c, h, w = 7, 64, 96
    pred, label = _maps(11, 2, c, h, w, torch.uint8)
    pred[0, h // 2, w // 2] = 1
    g = torch.Generator(device="cuda").manual_seed(5)
    refs = torch.where(torch.rand(3, h, w, device="cuda", generator=g) < 0.2, torch.randint(0, c, (3, h, w), device="cuda", generator=g),
                       label[0].long()[None].expand(3, h, w)).to(torch.uint8).contiguous()
    refs[1, 40, 40] = 77                                             # one reference value >= C on a live pixel of frame 0
    assert int(label[0, 40, 40]) < c
    want, want_oob, _, _ = check(P, pred, label, c, "refs [1, -1]", ref_maps=refs, frame_ref=[1, -1], cond=[0, 1], n_slots=3)
    cells = want[:, :, :, :42].reshape(3, c, 11, 6, 7)
    assert want_oob == 1 and not cells[2, ..., :6].any() and cells[2, ..., 6].any()          # frame 1: no reference, rc = 6
    assert cells[1, ..., :6].any() and not cells[1, ..., 6].any()
    want, want_oob, _, _ = check(P, pred, label, c, "refs [3, 0]", ref_maps=refs, frame_ref=[3, 0])
    assert want_oob == h * w
    none = run(P, pred, label, c)[0]
    both = run(P, pred, label, c, ref_maps=refs, frame_ref=[-1, -5])[0]
    assert torch.equal(none, both)
    # a lost and a recovered segment with known cells: the prediction finds square 1 and not square 2, the reference the reverse
    label = np.zeros((1, 16, 16), dtype=np.uint8)
    label[0, 2:6, 2:6], label[0, 9:13, 9:13] = 1, 2
    pred, ref = label.copy(), label.copy()
    pred[0, 9:13, 9:13], ref[0, 2:6, 2:6] = 0, 0
    want = check(P, pred, label, c, "lost / recovered", ref_maps=ref, frame_ref=[0])[0]
    assert want[0, 1, 2, 5 * 7 + 0] == 1 and want[0, 2, 2, 0 * 7 + 5] == 1 and want[0, 0, 3, 5 * 7 + 5] == 1
    assert want[0, :, :, :42].sum() == 3 and want[0, :, :, 42:].sum() == 2                  # prediction: the background and square 1


def test_additivity_and_null_id_maps(P):
    c = 7
    pred, label = _maps(13, 4, c, 31, 53, torch.uint8)
    pred[0, 15, 26] = 1                                              # no oob in this test
    cond = [2, -1, 0, 7]                                             # 7 and -1: out of range, slot 0 only
    stats, oob, _, _ = run(P, pred, label, c, cond=cond, n_slots=4)
    want = model(pred, label, c, cond=cond, n_slots=4)[0]
    assert np.array_equal(stats.cpu().numpy(), want) and not want[2].any() and want[1].any() and want[3].any()
    split = P.ops.new_segment_stats(c, "cuda", 4)
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    run(P, pred[:2].contiguous(), label[:2].contiguous(), c, cond=cond[:2], n_slots=4, stats=split, oob=zero)
    run(P, pred[2:].contiguous(), label[2:].contiguous(), c, cond=cond[2:], n_slots=4, stats=split, oob=zero, ids=False)
    assert torch.equal(split, stats)
    run(P, pred, label, c, cond=cond, n_slots=4, stats=split, oob=zero, ids=False)
    assert torch.equal(split, 2 * stats) and int(zero.item()) == 0
    none, _, _, _ = run(P, pred, label, c, cond=None, n_slots=4, ids=False)
    assert torch.equal(none[0], stats[0]) and not none[1:].any()


def test_refusals(P):
    N = P.N
    c, h, w = 7, 8, 16
    pred = torch.zeros(1, h, w, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(1, h, w, dtype=torch.uint8, device="cuda")
    stats = P.ops.new_segment_stats(c, "cuda", 2)
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert N.lib().awseg_segment_workspace(3, h, w) == 3 * h * w * 30
    ws = torch.zeros(int(N.lib().awseg_segment_workspace(1, h, w)), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())         # noqa: E731

    def call(pr=pred, label=lab, ldt=0, batch=1, hh=h, ww=w, cc=c, st=stats, slots=2, ob=oob, wk=ws):
        N.call("awseg_segment_stats", p(pr), p(label), ldt, 255, batch, hh, ww, cc, None, 0, None, None, p(st), slots, p(ob), None, None,
               p(wk), None)
    for kw in (dict(pr=None), dict(label=None), dict(st=None), dict(ob=None), dict(wk=None), dict(batch=0), dict(hh=0), dict(ww=0),
               dict(cc=0), dict(cc=33), dict(slots=0), dict(ldt=2)):
        with pytest.raises(N.AwsegError, match="code -1"):
            call(**kw)
    for kw in (dict(batch=65536), dict(hh=65536, ww=32768)):
        with pytest.raises(N.AwsegError, match="code -2"):
            call(**kw)
    torch.cuda.synchronize()
    assert not stats.any() and not oob.any()                         # nothing was launched
    call()
    torch.cuda.synchronize()
    assert int(stats[0, 0, 3, 5 * 7 + 6]) == 1 and int(stats[0, 0, 3, 42 + 5]) == 1 and int(stats.sum()) == 2     # 128 pixels: bucket 3
    good = dict(pred=pred, label=lab, num_classes=c, stats=stats, oob=oob)
    for kw in (dict(pred=pred.long()), dict(pred=pred[0]), dict(label=lab.int()), dict(label=lab[:, :4].contiguous()),
               dict(stats=stats[:, :2]), dict(stats=stats.int()), dict(num_classes=33), dict(ref_maps=pred),
               dict(oob=torch.zeros(2, dtype=torch.int64, device="cuda")), dict(cond=torch.zeros(1, dtype=torch.int64, device="cuda")),
               dict(ref_maps=pred, frame_ref=torch.zeros(1, dtype=torch.int64, device="cuda")),
               dict(label_ids=torch.zeros(1, h, w, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            P.ops.segment_stats(**dict(good, **kw))
    torch.cuda.synchronize()
    assert int(stats.sum()) == 2                                     # refused before any launch


# ----------------------------------------------------------------------------- the harness end to end
def _spy(P, monkeypatch):
    """Keeps what every ops.segment_stats call was handed."""
    seen, real = [], P.ops.segment_stats

    def spy(pred, label, c, stats, oob, cond=None, ref_maps=None, frame_ref=None, **k):
        np_ = lambda t: None if t is None else t.clone().cpu().numpy()                       # noqa: E731
        seen.append((np_(pred), np_(label), np_(cond), np_(ref_maps), np_(frame_ref)))
        return real(pred, label, c, stats, oob, cond, ref_maps=ref_maps, frame_ref=frame_ref, **k)
    monkeypatch.setattr(P.ops, "segment_stats", spy)
    return seen


def _recount(seen, n_slots):
    total = 0
    for pred, label, cond, refs, fr in seen:
        st, oob, _, _ = SR.segment_counters(pred, label, 19, cond=cond, n_slots=n_slots, ref_maps=refs, frame_ref=fr)
        assert oob == 0
        total = total + st
    return total


def test_harness_option_off_changes_nothing_and_on_equals_the_model(P, monkeypatch):
    from tests.test_gpu_failure import _dataset, _evaluate, _model
    model_ = _model(P)
    ds = _dataset(P)
    conds = list(ds.weather_conditions)
    base = {"data.weather_conditions": conds}
    seen = _spy(P, monkeypatch)
    made = []
    real_new = P.ops.new_segment_stats
    monkeypatch.setattr(P.ops, "new_segment_stats", lambda *a, **k: (made.append(1), real_new(*a, **k))[1])
    absent = _evaluate(P, model_, ds, base)
    off = _evaluate(P, model_, ds, dict(base, **{"evaluation.segment_metrics": False, "evaluation.segment_min_area": 1}))
    assert not seen and not made and not any(k.startswith("segment_") for k in off)
    assert list(absent) == list(off) and repr([absent[k] for k in absent]) == repr([off[k] for k in off])
    # the synthetic set labels every pixel independently: nearly every segment is below 16 pixels, so count them all
    on = _evaluate(P, model_, ds, dict(base, **{"evaluation.segment_metrics": True, "evaluation.segment_min_area": 1,
                                               "evaluation.segment_threshold": 0.75}))
    assert len(made) == 1 and len(seen) == 3 and all(s[3] is None for s in seen)
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k                             # every old key keeps its value, bit for bit
    want = P.metrics.segment_metrics_from_stats(_recount(seen, 1 + len(conds)), conds, 19, threshold=0.75, min_area=1)
    new = {k: v for k, v in on.items() if k not in off}
    assert new == want and all(isinstance(v, float) for v in want.values())
    for k in ("segment_recall", "segment_precision_fog", "segment_f1_night", "segment_miss_rate_clean", "segment_false_rate",
              "segment_count_fog", "segment_recall_small", "segment_recall_drop_fog", "segment_miss_rate_rise_night", "segment_recall_class3"):
        assert k in want, k
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    assert "## Segments" in report_markdown(on) and "## Segments" not in report_markdown(off)


def test_harness_raises_on_an_out_of_range_prediction(P):
    metrics = P.RobustnessMetrics(19, ["clean"])
    st = P.harness.EvalState(metrics, ["clean"], "cuda", 15, False, segments={"threshold": 0.5, "min_area": 16})
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    pred = lab.clone()
    pred[0, 3, 3] = 19
    P.ops.segment_stats(pred, lab, 19, st.segments["stats"], st.segments["oob"])
    with pytest.raises(IndexError, match="segment"):
        P.harness.finalize(st, metrics)


def test_harness_sweep_uses_the_clean_rows_as_references(P, monkeypatch):
    from tests.test_gpu_failure import _dataset, _evaluate, _model
    model_ = _model(P)
    ds = _dataset(P, n=4, sev=(0.3, 0.8))
    slots = ds.sweep.slots()
    cfg = {"data.weather_conditions": list(ds.weather_conditions), "evaluation.severities": [0.3, 0.8]}
    off = _evaluate(P, model_, ds, cfg)
    seen = _spy(P, monkeypatch)
    on = _evaluate(P, model_, ds, dict(cfg, **{"evaluation.segment_metrics": True, "evaluation.segment_min_area": 1}))
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k
    assert len(seen) == 10 and sum(s[3] is None for s in seen) == 2  # 2 source groups x (clean + 2 kinds x 2 levels); clean: no reference
    want = P.metrics.segment_metrics_from_stats(_recount(seen, 1 + len(slots)), slots, 19, min_area=1, kinds=["fog", "night"], levels=2)
    assert {k: v for k, v in on.items() if k not in off} == want
    for k in ("segment_recall_fog_s1", "segment_recall_night", "segment_lost_fog_s2", "segment_lost_night", "segment_recovered_fog",
              "segment_recall_drop_night", "segment_miss_rate_clean"):
        assert k in want, k
    assert "segment_lost_clean" not in want and "segment_lost" not in want


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
                     {"data.weather_conditions": conds, "evaluation.severities": [0.3, 0.8], "evaluation.segment_metrics": True,
                      "evaluation.segment_min_area": 1})
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
    for k in ("segment_recall_fog_s2", "segment_f1_night", "segment_lost_fog", "segment_count_clean"):
        assert k in a, k
    assert a == b
