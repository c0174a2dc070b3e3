"""The numpy model of the segment-level counters (tests/segments_ref.py) against scipy and hand-made maps, and the host side of the
feature: segment_metrics_from_stats, the option validator, the report section (no GPU)."""
import numpy as np
import pytest

from tests import segments_ref as SR


def _pkg():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics, report
    return ops, harness, metrics, report


def _case(seed, c=5, shape=(2, 40, 70), block=8, flip=0.15):
    """Frame 0 in blocks of one class, the last frame independent noise; the prediction flips pixels; a stripe of 255."""
    rng = np.random.default_rng(seed)
    b, h, w = shape
    label = rng.integers(0, c, shape)
    coarse = np.repeat(np.repeat(label[:, ::block, ::block], block, 1), block, 2)[:, :h, :w]
    label[:max(1, b - 1)] = coarse[:max(1, b - 1)]
    pred = np.where(rng.random(shape) < flip, rng.integers(0, c, shape), label)
    label[:, min(2, h - 1), w // 3] = 255
    if h > 2:
        label[:, 2, :] = 255
    return pred.astype(np.uint8), label.astype(np.uint8)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 40, 70), (1, 1, 33), (1, 33, 1)])
def test_label_components_equal_scipy_and_the_python_union_find(seed, shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    c = 5
    _, label = _case(seed, c, shape)
    stats, oob, lid, pid = SR.segment_counters(label.copy(), label, c)
    for b in range(shape[0]):
        live = SR.live_mask(label[b], c)
        t = np.where(live, label[b].astype(np.int64), -1)
        assert np.array_equal(lid[b], SR.components_python(t))
        n_total = 0
        for k in range(c):
            lab, n = ndimage.label(t == k, structure=np.ones((3, 3), dtype=int))
            n_total += n
            for s in range(1, n + 1):
                ids = np.unique(lid[b][lab == s])
                assert len(ids) == 1 and ids[0] == np.flatnonzero(lab.reshape(-1) == s)[0]   # one id: the first pixel in raster order
                assert (lid[b] == ids[0]).sum() == (lab == s).sum()
        assert len(np.unique(lid[b][live])) == n_total and (lid[b][~live] == -1).all()
    assert oob == 0 and stats[0, :, :, :42].sum() == sum(len(np.unique(a[a >= 0])) for a in lid)
    assert stats[0, :, :, 5 * 7 + 6].sum() == stats[0, :, :, :42].sum()                      # pred == label: every segment fully covered
    assert np.array_equal(lid, pid)


def test_hand_made_maps():
    yy, xx = np.mgrid[:6, :9]
    board = ((yy + xx) & 1).astype(np.uint8)[None]
    stats, oob, lid, _ = SR.segment_counters(board.copy(), board, 3)
    assert len(np.unique(lid)) == 2 and set(np.unique(lid)) == {0, 1}                        # two segments under 8-connectivity
    assert stats[0, 0, 2, 41] == 1 and stats[0, 1, 2, 41] == 1 and stats[0, :, :, :42].sum() == 2          # 27 pixels each: bucket 2
    # one segment of 8 x 8 half covered: cov = 1 + floor(4 * 32 / 64) = 3; fully covered: 5; not at all: 0
    label = np.zeros((3, 8, 8), dtype=np.uint8)
    pred = np.zeros((3, 8, 8), dtype=np.uint8)
    pred[0, :, 4:] = 1
    pred[2] = 1
    stats, oob, _, _ = SR.segment_counters(pred, label, 2, cond=[0, 1, 2], n_slots=4)
    assert stats[1, 0, 3, 3 * 7 + 6] == 1 and stats[2, 0, 3, 5 * 7 + 6] == 1 and stats[3, 0, 3, 0 * 7 + 6] == 1
    assert stats[0, 0, 3, :42].sum() == 3 and oob == 0
    # prediction segments: frame 0 has a true one (class 0, fully on label 0) and an invented one (class 1)
    assert stats[1, 0, 2, 42 + 5] == 1 and stats[1, 1, 2, 42 + 0] == 1
    # an out-of-range prediction: oob, a non-hit in its label segment, in no prediction segment
    pred = np.zeros((1, 4, 4), dtype=np.uint8)
    pred[0, 1, 1] = 9
    stats, oob, lid, pid = SR.segment_counters(pred, np.zeros((1, 4, 4), dtype=np.uint8), 2)
    assert oob == 1 and pid[0, 1, 1] == -1 and lid[0, 1, 1] == 0 and stats[0, 0, 2, 4 * 7 + 6] == 1 and stats[0, 0, 1, 42 + 5] == 1


def test_cov_and_bucket_edges():
    assert [int(SR.bucket(a)) for a in (1, 3, 4, 15, 16, 63, 64, 2 ** 20 - 1, 2 ** 20, 2 ** 30)] == [0, 0, 1, 1, 2, 2, 3, 9, 10, 10]
    for area in (3, 4, 15, 16, 2 ** 20):
        got = [int(SR.cov(h, area)) for h in range(0, area + 1)] if area <= 16 else None
        if got is not None:
            assert got == [0 if h == 0 else 1 + (4 * h) // area for h in range(area + 1)] and got[-1] == 5 and max(got[:-1]) <= 4
        for j in (1, 2, 3, 4):                                       # h / A >= j / 4  <=>  cov >= j + 1, at the edge and one below
            h = -(-j * area // 4)
            assert SR.cov(h, area) >= j + 1 and (h - 1 == 0 or SR.cov(h - 1, area) < j + 1)
    assert SR.cov(2 ** 30, 2 ** 31 - 1) == 3 and SR.cov(2 ** 31 - 1, 2 ** 31 - 1) == 5       # no 32-bit overflow of 4 h
    assert SR.cov(1, 3) == 2 and SR.cov(2, 3) == 3 and SR.cov(1, 4) == 2 and SR.cov(1, 16) == 1 and SR.cov(4, 16) == 2


def _stats(C=3, slots=1):
    ops = _pkg()[0]
    return np.zeros((slots, C, ops.SEGMENT_BUCKETS, ops.SEGMENT_CELLS), dtype=np.int64)


def test_metrics_from_constructed_counters():
    ops, harness, metrics, report = _pkg()
    assert ops.SEGMENT_BUCKETS == SR.BUCKETS == 11 and ops.SEGMENT_CELLS == SR.CELLS == 48
    C = 3
    st = _stats(C, 3)
    # slot 1 'clean': class 0 has 4 label segments in bucket 2 (cov 5, 3, 2, 0), class 1 has 2 in bucket 6 (cov 5, 5); class 2 none
    for cv in (5, 3, 2, 0):
        st[1, 0, 2, cv * 7 + 6] += 1
    st[1, 1, 6, 5 * 7 + 6] += 2
    # prediction segments: class 0: 3 in bucket 2 (cov 5, 5, 0); class 2: 1 in bucket 3 (cov 1)
    st[1, 0, 2, 42 + 5] += 2
    st[1, 0, 2, 42 + 0] += 1
    st[1, 2, 3, 42 + 1] += 1
    # slot 2 'fog': class 0 one label segment below the smallest counted area, class 1 one missed
    st[2, 0, 1, 5 * 7 + 6] += 1
    st[2, 1, 6, 0 * 7 + 6] += 1
    st[0] = st[1] + st[2]
    res = metrics.segment_metrics_from_stats(st, ["clean", "fog"], C)
    assert res["segment_count_clean"] == 6.0 and res["segment_pred_count_clean"] == 4.0
    assert res["segment_recall_clean"] == pytest.approx((2 / 4 + 2 / 2) / 2)                 # threshold 0.5: cov >= 3
    assert res["segment_precision_clean"] == pytest.approx((2 / 3 + 0 / 1) / 2)
    # F1 per class: class 0: TP 2, FN 2, FP 1 -> 4 / 7; class 1: TP 2 -> 1; class 2: FP 1 only -> 0
    assert res["segment_f1_clean"] == pytest.approx((4 / 7 + 1 + 0) / 3)
    assert res["segment_miss_rate_clean"] == pytest.approx(1 / 6) and res["segment_false_rate_clean"] == pytest.approx(1 / 4)
    assert res["segment_recall_class0_clean"] == 0.5 and res["segment_recall_class1_clean"] == 1.0
    assert "segment_recall_class2_clean" not in res
    assert res["segment_recall_small_clean"] == 0.5 and res["segment_recall_medium_clean"] == 1.0
    assert "segment_recall_large_clean" not in res and "segment_miss_rate_large_clean" not in res
    assert res["segment_miss_rate_small_clean"] == 0.25 and res["segment_miss_rate_medium_clean"] == 0.0
    # fog: the bucket-1 segment is not counted at min_area 16
    assert res["segment_count_fog"] == 1.0 and res["segment_recall_fog"] == 0.0 and res["segment_miss_rate_fog"] == 1.0
    assert "segment_precision_fog" not in res and "segment_false_rate_fog" not in res      # no prediction segment: absent, not NaN
    assert res["segment_recall_drop_fog"] == pytest.approx(0.75) and res["segment_miss_rate_rise_fog"] == pytest.approx(1 - 1 / 6)
    assert not any(k.startswith("segment_lost") or k.startswith("segment_recovered") for k in res)         # no reference anywhere
    assert all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    # the thresholds and the smallest area are host choices over the same counters
    assert metrics.segment_metrics_from_stats(st, ["clean", "fog"], C, threshold=0.25)["segment_recall_class0_clean"] == 0.75
    assert metrics.segment_metrics_from_stats(st, ["clean", "fog"], C, threshold=1.0)["segment_recall_class0_clean"] == 0.25
    assert metrics.segment_metrics_from_stats(st, ["clean", "fog"], C, min_area=4)["segment_count_fog"] == 2.0
    assert metrics.segment_metrics_from_stats(st, ["clean", "fog"], C, min_area=4096)["segment_count_clean"] == 2.0
    assert metrics.segment_metrics_from_stats(_stats(C, 3), ["clean", "fog"], C) == {}
    for bad in (0.3, 0, 2, "0.5", None, True):
        with pytest.raises(ValueError):
            metrics.segment_metrics_from_stats(st, ["clean", "fog"], C, threshold=bad)
    for bad in (0, 2, 8, 4 ** 11, 16.0, "16", True, -4):
        with pytest.raises(ValueError):
            metrics.segment_metrics_from_stats(st, ["clean", "fog"], C, min_area=bad)
    with pytest.raises(ValueError):
        metrics.segment_metrics_from_stats(st[:, :2], ["clean", "fog"], C)
    with pytest.raises(ValueError):
        metrics.segment_metrics_from_stats(st, ["clean"], C)


def test_metrics_sweep_lost_and_recovered():
    ops, harness, metrics, report = _pkg()
    C = 2
    slots = ["clean", "fog_s1", "fog_s2"]
    st = _stats(C, 4)
    st[1, 0, 3, 5 * 7 + 6] = 4                                       # clean frames: no reference
    # fog_s1: of 5 segments the clean twin detects (rc >= 3) the corrupted frame keeps 4; of 3 it misses (rc < 3) it finds 1
    st[2, 0, 3, 5 * 7 + 5] = 4
    st[2, 0, 3, 1 * 7 + 4] = 1
    st[2, 1, 3, 3 * 7 + 0] = 1
    st[2, 1, 3, 0 * 7 + 2] = 2
    # fog_s2: loses all 2
    st[3, 0, 3, 2 * 7 + 5] = 2
    st[0] = st[1:].sum(0)
    res = metrics.segment_metrics_from_stats(st, slots, C, kinds=["fog"], levels=2)
    assert res["segment_lost_fog_s1"] == pytest.approx(1 / 5) and res["segment_recovered_fog_s1"] == pytest.approx(1 / 3)
    assert res["segment_lost_fog_s2"] == 1.0 and "segment_recovered_fog_s2" not in res
    assert res["segment_lost_fog"] == pytest.approx(3 / 7) and res["segment_recovered_fog"] == pytest.approx(1 / 3)
    assert "segment_lost_clean" not in res and "segment_lost" not in res
    assert res["segment_recall_fog"] == pytest.approx((4 / 7 + 1 / 3) / 2) and res["segment_count_fog"] == 10.0
    assert res["segment_recall_drop_fog"] == pytest.approx(1.0 - res["segment_recall_fog"]) and "segment_recall_drop_fog_s1" not in res
    # counters of the model on a planted pair: the prediction finds square 1 only, the clean twin's map square 2 only
    label = np.zeros((1, 16, 16), dtype=np.uint8)
    label[0, 2:6, 2:6], label[0, 9:13, 9:13] = 1, 2
    pred, ref = label.copy(), label.copy()
    pred[0, 9:13, 9:13], ref[0, 2:6, 2:6] = 0, 0
    one, oob, _, _ = SR.segment_counters(pred, label, 3, cond=[1], n_slots=3, ref_maps=ref, frame_ref=[0])
    res = metrics.segment_metrics_from_stats(one, ["clean", "fog_s1"], 3, kinds=["fog"], levels=1)
    assert oob == 0 and res["segment_lost_fog_s1"] == 0.5 and res["segment_recovered_fog_s1"] == 1.0      # background + square 2; square 1


class Cfg(dict):
    def get(self, key, default=None):
        return dict.get(self, key, default)


def test_option_validator():
    ops, harness, metrics, report = _pkg()
    assert harness.segment_option(Cfg()) is None and harness.segment_option(Cfg({"evaluation.segment_metrics": False})) is None
    assert harness.segment_option(Cfg({"evaluation.segment_metrics": True})) == {"threshold": 0.5, "min_area": 16}
    assert harness.segment_option(Cfg({"evaluation.segment_metrics": True, "evaluation.segment_threshold": 1, "evaluation.segment_min_area": 1})) \
        == {"threshold": 1.0, "min_area": 1}
    for bad in (1, "yes", [True]):
        with pytest.raises(ValueError, match="evaluation.segment_metrics"):
            harness.segment_option(Cfg({"evaluation.segment_metrics": bad}))
    for on in (True, False):                                          # the values are checked also when the option is off
        for key, bad in (("evaluation.segment_threshold", 0.4), ("evaluation.segment_threshold", "0.5"), ("evaluation.segment_threshold", True),
                         ("evaluation.segment_min_area", 8), ("evaluation.segment_min_area", 0), ("evaluation.segment_min_area", 16.0),
                         ("evaluation.segment_min_area", 4 ** 11)):
            with pytest.raises(ValueError, match="evaluation.segment_"):
                harness.segment_option(Cfg({"evaluation.segment_metrics": on, key: bad}))


def test_option_off_leaves_the_results_unchanged():
    """A state built without the option (absent or false) allocates nothing for it and finalises to the same dictionary."""
    import torch
    ops, harness, metrics, report = _pkg()
    conds = ["clean", "fog"]

    def results(option):
        m = metrics.RobustnessMetrics(5, conds)
        st = harness.EvalState(m, conds, "cpu", 15, False, segments=option)
        g = torch.Generator().manual_seed(1)
        st.acc.counts.copy_(torch.randint(0, 50, st.acc.counts.shape, generator=g))
        st.ece.copy_(torch.randint(0, 50, st.ece.shape, generator=g))
        return st, harness.finalize(st, m)
    st0, base = results(None)
    st1, off = results(harness.segment_option(Cfg({"evaluation.segment_metrics": False, "evaluation.segment_min_area": 4})))
    assert st0.segments is None and st1.segments is None
    assert list(base) == list(off) and repr(list(base.values())) == repr(list(off.values()))
    st2, on = results(harness.segment_option(Cfg({"evaluation.segment_metrics": True})))
    assert tuple(st2.segments["stats"].shape) == (3, 5, 11, 48) and st2.pred_scratch is None
    assert {k: on[k] for k in base} == base and not any(k.startswith("segment_") for k in on)            # no segment was counted
    one = SR.segment_counters(*_case(3), 5, cond=[0, 1], n_slots=3)[0]
    st2.segments["stats"].copy_(torch.from_numpy(one))
    on = harness.finalize(st2, metrics.RobustnessMetrics(5, conds))
    want = metrics.segment_metrics_from_stats(one, conds, 5)
    assert want and {k: v for k, v in on.items() if k not in base} == want
    for k, v in base.items():
        assert repr(on[k]) == repr(v), k
    st2.segments["oob"].fill_(1)
    with pytest.raises(IndexError, match="segment"):
        harness.finalize(st2, metrics.RobustnessMetrics(5, conds))


def test_report_section():
    ops, harness, metrics, report = _pkg()
    pred, label = _case(1)
    stats = SR.segment_counters(pred, label, 5, cond=[0, 1], n_slots=3)[0]
    res = metrics.segment_metrics_from_stats(stats, ["clean", "fog"], 5, min_area=1)
    base = {"overall_miou": 0.5}
    assert "## Segments" not in report.report_markdown(base)
    text = report.report_markdown(dict(base, **res))
    assert "## Segments" in text and "Lost" not in text
    row = [ln for ln in text.splitlines() if ln.startswith("| fog |")][0]
    for key in ("segment_recall_fog", "segment_f1_fog", "segment_miss_rate_fog", "segment_false_rate_fog", "segment_recall_small_fog"):
        assert f"{res[key]:.3f}" in row
    text = report.report_markdown(dict(base, **res, segment_lost_fog_s1=0.25, segment_recovered_fog_s1=0.5))
    assert "| fog_s1 | 0.250 | 0.500 |" in text
