"""awseg_change_strata and awseg_stratified_stats on the device against the numpy model of tests/strata_ref.py (exact: a stratum is
a byte decided by float32 compares that numpy reproduces bit for bit, every counter an integer), and the harness option
evaluation.change_strata end to end.

csrc/strata.hip: change_strata serves an image with ceil(hw / 4 / 256) blocks on the 16-byte path (64 x 128: 8 blocks) and
ceil(hw / 256) on the scalar one; stratified_stats gives a lane 16 pixels and a block 512 lanes (67 x 131: two blocks, the second
ragged)."""
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

from tests import strata_ref as SR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEFAULT = [0.5, 4.5, 16.5, 64.5]
K8 = [0.0, 1.0, 2.5, 3.0, 17.0, 64.5, 199.5]
FRAMES = [(2, 3, 32, 64), (3, 3, 31, 53), (1, 1, 1, 5), (1, 3, 1, 1), (2, 3, 64, 128), (2, 3, 67, 131)]


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import loader
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    return SimpleNamespace(ops=ops, N=native, loader=loader, harness=harness, metrics=metrics, EnsembleModel=pkg.EnsembleModel,
                           RobustnessMetrics=pkg.RobustnessMetrics, pkg=pkg)


# ----------------------------------------------------------------------------- change_strata
def _frames(seed, b, ch, h, w, refs=3):
    """float32 frames as the loader normalises 8-bit data: `refs` clean frames, b variants of rows frame_ref that change a part of
    the pixels by a few to many grey levels; NaN, +-inf and values exactly on an edge planted where the frame has room."""
    rng = np.random.default_rng(seed)
    std = SR.IMAGENET_STD[:ch] if ch <= 3 else np.full(ch, 0.25, np.float32)
    u8 = rng.integers(0, 256, (refs, ch, h * w))
    norm = lambda x: (((x / 255.0).astype(np.float32) - np.float32(0.45)) / std[:, None]).astype(np.float32)   # noqa: E731
    fr = rng.integers(0, refs, b).astype(np.int32)
    delta = rng.choice([0, 0, 0, 0, 1, 3, 5, 17, 40, 65, 200], (b, 1, h * w)) * (rng.random((b, ch, h * w)) < 0.7)
    clean, var = norm(u8), norm(np.clip(u8[fr] + delta, 0, 255))
    if h * w > 16:
        r0 = int(fr[0])
        var[0, 0, 3] = np.nan
        var[0, ch - 1, 4] = np.inf
        var[0, 0, 5] = -np.inf
        clean[r0, 0, 6] = np.nan
        clean[r0, 0, 7] = np.inf
        var[0, 0, 7] = np.inf                                         # inf - inf: a NaN difference
        for i, e in enumerate(K8 + DEFAULT):                          # exactly on an edge (scale 1 on channel 0 in those tests)
            clean[r0, :, 8 + i] = 0.0
            var[0, :, 8 + i] = 0.0
            var[0, 0, 8 + i] = e
    return var, clean, fr


def _change(P, var, clean, fr, edges, scale=None, shape=None, offset=False):
    b, ch, hw = var.shape
    shape = shape or (hw,)

    def dev(a, dtype):
        t = torch.from_numpy(a).cuda()
        if offset:                                                    # the same data one element behind a 16-byte boundary
            buf = torch.empty(t.numel() + 1, dtype=dtype, device="cuda")
            buf[1:].copy_(t.reshape(-1))
            t = buf[1:].view(t.shape)
            assert t.data_ptr() % 16 != 0
        return t
    image, refs = dev(var.reshape((b, ch) + shape), torch.float32), dev(clean.reshape((clean.shape[0], ch) + shape), torch.float32)
    out = None
    if offset:
        out = torch.empty(b * hw + 1, dtype=torch.uint8, device="cuda")[1:].view((b,) + shape)
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = P.ops.change_strata(image, refs, torch.from_numpy(np.asarray(fr, np.int32)).cuda(), edges, out=out, scale=scale, oob=oob)
    assert got.shape == (b,) + shape and got.dtype == torch.uint8
    return got.reshape(b, hw).cpu().numpy(), int(oob.item())


@pytest.mark.parametrize("edges", [[0.5], DEFAULT, K8], ids=["K=2", "K=5", "K=8"])
@pytest.mark.parametrize("shape", FRAMES, ids=str)
def test_change_strata_equals_the_model(P, shape, edges):
    b, ch, h, w = shape
    var, clean, fr = _frames(5, b, ch, h, w)
    scale = None if ch == 3 else [0.25 * 255] * ch
    got, oob = _change(P, var, clean, fr, edges, scale=scale, shape=(h, w))
    want, want_oob = SR.change_strata(var, clean, fr, edges, scale=scale)
    assert oob == want_oob == 0
    bad = np.argwhere(got != want)
    assert not len(bad), f"{len(bad)} strata differ, first (frame, pixel) {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    if h * w > 16:
        assert (want[0] == 255).sum() == 3 and len(np.unique(want)) >= min(len(edges) + 1, 4)


@pytest.mark.parametrize("shape", [(2, 3, 32, 64), (3, 3, 31, 53), (2, 3, 67, 131)], ids=str)
def test_change_strata_edge_equality_nonfinite_values_and_the_scalar_path(P, shape):
    b, ch, h, w = shape
    var, clean, fr = _frames(6, b, ch, h, w)
    ones = [1.0] * ch
    for edges in (K8, DEFAULT):
        want, _ = SR.change_strata(var, clean, fr, edges, scale=ones)
        first = 8 if edges is K8 else 8 + len(K8)
        assert want[0, first:first + len(edges)].tolist() == list(range(1, len(edges) + 1))      # on the edge: the upper stratum
        assert want[0, 3] == 255 and want[0, 6] == 255 and want[0, 7] == 255                        # NaN, NaN in the twin, inf - inf
        assert want[0, 4] == len(edges) and want[0, 5] == len(edges)                                # +-inf: the top stratum
        for offset in (False, True):
            got, oob = _change(P, var, clean, fr, edges, scale=ones, shape=(h, w), offset=offset)
            assert np.array_equal(got, want) and oob == 0, (edges, offset)


def test_change_strata_rows_without_a_twin_and_a_side_stream(P):
    for b, ch, h, w in ((3, 3, 32, 64), (3, 3, 31, 53)):
        var, clean, fr = _frames(7, b, ch, h, w)
        fr = np.array([1, -1, 3], np.int32)                           # frame 1: no twin; frame 2: a row the buffer does not have
        want, want_oob = SR.change_strata(var, clean, fr, DEFAULT)
        assert want_oob == h * w and (want[1:] == 255).all() and not (want[0] == 255).all()
        got, oob = _change(P, var, clean, fr, DEFAULT, shape=(h, w))
        assert np.array_equal(got, want) and oob == want_oob
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            other, oob2 = _change(P, var, clean, fr, DEFAULT, shape=(h, w))
        s.synchronize()
        assert np.array_equal(other, want) and oob2 == want_oob


def test_change_strata_refusals(P):
    N, ops = P.N, P.ops
    ch, hw = 3, 64
    img = torch.zeros(1, ch, hw, device="cuda")
    ref = torch.zeros(2, ch, hw, device="cuda")
    fr = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((1, hw), 7, dtype=torch.uint8, device="cuda")
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())         # noqa: E731

    def call(image=img, refs=ref, n_refs=2, batch=1, channels=ch, size=hw, frame_ref=fr, scale=(1.0, 1.0, 1.0, 1.0), edges=(0.5, 4.5),
             k=None, o=out, ob=oob):
        sc = None if scale is None else np.asarray(scale, dtype=np.float32)
        ed = None if edges is None else np.asarray(edges, dtype=np.float32)
        N.call("awseg_change_strata", p(image), p(refs), n_refs, batch, channels, size, p(frame_ref), None if sc is None else N.host(sc),
               None if ed is None else N.host(ed), (len(edges) + 1) if k is None else k, p(o), p(ob), None)
    nan, inf = float("nan"), float("inf")
    einval = [dict(image=None), dict(refs=None), dict(frame_ref=None), dict(scale=None), dict(edges=None, k=3), dict(o=None), dict(ob=None),
              dict(n_refs=0), dict(batch=-1), dict(channels=0), dict(channels=5), dict(size=0), dict(k=1), dict(edges=(1.0,) * 8),
              dict(edges=(2.0, 1.0)), dict(edges=(1.0, 1.0)), dict(edges=(-0.5, 1.0)), dict(edges=(1.0, inf)), dict(edges=(nan,)),
              dict(scale=(1.0, 0.0, 1.0)), dict(scale=(1.0, nan, 1.0)), dict(scale=(inf, 1.0, 1.0)), dict(scale=(1.0, 1.0, -2.0))]
    for kw in einval:
        with pytest.raises(N.AwsegError, match="code -1"):
            call(**kw)
    for kw in (dict(batch=65536), dict(size=1 << 31)):
        with pytest.raises(N.AwsegError, match="code -2"):
            call(**kw)
    call(batch=0)                                                     # nothing to do: returns 0
    torch.cuda.synchronize()
    assert (out == 7).all() and not oob.any()                         # nothing was launched
    call()
    torch.cuda.synchronize()
    assert not out.any()
    good = dict(image=img, ref_images=ref, frame_ref=fr, edges=[0.5, 4.5])
    for kw in (dict(image=img.double()), dict(image=img[0]), dict(image=torch.zeros(1, 5, hw, device="cuda")), dict(ref_images=ref[:, :2]),
               dict(ref_images=ref.half()), dict(frame_ref=fr.long()), dict(frame_ref=torch.zeros(2, dtype=torch.int32, device="cuda")),
               dict(edges=[2, 1]), dict(edges=[]), dict(edges=[-1.0]), dict(edges=list(range(8))), dict(edges=[nan]), dict(scale=[1.0, 1.0]),
               dict(scale=[1.0, 0.0, 1.0]), dict(out=torch.zeros(1, hw - 1, dtype=torch.uint8, device="cuda")), dict(out=out.int()),
               dict(oob=torch.zeros(2, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            ops.change_strata(**dict(good, **kw))
    with pytest.raises(ValueError, match="three channels"):           # the default scale is the loader's RGB normalisation
        ops.change_strata(torch.zeros(1, 1, hw, device="cuda"), torch.zeros(1, 1, hw, device="cuda"), fr, [0.5])


# ----------------------------------------------------------------------------- stratified_stats
def _maps(seed, b, c, h, w, ldt, K, coherent=True, refs=3):
    """Clean maps in blocks of one class, variants that flip pixels, labels that follow the clean map half of the time, strata in
    blocks (or all of it independent noise); labels of 255 and out of range, stratum values 255 and K, and one prediction and one
    reference value outside the classes, where the frame has room."""
    rng = np.random.default_rng(seed)
    n = h * w

    def field(hi, count):
        m = rng.integers(0, hi, (count, h, w))
        if coherent:
            m = np.repeat(np.repeat(m[:, ::5, ::7], 5, 1), 7, 2)[:, :h, :w]
        return m.reshape(count, n)
    ref = field(c, refs)
    fr = rng.integers(0, refs, b).astype(np.int32)
    pred = np.where(rng.random((b, n)) < 0.3, rng.integers(0, c, (b, n)), ref[fr])
    label = np.where(rng.random((b, n)) < 0.5, ref[fr], rng.integers(0, c, (b, n)))
    stratum = field(K, b)
    want_oob = 0
    if n > 16:
        label[:, :3] = 255
        label[:, 3:5] = c + 2                                         # outside [0, C): not a labelled pixel
        if ldt == torch.int64:
            label[:, 5] = -1
            label[:, 9] = 300
        stratum[:, 6] = 255
        stratum[:, 7] = K
        stratum[:, 10] = 254
        pred[0, 8] = c
        ref[fr[b - 1], 11] = 250
        want_oob = 1 + int((fr == fr[b - 1]).sum())
    return pred.astype(np.uint8), label, stratum.astype(np.uint8), ref.astype(np.uint8), fr, want_oob


def _cuda(a, dtype=None, offset=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = t if dtype is None else t.to(dtype)
    if offset:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:].copy_(t.reshape(-1))
        t = buf[1:].view(t.shape)
    return t


def _stats(P, pred, label, stratum, K, c, ldt, ref=None, fr=None, cond=None, n_slots=1, stats=None, oob=None, offset=False):
    stats = P.ops.new_strata_stats(c, K, "cuda", n_slots) if stats is None else stats
    oob = torch.zeros(1, dtype=torch.int64, device="cuda") if oob is None else oob
    P.ops.stratified_stats(_cuda(pred, offset=offset), _cuda(label, ldt), _cuda(stratum), K, c, stats, oob,
                           ref_maps=None if ref is None else _cuda(ref), frame_ref=None if fr is None else _cuda(np.asarray(fr, np.int32)),
                           cond=None if cond is None else torch.tensor(list(cond), dtype=torch.int32, device="cuda"))
    return stats, oob


STAT_CASES = [(19, torch.uint8, 5), (19, torch.int64, 8), (7, torch.uint8, 8), (7, torch.int64, 2)]


@pytest.mark.parametrize("c,ldt,K", STAT_CASES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("shape", FRAMES, ids=str)
def test_stratified_stats_equal_the_model(P, shape, c, ldt, K):
    b, _, h, w = shape
    b += 1                                                            # one more frame: the second one is skipped
    pred, label, stratum, ref, fr, _ = _maps(11, b, c, h, w, ldt, K, coherent=(c == 19))
    fr[1] = -1
    lab = label.astype(np.uint8) if ldt == torch.uint8 else label
    cond = ([1, 0, 7, -1] * 2)[:b]                                    # 7 and -1: outside the slots, slot 0 only
    for paired in (True, False):
        kw = dict(ref=ref, fr=fr) if paired else {}
        stats, oob = _stats(P, pred, lab, stratum, K, c, ldt, cond=cond, n_slots=3, **kw)
        want, bad = SR.stratified_stats(pred, lab, stratum, K, c, refs=ref if paired else None, frame_ref=fr, cond=cond, n_slots=3)
        got = stats.cpu().numpy()
        assert got.shape == want.shape == (3, K + 1, c * c + 6)
        diff = np.argwhere(got != want)
        assert not len(diff), f"paired={paired}: {len(diff)} counters differ, first (slot, stratum, cell) {diff[0]}: " \
                              f"{got[tuple(diff[0])]} != {want[tuple(diff[0])]}"
        assert int(oob.item()) == bad and (bad > 0 or h * w <= 16)
        if not paired:
            assert not got[..., c * c:c * c + 5].any()
        if h * w > 16:
            assert want[0, K, c * c + 5] == 3 * (b - 1 if paired else b)     # 255, 254 and K: the unmeasured row
    # byte loads from an unaligned prediction map give the same
    stats2, oob2 = _stats(P, pred, lab, stratum, K, c, ldt, ref=ref, fr=fr, cond=cond, n_slots=3, offset=True)
    want, bad = SR.stratified_stats(pred, lab, stratum, K, c, refs=ref, frame_ref=fr, cond=cond, n_slots=3)
    assert np.array_equal(stats2.cpu().numpy(), want) and int(oob2.item()) == bad


def test_stratified_stats_skipped_frames_and_rows_outside_the_buffer(P):
    c, K, h, w = 7, 5, 31, 53
    pred, label, stratum, ref, fr, _ = _maps(12, 4, c, h, w, torch.int64, K)
    fr = np.array([2, -1, 3, 0], np.int32)                            # frame 1 skipped, frame 2 names a row the buffer does not have
    stats, oob = _stats(P, pred, label, stratum, K, c, torch.int64, ref=ref, fr=fr, cond=[0, 0, 1, 1], n_slots=3)
    want, bad = SR.stratified_stats(pred, label, stratum, K, c, refs=ref, frame_ref=fr, cond=[0, 0, 1, 1], n_slots=3)
    assert np.array_equal(stats.cpu().numpy(), want) and int(oob.item()) == bad and bad >= h * w
    assert want[0, :, c * c + 5].sum() + bad == 3 * h * w             # every pixel of a counted frame is a count or an oob


def test_stratified_stats_additivity_batch_split_and_stream(P):
    c, K, h, w = 19, 5, 67, 131
    pred, label, stratum, ref, fr, _ = _maps(13, 4, c, h, w, torch.uint8, K)
    label = label.astype(np.uint8)
    cond = [2, -1, 0, 7]
    stats, oob = _stats(P, pred, label, stratum, K, c, torch.uint8, ref=ref, fr=fr, cond=cond, n_slots=4)
    assert not stats[2].any() and stats[1].any() and stats[3].any()
    # two launches equal one launch on the concatenation, whatever the split
    for cut in (1, 2, 3):
        split = P.ops.new_strata_stats(c, K, "cuda", 4)
        zero = torch.zeros(1, dtype=torch.int64, device="cuda")
        for sl in (slice(0, cut), slice(cut, 4)):
            _stats(P, pred[sl], label[sl], stratum[sl], K, c, torch.uint8, ref=ref, fr=fr[sl], cond=cond[sl], n_slots=4, stats=split, oob=zero)
        assert torch.equal(split, stats) and torch.equal(zero, oob)
    _stats(P, pred, label, stratum, K, c, torch.uint8, ref=ref, fr=fr, cond=cond, n_slots=4, stats=split, oob=zero)
    assert torch.equal(split, 2 * stats)
    perm = [2, 0, 3, 1]
    other, _ = _stats(P, pred[perm], label[perm], stratum[perm], K, c, torch.uint8, ref=ref, fr=fr[perm], cond=[cond[i] for i in perm], n_slots=4)
    assert torch.equal(other, stats)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other, _ = _stats(P, pred, label, stratum, K, c, torch.uint8, ref=ref, fr=fr, cond=cond, n_slots=4)
    s.synchronize()
    assert torch.equal(other, stats)


@pytest.mark.parametrize("c,ldt,h,w", [(19, torch.uint8, 32, 64), (7, torch.int64, 31, 53), (19, torch.int64, 67, 131)], ids=str)
def test_summed_over_the_strata_the_counters_are_the_consistency_scan(P, c, ldt, h, w):
    K = 5
    pred, label, stratum, ref, fr, want_oob = _maps(14, 4, c, h, w, ldt, K)
    lab = label.astype(np.uint8) if ldt == torch.uint8 else label
    cond = [0, 1, 1, -1]
    stats, oob = _stats(P, pred, lab, stratum, K, c, ldt, ref=ref, fr=fr, cond=cond, n_slots=3)
    cons, coob = P.ops.new_consistency_stats(c, "cuda", 3), torch.zeros(1, dtype=torch.int64, device="cuda")
    P.ops.prediction_consistency(_cuda(pred), _cuda(ref), _cuda(fr), _cuda(lab, ldt), c, cons, coob, torch.tensor(cond, dtype=torch.int32, device="cuda"))
    dec, agreement = P.ops.strata_stats_to_numpy(stats, c), P.ops.consistency_stats_to_numpy(cons, c)
    assert np.array_equal(dec["transitions"].sum(1), agreement["transitions"]) and torch.equal(oob, coob) and int(oob.item()) == want_oob
    assert np.array_equal(dec["agree"].sum(1), np.trace(agreement["agreement"], axis1=1, axis2=2))
    assert np.array_equal(dec["pixels"].sum(1), agreement["agreement"].sum((1, 2)))
    assert dec["transitions"][0].sum() > 0


def test_stratified_stats_refusals(P):
    N, ops = P.N, P.ops
    c, K, hw = 7, 3, 64
    pred = torch.zeros(1, hw, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(1, hw, dtype=torch.uint8, device="cuda")
    strat = torch.zeros(1, hw, dtype=torch.uint8, device="cuda")
    ref = torch.zeros(2, hw, dtype=torch.uint8, device="cuda")
    fr = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats = ops.new_strata_stats(c, K, "cuda", 2)
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(int(N.lib().awseg_strata_workspace(1, c, hw, K)), dtype=torch.uint8, device="cuda")
    assert ws.numel() == (K + 1) * (c * c + 6) * 4
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())         # noqa: E731

    def call(pr=pred, label=lab, ldt=0, s=strat, k=K, refs=ref, n_refs=2, frame_ref=fr, batch=1, size=hw, cc=c, st=stats, slots=2, ob=oob, wk=ws):
        N.call("awseg_stratified_stats", p(pr), p(label), ldt, 255, p(s), k, p(refs), n_refs, p(frame_ref), batch, size, cc, None, p(st),
               slots, p(ob), p(wk), None)
    einval = [dict(pr=None), dict(label=None), dict(s=None), dict(st=None), dict(ob=None), dict(wk=None), dict(refs=None), dict(frame_ref=None),
              dict(n_refs=0), dict(batch=0), dict(size=0), dict(cc=0), dict(cc=33), dict(slots=0), dict(ldt=2), dict(k=0), dict(k=9)]
    for kw in einval:
        with pytest.raises(N.AwsegError, match="code -1"):
            call(**kw)
    for kw in (dict(batch=65536), dict(size=1 << 31)):
        with pytest.raises(N.AwsegError, match="code -2"):
            call(**kw)
    torch.cuda.synchronize()
    assert not stats.any() and not oob.any()                          # nothing was launched
    call()
    call(refs=None, frame_ref=None, n_refs=0)                         # the unpaired form
    torch.cuda.synchronize()
    row = stats[0, 0].cpu().numpy()
    assert row[0] == 2 * hw and row[c * c + 5] == 2 * hw and row[c * c + 4] == hw and row[c * c] == hw and not stats[0, 1:].any()
    good = dict(pred=pred, label=lab, stratum=strat, n_strata=K, num_classes=c, stats=stats, oob=oob)
    for kw in (dict(pred=pred.long()), dict(stratum=strat.int()), dict(stratum=strat[:, :4].contiguous()), dict(label=lab.int()),
               dict(label=lab[:, :4].contiguous()), dict(n_strata=0), dict(n_strata=9), dict(num_classes=33), dict(stats=stats[:, :2]),
               dict(stats=stats.int()), dict(oob=torch.zeros(2, dtype=torch.int64, device="cuda")), dict(ref_maps=ref), dict(frame_ref=fr),
               dict(ref_maps=ref.long(), frame_ref=fr), dict(ref_maps=ref, frame_ref=fr.long()), dict(ref_maps=ref[:, :4].contiguous(), frame_ref=fr),
               dict(cond=torch.zeros(1, dtype=torch.int64, device="cuda")), dict(cond=torch.zeros(2, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            ops.stratified_stats(**dict(good, **kw))
    torch.cuda.synchronize()
    assert int(stats[0, 0, 0]) == 2 * hw                              # refused before any launch


# ----------------------------------------------------------------------------- the harness end to end
def _dataset(P, n=4, hw=(128, 256), kinds=("fog", "night"), sev=(0.3, 0.8)):
    return P.loader.CityscapesKITTIDataset(split="test", image_size=hw, weather_conditions=["clean", *kinds], include_depth=False,
                                           device="cuda", num_samples=n, weather_schedule="paired", severities=list(sev))


def _sweep_run(P, monkeypatch, model, ds, change, ensemble, identical=None):
    """eval_batch over the paired batches.  identical = (kind, level): that variant is replaced by its clean frames, what a renderer
    gives at intensity 0.  -> (state, results, what the two entry points were handed, in call order)."""
    seen = []
    real_c, real_s = P.ops.change_strata, P.ops.stratified_stats

    def spy_change(image, ref_images, frame_ref, edges, out=None, scale=None, oob=None):
        got = real_c(image, ref_images, frame_ref, edges, out=out, scale=scale, oob=oob)
        seen.append(dict(image=image.cpu().numpy(), twins=ref_images[frame_ref.long()].cpu().numpy(), edges=list(edges)))
        return got

    def spy_stats(pred, label, stratum, K, c, stats, oob, ref_maps=None, frame_ref=None, cond=None, **k):
        seen[-1].update(pred=pred.cpu().numpy(), label=label.cpu().numpy(), stratum=stratum.cpu().numpy(), K=K,
                        ref=ref_maps[frame_ref.long()].cpu().numpy(), cond=cond.cpu().numpy())
        return real_s(pred, label, stratum, K, c, stats, oob, ref_maps=ref_maps, frame_ref=frame_ref, cond=cond, **k)
    monkeypatch.setattr(P.ops, "change_strata", spy_change)
    monkeypatch.setattr(P.ops, "stratified_stats", spy_stats)
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    st = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, ensemble, sweep=ds.sweep, change=change)
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


def _single_model(P):
    from tests.test_gpu_models import calibrate_bn
    torch.manual_seed(3)
    return calibrate_bn(P.pkg.DeepLabV3PlusModel(num_classes=19, include_depth=False, pretrained=False)).cuda().eval()


@pytest.mark.parametrize("ensemble", [True, False], ids=["ensemble", "single model"])
def test_harness_counters_equal_the_model_on_the_kept_tensors(P, monkeypatch, ensemble):
    from tests.test_gpu_paired import _model
    model = _model() if ensemble else _single_model(P)
    ds = _dataset(P)
    slots = ds.sweep.slots()
    _, off, none, _, _ = _sweep_run(P, monkeypatch, model, ds, None, ensemble, identical=("night", 1))
    assert not none                                                   # off: neither entry point is called
    st, on, seen, order, clean = _sweep_run(P, monkeypatch, model, ds, DEFAULT, ensemble, identical=("night", 1))
    assert len(seen) == len(order) == 8                               # 2 source groups x 2 kinds x 2 levels; no clean batch
    total = np.zeros((1 + len(slots), 6, 19 * 19 + 6), np.int64)
    for call, (kind, level, sources) in zip(seen, order):
        b = len(sources)
        # the rows the harness kept are the sources' clean frames
        assert np.array_equal(call["twins"].reshape(b, 3, -1), torch.stack([clean[s] for s in sources]).reshape(b, 3, -1).cpu().numpy())
        want, bad = SR.change_strata(call["image"].reshape(b, 3, -1), call["twins"].reshape(b, 3, -1), np.arange(b), DEFAULT)
        assert bad == 0 and np.array_equal(call["stratum"].reshape(b, -1), want) and call["K"] == 5
        if (kind, level) == ("night", 1):
            assert not want.any()                                     # the identical variant: all stratum 0
        else:
            assert want.any()
        slot = slots.index(f"{kind}_s{level}")
        assert call["cond"].tolist() == [slot] * b
        rows, bad = SR.stratified_stats(call["pred"].reshape(b, -1), call["label"].reshape(b, -1), want, 5, 19, refs=call["ref"].reshape(b, -1),
                                        frame_ref=np.arange(b), cond=call["cond"], n_slots=1 + len(slots))
        assert bad == 0
        total += rows
    assert np.array_equal(st.change["stats"].cpu().numpy(), total) and int(st.change["oob"].item()) == 0
    c2 = 19 * 19
    assert torch.equal(st.change["stats"][..., c2:c2 + 4].sum(1), st.paired["stats"][:, c2:])     # the sweep's own counters, split
    # with the option on, every old key keeps its value bit for bit, in the same order
    assert list(off) == [k for k in on if k in off]
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k
    new = {k: v for k, v in on.items() if k not in off}
    want = P.metrics.change_metrics_from_stats(total, DEFAULT, slots, ["fog", "night"], 2, 19)
    assert new == want and all(isinstance(v, float) for v in new.values())
    names = ["fog_s1", "fog_s2", "fog", "night_s1", "night_s2", "night"]
    keys = {f"change_edge_{k}" for k in range(4)} | {f"mean_change_fraction_chg{k}" for k in range(5)}
    keys |= {f"change_fraction_{n}_chg{k}" for n in names for k in range(5)}
    keys |= {f"{m}_night_s1_chg0" for m in ("miou", "accuracy", "consistency", "corruption_error_rate")}
    assert keys <= set(new) and all(k.startswith(("change_", "mean_")) or "_chg" in k for k in new), sorted(keys - set(new))
    assert new["change_fraction_night_s1_chg0"] == 1.0 and new["consistency_night_s1_chg0"] == 1.0
    assert new["corruption_error_rate_night_s1_chg0"] == 0.0 and "miou_night_s1_chg1" not in new
    assert abs(sum(new[f"change_fraction_fog_chg{k}"] for k in range(5)) - 1.0) < 1e-12 and "change_unmeasured_pixels" not in new
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    assert "## Change Strata" in report_markdown(on) and "## Change Strata" not in report_markdown(off)


def test_harness_option_through_evaluate_model_and_its_refusals(P):
    from tests.test_gpu_paired import _model
    model = _model()
    ds = _dataset(P)
    conds = list(ds.weather_conditions)
    loader = lambda: P.loader.create_dataloader(ds, batch_size=2, shuffle=False)      # noqa: E731
    cfg = {"data.weather_conditions": conds, "evaluation.severities": [0.3, 0.8]}
    off = P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda", cfg)
    on = P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda", dict(cfg, **{"evaluation.change_strata": "default"}))
    for k, v in off.items():
        assert repr(on[k]) == repr(v), k
    assert "corruption_error_share_fog_chg4" in on or "change_fraction_fog_chg4" in on
    assert not any("_chg" in k for k in off)
    with pytest.raises(ValueError, match="severity sweep"):
        P.harness.evaluate_model(model, loader(), P.RobustnessMetrics(19, conds), "cuda",
                                 {"data.weather_conditions": conds, "evaluation.change_strata": "default"})
    metrics = P.RobustnessMetrics(19, conds)
    st = P.harness.EvalState(metrics, conds, "cuda", 15, True, sweep=ds.sweep, change=[1.5])
    bad = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    bad[0, 3, 3] = 19
    P.ops.stratified_stats(bad, torch.zeros_like(bad), torch.zeros_like(bad), 2, 19, st.change["stats"], st.change["oob"])
    with pytest.raises(IndexError, match="change-strata"):
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
model = calibrate_bn(pkg.EnsembleModel(num_classes=19, include_depth=False, pretrained=False)).cuda().eval()
conds = ["clean", "fog", "night"]
ds = CityscapesKITTIDataset(split="test", image_size=(128, 256), weather_conditions=conds, include_depth=False, device="cuda",
                            num_samples=4, weather_schedule="paired", severities=[0.3, 0.8])
loader = create_dataloader(ds, batch_size=2, shuffle=False, rank=rank, world_size=world)
res = evaluate_model(model, loader, RobustnessMetrics(19, conds), "cuda",
                     {"data.weather_conditions": conds, "evaluation.severities": [0.3, 0.8], "evaluation.change_strata": "default"})
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
    for k in ("change_fraction_fog_s2_chg0", "mean_change_fraction_chg4", "change_fraction_night_chg2", "change_edge_3"):
        assert k in a, k
    assert a == b


# ----------------------------------------------------------------------------- full size
def test_fullsize_batch_through_both_kernels(P):
    B, H, W, c, K = 8, 1024, 2048, 19, 5
    g = torch.Generator(device="cuda").manual_seed(21)
    std = torch.tensor(SR.IMAGENET_STD, device="cuda").view(1, 3, 1, 1)
    u8 = torch.randint(0, 256, (B, 3, H, W), device="cuda", generator=g)
    # a veil over everything in the upper half (fog-like), flakes of 16 x 16 pixels elsewhere
    flakes = (torch.rand(B, 1, H // 16, W // 16, device="cuda", generator=g) < 0.1).repeat_interleave(16, 2).repeat_interleave(16, 3)
    delta = torch.where(flakes, torch.randint(0, 120, (B, 3, H, W), device="cuda", generator=g), torch.zeros_like(u8))
    delta[:, :, :H // 2] += torch.randint(0, 9, (B, 3, H // 2, W), device="cuda", generator=g)
    norm = lambda x: ((x.float() / 255.0) - 0.45) / std              # noqa: E731
    fr = torch.tensor([3, 0, 7, 1, 2, 6, 5, 4], dtype=torch.int32, device="cuda")
    clean, var = norm(u8), norm((u8[fr.long()] + delta).clamp_(0, 255))       # frame b is a variant of clean frame fr[b]
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    strata = P.ops.change_strata(var, clean, fr, DEFAULT, oob=oob)
    want_s, bad = SR.change_strata(var.reshape(B, 3, -1).cpu().numpy(), clean.reshape(B, 3, -1).cpu().numpy(), fr.cpu().numpy(), DEFAULT)
    assert bad == 0 and int(oob.item()) == 0 and np.array_equal(strata.reshape(B, -1).cpu().numpy(), want_s)
    assert np.bincount(want_s.reshape(-1), minlength=5).min() > 0     # every stratum occurs
    del clean, var, u8, delta
    from tests.test_gpu_paired import _maps as paired_maps
    ref, pred, label = paired_maps(22, B, c, H, W, torch.uint8)
    pred[2, 5, 9] = c                                                 # one oob pixel
    cond = torch.tensor([0, 1, 2, 0, 1, 2, -1, 0], dtype=torch.int32, device="cuda")
    stats = P.ops.new_strata_stats(c, K, "cuda", 4)
    P.ops.stratified_stats(pred, label, strata, K, c, stats, oob, ref_maps=ref, frame_ref=fr, cond=cond)
    want, bad = SR.stratified_stats(pred.reshape(B, -1).cpu().numpy(), label.reshape(B, -1).cpu().numpy(), want_s, K, c,
                                    refs=ref.reshape(B, -1).cpu().numpy(), frame_ref=fr.cpu().numpy(), cond=cond.tolist(), n_slots=4)
    assert bad == 1 and int(oob.item()) == 1
    assert np.array_equal(stats.cpu().numpy(), want) and want[0, :, c * c + 5].sum() == B * H * W - 1
