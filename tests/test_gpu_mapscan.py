"""The seams of the shared map scan (csrc/awseg_mapscan.h): bases that are not 16-byte aligned, frames around one
chunk of 16 pixels and around one grid-stride step of a block, and the strided confusion scan.  Exact equality against the numpy
models of the passes that sit on the scan."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import bootstrap_ref as BR
from tests import paired_ref as PR
from tests import strata_ref as SR

pytestmark = pytest.mark.gpu

C, K, REFS = 19, 5, 3
# B = 9 caps the 256-thread scans at ceil(1024 / 9) = 114 blocks per frame and the 512-thread one at ceil(512 / 9) = 57: either way
# a frame's blocks cover 114 * 4096 pixels in one step, and the first block takes a second step behind that
STEP = 114 * 4096
HW_CASES = [(hw, ldt) for hw in (1, 15, 16, 17) for ldt in (torch.uint8, torch.int64)] + \
           [(STEP - 1, torch.uint8), (STEP + 1, torch.int64), (STEP + 17, torch.uint8), (STEP + 17, torch.int64)]


@pytest.fixture(scope="module")
def ops(native):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    return ops


@lru_cache(maxsize=None)                                             # a scene is made once and shared by the tests that scan it
def _scene(b, hw, seed=0):
    """numpy maps of b frames of hw pixels in runs of one value, read-only: clean maps [REFS, hw], their rows per frame (one frame
    skipped and one behind the buffer when b allows), predictions that flip pixels, labels, strata.  Where a frame has room:
    ignored and out-of-range labels, strata of K and 255, a prediction and a clean value no argmax over C classes gives."""
    rng = np.random.default_rng(seed + hw)

    def runs(hi, n):
        return np.repeat(rng.integers(0, hi, (n, hw // 7 + 1)), 7, 1)[:, :hw]
    ref = runs(C, REFS)
    fr = rng.integers(0, REFS, b).astype(np.int32)
    if b >= 4:
        fr[1], fr[3] = -1, REFS + 1
    rows = np.clip(fr, 0, REFS - 1)
    pred = np.where(rng.random((b, hw)) < 0.2, rng.integers(0, C, (b, hw)), ref[rows])
    label = np.where(rng.random((b, hw)) < 0.5, ref[rows], runs(C, b))
    stratum = runs(K, b)
    if hw > 16:
        label[:, 2:4] = 255
        label[:, hw - 1] = 255
        label[:, 5] = C + 2
        stratum[:, 6], stratum[:, 7] = K, 255
        pred[0, 8] = C
        pred[b - 1, hw - 3] = 200                                    # in the last, ragged chunk
        ref[0, 11] = 250
    out = tuple(a.astype(t) for a, t in ((pred, np.uint8), (ref, np.uint8), (fr, np.int32), (label, np.int64), (stratum, np.uint8)))
    for a in out:
        a.setflags(write=False)
    return out


def _dev(a, dtype=None, off=0):
    """`a` on the device, contiguous, its first element `off` elements behind a 16-byte aligned base."""
    t = torch.from_numpy(np.array(a))                                # a copy: the scenes are read-only
    t = t if dtype is None else t.to(dtype)
    buf = torch.zeros(t.numel() + off + 16, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + t.numel()].copy_(t.reshape(-1))
    return buf[off:off + t.numel()].view(t.shape)


def _label(label, ldt):
    return label.astype(np.uint8) if ldt == torch.uint8 else label


def _consistency(ops, scene, ldt, cond, off=()):
    pred, ref, fr, label, _ = scene
    st, oob = ops.new_consistency_stats(C, "cuda", 3), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.prediction_consistency(_dev(pred, off="pred" in off), _dev(ref, off="ref_maps" in off), _dev(fr), _dev(label, ldt, off="label" in off),
                               C, st, oob, torch.tensor(cond, dtype=torch.int32, device="cuda"))
    return st.cpu().numpy(), int(oob.item())


def _consistency_model(scene, ldt, cond):
    pred, ref, fr, label, _ = scene
    counted = [b for b in range(len(fr)) if 0 <= fr[b] < REFS]
    want, bad = PR.consistency_stats(pred, [ref[r] if 0 <= r < REFS else None for r in fr], _label(label, ldt), C, cond=cond, n_slots=3,
                                     skip=set(range(len(fr))) - set(counted))
    return want, bad + pred.shape[1] * int((fr >= REFS).sum())


def _strata(ops, scene, ldt, cond, paired, off=()):
    pred, ref, fr, label, stratum = scene
    st, oob = ops.new_strata_stats(C, K, "cuda", 3), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.stratified_stats(_dev(pred, off="pred" in off), _dev(label, ldt, off="label" in off), _dev(stratum, off="stratum" in off), K, C, st, oob,
                         ref_maps=_dev(ref, off="ref_maps" in off) if paired else None, frame_ref=_dev(fr) if paired else None,
                         cond=torch.tensor(cond, dtype=torch.int32, device="cuda"))
    return st.cpu().numpy(), int(oob.item())


def _strata_model(scene, ldt, cond, paired):
    pred, ref, fr, label, stratum = scene
    return SR.stratified_stats(pred, _label(label, ldt), stratum, K, C, refs=ref if paired else None, frame_ref=fr, cond=cond, n_slots=3)


def _cond(b):
    return ([0, 1, 5, -1] * 3)[:b]                                   # 5 and -1: outside the slots, slot 0 only


# ----------------------------------------------------------------------------- a base that is not 16-byte aligned
@pytest.mark.parametrize("ldt", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("off", [("pred",), ("ref_maps",), ("label",), ("pred", "ref_maps", "label")], ids="+".join)
def test_consistency_from_a_base_off_alignment(ops, ldt, off):
    """hw % 16 == 0, one map (or all) starts one element behind a 16-byte boundary: byte loads, the same counts."""
    scene = _scene(2, 16 * 48)
    got = _consistency(ops, scene, ldt, _cond(2), off)
    want, bad = _consistency_model(scene, ldt, _cond(2))
    assert bad > 0 and got[1] == bad and np.array_equal(got[0], want)
    assert np.array_equal(_consistency(ops, scene, ldt, _cond(2))[0], want)   # and the 16-byte loads count the same


@pytest.mark.parametrize("ldt", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("off", [("pred",), ("ref_maps",), ("stratum",), ("label",), ("pred", "ref_maps", "stratum", "label")], ids="+".join)
def test_stratified_stats_from_a_base_off_alignment(ops, ldt, off):
    scene = _scene(2, 16 * 48)
    for paired in (True, False):
        if not paired and off == ("ref_maps",):
            continue
        got = _strata(ops, scene, ldt, _cond(2), paired, off)
        want, bad = _strata_model(scene, ldt, _cond(2), paired)
        assert bad > 0 and got[1] == bad and np.array_equal(got[0], want), paired
        assert np.array_equal(_strata(ops, scene, ldt, _cond(2), paired)[0], want)


def test_the_maps_really_start_off_alignment():
    assert _dev(np.zeros(32, np.uint8), off=1).data_ptr() % 16 == 1
    assert _dev(np.zeros(32, np.int64), off=1).data_ptr() % 16 == 8 and _dev(np.zeros(32, np.uint8)).data_ptr() % 16 == 0


# ----------------------------------------------------------------------------- hw around one chunk and one grid-stride step
@pytest.mark.parametrize("hw,ldt", HW_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_consistency_around_a_chunk_and_a_step(ops, hw, ldt):
    scene = _scene(9, hw)
    got = _consistency(ops, scene, ldt, _cond(9))
    want, bad = _consistency_model(scene, ldt, _cond(9))
    assert got[1] == bad and bad >= hw and np.array_equal(got[0], want)
    assert want[0, :C * C].sum() + bad == 8 * hw                     # every pixel of a frame that is not skipped: a count or an oob


@pytest.mark.parametrize("hw,ldt", HW_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_stratified_stats_around_a_chunk_and_a_step(ops, hw, ldt):
    scene = _scene(9, hw)
    for paired in (True, False):
        got = _strata(ops, scene, ldt, _cond(9), paired)
        want, bad = _strata_model(scene, ldt, _cond(9), paired)
        assert got[1] == bad and np.array_equal(got[0], want), paired
        assert want[0, :, C * C + 5].sum() + bad == (8 if paired else 9) * hw


@pytest.mark.parametrize("hw,ldt", HW_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_frame_counts_around_a_chunk_and_a_step(ops, hw, ldt):
    pred, _, fr, label, _ = _scene(9, hw)
    table, oob = ops.new_frame_counts(REFS, C, "cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.frame_iou_counts(_dev(pred), _dev(label, ldt), C, _dev(fr), table, oob)
    want, bad = BR.frame_counts(pred, _label(label, ldt), C, fr, REFS)
    assert int(oob.item()) == bad and bad >= hw and np.array_equal(table.cpu().numpy(), want)


# ----------------------------------------------------------------------------- the strided confusion scan
@pytest.mark.parametrize("ldt", [torch.uint8, torch.int64], ids=["u8 labels", "i64 labels"])
@pytest.mark.parametrize("pdt", [torch.uint8, torch.int64], ids=["u8 pred", "i64 pred"])
@pytest.mark.parametrize("n", [15, 16, 17, 4096 * 1024 + 5])
def test_confusion_accumulate_around_a_chunk_and_past_the_block_cap(ops, n, pdt, ldt):
    """4096 * 1024 + 5 elements: every one of the 1024 blocks is full and the first strides on into a last, ragged chunk."""
    rng = np.random.default_rng(n)
    t = np.repeat(rng.integers(0, C, n // 5 + 1), 5)[:n]
    p = np.where(rng.random(n) < 0.2, rng.integers(0, C, n), t)
    t[1], t[n - 1] = 255, 255
    p[3], p[n - 2] = C, 200                                          # values no class has: oob, not counted
    base = (t * C) & 0xFF if ldt == torch.uint8 else t * C           # the reference's uint8 index wrap
    keep = (t != 255) & (p < C) & (base + p < C * C)
    want = np.bincount((base + p)[keep], minlength=C * C).reshape(C, C)
    counts, oob = ops.new_counts(C, "cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    for off in (0, 1) if pdt == ldt == torch.int64 else (0,):        # int64 maps need 8-byte alignment only
        counts.zero_(); oob.zero_()
        ops.confusion_accumulate(_dev(p, pdt, off), _dev(t, ldt, off), C, counts, oob)
        assert np.array_equal(counts.view(C, C).cpu().numpy(), want), off
        assert int(oob.item()) == int(((t != 255) & ~keep).sum()) >= 2
