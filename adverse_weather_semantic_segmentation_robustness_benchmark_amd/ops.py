"""Functional host wrappers over the C ABI (``include/awseg.h``) for torch device tensors.

Each function cites the reference function it replaces (PKG = the reference package
``adverse_weather_semantic_segmentation_robustness_benchmark``).  All of them launch on the
current torch stream, never synchronise, and raise if handed CPU tensors.
"""
from __future__ import annotations

import math
import os

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N

IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)   # PKG/data/loader.py:196
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
NIGHT_GAINS = np.array([0.8, 0.85, 1.2], dtype=np.float32)          # PKG/data/preprocessing.py:55
CONDITIONS = ("clean", "fog", "rain", "snow", "night")               # PKG/evaluation/metrics.py:491


def gaussian_taps(sigma: float = 2.0, truncate: float = 4.0) -> np.ndarray:
    """The 17 float64 weights scipy.ndimage.gaussian_filter(sigma=2) uses
    (PKG/data/preprocessing.py:243): same numpy expressions as scipy's _gaussian_kernel1d."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


_TAPS = gaussian_taps()


def _mean_std(mean, std):
    m = np.ascontiguousarray(IMAGENET_MEAN if mean is None else mean, dtype=np.float32)
    s = np.ascontiguousarray(IMAGENET_STD if std is None else std, dtype=np.float32)
    return m, s


# ----------------------------------------------------------------------------- metrics
def new_counts(num_classes: int, device, n_slots: int = 1) -> torch.Tensor:
    return torch.zeros(n_slots, num_classes * num_classes, dtype=torch.int64, device=device)


def confusion_accumulate(pred: torch.Tensor, label: torch.Tensor, num_classes: int, counts: torch.Tensor,
                         oob: torch.Tensor, ignore_index: int = 255, wrap_u8: Optional[bool] = None) -> None:
    """PKG/evaluation/metrics.py:54-71.  `wrap_u8` defaults to the reference's behaviour: on
    for uint8 label tensors (their `targets*C` wraps mod 256), off for int64."""
    pred, label = pred.contiguous().view(-1), label.contiguous().view(-1)
    if wrap_u8 is None:
        wrap_u8 = label.dtype == torch.uint8
    n = pred.numel()
    ws = N.workspace.get(pred.device, N.lib().awseg_metrics_workspace(1, num_classes, n))
    N.call("awseg_confusion_accumulate", N.ptr(pred), N.label_dtype(pred), N.ptr(label), N.label_dtype(label), n,
                                               num_classes, ignore_index, int(wrap_u8), N.ptr(counts), N.ptr(oob),
                                               N.ptr(ws), N.stream())


def argmax(logits: torch.Tensor, out_dtype=torch.int64) -> torch.Tensor:
    """logits.argmax(dim=1), REF/scripts/evaluate.py:179."""
    logits = logits.contiguous()
    b, c = logits.shape[0], logits.shape[1]
    hw = logits[0, 0].numel()
    pred = torch.empty((b,) + tuple(logits.shape[2:]), dtype=out_dtype, device=logits.device)
    N.call("awseg_argmax", N.ptr(logits), b, c, hw, N.ptr(pred), N.label_dtype(pred), N.stream())
    return pred


def combine_argmax_confusion(seg1: torch.Tensor, seg2: Optional[torch.Tensor], mode: int,
                             weights: Optional[torch.Tensor] = None, temperature: Optional[torch.Tensor] = None,
                             want_logits: bool = True, want_pred: bool = False, pred_dtype=torch.int64,
                             label: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                             oob: Optional[torch.Tensor] = None, cond: Optional[torch.Tensor] = None,
                             ignore_index: int = 255, wrap_u8: Optional[bool] = None, pred_out: Optional[torch.Tensor] = None):
    """PKG/models/model.py:443-462 (+ argmax evaluate.py:179, + confusion metrics.py:54-71).
    seg2 None -> single-model argmax(+confusion).  pred_out: the prediction map goes there (its dtype, uint8 or int64;
    want_pred and pred_dtype are then implied)."""
    seg1 = seg1.contiguous()
    b, c = seg1.shape[0], seg1.shape[1]
    hw = seg1[0, 0].numel()
    out = torch.empty_like(seg1) if (want_logits and seg2 is not None) else None
    if pred_out is not None:
        if pred_out.numel() != b * hw or pred_out.device != seg1.device:
            raise ValueError(f"pred_out must hold {b} x {hw} predictions on {seg1.device}")
        pred = pred_out
    else:
        pred = torch.empty((b,) + tuple(seg1.shape[2:]), dtype=pred_dtype, device=seg1.device) if want_pred else None
    ws = None
    ldt = N.U8
    if label is not None:
        label = label.contiguous()
        ldt = N.label_dtype(label)
        if wrap_u8 is None:
            wrap_u8 = label.dtype == torch.uint8
        ws = N.workspace.get(seg1.device, N.lib().awseg_metrics_workspace(b, c, hw))
    n_slots = 0 if counts is None else counts.shape[0]
    pdt = N.label_dtype(pred) if pred is not None else N.U8
    if seg2 is None:
        N.call("awseg_argmax_confusion", N.ptr(seg1), b, c, hw, N.ptr(pred), pdt, N.ptr(label), ldt, ignore_index,
                                            int(bool(wrap_u8)), N.ptr(cond), N.ptr(counts), n_slots, N.ptr(oob),
                                            N.ptr(ws), N.stream())
        return seg1, pred
    seg2 = seg2.contiguous()
    N.call("awseg_combine_argmax_confusion", N.ptr(seg1), N.ptr(seg2), b, c, hw, mode, N.ptr(weights),
                                                N.ptr(temperature), N.ptr(out), N.ptr(pred), pdt, N.ptr(label), ldt,
                                                ignore_index, int(bool(wrap_u8)), N.ptr(cond), N.ptr(counts), n_slots,
                                                N.ptr(oob), N.ptr(ws), N.stream())
    return out, pred


ECE_BIN_DTYPE = np.dtype([("count", "<i8"), ("sum_conf", "<f8"), ("sum_correct", "<i8")])


def new_ece_bins(n_bins: int, device, n_slots: int = 1) -> torch.Tensor:
    return torch.zeros(n_slots, n_bins, 3, dtype=torch.int64, device=device)   # 24 B / bin, raw


def ece_accumulate(logits: torch.Tensor, label: torch.Tensor, bins: torch.Tensor, edges: torch.Tensor,
                   cond: Optional[torch.Tensor] = None) -> None:
    """PKG/evaluation/metrics.py:161-194, per-pixel part, accumulated on device."""
    logits, label = logits.contiguous(), label.contiguous()
    b, c = logits.shape[0], logits.shape[1]
    hw = logits[0, 0].numel()
    ws = N.workspace.get(logits.device, N.lib().awseg_metrics_workspace(b, c, hw))
    N.call("awseg_ece_accumulate", N.ptr(logits), b, c, hw, N.ptr(label), N.label_dtype(label), N.ptr(cond),
                                         N.ptr(edges), bins.shape[1], N.ptr(bins), bins.shape[0], N.ptr(ws), N.stream())


def ensemble_eval_stats(seg1: torch.Tensor, seg2: torch.Tensor, mode: int, weights, temperature, label: torch.Tensor,
                        cond, edges: torch.Tensor, ece_bins: torch.Tensor, auroc_hist: torch.Tensor, lo: float, hi: float) -> None:
    """ECE accumulators of the combined logits + disagreement-score histogram by error flag, one pass
    over the member logits (REF/scripts/evaluate.py:230-255)."""
    seg1, seg2, label = seg1.contiguous(), seg2.contiguous(), label.contiguous()
    b, c = seg1.shape[0], seg1.shape[1]
    hw = seg1[0, 0].numel()
    ws = N.workspace.get(seg1.device, N.lib().awseg_metrics_workspace(b, c, hw))
    N.call("awseg_ensemble_eval_stats", N.ptr(seg1), N.ptr(seg2), b, c, hw, mode, N.ptr(weights), N.ptr(temperature), N.ptr(label),
           N.label_dtype(label), N.ptr(cond), N.ptr(edges), ece_bins.shape[1], N.ptr(ece_bins), ece_bins.shape[0],
           N.ptr(auroc_hist), auroc_hist.shape[1], float(lo), float(hi), N.ptr(ws), N.stream())


def combine_confusion_stats(seg1: torch.Tensor, seg2: torch.Tensor, mode: int, weights, temperature, label: torch.Tensor, cond,
                            counts: torch.Tensor, oob: torch.Tensor, edges: torch.Tensor, ece_bins: torch.Tensor,
                            auroc_hist: torch.Tensor, lo: float, hi: float, ignore_index: int = 255, wrap_u8: Optional[bool] = None,
                            pred_out: Optional[torch.Tensor] = None) -> None:
    """combine_argmax_confusion (confusion counters only) + ensemble_eval_stats in one pass over the member logits.
    pred_out (uint8 [B, H, W]): the same pass also writes the prediction map there (awseg_combine_confusion_stats_pred)."""
    seg1, seg2, label = seg1.contiguous(), seg2.contiguous(), label.contiguous()
    b, c = seg1.shape[0], seg1.shape[1]
    hw = seg1[0, 0].numel()
    if wrap_u8 is None:
        wrap_u8 = label.dtype == torch.uint8
    ws = N.workspace.get(seg1.device, N.lib().awseg_metrics_workspace(b, c, hw))
    args = (N.ptr(seg1), N.ptr(seg2), b, c, hw, mode, N.ptr(weights), N.ptr(temperature), N.ptr(label), N.label_dtype(label),
            int(ignore_index), int(bool(wrap_u8)), N.ptr(cond), N.ptr(counts), counts.shape[0], N.ptr(oob), N.ptr(edges),
            ece_bins.shape[1], N.ptr(ece_bins), ece_bins.shape[0], N.ptr(auroc_hist), auroc_hist.shape[1], float(lo), float(hi))
    if pred_out is None:
        N.call("awseg_combine_confusion_stats", *args, N.ptr(ws), N.stream())
        return
    if pred_out.dtype != torch.uint8 or pred_out.numel() != b * hw:
        raise ValueError(f"pred_out must be uint8 with {b} x {hw} elements")
    N.call("awseg_combine_confusion_stats_pred", *args, N.ptr(pred_out), N.ptr(ws), N.stream())


def new_consistency_stats(num_classes: int, device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, C*C + 4]: the agreement matrix A[ref class, variant class] and four transition counts per slot."""
    return torch.zeros(n_slots, num_classes * num_classes + 4, dtype=torch.int64, device=device)


def prediction_consistency(pred: torch.Tensor, ref_maps: torch.Tensor, frame_ref: torch.Tensor, label: torch.Tensor, num_classes: int,
                           stats: torch.Tensor, oob: torch.Tensor, cond: Optional[torch.Tensor] = None, ignore_index: int = 255) -> None:
    """Count the uint8 prediction maps `pred` [B, ...] against rows `frame_ref` (device int32 [B], < 0 skips a frame) of the clean
    maps `ref_maps` [R, ...] into `stats` (new_consistency_stats; slot 0 + slot 1 + cond[b]); map values >= C go to `oob`."""
    pred, ref_maps, label = pred.contiguous(), ref_maps.contiguous(), label.contiguous()
    b, r = pred.shape[0], ref_maps.shape[0]
    hw = pred[0].numel()
    if pred.dtype != torch.uint8 or ref_maps.dtype != torch.uint8:
        raise ValueError("prediction maps must be uint8")
    if ref_maps[0].numel() != hw or label.numel() != b * hw or frame_ref.numel() != b or frame_ref.dtype != torch.int32:
        raise ValueError("prediction_consistency: pred [B, HW], ref_maps [R, HW], label [B, HW], frame_ref int32 [B]")
    if stats.shape[-1] != num_classes * num_classes + 4:
        raise ValueError(f"consistency stats rows hold {num_classes}^2 + 4 counters")
    ws = N.workspace.get(pred.device, N.lib().awseg_consistency_workspace(b, num_classes, hw), tag="consistency")
    N.call("awseg_prediction_consistency", N.ptr(pred), N.ptr(ref_maps), r, b, hw, N.ptr(frame_ref), N.ptr(label), N.label_dtype(label),
           int(ignore_index), int(num_classes), N.ptr(cond), N.ptr(stats), stats.shape[0], N.ptr(oob), N.ptr(ws), N.stream())


def consistency_stats_to_numpy(stats, num_classes: int) -> dict:
    """int64 [slots, C*C + 4] -> {'agreement' [slots, C, C] (rows: clean class, columns: variant class), 'transitions' [slots, 4]
    (both correct, clean correct + variant wrong, clean wrong + variant correct, both wrong)}."""
    raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
    c2 = num_classes * num_classes
    return {"agreement": raw[..., :c2].reshape(raw.shape[:-1] + (num_classes, num_classes)), "transitions": raw[..., c2:c2 + 4]}


# ----------------------------------------------------------------------------- boundary-band counters (include/awseg.h)
BOUNDARY_MAX_WIDTHS = 4                # AWSEG_BOUNDARY_MAX_WIDTHS
BOUNDARY_MAX_RADIUS = 16               # AWSEG_BOUNDARY_MAX_RADIUS


def boundary_widths(widths) -> np.ndarray:
    """The band widths as a host int32 array, checked before any launch (the C ABI refuses the same lists with AWSEG_EINVAL)."""
    w = [widths] if isinstance(widths, (int, np.integer)) and not isinstance(widths, (bool, np.bool_)) else list(widths)
    if any(isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, np.integer)) for d in w):
        raise ValueError(f"band widths are integers, got {widths!r}")
    if not 1 <= len(w) <= BOUNDARY_MAX_WIDTHS:
        raise ValueError(f"1 .. {BOUNDARY_MAX_WIDTHS} band widths, got {len(w)}")
    if any(d < 1 or d > BOUNDARY_MAX_RADIUS for d in w) or any(b <= a for a, b in zip(w, w[1:])):
        raise ValueError(f"band widths must be strictly increasing within [1, {BOUNDARY_MAX_RADIUS}], got {list(w)}")
    return np.ascontiguousarray(w, dtype=np.int32)


def new_boundary_stats(num_classes: int, n_widths: int, device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, n_widths + 1, C*C + 2 C]: per slot and ring (ring k < n: edge distance within width k but not k - 1; ring n:
    the interior) the row C*C conf | C inter | C pr of include/awseg.h (zeroed: the launches accumulate)."""
    return torch.zeros(n_slots, n_widths + 1, num_classes * (num_classes + 2), dtype=torch.int64, device=device)


def boundary_stats(pred: torch.Tensor, label: torch.Tensor, widths, num_classes: int, stats: torch.Tensor, oob: torch.Tensor,
                   cond: Optional[torch.Tensor] = None, ignore_index: int = 255) -> None:
    """Boundary-band counters of the uint8 prediction maps `pred` [B, H, W] against `label` [B, H, W] (uint8 or int64) for the band
    widths `widths`, accumulated into `stats` (new_boundary_stats; slot 0 + slot 1 + cond[b]); labelled pixels whose prediction
    value is >= C go to `oob` (int64 [1])."""
    w = boundary_widths(widths)
    if pred.dim() != 3 or pred.dtype != torch.uint8:
        raise ValueError(f"boundary_stats: pred is uint8 [B, H, W], got {pred.dtype} {tuple(pred.shape)}")
    if label.dtype not in (torch.uint8, torch.int64) or tuple(label.shape) != tuple(pred.shape):
        raise ValueError(f"boundary_stats: label is uint8 or int64 {tuple(pred.shape)}, got {label.dtype} {tuple(label.shape)}")
    if pred.numel() < 1:
        raise ValueError(f"boundary_stats: empty maps {tuple(pred.shape)}")
    if not 1 <= int(num_classes) <= N.MAX_CLASSES:
        raise ValueError(f"boundary_stats: 1 .. {N.MAX_CLASSES} classes, got {num_classes}")
    if stats.dim() != 3 or stats.dtype != torch.int64 or tuple(stats.shape[1:]) != (w.size + 1, num_classes * (num_classes + 2)):
        raise ValueError(f"stats must be int64 [slots, {w.size + 1}, {num_classes * (num_classes + 2)}] (new_boundary_stats), got "
                         f"{stats.dtype} {tuple(stats.shape)}")
    if oob.dtype != torch.int64 or oob.numel() != 1:
        raise ValueError("oob must be int64 [1]")
    b, H, W = pred.shape
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    pred, label = pred.contiguous(), label.contiguous()
    ws = N.workspace.get(pred.device, N.lib().awseg_boundary_workspace(b, int(num_classes), H, W, int(w.size)), tag="boundary")
    N.call("awseg_boundary_stats", N.ptr(pred), N.ptr(label), N.label_dtype(label), int(ignore_index), b, H, W, int(num_classes),
           N.host(w), int(w.size), N.ptr(cond), N.ptr(stats), stats.shape[0], N.ptr(oob), N.ptr(ws), N.stream())


def boundary_stats_to_numpy(stats, num_classes: int) -> dict:
    """int64 [slots, rings, C*C + 2 C] -> {'conf' [slots, rings, C, C] (rows: label, columns: prediction; ring of the label's edge
    distance), 'inter' [slots, rings, C] (label == prediction; ring of the larger distance), 'pr' [slots, rings, C] (ring of the
    prediction's distance)}."""
    raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
    c, c2 = num_classes, num_classes * num_classes
    if raw.shape[-1] != c2 + 2 * c:
        raise ValueError(f"boundary stats rows hold {c}^2 + 2 x {c} counters, got {raw.shape[-1]}")
    return {"conf": raw[..., :c2].reshape(raw.shape[:-1] + (c, c)), "inter": raw[..., c2:c2 + c], "pr": raw[..., c2 + c:]}


# ----------------------------------------------------------------------------- segment-level counters (include/awseg.h)
SEGMENT_BUCKETS = 11                   # AWSEG_SEGMENT_BUCKETS
SEGMENT_CELLS = 48                     # AWSEG_SEGMENT_CELLS


def new_segment_stats(num_classes: int, device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, C, 11, 48]: per slot, class and size bucket (bucket k: area in [4^k, 4^(k+1)), the last from 2^20) the cells
    cov * 7 + rc of the label segments (42) and 42 + cov of the prediction segments (6) of include/awseg.h (zeroed: the launches
    accumulate).  Replaces nothing in the reference, which counts pixels only."""
    if n_slots < 1 or not 1 <= int(num_classes) <= N.MAX_CLASSES:
        raise ValueError(f"new_segment_stats: n_slots >= 1 and 1 .. {N.MAX_CLASSES} classes, got {n_slots}, {num_classes}")
    return torch.zeros(n_slots, int(num_classes), SEGMENT_BUCKETS, SEGMENT_CELLS, dtype=torch.int64, device=device)


def segment_stats(pred: torch.Tensor, label: torch.Tensor, num_classes: int, stats: torch.Tensor, oob: torch.Tensor,
                  cond: Optional[torch.Tensor] = None, ref_maps: Optional[torch.Tensor] = None,
                  frame_ref: Optional[torch.Tensor] = None, label_ids: Optional[torch.Tensor] = None,
                  pred_ids: Optional[torch.Tensor] = None, ignore_index: int = 255) -> None:
    """Segment-level counters of the uint8 prediction maps `pred` [B, H, W] against `label` [B, H, W] (uint8 or int64): every
    8-connected label segment and prediction segment adds 1 to its (class, size bucket, coverage cell) of `stats`
    (new_segment_stats; slot 0 + slot 1 + cond[b]).  ref_maps uint8 [R, H, W] with frame_ref int32 [B] (< 0: no reference): the
    clean twins' maps, for the rc half of the label cells.  label_ids / pred_ids int32 [B, H, W]: receive the canonical segment id
    of every pixel (-1: in no segment).  Live pixels whose prediction or reference value is >= C go to `oob` (int64 [1])."""
    if pred.dim() != 3 or pred.dtype != torch.uint8:
        raise ValueError(f"segment_stats: pred is uint8 [B, H, W], got {pred.dtype} {tuple(pred.shape)}")
    if label.dtype not in (torch.uint8, torch.int64) or tuple(label.shape) != tuple(pred.shape):
        raise ValueError(f"segment_stats: label is uint8 or int64 {tuple(pred.shape)}, got {label.dtype} {tuple(label.shape)}")
    if pred.numel() < 1:
        raise ValueError(f"segment_stats: empty maps {tuple(pred.shape)}")
    if not 1 <= int(num_classes) <= N.MAX_CLASSES:
        raise ValueError(f"segment_stats: 1 .. {N.MAX_CLASSES} classes, got {num_classes}")
    if stats.dim() != 4 or stats.dtype != torch.int64 or tuple(stats.shape[1:]) != (int(num_classes), SEGMENT_BUCKETS, SEGMENT_CELLS):
        raise ValueError(f"stats must be int64 [slots, {num_classes}, {SEGMENT_BUCKETS}, {SEGMENT_CELLS}] (new_segment_stats), got "
                         f"{stats.dtype} {tuple(stats.shape)}")
    if oob.dtype != torch.int64 or oob.numel() != 1:
        raise ValueError("oob must be int64 [1]")
    b, H, W = pred.shape
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    if (ref_maps is None) != (frame_ref is None):
        raise ValueError("segment_stats: ref_maps and frame_ref come together")
    n_refs = 0
    if ref_maps is not None:
        if ref_maps.dim() != 3 or ref_maps.dtype != torch.uint8 or tuple(ref_maps.shape[1:]) != (H, W) or ref_maps.shape[0] < 1:
            raise ValueError(f"segment_stats: ref_maps is uint8 [R, {H}, {W}], got {ref_maps.dtype} {tuple(ref_maps.shape)}")
        if frame_ref.dtype != torch.int32 or frame_ref.numel() != b:
            raise ValueError("frame_ref must be int32 [B]")
        n_refs = int(ref_maps.shape[0])
    for name, ids in (("label_ids", label_ids), ("pred_ids", pred_ids)):
        if ids is not None and (ids.dtype != torch.int32 or tuple(ids.shape) != tuple(pred.shape) or not ids.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 {tuple(pred.shape)}")
    pred, label = pred.contiguous(), label.contiguous()
    if ref_maps is not None:
        ref_maps = ref_maps.contiguous()
    ws = N.workspace.get(pred.device, N.lib().awseg_segment_workspace(b, H, W), tag="segments")
    N.call("awseg_segment_stats", N.ptr(pred), N.ptr(label), N.label_dtype(label), int(ignore_index), b, H, W, int(num_classes),
           N.ptr(ref_maps), n_refs, N.ptr(frame_ref), N.ptr(cond), N.ptr(stats), stats.shape[0], N.ptr(oob), N.ptr(label_ids),
           N.ptr(pred_ids), N.ptr(ws), N.stream())


# ----------------------------------------------------------------------------- frame bootstrap (include/awseg.h)
BOOTSTRAP_STAGED_DRAWS = 4096          # AWSEG_BOOTSTRAP_STAGED_DRAWS
BOOTSTRAP_CHUNK_BYTES = 64 << 20       # replicate rows asked for per launch: bootstrap_counts splits R so that a chunk stays below this


def new_frame_counts(n_rows: int, num_classes: int, device) -> torch.Tensor:
    """int64 [n_rows, 3 C]: one row C intersection | C label count | C prediction count per frame (zeroed: the launches accumulate).
    Replaces nothing in the reference, which keeps no per-frame statistics."""
    if n_rows < 1 or not 1 <= int(num_classes) <= N.MAX_CLASSES:
        raise ValueError(f"new_frame_counts: n_rows >= 1 and 1 .. {N.MAX_CLASSES} classes, got {n_rows}, {num_classes}")
    return torch.zeros(int(n_rows), 3 * int(num_classes), dtype=torch.int64, device=device)


def frame_iou_counts(pred: torch.Tensor, label: torch.Tensor, num_classes: int, frame_row: torch.Tensor, table: torch.Tensor,
                     oob: torch.Tensor, ignore_index: int = 255) -> None:
    """Per-frame IoU counters of the uint8 prediction maps `pred` [B, ...] against `label` [B, ...] (uint8 or int64): frame b adds
    into row `frame_row[b]` (device int32 [B]; < 0 skips the frame) of `table` (new_frame_counts, viewed as [rows, 3 C]).  Prediction
    values >= C, labels outside [0, C) other than ignore_index and frames whose row the table lacks go to `oob` (int64 [1])."""
    if pred.dim() < 2 or pred.dtype != torch.uint8:
        raise ValueError(f"frame_iou_counts: pred is uint8 [B, ...], got {pred.dtype} {tuple(pred.shape)}")
    if label.dtype not in (torch.uint8, torch.int64) or label.numel() != pred.numel() or label.shape[0] != pred.shape[0]:
        raise ValueError(f"frame_iou_counts: label is uint8 or int64 with pred's {tuple(pred.shape)} elements, got {label.dtype} "
                         f"{tuple(label.shape)}")
    if pred.numel() < 1:
        raise ValueError(f"frame_iou_counts: empty maps {tuple(pred.shape)}")
    if not 1 <= int(num_classes) <= N.MAX_CLASSES:
        raise ValueError(f"frame_iou_counts: 1 .. {N.MAX_CLASSES} classes, got {num_classes}")
    b = pred.shape[0]
    hw = pred[0].numel()
    if frame_row.dtype != torch.int32 or frame_row.numel() != b:
        raise ValueError("frame_row must be int32 [B]")
    if table.dtype != torch.int64 or table.dim() < 2 or table.shape[-1] != 3 * int(num_classes) or table.numel() < 1:
        raise ValueError(f"table must be int64 [..., {3 * int(num_classes)}] (new_frame_counts), got {table.dtype} {tuple(table.shape)}")
    if oob.dtype != torch.int64 or oob.numel() != 1:
        raise ValueError("oob must be int64 [1]")
    pred, label = pred.contiguous(), label.contiguous()
    ws = N.workspace.get(pred.device, N.lib().awseg_frame_iou_workspace(b, int(num_classes), hw), tag="frame_iou")
    N.call("awseg_frame_iou_counts", N.ptr(pred), N.ptr(label), N.label_dtype(label), int(ignore_index), b, hw, int(num_classes),
           N.ptr(frame_row), N.ptr(table), table.numel() // table.shape[-1], N.ptr(oob), N.ptr(ws), N.stream())


def bootstrap_counts(table: torch.Tensor, slots: torch.Tensor, n_slots: int, seed: int, replicates: int, oob: torch.Tensor,
                     r0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Replicate sums of a paired bootstrap over sources: `table` int64 [n, V, W] (the per-frame rows of n sources x V variants),
    `slots` int32 [n, V] (0: no such frame, s >= 1: the frame's counter slot) -> int64 [replicates, n_slots, W], row r the sum over
    the n draws of replicate r0 + r of the drawn sources' frames, into slot 0 and their own slot.  The draw rule is in
    include/awseg.h; rows depend on (seed, replicate index, table, slots) only, so the launches this splits large requests into give
    what one would.  Slot values outside [0, n_slots) are skipped and counted into `oob` (int64 [1]) once per launch."""
    if table.dim() != 3 or table.dtype != torch.int64 or table.numel() < 1:
        raise ValueError(f"bootstrap_counts: table is int64 [n, V, W], got {table.dtype} {tuple(table.shape)}")
    n, v, w = (int(d) for d in table.shape)
    if slots.dtype != torch.int32 or tuple(slots.shape) != (n, v):
        raise ValueError(f"bootstrap_counts: slots is int32 [{n}, {v}], got {slots.dtype} {tuple(slots.shape)}")
    for name, val, lo, hi in (("n_slots", n_slots, 1, 2 ** 31 - 1), ("seed", seed, 0, 2 ** 64 - 1), ("replicates", replicates, 1, 2 ** 31 - 1),
                              ("r0", r0, 0, 2 ** 62)):
        if isinstance(val, (bool, np.bool_)) or not isinstance(val, (int, np.integer)) or not lo <= int(val) <= hi:
            raise ValueError(f"bootstrap_counts: {name} is an integer in [{lo}, {hi}], got {val!r}")
    if oob.dtype != torch.int64 or oob.numel() != 1:
        raise ValueError("oob must be int64 [1]")
    n_slots, replicates, r0 = int(n_slots), int(replicates), int(r0)
    if out is None:
        out = torch.empty(replicates, n_slots, w, dtype=torch.int64, device=table.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (replicates, n_slots, w) or not out.is_contiguous():
        raise ValueError(f"bootstrap_counts: out is contiguous int64 [{replicates}, {n_slots}, {w}]")
    table, slots = table.contiguous(), slots.contiguous()
    step = max(1, BOOTSTRAP_CHUNK_BYTES // (n_slots * w * 8))
    for a in range(0, replicates, step):
        m = min(step, replicates - a)
        N.call("awseg_bootstrap_counts", N.ptr(table), N.ptr(slots), n, v, w, n_slots, int(seed), r0 + a, m, N.ptr(out[a:a + m]),
               N.ptr(oob), N.stream())
    return out


def frame_counts_to_numpy(counts, num_classes: int) -> dict:
    """int64 [..., 3 C] (a table of per-frame rows or replicate sums) -> {'intersection', 'label', 'prediction'}, each [..., C]."""
    raw = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts, dtype=np.int64)
    c = int(num_classes)
    if raw.shape[-1] != 3 * c:
        raise ValueError(f"frame count rows hold 3 x {c} counters, got {raw.shape[-1]}")
    return {"intersection": raw[..., :c], "label": raw[..., c:2 * c], "prediction": raw[..., 2 * c:]}


# ----------------------------------------------------------------------------- change strata (include/awseg.h)
MAX_STRATA = 8                         # AWSEG_MAX_STRATA
STRATUM_NONE = 255                     # AWSEG_STRATUM_NONE: no measured change (NaN difference, no clean twin)
STRATA_SMALL = ("both_correct", "clean_correct_variant_wrong", "clean_wrong_variant_correct", "both_wrong", "agree", "pixels")
DEFAULT_CHANGE_EDGES = (0.5, 4.5, 16.5, 64.5)     # 8-bit grey levels; half integers: see change_edges


def change_edges(spec) -> np.ndarray:
    """The stratum edges as a host float32 array, checked before any launch (the C ABI refuses the same lists with AWSEG_EINVAL):
    1 .. MAX_STRATA - 1 finite numbers >= 0, strictly increasing (also after rounding to float32), or 'default' =
    DEFAULT_CHANGE_EDGES.  With the default scale the change of a frame rendered from 8-bit data lies within 3.1e-5 of an integer
    number of grey levels, so half-integer edges never sit on a rounding seam."""
    if isinstance(spec, str):
        if spec != "default":
            raise ValueError(f"stratum edges are a list of numbers or 'default', got {spec!r}")
        spec = DEFAULT_CHANGE_EDGES
    if isinstance(spec, (bool, np.bool_, bytes, dict, int, float, np.number)):
        raise ValueError(f"stratum edges are a list of numbers, got {spec!r}")
    e = list(spec)
    if any(isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in e):
        raise ValueError(f"stratum edges are numbers, got {spec!r}")
    if not 1 <= len(e) <= MAX_STRATA - 1:
        raise ValueError(f"1 .. {MAX_STRATA - 1} stratum edges, got {len(e)}")
    with np.errstate(over="ignore"):
        out = np.ascontiguousarray(e, dtype=np.float32)
    if not np.isfinite(out).all() or (out < 0).any() or (np.diff(out) <= 0).any():
        raise ValueError(f"stratum edges must be finite, >= 0 and strictly increasing, got {e}")
    return out


def change_strata(image: torch.Tensor, ref_images: torch.Tensor, frame_ref: torch.Tensor, edges, out: Optional[torch.Tensor] = None,
                  scale=None, oob: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B, ...] stratum map of the float32 frames `image` [B, Ch, ...] against rows `frame_ref` (device int32 [B]; < 0: no
    twin, the frame's map is STRATUM_NONE) of the clean frames `ref_images` [R, Ch, ...]: per pixel the number of `edges` at or
    below max_c |image - ref| * scale[c].  `scale` defaults to 255 * IMAGENET_STD (Ch = 3): the change in 8-bit grey levels of a
    frame the loader normalised.  A row index outside `ref_images` adds the frame's pixels to `oob` (int64 [1])."""
    e = change_edges(edges)
    if image.dim() < 3 or image.dtype != torch.float32 or ref_images.dtype != torch.float32 or ref_images.dim() < 1:
        raise ValueError(f"change_strata: image is float32 [B, Ch, ...], got {image.dtype} {tuple(image.shape)}")
    b, ch = image.shape[0], image.shape[1]
    hw = int(np.prod(image.shape[2:]))
    if not 1 <= ch <= 4 or hw < 1:
        raise ValueError(f"change_strata: 1 .. 4 channels and at least one pixel, got {tuple(image.shape)}")
    r = ref_images.shape[0]
    if r < 1 or ref_images[0].numel() != ch * hw:
        raise ValueError(f"change_strata: ref_images holds rows of {ch} x {hw} float32, got {tuple(ref_images.shape)}")
    if frame_ref.dtype != torch.int32 or frame_ref.numel() != b:
        raise ValueError("frame_ref must be int32 [B]")
    if scale is None:
        if ch != 3:
            raise ValueError("change_strata: the default scale (255 * IMAGENET_STD) is for three channels")
        scale = 255.0 * IMAGENET_STD
    sc = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
    if sc.size != ch or not np.isfinite(sc).all() or (sc <= 0).any():
        raise ValueError(f"change_strata: scale holds {ch} finite numbers > 0, got {scale!r}")
    if out is None:
        out = torch.empty((b,) + tuple(image.shape[2:]), dtype=torch.uint8, device=image.device)
    if out.dtype != torch.uint8 or out.numel() != b * hw:
        raise ValueError(f"out must be uint8 with {b} x {hw} elements")
    if oob is None:
        oob = torch.zeros(1, dtype=torch.int64, device=image.device)
    if oob.dtype != torch.int64 or oob.numel() != 1:
        raise ValueError("oob must be int64 [1]")
    image, ref_images = image.contiguous(), ref_images.contiguous()
    N.call("awseg_change_strata", N.ptr(image), N.ptr(ref_images), r, b, ch, hw, N.ptr(frame_ref), N.host(sc), N.host(e), int(e.size) + 1,
           N.ptr(out), N.ptr(oob), N.stream())
    return out


def new_strata_stats(num_classes: int, n_strata: int, device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, n_strata + 1, C*C + 6]: per slot and stratum (row n_strata: unmeasured pixels) the row C*C conf | 4 paired
    cells | agree | pixels of include/awseg.h (zeroed: the launches accumulate)."""
    return torch.zeros(n_slots, n_strata + 1, num_classes * num_classes + 6, dtype=torch.int64, device=device)


def stratified_stats(pred: torch.Tensor, label: torch.Tensor, stratum: torch.Tensor, n_strata: int, num_classes: int,
                     stats: torch.Tensor, oob: torch.Tensor, ref_maps: Optional[torch.Tensor] = None,
                     frame_ref: Optional[torch.Tensor] = None, cond: Optional[torch.Tensor] = None, ignore_index: int = 255) -> None:
    """Count the uint8 prediction maps `pred` [B, ...] against `label` (uint8 or int64) and, when given, rows `frame_ref` (device
    int32 [B], < 0 skips a frame) of the clean maps `ref_maps` [R, ...], split by the uint8 map `stratum` [B, ...] (values >=
    n_strata: the unmeasured row), into `stats` (new_strata_stats; slot 0 + slot 1 + cond[b]); map values >= C go to `oob`."""
    k, c = int(n_strata), int(num_classes)
    if not 1 <= k <= MAX_STRATA:
        raise ValueError(f"stratified_stats: 1 .. {MAX_STRATA} strata, got {n_strata}")
    if not 1 <= c <= N.MAX_CLASSES:
        raise ValueError(f"stratified_stats: 1 .. {N.MAX_CLASSES} classes, got {num_classes}")
    if pred.dtype != torch.uint8 or stratum.dtype != torch.uint8 or pred.dim() < 1 or pred.numel() < 1:
        raise ValueError("stratified_stats: pred and stratum are non-empty uint8 maps [B, ...]")
    b = pred.shape[0]
    hw = pred[0].numel()
    if stratum.numel() != b * hw or label.numel() != b * hw or label.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"stratified_stats: stratum uint8 and label uint8 / int64 with {b} x {hw} elements")
    if (ref_maps is None) != (frame_ref is None):
        raise ValueError("stratified_stats: ref_maps and frame_ref come together")
    r = 0
    if ref_maps is not None:
        r = ref_maps.shape[0]
        if ref_maps.dtype != torch.uint8 or r < 1 or ref_maps[0].numel() != hw or frame_ref.dtype != torch.int32 or frame_ref.numel() != b:
            raise ValueError("stratified_stats: ref_maps uint8 [R, HW], frame_ref int32 [B]")
        ref_maps = ref_maps.contiguous()
    if stats.dim() != 3 or stats.dtype != torch.int64 or tuple(stats.shape[1:]) != (k + 1, c * c + 6):
        raise ValueError(f"stats must be int64 [slots, {k + 1}, {c * c + 6}] (new_strata_stats), got {stats.dtype} {tuple(stats.shape)}")
    if oob.dtype != torch.int64 or oob.numel() != 1:
        raise ValueError("oob must be int64 [1]")
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    pred, label, stratum = pred.contiguous(), label.contiguous(), stratum.contiguous()
    ws = N.workspace.get(pred.device, N.lib().awseg_strata_workspace(b, c, hw, k), tag="strata")
    N.call("awseg_stratified_stats", N.ptr(pred), N.ptr(label), N.label_dtype(label), int(ignore_index), N.ptr(stratum), k,
           N.ptr(ref_maps), r, N.ptr(frame_ref), b, hw, c, N.ptr(cond), N.ptr(stats), stats.shape[0], N.ptr(oob), N.ptr(ws), N.stream())


def strata_stats_to_numpy(stats, num_classes: int) -> dict:
    """int64 [..., strata + 1, C*C + 6] -> {'conf' [..., strata + 1, C, C] (rows: label, columns: prediction), 'transitions'
    [..., strata + 1, 4] (both correct, clean correct + variant wrong, clean wrong + variant correct, both wrong), 'agree' and
    'pixels' [..., strata + 1]}; the last stratum row holds the unmeasured pixels."""
    raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
    c, c2 = num_classes, num_classes * num_classes
    if raw.shape[-1] != c2 + 6:
        raise ValueError(f"strata stats rows hold {c}^2 + 6 counters, got {raw.shape[-1]}")
    return {"conf": raw[..., :c2].reshape(raw.shape[:-1] + (c, c)), "transitions": raw[..., c2:c2 + 4], "agree": raw[..., c2 + 4],
            "pixels": raw[..., c2 + 5]}


# ----------------------------------------------------------------------------- image quality (include/awseg.h)
IQ_FIELDS = ("frames", "error_terms", "sum_abs", "sum_sq", "error_terms_unmeasured", "windows", "sum_luminance", "sum_contrast",
             "sum_ssim", "windows_unmeasured")
IQ_ROW = len(IQ_FIELDS)                # AWSEG_IQ_ROW
IQ_UNIT = 2.0 ** -24                   # the sums are int64 in fixed point: exact, order-independent
IQ_TERM_BUDGET = 1 << 36               # AWSEG_IQ_TERM_BUDGET: pixel-channels one stats tensor holds, summed over ranks (x 2^26 < 2^63)
IQ_TILE_H, IQ_TILE_W = 32, 64          # AWSEG_IQ_TILE_H, AWSEG_IQ_TILE_W: window centres per block
IQ_TAPS = 11


def ssim_taps() -> np.ndarray:
    """The 11 float32 weights of the SSIM window of Wang et al. 2004: a Gaussian of sigma 1.5 over 11 pixels, normalised."""
    return np.ascontiguousarray(gaussian_taps(1.5, 3.5), dtype=np.float32)


def new_image_quality_stats(device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, IQ_ROW]: per slot the row IQ_FIELDS of include/awseg.h (zeroed: the launches accumulate)."""
    if isinstance(n_slots, (bool, np.bool_)) or not isinstance(n_slots, (int, np.integer)) or n_slots < 1:
        raise ValueError(f"new_image_quality_stats: n_slots is an integer >= 1, got {n_slots!r}")
    return torch.zeros(int(n_slots), IQ_ROW, dtype=torch.int64, device=device)


def _iq_positive(name: str, v) -> float:
    if isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"image_quality: {name} is a finite number > 0, got {v!r}")
    with np.errstate(over="ignore"):
        f = float(np.float32(v))
    if not (np.isfinite(f) and f > 0):
        raise ValueError(f"image_quality: {name} is a finite number > 0 (also as float32), got {v!r}")
    return f


def image_quality(image: torch.Tensor, ref_images: torch.Tensor, frame_ref: torch.Tensor, stats: torch.Tensor,
                  cond: Optional[torch.Tensor] = None, oob: Optional[torch.Tensor] = None, mean=None, std=None,
                  c1: float = 1e-4, c2: float = 9e-4, taps=None) -> None:
    """Image-quality counters of the float32 frames `image` [B, Ch, H, W] against rows `frame_ref` (device int32 [B]; < 0: no twin,
    the frame is skipped) of the clean frames `ref_images` [R, Ch, H, W], into `stats` (new_image_quality_stats; slot 0 + slot
    1 + cond[b]): the error terms of MSE / PSNR at every pixel and the luminance, contrast-structure and SSIM terms of every whole
    11 x 11 window, as include/awseg.h defines them.  `mean`, `std`: the loader's normalisation (default: ImageNet's, Ch = 3), so
    that image * std + mean lies in [0, 1]; c1, c2: the SSIM constants for that range ((0.01)^2, (0.03)^2); `taps`: the window
    (default ssim_taps()).  A row index outside `ref_images` adds the frame's pixels to `oob` (int64 [1])."""
    if image.dim() != 4 or image.dtype != torch.float32:
        raise ValueError(f"image_quality: image is float32 [B, Ch, H, W], got {image.dtype} {tuple(image.shape)}")
    b, ch, h, w = (int(d) for d in image.shape)
    if not 1 <= ch <= 4 or h < 1 or w < 1:
        raise ValueError(f"image_quality: 1 .. 4 channels and at least one pixel, got {tuple(image.shape)}")
    if ref_images.dim() != 4 or ref_images.dtype != torch.float32 or ref_images.shape[0] < 1:
        raise ValueError(f"image_quality: ref_images is float32 [R, Ch, H, W] with R >= 1, got {ref_images.dtype} {tuple(ref_images.shape)}")
    if tuple(ref_images.shape[1:]) != (ch, h, w):
        raise ValueError(f"image_quality: frames {(ch, h, w)} and twins {tuple(ref_images.shape[1:])} differ in size")
    if b > 65535 or h * w >= 2 ** 31:
        raise ValueError(f"image_quality: at most 65535 frames of fewer than 2^31 pixels per launch, got {tuple(image.shape)}")
    r = int(ref_images.shape[0])
    if frame_ref.dtype != torch.int32 or frame_ref.numel() != b:
        raise ValueError("frame_ref must be int32 [B]")
    if mean is None and std is None and ch != 3:
        raise ValueError("image_quality: the default normalisation (ImageNet mean and std) is for three channels")
    if (mean is None) != (std is None):
        raise ValueError("image_quality: mean and std come together")
    m, s = _mean_std(mean, std)
    m, s = m.reshape(-1), s.reshape(-1)
    if m.size != ch or s.size != ch or not np.isfinite(m).all() or not np.isfinite(s).all() or (s <= 0).any():
        raise ValueError(f"image_quality: mean holds {ch} finite numbers and std {ch} finite numbers > 0, got {mean!r}, {std!r}")
    t = np.ascontiguousarray(ssim_taps() if taps is None else taps, dtype=np.float32).reshape(-1)
    if t.size != IQ_TAPS or not np.isfinite(t).all():
        raise ValueError(f"image_quality: taps holds {IQ_TAPS} finite numbers, got {taps!r}")
    c1, c2 = _iq_positive("c1", c1), _iq_positive("c2", c2)
    if stats.dim() != 2 or stats.dtype != torch.int64 or stats.shape[0] < 1 or stats.shape[1] != IQ_ROW:
        raise ValueError(f"stats must be int64 [slots, {IQ_ROW}] (new_image_quality_stats), got {stats.dtype} {tuple(stats.shape)}")
    if oob is None:
        oob = torch.zeros(1, dtype=torch.int64, device=image.device)
    if oob.dtype != torch.int64 or oob.numel() != 1:
        raise ValueError("oob must be int64 [1]")
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    if b == 0:
        return
    image, ref_images = image.contiguous(), ref_images.contiguous()
    ws = N.workspace.get(image.device, N.lib().awseg_image_quality_workspace(b, ch, h, w), tag="image_quality")
    N.call("awseg_image_quality", N.ptr(image), N.ptr(ref_images), r, b, ch, h, w, N.ptr(frame_ref), N.host(m), N.host(s), N.host(t),
           c1, c2, N.ptr(cond), N.ptr(stats), stats.shape[0], N.ptr(oob), N.ptr(ws), N.stream())


def image_quality_to_numpy(stats) -> dict:
    """int64 [..., IQ_ROW] -> {field: int64 [...]} for IQ_FIELDS; the four sums stay in units of IQ_UNIT (exact integers)."""
    raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
    if raw.shape[-1] != IQ_ROW:
        raise ValueError(f"image quality rows hold {IQ_ROW} counters, got {raw.shape[-1]}")
    return {f: raw[..., i] for i, f in enumerate(IQ_FIELDS)}


# ----------------------------------------------------------------------------- dehazing (include/awseg_restore.h)
DEHAZE_FIELDS = ("frames", "sum_airlight_0", "sum_airlight_1", "sum_airlight_2", "pixels", "sum_transmission", "nonfinite_values",
                 "airlight_floored_frames")
DEHAZE_ROW = len(DEHAZE_FIELDS)        # AWSEG_DEHAZE_ROW
DEHAZE_UNIT = 2.0 ** -16               # the airlight and transmission sums are int64 in fixed point: exact, order-independent
DEHAZE_TILE_H, DEHAZE_TILE_W = 32, 64  # AWSEG_DEHAZE_TILE_H, AWSEG_DEHAZE_TILE_W: pixels per block
DEHAZE_MAX_RADIUS = 15                 # AWSEG_DEHAZE_MAX_RADIUS
DEHAZE_FRAME_RECORD = 1064             # AWSEG_DEHAZE_FRAME_RECORD: workspace bytes per frame beside its H * W bins
DEHAZE_DEFAULTS = {"radius": 7, "omega": 0.95, "t_min": 0.1, "airlight_min": 0.1, "refine": 1}


def _stats_rows(name: str, fields, units: str = ""):
    """-> (new_<name>_stats, <name>_stats_to_numpy) for the counter row `fields` of include/awseg_restore.h; `units`: what the
    docstrings say about the row's fixed-point sums."""
    row, upper = len(fields), name.upper()

    def new_stats(device, n_slots: int = 1) -> torch.Tensor:
        if isinstance(n_slots, (bool, np.bool_)) or not isinstance(n_slots, (int, np.integer)) or n_slots < 1:
            raise ValueError(f"new_{name}_stats: n_slots is an integer >= 1, got {n_slots!r}")
        return torch.zeros(int(n_slots), row, dtype=torch.int64, device=device)

    def stats_to_numpy(stats) -> dict:
        raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
        if raw.shape[-1] != row:
            raise ValueError(f"{name} rows hold {row} counters, got {raw.shape[-1]}")
        return {f: raw[..., i] for i, f in enumerate(fields)}

    new_stats.__name__ = new_stats.__qualname__ = f"new_{name}_stats"
    new_stats.__doc__ = (f"int64 [n_slots, {upper}_ROW]: per slot the row {upper}_FIELDS of include/awseg_restore.h (zeroed: the launches "
                         f"accumulate){units and '; ' + units}.")
    stats_to_numpy.__name__ = stats_to_numpy.__qualname__ = f"{name}_stats_to_numpy"
    stats_to_numpy.__doc__ = f"int64 [..., {upper}_ROW] -> {{field: int64 [...]}} for {upper}_FIELDS{units and '; ' + units}."
    return new_stats, stats_to_numpy


def _integer(who: str, name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{who}: {name} is an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def _number(who: str, name: str, v, lo: float, hi: float, open_below: bool = False, open_above: bool = False) -> float:
    """v as float32, in the interval from lo to hi (NaN is refused)."""
    ok = not isinstance(v, (bool, np.bool_, str, bytes)) and isinstance(v, (int, float, np.integer, np.floating))
    f = float(np.float32(v)) if ok else float("nan")
    if not (ok and (lo < f if open_below else lo <= f) and (f < hi if open_above else f <= hi)):
        raise ValueError(f"{who}: {name} is a number in {'(' if open_below else '['}{lo:g}, {hi:g}{')' if open_above else ']'} "
                         f"(also as float32), got {v!r}")
    return f


new_dehaze_stats, dehaze_stats_to_numpy = _stats_rows("dehaze", DEHAZE_FIELDS, "the four sums are in units of DEHAZE_UNIT")


def dehaze_parameters(radius=7, omega=0.95, t_min=0.1, airlight_min=0.1, refine=1) -> dict:
    """The checked parameters of dehaze(): radius an integer in [1, 15]; omega, t_min, airlight_min numbers in (0, 1] (also as
    float32); refine 0 or 1.  ValueError otherwise."""
    unit = lambda name, v: _number("dehaze", name, v, 0.0, 1.0, open_below=True)      # noqa: E731
    return {"radius": _integer("dehaze", "radius", radius, 1, DEHAZE_MAX_RADIUS), "omega": unit("omega", omega),
            "t_min": unit("t_min", t_min), "airlight_min": unit("airlight_min", airlight_min),
            "refine": _integer("dehaze", "refine", refine, 0, 1)}


def _restore_frames(who: str, image, stats, cond, mean, std, row: int, new_stats):
    """The checks of the frames, the normalisation, the counters and the conditions that every restoration entry point makes ->
    (contiguous image, B, H, W, mean, std, stats).  `row`, `new_stats`: the width of a counter row and what makes one."""
    if image.dim() != 4 or image.dtype != torch.float32 or image.shape[1] != 3:
        raise ValueError(f"{who}: image is float32 [B, 3, H, W], got {image.dtype} {tuple(image.shape)}")
    b, _, h, w = (int(d) for d in image.shape)
    if h < 1 or w < 1:
        raise ValueError(f"{who}: frames of at least one pixel, got {tuple(image.shape)}")
    if b > 65535 or h * w >= 2 ** 31:
        raise ValueError(f"{who}: at most 65535 frames of fewer than 2^31 pixels per launch, got {tuple(image.shape)}")
    if (mean is None) != (std is None):
        raise ValueError(f"{who}: mean and std come together")
    m, s = _mean_std(mean, std)
    m, s = m.reshape(-1), s.reshape(-1)
    if m.size != 3 or s.size != 3 or not np.isfinite(m).all() or not np.isfinite(s).all() or (s <= 0).any():
        raise ValueError(f"{who}: mean holds 3 finite numbers and std 3 finite numbers > 0, got {mean!r}, {std!r}")
    if stats is None:
        stats = new_stats(image.device, 1)
    if stats.dim() != 2 or stats.dtype != torch.int64 or stats.shape[0] < 1 or stats.shape[1] != row:
        raise ValueError(f"stats must be int64 [slots, {row}] ({new_stats.__name__}), got {stats.dtype} {tuple(stats.shape)}")
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    return image.contiguous(), b, h, w, m, s, stats


def _restore_outputs(who: str, image, out):
    """-> (`out` checked, or new frames like `image`; a new float32 [B, 3] for the per-frame side output)."""
    if out is None:
        out = torch.empty_like(image)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(image.shape) or not out.is_contiguous():
        raise ValueError(f"{who}: out is a contiguous float32 tensor of the frames' shape, got {out.dtype} {tuple(out.shape)}")
    if image.shape[0] and out.data_ptr() == image.data_ptr():
        raise ValueError(f"{who}: out must not be the input (a block reads its neighbours' pixels)")
    return out, torch.empty(image.shape[0], 3, dtype=torch.float32, device=image.device)


def dehaze(image: torch.Tensor, stats: Optional[torch.Tensor] = None, cond: Optional[torch.Tensor] = None, *, radius: int = 7,
           omega: float = 0.95, t_min: float = 0.1, airlight_min: float = 0.1, refine: int = 1, mean=None, std=None,
           out: Optional[torch.Tensor] = None):
    """Dark-channel-prior dehazing (He, Sun, Tang 2009) of the loader's normalised float32 frames `image` [B, 3, H, W], as
    include/awseg_restore.h defines it step by step: -> (restored float32 [B, 3, H, W], airlight float32 [B, 3]).  `stats`
    (new_dehaze_stats; slot 0 + slot 1 + cond[b], cond device int32 [B]) takes the counters of DEHAZE_FIELDS; without it they go
    to a tensor nobody reads.  `refine` 1: the transmission comes from the morphological opening of the normalised dark channel,
    0: from He's patch minimum.  `mean`, `std`: the loader's normalisation (default: ImageNet's).  `out`: where the restored frames
    go (contiguous, not `image`)."""
    p = dehaze_parameters(radius, omega, t_min, airlight_min, refine)
    image, b, h, w, m, s, stats = _restore_frames("dehaze", image, stats, cond, mean, std, DEHAZE_ROW, new_dehaze_stats)
    out, airlight = _restore_outputs("dehaze", image, out)
    if b == 0:
        return out, airlight
    ws = N.workspace.get(image.device, N.lib().awseg_dehaze_workspace(b, h, w), tag="dehaze")
    N.call("awseg_dehaze", N.ptr(image), b, 3, h, w, N.host(m), N.host(s), p["radius"], p["omega"], p["t_min"], p["airlight_min"],
           p["refine"], N.ptr(cond), N.ptr(out), N.ptr(airlight), N.ptr(stats), stats.shape[0], N.ptr(ws), N.stream())
    return out, airlight


# ------------------------------------------------ guided-filter transmission (include/awseg_restore.h)
GUIDED_FIELDS = ("above_one_pixels", "below_floor_pixels", "sum_transmission_moved", "pixels")
GUIDED_ROW = len(GUIDED_FIELDS)        # AWSEG_GUIDED_ROW
GUIDED_MAX_RADIUS = 32                 # AWSEG_GUIDED_MAX_RADIUS
GUIDED_EPS_RANGE = (1e-4, 1.0)         # as float32: what the launcher accepts
GUIDED_DEFAULT_EPS = 1e-3
new_guided_stats, guided_stats_to_numpy = _stats_rows("guided", GUIDED_FIELDS, "sum_transmission_moved is in units of DEHAZE_UNIT")


def default_guided_radius(radius: int) -> int:
    return min(4 * int(radius), GUIDED_MAX_RADIUS)


def dehaze_guided_parameters(radius=7, omega=0.95, t_min=0.1, airlight_min=0.1, guided_radius=None, guided_eps=GUIDED_DEFAULT_EPS) -> dict:
    """The checked parameters of dehaze_guided(): those of dehaze_parameters (without refine); guided_radius an integer in [1, 32]
    (None: min(4 radius, 32)); guided_eps a number in [1e-4, 1] as float32.  ValueError otherwise."""
    p = dehaze_parameters(radius, omega, t_min, airlight_min, 0)
    del p["refine"]
    if guided_radius is None:
        guided_radius = default_guided_radius(p["radius"])
    p["guided_radius"] = _integer("dehaze_guided", "guided_radius", guided_radius, 1, GUIDED_MAX_RADIUS)
    ok = not isinstance(guided_eps, (bool, np.bool_, str, bytes)) and isinstance(guided_eps, (int, float, np.integer, np.floating))
    eps = float(np.float32(guided_eps)) if ok else 0.0
    if not (ok and float(np.float32(GUIDED_EPS_RANGE[0])) <= eps <= GUIDED_EPS_RANGE[1]):
        raise ValueError(f"dehaze_guided: guided_eps is a number in [1e-4, 1] (also as float32), got {guided_eps!r}")
    p["guided_eps"] = eps                                              # the bound is float32(1e-4), the text 1e-4: not _number's
    return p


def dehaze_guided_workspace_bytes(b: int, h: int, w: int) -> int:
    """The closed form of awseg_dehaze_guided_workspace: the records and bin map of awseg_dehaze, then three float32 maps, every
    region rounded up to 8 bytes."""
    b, h, w = max(int(b), 1), max(int(h), 1), max(int(w), 1)
    ceil8 = lambda x: (x + 7) & ~7                                      # noqa: E731
    return ceil8(b * (DEHAZE_FRAME_RECORD + h * w)) + 3 * ceil8(4 * b * h * w)


def dehaze_guided(image: torch.Tensor, stats: Optional[torch.Tensor] = None, guided_stats: Optional[torch.Tensor] = None,
                  cond: Optional[torch.Tensor] = None, *, radius: int = 7, omega: float = 0.95, t_min: float = 0.1,
                  airlight_min: float = 0.1, guided_radius: Optional[int] = None, guided_eps: float = GUIDED_DEFAULT_EPS, mean=None,
                  std=None, out: Optional[torch.Tensor] = None, transmission: bool = False):
    """dehaze() with the guided-filter refinement of the transmission (He, Sun, Tang 2010/2013): the patch transmission filtered
    over (2 guided_radius + 1)^2 windows with the frame's luma as the guide, as include/awseg_restore.h defines it step by step
    -> (restored float32 [B, 3, H, W], airlight float32 [B, 3][, t float32 [B, H, W] when `transmission`]).  `stats` as for
    dehaze(); `guided_stats` (new_guided_stats, the same slots) takes the counters of GUIDED_FIELDS.  guided_radius None:
    min(4 radius, 32).  There is no CPU path."""
    p = dehaze_guided_parameters(radius, omega, t_min, airlight_min, guided_radius, guided_eps)
    image, b, h, w, m, s, stats = _restore_frames("dehaze_guided", image, stats, cond, mean, std, DEHAZE_ROW, new_dehaze_stats)
    out, airlight = _restore_outputs("dehaze_guided", image, out)
    if guided_stats is None:
        guided_stats = new_guided_stats(image.device, stats.shape[0])
    if guided_stats.dim() != 2 or guided_stats.dtype != torch.int64 or tuple(guided_stats.shape) != (stats.shape[0], GUIDED_ROW):
        raise ValueError(f"guided_stats must be int64 [{stats.shape[0]}, {GUIDED_ROW}] (new_guided_stats, the slots of stats), got "
                         f"{guided_stats.dtype} {tuple(guided_stats.shape)}")
    t = torch.empty(b, h, w, dtype=torch.float32, device=image.device) if transmission else None
    if b:
        ws = N.workspace.get(image.device, N.lib().awseg_dehaze_guided_workspace(b, h, w), tag="dehaze_guided")
        N.call("awseg_dehaze_guided", N.ptr(image), b, 3, h, w, N.host(m), N.host(s), p["radius"], p["omega"], p["t_min"],
               p["airlight_min"], p["guided_radius"], p["guided_eps"], N.ptr(cond), N.ptr(out), N.ptr(airlight), N.ptr(t), N.ptr(stats),
               N.ptr(guided_stats), stats.shape[0], N.ptr(ws), N.stream())
    return (out, airlight, t) if transmission else (out, airlight)


# ------------------------------------------------ night relighting: CLAHE + grey world (include/awseg_restore.h)
RELIGHT_FIELDS = ("frames", "sum_gain_0", "sum_gain_1", "sum_gain_2", "pixels", "sum_luma", "sum_luma_restored", "nonfinite_values",
                  "capped_pixels", "saturated_values")
RELIGHT_ROW = len(RELIGHT_FIELDS)      # AWSEG_RELIGHT_ROW
RELIGHT_MAX_TILES = 16                 # AWSEG_RELIGHT_MAX_TILES
RELIGHT_FRAME_RECORD = 48              # AWSEG_RELIGHT_FRAME_RECORD: workspace bytes per frame beside its tiles
RELIGHT_TILE_BYTES = 1536              # AWSEG_RELIGHT_TILE_BYTES: 256 uint32 histogram words and 256 uint16 table entries per tile
RELIGHT_RANGE = (1.0, 64.0)            # clip_limit and max_gain
RELIGHT_UNIT = 2.0 ** -16              # the gain and luma sums are int64 in fixed point: exact, order-independent
new_relight_stats, relight_stats_to_numpy = _stats_rows("relight", RELIGHT_FIELDS, "the gain and luma sums are in units of RELIGHT_UNIT")


def relight_parameters(grid=(8, 8), clip_limit=2.0, max_gain=8.0, white_balance=True) -> dict:
    """The checked parameters of relight(): grid an integer n (n x n tiles) or a pair (tiles_y, tiles_x) of integers in [1, 16];
    clip_limit, max_gain numbers in [1, 64] (also as float32); white_balance a bool (or 0 / 1).  ValueError otherwise.
    -> {'grid': (ty, tx), 'clip_limit', 'max_gain', 'white_balance': bool}."""
    def tile_count(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= RELIGHT_MAX_TILES:
            raise ValueError(f"relight: grid is an integer or a pair of integers in [1, {RELIGHT_MAX_TILES}], got {grid!r}")
        return int(v)

    if isinstance(grid, (list, tuple)):
        if len(grid) != 2:
            raise ValueError(f"relight: grid is an integer or a pair of integers in [1, {RELIGHT_MAX_TILES}], got {grid!r}")
        tiles = (tile_count(grid[0]), tile_count(grid[1]))
    else:
        tiles = (tile_count(grid),) * 2
    if not isinstance(white_balance, (bool, np.bool_)) and not (isinstance(white_balance, (int, np.integer)) and white_balance in (0, 1)):
        raise ValueError(f"relight: white_balance is a bool, got {white_balance!r}")
    return {"grid": tiles, "clip_limit": _number("relight", "clip_limit", clip_limit, *RELIGHT_RANGE),
            "max_gain": _number("relight", "max_gain", max_gain, *RELIGHT_RANGE), "white_balance": bool(white_balance)}


def relight_workspace_bytes(b: int, tiles_y: int, tiles_x: int) -> int:
    """The closed form of awseg_relight_workspace: per frame a record, and per tile a histogram and a table."""
    b, tiles_y, tiles_x = max(int(b), 1), max(int(tiles_y), 1), max(int(tiles_x), 1)
    return b * (RELIGHT_FRAME_RECORD + tiles_y * tiles_x * RELIGHT_TILE_BYTES)


def relight(image: torch.Tensor, stats: Optional[torch.Tensor] = None, cond: Optional[torch.Tensor] = None, *, grid=(8, 8),
            clip_limit: float = 2.0, max_gain: float = 8.0, white_balance=True, mean=None, std=None,
            out: Optional[torch.Tensor] = None):
    """Night relighting of the loader's normalised float32 frames `image` [B, 3, H, W]: contrast-limited adaptive histogram
    equalisation of the luma (CLAHE, Zuiderveld 1994) on a `grid` of tiles with a grey-world white balance, as
    include/awseg_restore.h defines it step by step -> (restored float32 [B, 3, H, W], gains float32 [B, 3]: the white-balance
    gains).  `stats` (new_relight_stats; slot 0 + slot 1 + cond[b], cond device int32 [B]) takes the counters of RELIGHT_FIELDS;
    without it they go to a tensor nobody reads.  `mean`, `std`: the loader's normalisation (default: ImageNet's).  `out`: where
    the restored frames go (contiguous, not `image`).  The grid may not have more tiles than the frame has rows or columns.  There
    is no CPU path."""
    p = relight_parameters(grid, clip_limit, max_gain, white_balance)
    image, b, h, w, m, s, stats = _restore_frames("relight", image, stats, cond, mean, std, RELIGHT_ROW, new_relight_stats)
    out, gains = _restore_outputs("relight", image, out)
    ty, tx = p["grid"]
    if ty > h or tx > w:
        raise ValueError(f"relight: a grid of {ty} x {tx} tiles does not fit frames of {h} x {w} pixels (a tile is never empty)")
    if b == 0:
        return out, gains
    ws = N.workspace.get(image.device, N.lib().awseg_relight_workspace(b, ty, tx), tag="relight")
    N.call("awseg_relight", N.ptr(image), b, 3, h, w, N.host(m), N.host(s), ty, tx, p["clip_limit"], p["max_gain"],
           int(p["white_balance"]), N.ptr(cond), N.ptr(out), N.ptr(gains), N.ptr(stats), stats.shape[0], N.ptr(ws), N.stream())
    return out, gains


# ------------------------------------------------ rain and snow removal: top-hat mask + masked fill (include/awseg_restore.h)
DEOCCLUDE_FIELDS = ("frames", "pixels", "seed_pixels", "masked_pixels", "unfilled_pixels", "sum_change", "nonfinite_values")
DEOCCLUDE_ROW = len(DEOCCLUDE_FIELDS)  # AWSEG_DEOCCLUDE_ROW
DEOCCLUDE_MAX_DILATE = 2               # AWSEG_DEOCCLUDE_MAX_DILATE
DEOCCLUDE_UNIT = 2.0 ** -16            # the change sum is int64 in fixed point: exact, order-independent
DEOCCLUDE_DEFAULTS = {"radius": 9, "threshold": 0.06, "bright_min": 0.5, "dilate": 1}    # the prototype's: a stated choice, not a tuned one

new_deocclude_stats, deocclude_stats_to_numpy = _stats_rows("deocclude", DEOCCLUDE_FIELDS, "the change sum is in units of DEOCCLUDE_UNIT")


def deocclude_parameters(radius=9, threshold=0.06, bright_min=0.5, dilate=1) -> dict:
    """The checked parameters of deocclude(): radius an integer in [1, 15]; threshold a number in (0, 1], bright_min one in [0, 1]
    (also as float32); dilate an integer in [0, 2].  ValueError otherwise."""
    return {"radius": _integer("deocclude", "radius", radius, 1, DEHAZE_MAX_RADIUS),
            "threshold": _number("deocclude", "threshold", threshold, 0.0, 1.0, open_below=True),
            "bright_min": _number("deocclude", "bright_min", bright_min, 0.0, 1.0),
            "dilate": _integer("deocclude", "dilate", dilate, 0, DEOCCLUDE_MAX_DILATE)}


def deocclude_workspace_bytes(b: int, h: int, w: int) -> int:
    """The closed form of awseg_deocclude_workspace: nothing.  The mask is all one kernel leaves for the other, and it is an output."""
    return 0


def deocclude(image: torch.Tensor, stats: Optional[torch.Tensor] = None, cond: Optional[torch.Tensor] = None, *, radius: int = 9,
              threshold: float = 0.06, bright_min: float = 0.5, dilate: int = 1, mean=None, std=None,
              out: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """Rain and snow removal from the loader's normalised float32 frames `image` [B, 3, H, W]: the pixels where the white top-hat
    ((2 radius + 1)^2 windows) of all three channels exceeds `threshold` and the darkest channel is at least `bright_min`, dilated
    by `dilate`, are replaced by the mean of the unmasked pixels of their window, as include/awseg_restore.h defines it step by
    step -> (restored float32 [B, 3, H, W], mask uint8 [B, H, W]: 1 where a pixel was taken for an occluder).  `stats`
    (new_deocclude_stats; slot 0 + slot 1 + cond[b], cond device int32 [B]) takes the counters of DEOCCLUDE_FIELDS; without it they
    go to a tensor nobody reads.  `mean`, `std`: the loader's normalisation (default: ImageNet's).  `out`, `mask`: where the
    restored frames and the mask go (contiguous; `out` not `image`).  There is no CPU path."""
    p = deocclude_parameters(radius, threshold, bright_min, dilate)
    image, b, h, w, m, s, stats = _restore_frames("deocclude", image, stats, cond, mean, std, DEOCCLUDE_ROW, new_deocclude_stats)
    out, _ = _restore_outputs("deocclude", image, out)
    if mask is None:
        mask = torch.empty(b, h, w, dtype=torch.uint8, device=image.device)
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (b, h, w) or not mask.is_contiguous() or mask.device != image.device:
        raise ValueError(f"deocclude: mask is a contiguous uint8 tensor [B, H, W] on the frames' device, got {mask.dtype} {tuple(mask.shape)}")
    if b == 0:
        return out, mask
    need = N.lib().awseg_deocclude_workspace(b, h, w)                  # 0: the launcher takes NULL for a workspace of no bytes
    ws = N.workspace.get(image.device, need, tag="deocclude") if need else None
    N.call("awseg_deocclude", N.ptr(image), b, 3, h, w, N.host(m), N.host(s), p["radius"], p["threshold"], p["bright_min"], p["dilate"],
           N.ptr(cond), N.ptr(out), N.ptr(mask), N.ptr(stats), stats.shape[0], N.ptr(ws), N.stream())
    return out, mask


# ------------------------------------------------ weather estimate: which front-end a frame needs (include/awseg_restore.h)
ESTIMATE_FIELDS = ("frames", "pixels", "sum_dark", "sum_luma", "sum_channel_0", "sum_channel_1", "sum_channel_2", "seed_pixels",
                   "nonfinite_values", "routed_none", "routed_dark_channel", "routed_clahe", "routed_tophat")
ESTIMATE_ROW = len(ESTIMATE_FIELDS)    # AWSEG_ESTIMATE_ROW
ESTIMATE_DESCRIPTORS = ("dark_channel", "luma", "mean_0", "mean_1", "mean_2", "seed_fraction")      # AWSEG_ESTIMATE_DESCRIPTORS of them
ESTIMATE_FRAME_RECORD = 64             # AWSEG_ESTIMATE_FRAME_RECORD: workspace bytes per frame
ESTIMATE_UNIT = 2.0 ** -16             # the dark-channel, luma and channel sums are int64 in fixed point: exact, order-independent
ESTIMATE_ROUTES = ("none", "dark_channel", "clahe", "tophat")          # route 0 .. 3: the method a frame is sent to
# the route a rule that knew the weather would take, by the condition's name (other names: none): what `route: oracle` applies and
# what route_accuracy counts as right
ESTIMATE_EXPECTED_ROUTE = {"clean": "none", "fog": "dark_channel", "night": "clahe", "rain": "tophat", "snow": "tophat"}
# the prototype's thresholds on the renderer's street scenes at 256 x 512 and above: a stated choice, not a tuned one.  seed_min
# depends on the resolution (the renderer's drop count does not grow with the frame)
ESTIMATE_DEFAULTS = {"radius": 7, "threshold": 0.06, "bright_min": 0.5, "cast_max": 0.65, "luma_max": 0.5, "dark_min": 0.47,
                     "seed_min": 0.001}
new_estimate_stats, estimate_stats_to_numpy = _stats_rows("estimate", ESTIMATE_FIELDS, "the five sums are in units of ESTIMATE_UNIT")


def weather_estimate_parameters(radius=7, threshold=0.06, bright_min=0.5, cast_max=0.65, luma_max=0.5, dark_min=0.47,
                                seed_min=0.001) -> dict:
    """The checked parameters of weather_estimate(): radius an integer in [1, 15]; threshold a number in (0, 1], bright_min one in
    [0, 1], cast_max in (0, 4], luma_max in (0, 1], dark_min and seed_min in [0, 1) (all also as float32; NaN is refused).
    ValueError otherwise."""
    number = lambda *a, **k: _number("weather_estimate", *a, **k)      # noqa: E731
    return {"radius": _integer("weather_estimate", "radius", radius, 1, DEHAZE_MAX_RADIUS),
            "threshold": number("threshold", threshold, 0.0, 1.0, open_below=True),
            "bright_min": number("bright_min", bright_min, 0.0, 1.0), "cast_max": number("cast_max", cast_max, 0.0, 4.0, open_below=True),
            "luma_max": number("luma_max", luma_max, 0.0, 1.0, open_below=True),
            "dark_min": number("dark_min", dark_min, 0.0, 1.0, open_above=True),
            "seed_min": number("seed_min", seed_min, 0.0, 1.0, open_above=True)}


def weather_estimate_workspace_bytes(b: int) -> int:
    """The closed form of awseg_weather_estimate_workspace: one record per frame."""
    return max(int(b), 0) * ESTIMATE_FRAME_RECORD


def weather_estimate(image: torch.Tensor, stats: Optional[torch.Tensor] = None, cond: Optional[torch.Tensor] = None, *, radius: int = 7,
                     threshold: float = 0.06, bright_min: float = 0.5, cast_max: float = 0.65, luma_max: float = 0.5,
                     dark_min: float = 0.47, seed_min: float = 0.001, mean=None, std=None, route: Optional[torch.Tensor] = None,
                     descriptors: Optional[torch.Tensor] = None):
    """Which front-end each of the loader's normalised float32 frames `image` [B, 3, H, W] needs, from its pixels alone, as
    include/awseg_restore.h defines it step by step -> (route int32 [B]: an index into ESTIMATE_ROUTES, descriptors float32 [B, 6]:
    ESTIMATE_DESCRIPTORS).  A dark frame with a blue cast (mean_0 < cast_max * mean_2 and luma < luma_max) goes to clahe, else a
    veiled one (dark_channel > dark_min) to dark_channel, else one with bright occluders (seed_fraction > seed_min; the seeds of
    deocclude() at `radius`, `threshold`, `bright_min`) to tophat, else to none.  `stats` (new_estimate_stats; slot 0 + slot
    1 + cond[b], cond device int32 [B]) takes the counters of ESTIMATE_FIELDS; without it they go to a tensor nobody reads.
    `mean`, `std`: the loader's normalisation (default: ImageNet's).  `route`, `descriptors`: where the results go (contiguous, on
    the frames' device).  The frames are read only.  There is no CPU path."""
    p = weather_estimate_parameters(radius, threshold, bright_min, cast_max, luma_max, dark_min, seed_min)
    image, b, h, w, m, s, stats = _restore_frames("weather_estimate", image, stats, cond, mean, std, ESTIMATE_ROW, new_estimate_stats)
    if not stats.is_contiguous():                                      # the one entry point that refuses it
        raise ValueError(f"stats must be int64 [slots, {ESTIMATE_ROW}] (new_estimate_stats), got {stats.dtype} {tuple(stats.shape)}")
    if route is None:
        route = torch.empty(b, dtype=torch.int32, device=image.device)
    if route.dtype != torch.int32 or tuple(route.shape) != (b,) or not route.is_contiguous() or route.device != image.device:
        raise ValueError(f"weather_estimate: route is a contiguous int32 tensor [B] on the frames' device, got {route.dtype} "
                         f"{tuple(route.shape)}")
    if descriptors is None:
        descriptors = torch.empty(b, len(ESTIMATE_DESCRIPTORS), dtype=torch.float32, device=image.device)
    if descriptors.dtype != torch.float32 or tuple(descriptors.shape) != (b, len(ESTIMATE_DESCRIPTORS)) \
            or not descriptors.is_contiguous() or descriptors.device != image.device:
        raise ValueError(f"weather_estimate: descriptors is a contiguous float32 tensor [B, {len(ESTIMATE_DESCRIPTORS)}] on the "
                         f"frames' device, got {descriptors.dtype} {tuple(descriptors.shape)}")
    if b == 0:
        return route, descriptors
    ws = N.workspace.get(image.device, N.lib().awseg_weather_estimate_workspace(b), tag="weather_estimate")
    N.call("awseg_weather_estimate", N.ptr(image), b, 3, h, w, N.host(m), N.host(s), p["radius"], p["threshold"], p["bright_min"],
           p["cast_max"], p["luma_max"], p["dark_min"], p["seed_min"], N.ptr(cond), N.ptr(route), N.ptr(descriptors), N.ptr(stats),
           stats.shape[0], N.ptr(ws), N.stream())
    return route, descriptors


# ------------------------------------------------ test-time augmentation: views and their average (include/awseg_restore.h)
TTA_SET, TTA_ADD, TTA_SCALE_ADD = 0, 1, 2      # AWSEG_TTA_SET, AWSEG_TTA_ADD, AWSEG_TTA_SCALE_ADD
TTA_MODES = {"set": TTA_SET, "add": TTA_ADD, "scale_add": TTA_SCALE_ADD}
TTA_VIEW_MAX_CHANNELS = 4                      # AWSEG_TTA_VIEW_MAX_CHANNELS


def _tta_map(who: str, name: str, t) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous() or min(t.shape) < 1:
        got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else repr(t)
        raise ValueError(f"{who}: {name} is a contiguous float32 [B, C, H, W] tensor of at least one element, got {got}")
    return t


def tta_view(images: torch.Tensor, size, flip: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A view of the frames for test-time augmentation: float32 `images` [B, C <= 4, H, W] resampled bilinearly (align_corners =
    False) to `size` = (h, w) and then mirrored left to right when `flip`, in the float32 arithmetic include/awseg_restore.h
    states step by step -> float32 [B, C, h, w].  At the frames' own size the values are copied bit for bit.  `out`: where the
    view goes (contiguous, not `images`).  There is no CPU path."""
    images = _tta_map("tta_view", "images", images)
    b, c, H, W = (int(d) for d in images.shape)
    if c > TTA_VIEW_MAX_CHANNELS:
        raise ValueError(f"tta_view: frames of 1 .. {TTA_VIEW_MAX_CHANNELS} channels, got {c}")
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"tta_view: size is (height, width), got {size!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"tta_view: size is at least 1 x 1, got {size!r}")
    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError(f"tta_view: flip is true or false, got {flip!r}")
    if out is None:
        out = torch.empty(b, c, h, w, dtype=torch.float32, device=images.device)
    out = _tta_map("tta_view", "out", out)
    if tuple(out.shape) != (b, c, h, w) or out.device != images.device or out.data_ptr() == images.data_ptr():
        raise ValueError(f"tta_view: out is float32 {(b, c, h, w)} on {images.device} and not the input, got {tuple(out.shape)}")
    N.call("awseg_tta_view", N.ptr(images), b, c, H, W, N.ptr(out), h, w, int(flip), N.stream())
    return out


def tta_accumulate(logits: torch.Tensor, acc: torch.Tensor, flip: bool, weight: float, mode="add") -> torch.Tensor:
    """Fold a view's float32 `logits` [B, C, h, w] into the running average `acc` [B, C, H, W], in place: the logits are mirrored
    back when `flip`, resampled bilinearly (align_corners = False) to the frame's size, multiplied by `weight` and, by `mode`
    ('set' / TTA_SET: acc = weight U; 'add' / TTA_ADD: acc += weight U; 'scale_add' / TTA_SCALE_ADD: acc = weight acc + weight U)
    written or added, in the float32 arithmetic include/awseg_restore.h states step by step -> acc.  There is no CPU path."""
    logits, acc = _tta_map("tta_accumulate", "logits", logits), _tta_map("tta_accumulate", "acc", acc)
    if tuple(acc.shape[:2]) != tuple(logits.shape[:2]) or acc.device != logits.device:
        raise ValueError(f"tta_accumulate: logits {tuple(logits.shape)} and acc {tuple(acc.shape)} share batch, channels and device")
    if acc.data_ptr() == logits.data_ptr():
        raise ValueError("tta_accumulate: acc must not be the logits")
    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError(f"tta_accumulate: flip is true or false, got {flip!r}")
    m = TTA_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or int(m) not in TTA_MODES.values():
        raise ValueError(f"tta_accumulate: mode is one of {sorted(TTA_MODES)} (TTA_SET, TTA_ADD, TTA_SCALE_ADD), got {mode!r}")
    with np.errstate(over="ignore"):
        finite = not isinstance(weight, (bool, np.bool_, str)) and isinstance(weight, (int, float, np.integer, np.floating)) \
            and bool(np.isfinite(np.float32(weight)))
    if not finite:
        raise ValueError(f"tta_accumulate: weight is a finite float32 number, got {weight!r}")
    b, c, h, w = (int(d) for d in logits.shape)
    N.call("awseg_tta_accumulate", N.ptr(logits), b, c, h, w, N.ptr(acc), int(acc.shape[2]), int(acc.shape[3]), int(flip),
           float(np.float32(weight)), int(m), N.stream())
    return acc


ECE_CONF_UNIT = 2.0 ** -30    # the device keeps the confidence sums in fixed point (int64, units of 2^-30): exact, order-independent


def ece_bins_to_numpy(bins: torch.Tensor) -> np.ndarray:
    """device bins int64 [slots, n_bins, {count, sum_conf_q30, sum_correct}] -> structured array with float64 sum_conf."""
    raw = bins.cpu().numpy()
    out = np.zeros(raw.shape[:2], dtype=ECE_BIN_DTYPE)
    out["count"], out["sum_conf"], out["sum_correct"] = raw[..., 0], raw[..., 1].astype(np.float64) * ECE_CONF_UNIT, raw[..., 2]
    return out


# ----------------------------------------------------------------------------- streaming temperature calibration
CALIB_MAX_TEMPS = 128                  # include/awseg.h AWSEG_CALIB_MAX_TEMPS
CALIB_NLL_UNIT = 2.0 ** -20            # per-pixel NLL fixed point (AWSEG_CALIB_NLL_FRAC_BITS)
CALIB_NLL_CAP = 2048.0                 # per-pixel NLL clamp, counted as saturated (AWSEG_CALIB_NLL_CAP)
CALIB_PIXEL_BUDGET = (1 << 32) - 1     # pixels one stats tensor holds, summed over ranks (AWSEG_CALIB_PIXEL_BUDGET: x 2^31 < 2^63)
# the reference's grid (metrics.py:293) as the float32 values it iterates over; its tenth point is 0.99999994, not 1
DEFAULT_TEMPERATURE_GRID = torch.linspace(0.1, 10.0, 100).numpy()


def calib_temperatures(temps) -> np.ndarray:
    """The grid as a host float32 array, checked before any launch (the C ABI refuses the same grids with AWSEG_EINVAL)."""
    t = np.ascontiguousarray(np.asarray(temps, dtype=np.float32).reshape(-1))
    if t.size < 1 or t.size > CALIB_MAX_TEMPS:
        raise ValueError(f"a temperature grid has 1 .. {CALIB_MAX_TEMPS} points, got {t.size}")
    if not (np.isfinite(t).all() and (t > 0).all()):
        raise ValueError(f"every grid temperature must be finite and > 0, got {t.tolist()}")
    return t


def new_temperature_grid_stats(n_temps: int, n_bins: int, device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, n_temps + 1, 4 + 3 n_bins], the layout include/awseg.h documents (zeroed: the launches accumulate)."""
    return torch.zeros(n_slots, n_temps + 1, 4 + 3 * n_bins, dtype=torch.int64, device=device)


def _tgrid_args(logits: torch.Tensor, stats: torch.Tensor, temps, edges: torch.Tensor):
    t = calib_temperatures(temps)
    n_bins = edges.numel() - 1
    if stats.dim() != 3 or stats.dtype != torch.int64 or stats.shape[1:] != (t.size + 1, 4 + 3 * n_bins):
        raise ValueError(f"stats must be int64 [slots, {t.size + 1}, {4 + 3 * n_bins}] (new_temperature_grid_stats), got "
                         f"{stats.dtype} {tuple(stats.shape)}")
    if logits[:, 0].numel() > CALIB_PIXEL_BUDGET:
        raise ValueError(f"{logits[:, 0].numel()} pixels exceed the {CALIB_PIXEL_BUDGET}-pixel budget of one stats tensor")
    return t, n_bins


def temperature_grid_stats(logits: torch.Tensor, label: torch.Tensor, stats: torch.Tensor, temps, edges: torch.Tensor,
                           cond: Optional[torch.Tensor] = None) -> None:
    """Per-pixel NLL and ECE bins of `logits` at every temperature of `temps`, accumulated into `stats` on device
    (PKG/evaluation/metrics.py:266-321 streamed: no logit outlives the call)."""
    t, n_bins = _tgrid_args(logits, stats, temps, edges)
    logits, label = logits.contiguous(), label.contiguous()
    b, c = logits.shape[0], logits.shape[1]
    hw = logits[0, 0].numel()
    N.call("awseg_temperature_grid_stats", N.ptr(logits), b, c, hw, N.ptr(label), N.label_dtype(label), N.ptr(cond), N.host(t),
           t.size, N.ptr(edges), n_bins, N.ptr(stats), stats.shape[0], N.stream())


def ensemble_temperature_grid_stats(seg1: torch.Tensor, seg2: torch.Tensor, mode: int, weights, temperature, label: torch.Tensor,
                                    stats: torch.Tensor, temps, edges: torch.Tensor, cond: Optional[torch.Tensor] = None) -> None:
    """temperature_grid_stats of r = combine(seg1, seg2)/T (WEIGHTED or MEAN, the roundings of ensemble_eval_stats) without
    materialising r.  C = 19, H*W % 4 == 0."""
    t, n_bins = _tgrid_args(seg1, stats, temps, edges)
    seg1, seg2, label = seg1.contiguous(), seg2.contiguous(), label.contiguous()
    b, c = seg1.shape[0], seg1.shape[1]
    hw = seg1[0, 0].numel()
    N.call("awseg_ensemble_temperature_grid_stats", N.ptr(seg1), N.ptr(seg2), b, c, hw, mode, N.ptr(weights), N.ptr(temperature),
           N.ptr(label), N.label_dtype(label), N.ptr(cond), N.host(t), t.size, N.ptr(edges), n_bins, N.ptr(stats), stats.shape[0],
           N.stream())


def temperature_grid_stats_to_numpy(stats) -> dict:
    """Decode the int64 counters (a device tensor or a numpy array) into exact integer arrays:
    count / nll_q (units CALIB_NLL_UNIT) / saturated / nonfinite [slots, K], bins [slots, K, n_bins] as ece_bins_to_numpy,
    out_of_range [slots]."""
    raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
    k = raw.shape[1] - 1
    n_bins = (raw.shape[2] - 4) // 3
    rows = raw[:, :k]
    b = rows[..., 4:].reshape(raw.shape[0], k, n_bins, 3)
    bins = np.zeros(b.shape[:3], dtype=ECE_BIN_DTYPE)
    bins["count"], bins["sum_conf"], bins["sum_correct"] = b[..., 0], b[..., 1].astype(np.float64) * ECE_CONF_UNIT, b[..., 2]
    return {"count": rows[..., 0].copy(), "nll_q": rows[..., 1].copy(), "saturated": rows[..., 2].copy(),
            "nonfinite": rows[..., 3].copy(), "bins": bins, "out_of_range": raw[:, k, 0].copy()}


# ----------------------------------------------------------------------------- ensemble weight sweep (include/awseg.h)
WGRID_MAX_POINTS = 64                  # include/awseg.h AWSEG_WGRID_MAX_POINTS


def check_weight_grid(weights) -> np.ndarray:
    """The grid as a host float32 array [G, 2], checked before any launch (the C ABI refuses the same grids with AWSEG_EINVAL)."""
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights)
    if w.dtype != np.float32:
        raise ValueError(f"a weight grid is float32 [G, 2] (the pairs enter the kernel as they are), got {w.dtype}")
    if w.ndim != 2 or w.shape[1] != 2 or not 1 <= w.shape[0] <= WGRID_MAX_POINTS:
        raise ValueError(f"a weight grid is float32 [G, 2] with 1 .. {WGRID_MAX_POINTS} points, got {tuple(w.shape)}")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError(f"every grid weight must be finite and >= 0, got {w.tolist()}")
    return np.ascontiguousarray(w)


def new_weight_grid_stats(n_slots: int, n_points: int, num_classes: int, device) -> torch.Tensor:
    """int64 [n_slots, n_points + 3, 2 C], the layout include/awseg.h documents (zeroed: the launches accumulate)."""
    if n_slots < 1 or not 1 <= n_points <= WGRID_MAX_POINTS or num_classes < 1:
        raise ValueError(f"new_weight_grid_stats: n_slots >= 1, 1 .. {WGRID_MAX_POINTS} points and >= 1 class, got {n_slots}, "
                         f"{n_points}, {num_classes}")
    return torch.zeros(n_slots, n_points + 3, 2 * num_classes, dtype=torch.int64, device=device)


def ensemble_weight_grid_stats(seg1: torch.Tensor, seg2: torch.Tensor, weights, labels: torch.Tensor, cond: Optional[torch.Tensor],
                               stats: torch.Tensor, ignore_index: int = 255) -> None:
    """The mIoU counters of argmax(w0 * seg1 + w1 * seg2) at every pair of `weights` (float32 CPU tensor or array [G, 2]) and the
    split of the labelled pixels by the members' own predictions, accumulated into `stats` (new_weight_grid_stats; slot 0 + slot
    1 + cond[b]) in one pass over the member maps.  C = 19, H*W % 4 == 0."""
    w = check_weight_grid(weights)
    if seg1.dtype != torch.float32 or seg2.dtype != torch.float32 or seg1.dim() < 3 or seg1.shape != seg2.shape:
        raise ValueError(f"ensemble_weight_grid_stats: the members are float32 [B, C, ...] of one shape, got {seg1.dtype} "
                         f"{tuple(seg1.shape)} and {seg2.dtype} {tuple(seg2.shape)}")
    b, c = seg1.shape[0], seg1.shape[1]
    if stats.dim() != 3 or stats.dtype != torch.int64 or stats.shape[1:] != (w.shape[0] + 3, 2 * c):
        raise ValueError(f"stats must be int64 [slots, {w.shape[0] + 3}, {2 * c}] (new_weight_grid_stats), got {stats.dtype} "
                         f"{tuple(stats.shape)}")
    if labels.numel() != seg1[:, 0].numel():
        raise ValueError(f"ensemble_weight_grid_stats: one label per pixel, got {tuple(labels.shape)} for {tuple(seg1.shape)}")
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    if b == 0:
        return
    seg1, seg2, labels = seg1.contiguous(), seg2.contiguous(), labels.contiguous()
    hw = seg1[0, 0].numel()
    N.call("awseg_ensemble_weight_grid_stats", N.ptr(seg1), N.ptr(seg2), b, c, hw, N.host(w), w.shape[0], N.ptr(labels),
           N.label_dtype(labels), int(ignore_index), N.ptr(cond), N.ptr(stats), stats.shape[0], N.stream())


# ----------------------------------------------------------------------------- depth error sums (include/awseg.h)
DEPTH_UNIT = 2.0 ** -20                # fixed point of every real-valued term (AWSEG_DEPTH_FRAC_BITS)
DEPTH_CAP = 2048.0                     # per-term clamp, counted as saturated (AWSEG_DEPTH_CAP)
DEPTH_PIXEL_BUDGET = (1 << 32) - 1     # pixels one stats tensor holds, summed over ranks (AWSEG_DEPTH_PIXEL_BUDGET: x 2^31 < 2^63)
DEPTH_SERIES = ("ensemble", "d1", "d2")            # AWSEG_DEPTH_SERIES_ENSEMBLE / _D1 / _D2; the one-series form fills row 0 only
# AWSEG_DEPTH_VALID .. AWSEG_DEPTH_SATURATED, in row order (AWSEG_DEPTH_ROW = 13)
DEPTH_FIELDS = ("valid", "masked", "nonfinite", "sum_abs", "sum_sq", "sum_abs_rel", "sum_sq_rel", "sum_log", "sum_log_sq",
                "delta1", "delta2", "delta3", "saturated")
DEPTH_ROW = len(DEPTH_FIELDS)
DEPTH_THRESHOLDS = (1.25, 1.5625, 1.953125)        # 1.25, 1.25^2, 1.25^3: exact in float32


def new_depth_eval_stats(device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, 3, 13], the layout include/awseg.h documents (zeroed: the launches accumulate)."""
    return torch.zeros(n_slots, len(DEPTH_SERIES), DEPTH_ROW, dtype=torch.int64, device=device)


def depth_eval_stats(d1: torch.Tensor, d2_low: Optional[torch.Tensor], weights: Optional[torch.Tensor], target: torch.Tensor,
                     stats: torch.Tensor, min_depth: float = 1e-3, cond: Optional[torch.Tensor] = None) -> None:
    """Depth error sums of d1 [B,(1,)H,W] (d2_low None: one series) or of the ensemble, d1 and the upsampled d2_low [B,(1,)h,w]
    (three series; combined with weights [2], mean when None, exactly as depth_upsample_combine) against target [B,H,W],
    accumulated into `stats` (new_depth_eval_stats; slot 0 + slot 1 + cond[b]).  No depth map is written."""
    if stats.dim() != 3 or stats.dtype != torch.int64 or tuple(stats.shape[1:]) != (len(DEPTH_SERIES), DEPTH_ROW):
        raise ValueError(f"stats must be int64 [slots, {len(DEPTH_SERIES)}, {DEPTH_ROW}] (new_depth_eval_stats), got "
                         f"{stats.dtype} {tuple(stats.shape)}")
    if d1.dtype != torch.float32 or target.dtype != torch.float32 or (d2_low is not None and d2_low.dtype != torch.float32):
        raise ValueError("depth maps and the depth target must be float32")
    H, W = d1.shape[-2:]
    b = d1.shape[0] if d1.dim() > 2 else 1
    if d1.numel() != b * H * W or tuple(target.shape[-2:]) != (H, W) or target.numel() != b * H * W:
        raise ValueError(f"depth_eval_stats: d1 [B,(1,)H,W] and target [B,H,W] must agree, got {tuple(d1.shape)} and {tuple(target.shape)}")
    h = w = 0
    if d2_low is not None:
        h, w = d2_low.shape[-2:]
        if d2_low.numel() != b * h * w:
            raise ValueError(f"depth_eval_stats: d2_low must be [B,(1,)h,w] with B = {b}, got {tuple(d2_low.shape)}")
        d2_low = d2_low.contiguous()
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    if d1.numel() > DEPTH_PIXEL_BUDGET:
        raise ValueError(f"{d1.numel()} pixels exceed the {DEPTH_PIXEL_BUDGET}-pixel budget of one stats tensor")
    md = float(min_depth)
    if not (np.isfinite(md) and md > 0):
        raise ValueError(f"min_depth must be finite and > 0, got {min_depth}")
    d1, target = d1.contiguous(), target.contiguous()
    N.call("awseg_depth_eval_stats", N.ptr(d1), N.ptr(d2_low), b, h, w, H, W, N.ptr(None if weights is None else weights.contiguous()),
           N.ptr(target), md, N.ptr(cond), N.ptr(stats), stats.shape[0], N.stream())


def depth_eval_stats_to_numpy(stats) -> dict:
    """Decode the int64 counters (a device tensor or a numpy array) into exact integer arrays [slots, series], one per name of
    DEPTH_FIELDS (the sums in units of DEPTH_UNIT)."""
    raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
    return {f: raw[..., i].copy() for i, f in enumerate(DEPTH_FIELDS)}


# ----------------------------------------------------------------------------- failure-detection counters (include/awseg.h)
FAIL_SCORES = ("mi", "entropy", "variance", "msp")     # AWSEG_FAIL_MI / _ENTROPY / _VARIANCE / _MSP, in row order
FAIL_BINS = 3072                                        # AWSEG_FAIL_BINS: 24 octaves from 2^-22 to 4.0, 128 steps each
FAIL_ROW = len(FAIL_SCORES) * 2 * FAIL_BINS + 4         # AWSEG_FAIL_ROW: [score][flag][bin] + {counted, non-finite, out of range, 0}
_FAIL_BIN_BASE = 105 << 23                              # bits of 2^-22


def failure_bin(values) -> np.ndarray:
    """Bin of each float32 score by the bit rule of include/awseg.h: clamp((int32(bits) - (105 << 23)) >> 16, 0, FAIL_BINS - 1).
    The values are taken as float32 (a float64 input is rounded first, as a store to float32 would)."""
    bits = np.ascontiguousarray(np.asarray(values, dtype=np.float32)).view(np.int32).astype(np.int64)
    return np.clip((bits - _FAIL_BIN_BASE) >> 16, 0, FAIL_BINS - 1)


def failure_bin_edges() -> np.ndarray:
    """float32 [FAIL_BINS]: the lower edge of every bin (bin b holds edge[b] <= s < edge[b + 1]; bin 0 also everything below its
    edge 2^-22, the last bin everything from its edge up)."""
    return (_FAIL_BIN_BASE + (np.arange(FAIL_BINS, dtype=np.int64) << 16)).astype(np.int32).view(np.float32)


def new_failure_stats(device, n_slots: int = 1) -> torch.Tensor:
    """int64 [n_slots, FAIL_ROW], the layout include/awseg.h documents (zeroed: the launches accumulate)."""
    return torch.zeros(n_slots, FAIL_ROW, dtype=torch.int64, device=device)


def _failure_args(logits: torch.Tensor, label: torch.Tensor, stats: torch.Tensor, cond):
    if stats.dim() != 2 or stats.dtype != torch.int64 or stats.shape[1] != FAIL_ROW:
        raise ValueError(f"stats must be int64 [slots, {FAIL_ROW}] (new_failure_stats), got {stats.dtype} {tuple(stats.shape)}")
    if logits.dim() < 3 or logits.dtype != torch.float32:
        raise ValueError(f"logits must be float32 [B, C, ...], got {logits.dtype} {tuple(logits.shape)}")
    b, c = logits.shape[0], logits.shape[1]
    hw = logits[0, 0].numel() if b else int(np.prod(logits.shape[2:]))
    if label.numel() != b * hw:
        raise ValueError(f"label must hold {b} x {hw} elements, got {tuple(label.shape)}")
    if cond is not None and (cond.dtype != torch.int32 or cond.numel() != b):
        raise ValueError("cond must be int32 [B]")
    return b, c, hw


def ensemble_failure_stats(seg1: torch.Tensor, seg2: torch.Tensor, mode: int, weights, temperature, label: torch.Tensor,
                           stats: torch.Tensor, cond: Optional[torch.Tensor] = None, combined: Optional[torch.Tensor] = None) -> None:
    """Failure-detection counters of an ensemble batch: the four scores of FAIL_SCORES per pixel, histogrammed by "right / wrong"
    into `stats` (new_failure_stats; slot 0 + slot 1 + cond[b]) in one pass over the member logits.  `combined` [B, C, ...]: the
    msp row reads the combined logits from it (mode, weights, temperature are then ignored), else forms them as
    ensemble_eval_stats does (mode WEIGHTED or MEAN)."""
    b, c, hw = _failure_args(seg1, label, stats, cond)
    if seg2.shape != seg1.shape or seg2.dtype != torch.float32 or (combined is not None and (combined.shape != seg1.shape or
                                                                                              combined.dtype != torch.float32)):
        raise ValueError("ensemble_failure_stats: seg1, seg2 (and combined) must be float32 of one shape")
    seg1, seg2, label = seg1.contiguous(), seg2.contiguous(), label.contiguous()
    N.call("awseg_ensemble_failure_stats", N.ptr(seg1), N.ptr(seg2), N.ptr(None if combined is None else combined.contiguous()), b, c, hw,
           int(mode), N.ptr(None if weights is None else weights.contiguous()), N.ptr(temperature), N.ptr(label), N.label_dtype(label),
           N.ptr(cond), N.ptr(stats), stats.shape[0], N.stream())


def failure_stats(logits: torch.Tensor, label: torch.Tensor, stats: torch.Tensor, cond: Optional[torch.Tensor] = None) -> None:
    """Failure-detection counters of one model's logits: rows 'entropy' and 'msp' of `stats` (the other two are not touched)."""
    b, c, hw = _failure_args(logits, label, stats, cond)
    logits, label = logits.contiguous(), label.contiguous()
    N.call("awseg_failure_stats", N.ptr(logits), b, c, hw, N.ptr(label), N.label_dtype(label), N.ptr(cond), N.ptr(stats), stats.shape[0],
           N.stream())


def failure_stats_to_numpy(stats) -> dict:
    """int64 [slots, FAIL_ROW] (a device tensor or a numpy array) -> {'hist' [slots, 4, 2, FAIL_BINS] (score, 0 right / 1 wrong,
    bin), 'pixels', 'nonfinite', 'out_of_range' [slots]}."""
    raw = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.int64)
    n = len(FAIL_SCORES) * 2 * FAIL_BINS
    return {"hist": raw[:, :n].reshape(raw.shape[0], len(FAIL_SCORES), 2, FAIL_BINS).copy(), "pixels": raw[:, n].copy(),
            "nonfinite": raw[:, n + 1].copy(), "out_of_range": raw[:, n + 2].copy()}


# ----------------------------------------------------------------------------- A7
def normalize(imgs: torch.Tensor, out: Optional[torch.Tensor] = None, sel: Optional[torch.Tensor] = None,
              mean=None, std=None) -> torch.Tensor:
    """PKG/data/loader.py:195-198: uint8 [B,H,W,3] -> float32 [B,3,H,W]."""
    imgs = imgs.contiguous()
    b, h, w, _ = imgs.shape
    if out is None:
        out = torch.empty(b, 3, h, w, dtype=torch.float32, device=imgs.device)
    m, s = _mean_std(mean, std)
    N.call("awseg_normalize", N.ptr(imgs), b, h, w, N.ptr(sel), 0 if sel is None else sel.numel(), N.host(m),
                                    N.host(s), N.ptr(out), N.stream())
    return out


# ----------------------------------------------------------------------------- weather
def _jobs(dtype, n):
    return np.zeros(n, dtype=dtype)


def fog_jobs(images: Sequence[int], intensities: Sequence[float], seeds: Optional[Sequence[int]] = None) -> np.ndarray:
    """beta / A from intensity exactly as PKG/data/preprocessing.py:110-114 (Python float math)."""
    j = _jobs(N.FOG_JOB, len(images))
    for k, (im, inten) in enumerate(zip(images, intensities)):
        inten = float(inten)
        j[k]["image"] = im
        j[k]["beta"] = 0.005 + inten * (0.05 - 0.005)
        j[k]["atmos"] = 0.7 + inten * (1.0 - 0.7)
        j[k]["seed"] = 0 if seeds is None else int(seeds[k]) & 0xFFFFFFFFFFFFFFFF
    return j


def night_jobs(images, brightness, intensities, seeds=None) -> np.ndarray:
    j = _jobs(N.NIGHT_JOB, len(images))
    for k in range(len(images)):
        j[k]["image"] = images[k]
        j[k]["brightness"] = float(brightness[k])
        j[k]["intensity"] = float(intensities[k])
        j[k]["seed"] = 0 if seeds is None else int(seeds[k]) & 0xFFFFFFFFFFFFFFFF
    return j


def prim_jobs(images, intensities, prim_lists, ksizes=None):
    """-> (jobs, concatenated int32 primitive array)."""
    j = _jobs(N.PRIM_JOB, len(images))
    off = 0
    for k in range(len(images)):
        j[k]["image"] = images[k]
        j[k]["prim_offset"] = off
        j[k]["prim_count"] = len(prim_lists[k])
        j[k]["blur_ksize"] = 3 if ksizes is None else int(ksizes[k])
        j[k]["intensity"] = float(intensities[k])
        off += len(prim_lists[k])
    width = prim_lists[0].shape[1] if len(prim_lists) and prim_lists[0].ndim == 2 else 1
    prims = np.concatenate([np.asarray(p, dtype=np.int32).reshape(-1, width) for p in prim_lists], axis=0) \
        if len(prim_lists) else np.zeros((0, width), np.int32)
    if prims.shape[0] == 0:
        prims = np.zeros((1, max(width, 1)), np.int32)
    return j, np.ascontiguousarray(prims)


def synthetic_depth(h: int, w: int, jobs: np.ndarray, device, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PKG/data/preprocessing.py:227-248 -> float64 [n_jobs,H,W]."""
    jd = N.host_jobs(jobs)
    out = torch.empty(len(jobs), h, w, dtype=torch.float64, device=device)
    N.call("awseg_synthetic_depth", h, w, jd, len(jobs), N.ptr(noise), N.host(_TAPS), N.ptr(out), N.stream())
    return out


def lut3_apply(imgs: torch.Tensor, luts: torch.Tensor, lut_of: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b,...,c] = luts[lut_of[b], c, imgs[b,...,c]] for uint8 [B,H,W,3] frames (lut_of < 0: unchanged)."""
    imgs = imgs.contiguous()
    b, h, w, _ = imgs.shape
    if out is None:
        out = torch.empty_like(imgs)
    N.call("awseg_lut3_apply", N.ptr(imgs), b, h, w, N.ptr(luts.contiguous()), int(luts.shape[0]), N.ptr(lut_of), N.ptr(out), N.stream())
    return out


def local_contrast(imgs: torch.Tensor) -> torch.Tensor:
    """sqrt(box5((gray - box5(gray))^2)) of uint8 [B,H,W,3] frames -> float32 [B,H,W]
    (PKG/data/preprocessing.py:270-278)."""
    imgs = imgs.contiguous()
    b, h, w, _ = imgs.shape
    out = torch.empty(b, h, w, dtype=torch.float32, device=imgs.device)
    N.call("awseg_local_contrast", N.ptr(imgs), b, h, w, N.ptr(out), N.stream())
    return out


def depth_estimate(imgs: torch.Tensor, out: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """DepthEstimationPreprocessor.estimate_depth (PKG/data/preprocessing.py:304-367) for a uint8
    [B,H,W,3] batch -> [B,H,W] depth target in [0,1]; float64 (reference dtype) or float32 (what
    the loader hands on, loader.py:290)."""
    imgs = imgs.contiguous()
    b, h, w, _ = imgs.shape
    if out is None:
        out = torch.empty(b, h, w, dtype=dtype, device=imgs.device)
    ws = torch.empty(max(1, b), dtype=torch.int32, device=imgs.device)
    o64 = out if out.dtype == torch.float64 else None
    o32 = out if out.dtype == torch.float32 else None
    N.call("awseg_depth_estimate", N.ptr(imgs), b, h, w, N.host(_TAPS), N.ptr(ws), N.ptr(o64), N.ptr(o32), N.stream())
    return out


def fog(imgs: torch.Tensor, jobs: np.ndarray, noise: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
        out: Optional[torch.Tensor] = None, norm_out: Optional[torch.Tensor] = None, depth_out: Optional[torch.Tensor] = None,
        mean=None, std=None) -> None:
    """_apply_fog (PKG/data/preprocessing.py:94-123).  depth given -> two-step form; else fused
    depth+fog with `noise` (parity mode) or in-kernel Philox (noise None)."""
    imgs = imgs.contiguous()
    _, h, w, _ = imgs.shape
    jd = N.host_jobs(jobs)
    m, s = _mean_std(mean, std)
    if depth is not None:
        N.call("awseg_fog_apply", N.ptr(imgs), h, w, jd, len(jobs), N.ptr(depth.contiguous()), N.ptr(out),
                                        N.ptr(norm_out), N.host(m), N.host(s), N.stream())
    else:
        N.call("awseg_fog_fused", N.ptr(imgs), h, w, jd, len(jobs), N.ptr(noise), N.host(_TAPS), N.ptr(out),
                                        N.ptr(norm_out), N.ptr(depth_out), N.host(m), N.host(s), N.stream())


def night(imgs: torch.Tensor, jobs: np.ndarray, noise: Optional[torch.Tensor] = None, out=None, norm_out=None,
          mean=None, std=None) -> None:
    """_apply_night (PKG/data/preprocessing.py:204-225)."""
    imgs = imgs.contiguous()
    _, h, w, _ = imgs.shape
    jd = N.host_jobs(jobs)
    m, s = _mean_std(mean, std)
    N.call("awseg_night_apply", N.ptr(imgs), h, w, jd, len(jobs), N.ptr(noise), N.host(NIGHT_GAINS), N.ptr(out),
                                      N.ptr(norm_out), N.host(m), N.host(s), N.stream())


WEATHER_BATCH = os.environ.get("AWSEG_WEATHER_BATCH", "1") != "0"   # one launch for a batch of mixed conditions (throughput mode)
WEATHER_BATCH_MAX = 16


def weather_batch_ok(h: int, w: int) -> bool:
    return WEATHER_BATCH and w % 4 == 0 and w >= 16


def weather_batch(imgs: torch.Tensor, jobs: np.ndarray, rain_drops: Optional[np.ndarray], snow_flakes: Optional[np.ndarray],
                  norm_out: torch.Tensor, out: Optional[torch.Tensor] = None, mean=None, std=None) -> bool:
    """apply_weather_effect + Normalize for <= 16 frames of mixed conditions in ONE launch (awseg_weather_batch; in-kernel Philox noise).
    jobs: np.ndarray of N.WEATHER_JOB.  Returns False when the launcher declines the geometry (the caller uses the per-kind calls)."""
    imgs = imgs.contiguous()
    _, h, w, _ = imgs.shape
    n_cov = int(((jobs["kind"] == N.WEATHER_RAIN) | (jobs["kind"] == N.WEATHER_SNOW)).sum())
    ws = N.workspace.get(imgs.device, N.lib().awseg_streak_workspace(n_cov, h, w), tag="streak") if n_cov else None
    rd = None if rain_drops is None else torch.from_numpy(np.ascontiguousarray(rain_drops, dtype=np.int32)).to(imgs.device, non_blocking=True)
    sf = None if snow_flakes is None else torch.from_numpy(np.ascontiguousarray(snow_flakes, dtype=np.int32)).to(imgs.device, non_blocking=True)
    m, s = _mean_std(mean, std)
    rc = N.try_call("awseg_weather_batch", N.ptr(imgs), h, w, N.host_jobs(jobs), len(jobs), N.ptr(rd), N.ptr(sf), N.host(_TAPS), N.host(NIGHT_GAINS),
                    N.ptr(out), N.ptr(norm_out), N.host(m), N.host(s), N.ptr(ws), N.stream())
    return rc == 0


def _streak(entry: str, imgs: torch.Tensor, jobs: np.ndarray, prims: np.ndarray, out, norm_out, mean, std) -> None:
    """awseg_rain_apply / awseg_snow_apply: the primitives are rasterised once per frame into a coverage bit map (a small kernel
    in front, its scratch from awseg_streak_workspace), the blur kernels are pure stencils."""
    imgs = imgs.contiguous()
    _, h, w, _ = imgs.shape
    jd = N.host_jobs(jobs)
    pd = torch.from_numpy(np.ascontiguousarray(prims, dtype=np.int32)).to(imgs.device, non_blocking=True)
    m, s = _mean_std(mean, std)
    ws = N.workspace.get(imgs.device, N.lib().awseg_streak_workspace(len(jobs), h, w), tag="streak") if len(jobs) else None
    N.call(entry, N.ptr(imgs), h, w, jd, len(jobs), N.ptr(pd), N.ptr(out), N.ptr(norm_out), N.host(m), N.host(s), N.ptr(ws), N.stream())


def rain(imgs: torch.Tensor, jobs: np.ndarray, drops: np.ndarray, out=None, norm_out=None, mean=None, std=None) -> None:
    """_apply_rain (PKG/data/preprocessing.py:125-168)."""
    _streak("awseg_rain_apply", imgs, jobs, drops, out, norm_out, mean, std)


def snow(imgs: torch.Tensor, jobs: np.ndarray, flakes: np.ndarray, out=None, norm_out=None, mean=None, std=None) -> None:
    """_apply_snow (PKG/data/preprocessing.py:170-202)."""
    _streak("awseg_snow_apply", imgs, jobs, flakes, out, norm_out, mean, std)


_DENSITY_TABLE = {"fog": (0.5, 0.5), "rain": (0.3, 0.2), "snow": (0.3, 0.2)}   # trainer.py:501-509, else (0.1, 0)


def fog_density_field(conditions: Sequence[str], h: int, w: int, device, seed: int,
                      uniform: Optional[torch.Tensor] = None) -> torch.Tensor:
    """AdverseWeatherTrainer._estimate_fog_density (PKG/training/trainer.py:480-511) on device.  `uniform` float32
    [B,h,w] (device): the host's torch.rand draws -> bit-identical to the reference (parity mode); None: in-kernel
    Philox keyed by `seed` (throughput mode)."""
    so = np.array([_DENSITY_TABLE.get(str(c), (0.1, 0.0)) for c in conditions], dtype=np.float32)
    sod = torch.from_numpy(so).to(device, non_blocking=True)
    out = torch.empty(len(conditions), h, w, dtype=torch.float32, device=device)
    if uniform is not None:
        uniform = uniform.to(device=device, dtype=torch.float32).contiguous()
        if tuple(uniform.shape) != (len(conditions), h, w):
            raise ValueError(f"uniform field must be [{len(conditions)},{h},{w}], got {tuple(uniform.shape)}")
    N.call("awseg_fog_density_field", N.ptr(sod), len(conditions), h * w, seed & 0xFFFFFFFFFFFFFFFF, N.ptr(uniform), N.ptr(out),
                                            N.stream())
    return out


# ----------------------------------------------------------------------------- loss
def fog_ce_forward(logits: torch.Tensor, label: torch.Tensor, density: Optional[torch.Tensor], focal: bool,
                   sensitivity: float, oob: torch.Tensor, want_pixel: bool = False):
    """FogDensityAwareLoss seg term, PKG/models/model.py:577-587 + mean :610 -> float32[1]."""
    logits, label = logits.contiguous(), label.contiguous()
    b, c = logits.shape[0], logits.shape[1]
    hw = logits[0, 0].numel()
    n_part = N.lib().awseg_loss_partials(b, hw)
    partials = N.workspace.get(logits.device, n_part * 8, "loss").view(torch.float64)
    mean = torch.empty(1, dtype=torch.float32, device=logits.device)
    pix = torch.empty((b,) + tuple(logits.shape[2:]), dtype=torch.float32, device=logits.device) if want_pixel else None
    dens = None if density is None else density.contiguous()
    N.call("awseg_fog_ce_forward", N.ptr(logits), N.ptr(label), N.label_dtype(label), N.ptr(dens), b, c, hw,
                                         N.LOSS_FOCAL if focal else N.LOSS_CE, float(sensitivity), N.ptr(pix),
                                         N.ptr(partials), N.ptr(mean), N.ptr(oob), N.stream())
    return mean, pix


def fog_ce_backward(logits, label, density, focal: bool, sensitivity: float, grad_scale: torch.Tensor) -> torch.Tensor:
    logits, label = logits.contiguous(), label.contiguous()
    b, c = logits.shape[0], logits.shape[1]
    hw = logits[0, 0].numel()
    grad = torch.empty_like(logits)
    dens = None if density is None else density.contiguous()
    gs = grad_scale.to(torch.float32).reshape(1).contiguous()
    N.call("awseg_fog_ce_backward", N.ptr(logits), N.ptr(label), N.label_dtype(label), N.ptr(dens), b, c, hw,
                                          N.LOSS_FOCAL if focal else N.LOSS_CE, float(sensitivity), N.ptr(gs), N.ptr(grad),
                                          N.stream())
    return grad


def fog_density_from_depth(depth: torch.Tensor) -> torch.Tensor:
    """FogDensityAwareLoss._estimate_fog_density_from_depth, PKG/models/model.py:644-677."""
    depth = depth.contiguous().float()
    b, h, w = depth.shape
    ws = N.workspace.get(depth.device, N.lib().awseg_density_workspace(b, h * w), "density")
    out = torch.empty_like(depth)
    N.call("awseg_fog_density_from_depth", N.ptr(depth), b, h, w, N.ptr(out), N.ptr(ws), N.stream())
    return out


# ----------------------------------------------------------------------------- heads
HEAD_SPLIT = os.environ.get("AWSEG_HEAD_SPLIT", "1") != "0"


def segformer_head_fused(g9: torch.Tensor, scale, shift, w2, b2, height: int, width: int, split: Optional[bool] = None) -> torch.Tensor:
    """Upsample-free SegFormer head (PKG/models/model.py:209-214).  g9 [B,h,w,9,Cmid].
    split: True = the split-operand f16-MFMA kernel where it applies (scale folded into g9, Cmid 128/256, tile geometry),
    False = the float32-input MFMA kernel; None takes the process default (HEAD_SPLIT, env AWSEG_HEAD_SPLIT=0/1)."""
    g9 = g9.contiguous()
    b, h, w, nine, cmid = g9.shape
    assert nine == 9
    cout = w2.shape[0]
    out = torch.empty(b, cout, height, width, dtype=torch.float32, device=g9.device)
    if (HEAD_SPLIT if split is None else split) and scale is None and cmid in (128, 256):
        if N.try_call("awseg_segformer_head_fused_split", N.ptr(g9), b, cmid, h, w, height, width, None, N.ptr(shift.contiguous()),
                      N.ptr(w2.contiguous()), N.ptr(b2.contiguous()), cout, N.ptr(out), N.stream()) == 0:
            return out
    N.call("awseg_segformer_head_fused", N.ptr(g9), b, cmid, h, w, height, width, N.ptr(None if scale is None else scale.contiguous()),
                                               N.ptr(shift.contiguous()), N.ptr(w2.contiguous()), N.ptr(b2.contiguous()),
                                               cout, N.ptr(out), N.stream())
    return out


def upconv3x3_bn_relu(g9: torch.Tensor, scale, shift, height: int, width: int, channels_last: bool = False) -> torch.Tensor:
    """relu(bn(conv3x3(interpolate(f)))) at full resolution without the upsampled tensor: the first
    stage of the fused head only (DepthEstimationHead's first 3x3 on the SegFormer branch)."""
    g9 = g9.contiguous()
    b, h, w, nine, cmid = g9.shape
    assert nine == 9
    shape = (b, height, width, cmid) if channels_last else (b, cmid, height, width)
    out = torch.empty(shape, dtype=torch.float32, device=g9.device)
    N.call("awseg_upconv3x3_bn_relu", N.ptr(g9), b, cmid, h, w, height, width, N.ptr(None if scale is None else scale.contiguous()),
           N.ptr(shift.contiguous()), N.ptr(out), int(channels_last), N.stream())
    return out.permute(0, 3, 1, 2) if channels_last else out          # logical NCHW either way


class _UpConv3x3(torch.autograd.Function):
    """conv3x3(F.interpolate(f, (H, W), bilinear, align_corners=False)) with zero padding, for TRAINING, without the
    upsampled tensor and without a full-resolution convolution (PKG/models/model.py:209-214, :219-221): forward = one small
    GEMM at the encoder's resolution + awseg_upconv3x3_linear; backward = awseg_upconv3x3_adjoint + two small GEMMs."""

    @staticmethod
    def forward(ctx, tok, weight, bias, height, width):
        B, h, w, cin = tok.shape
        cmid = weight.shape[0]
        w1r = weight.permute(1, 2, 3, 0).reshape(cin, 9 * cmid)                     # [Cin, (ky, kx, cout)]
        tok2 = tok.reshape(B * h * w, cin)
        g9 = (tok2 @ w1r).view(B, h, w, 9, cmid).contiguous()
        # NCHW out: the layers behind (BatchNorm, Conv2d) then run on MIOpen's NCHW kernels like the as-written graph — its
        # heuristic pick for channels_last weight gradients is a CK kernel 50x slower (profiles/r02_train_step_kernels.csv)
        z = torch.empty(B, cmid, height, width, dtype=torch.float32, device=tok.device)
        b = bias if bias is not None else torch.zeros(cmid, dtype=torch.float32, device=tok.device)
        N.call("awseg_upconv3x3_linear", N.ptr(g9), B, cmid, h, w, height, width, N.ptr(b.contiguous()), N.ptr(z), 0, N.stream())
        ctx.save_for_backward(tok2, w1r)
        ctx.shape = (B, h, w, cin, cmid, height, width, bias is not None)
        return z

    @staticmethod
    def backward(ctx, dz):
        tok2, w1r = ctx.saved_tensors
        B, h, w, cin, cmid, height, width, has_bias = ctx.shape
        dzl = dz.permute(0, 2, 3, 1).contiguous()                                   # NHWC for the adjoint kernel (one transpose pass)
        dg9 = torch.empty(B, h, w, 9, cmid, dtype=torch.float32, device=dz.device)
        N.call("awseg_upconv3x3_adjoint", N.ptr(dzl), B, cmid, h, w, height, width, N.ptr(dg9), N.stream())
        dg2 = dg9.view(B * h * w, 9 * cmid)
        dtok = (dg2 @ w1r.t()).view(B, h, w, cin)
        dweight = (tok2.t() @ dg2).view(cin, 3, 3, cmid).permute(3, 0, 1, 2).contiguous()
        # bias gradient = sum of dz over the pixels = sum of the CENTRE tap's low-resolution gradient: that tap is never clipped and the
        # bilinear weights of a pixel sum to one, so the adjoint has already done the 17 GB reduction (a torch sum over dz: 4 + 2 ms a step)
        dbias = dg9[:, :, :, 4, :].sum(dim=(0, 1, 2)) if has_bias else None
        return dtok, dweight, dbias, None, None


def upconv3x3_train(tok: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], height: int, width: int) -> torch.Tensor:
    """Differentiable conv3x3(interpolate(f)) for NHWC encoder tokens [B,h,w,Cin] -> [B,Cmid,H,W]."""
    return _UpConv3x3.apply(tok.contiguous(), weight, bias, int(height), int(width))


def upconv3x3_train_supported(cin: int, cmid: int, h: int, w: int, height: int, width: int) -> bool:
    return cmid % 32 == 0 and cmid <= 256 and height >= 32 * h and width >= 32 * w


def aspp_depthwise3(x_nhwc: torch.Tensor, wdw: torch.Tensor, rates) -> torch.Tensor:
    """Depthwise halves of smp's three ASPPSeparableConv branches in one pass.
    x [B,h,w,C] NHWC, wdw [3,9,C] -> [3,B,h,w,C]."""
    x = x_nhwc.contiguous()
    b, h, w, c = x.shape
    out = torch.empty(3, b, h, w, c, dtype=torch.float32, device=x.device)
    N.call("awseg_aspp_depthwise3", N.ptr(x), b, h, w, c, N.ptr(wdw.contiguous()), int(rates[0]), int(rates[1]),
                                          int(rates[2]), N.ptr(out), N.stream())
    return out


def aspp_depthwise3_mean(x_nhwc: torch.Tensor, wdw: torch.Tensor, rates):
    """aspp_depthwise3 that also returns the per-image channel means [B,C] of x (ASPPPooling's global average) from the same pass;
    the mean is None where the kernel that can do it does not take the shape (the caller then reduces x itself)."""
    x = x_nhwc.contiguous()
    b, h, w, c = x.shape
    out = torch.empty(3, b, h, w, c, dtype=torch.float32, device=x.device)
    mean = torch.empty(b, c, dtype=torch.float32, device=x.device)
    rc = N.try_call("awseg_aspp_depthwise3_mean", N.ptr(x), b, h, w, c, N.ptr(wdw.contiguous()), int(rates[0]), int(rates[1]), int(rates[2]),
                    N.ptr(out), N.ptr(mean), N.stream())
    if rc != 0:
        return aspp_depthwise3(x, wdw, rates), None
    return out, mean


# ----------------------------------------------------------------------------- backbone helpers
def dwconv3x3_nhwc(x: torch.Tensor, w9: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = 0,
                   dilation: int = 1) -> torch.Tensor:
    """Depthwise 3x3 (stride 1, zero pad = dilation) on [B,H,W,C] float32 with fused bias + activation.
    w9 [9,C] (tap-major).  act: 0 none, 1 ReLU, 2 exact GELU."""
    x = x.contiguous()
    b, h, w, c = x.shape
    out = torch.empty_like(x)
    N.call("awseg_dwconv3x3_nhwc", N.ptr(x), b, h, w, c, int(dilation), N.ptr(w9.contiguous()),
           N.ptr(None if bias is None else bias.contiguous()), int(act), N.ptr(out), N.stream())
    return out


def dwconv3x3_wgrad_nhwc(x: torch.Tensor, dy: torch.Tensor, dilation: int = 1, want_bias: bool = True):
    """Weight (and bias) gradient of the depthwise 3x3 on NHWC tensors: (dW9 [9,C] tap-major, db [C] or None)."""
    x, dy = x.contiguous(), dy.contiguous()
    b, h, w, c = x.shape
    ws = N.workspace.get(x.device, N.lib().awseg_dwconv3x3_wgrad_workspace(b, h, w, c), tag="dwgrad")
    dw9 = torch.empty(9, c, dtype=torch.float32, device=x.device)
    db = torch.empty(c, dtype=torch.float32, device=x.device) if want_bias else None
    N.call("awseg_dwconv3x3_wgrad_nhwc", N.ptr(x), N.ptr(dy), b, h, w, c, int(dilation), N.ptr(ws), N.ptr(dw9), N.ptr(db), N.stream())
    return dw9, db


DW_TRAIN = os.environ.get("AWSEG_DW_TRAIN", "1") != "0"          # depthwise 3x3 convolutions of the TRAINING graph on this repo's kernels


class _DepthwiseConv3x3NHWC(torch.autograd.Function):
    """Depthwise 3x3 (stride 1, padding = dilation, groups = channels) on an NHWC tensor under autograd: forward and input gradient on
    awseg_dwconv3x3_nhwc (the gradient with flipped taps), weight / bias gradient on awseg_dwconv3x3_wgrad_nhwc.  MIOpen's
    immediate-mode picks for these layers cost 37 ms (weight gradient), 5 ms (input gradient) and 6 ms (forward) per call at
    1024x2048 — 14 + 14 + 8 calls a training step (profiles/r03_train_step_kernels.csv)."""

    @staticmethod
    def forward(ctx, x, weight, bias, dilation):
        c = weight.shape[0]
        w9 = weight.view(c, 9).t().contiguous()
        ctx.save_for_backward(x, weight)
        ctx.dilation, ctx.has_bias = int(dilation), bias is not None
        return dwconv3x3_nhwc(x, w9, bias, 0, dilation=dilation)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        c = weight.shape[0]
        g = g.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dwconv3x3_nhwc(g, weight.view(c, 9).flip(1).t().contiguous(), None, 0, dilation=ctx.dilation)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw9, db = dwconv3x3_wgrad_nhwc(x, g, ctx.dilation, want_bias=ctx.has_bias)
            dw = dw9.t().reshape(c, 1, 3, 3)
        return dx, dw, db, None


def depthwise_conv3x3_train_ok(conv, x: torch.Tensor) -> bool:
    """An nn.Conv2d this Function computes: depthwise 3x3, stride 1, padding == dilation, float32 on the GPU, C % 4 == 0."""
    return (DW_TRAIN and x.is_cuda and x.dtype == torch.float32 and conv.kernel_size == (3, 3) and conv.stride == (1, 1)
            and conv.groups == conv.in_channels == conv.out_channels and conv.padding == conv.dilation and conv.dilation[0] == conv.dilation[1]
            and conv.in_channels % 4 == 0 and conv.padding_mode == "zeros")


def depthwise_conv3x3_nhwc_train(x_nhwc: torch.Tensor, conv) -> torch.Tensor:
    return _DepthwiseConv3x3NHWC.apply(x_nhwc, conv.weight, conv.bias, conv.dilation[0])


BN_TRAIN = os.environ.get("AWSEG_BN_TRAIN", "1") != "0"          # BatchNorm2d -> ReLU -> Dropout2d of the training heads as fused HIP passes


class _BNReLUDropout2d(torch.autograd.Function):
    """BatchNorm2d (batch statistics) -> ReLU -> Dropout2d(p) on an NCHW map under autograd (csrc/bntrain.hip): one forward pass
    and two backward passes instead of ~15, and autograd keeps x + two per-channel vectors + the [B, C] noise instead of three
    full-size maps.  The Dropout2d mask is drawn exactly as F.dropout2d draws it (a [B, C, 1, 1] Bernoulli(1 - p) / (1 - p) from the
    device generator), so a seeded run consumes the same random numbers as the module graph."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, p, dx_channels_last=False):
        ctx.dx_cl = bool(dx_channels_last) and x.shape[1] % 32 == 0
        b, c, h, w = x.shape
        hw = h * w
        ws = N.workspace.get(x.device, N.lib().awseg_bn_train_workspace(b, c, hw), tag="bntrain")
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        var = torch.empty_like(mean)
        N.call("awseg_bn_train_stats", N.ptr(x), b, c, hw, N.ptr(ws), N.ptr(mean), N.ptr(var), N.stream())
        invstd = torch.rsqrt(var + eps)
        if running_mean is not None and momentum is not None:
            n = b * hw
            running_mean.mul_(1.0 - momentum).add_(mean, alpha=momentum)
            running_var.mul_(1.0 - momentum).add_(var, alpha=momentum * n / max(n - 1, 1))       # running statistics keep the UNBIASED variance
        noise = None
        if p > 0.0:
            noise = x.new_empty(b, c, 1, 1).bernoulli_(1.0 - p).div_(1.0 - p)                      # F.dropout2d's own draw
        out = torch.empty_like(x)
        N.call("awseg_bn_relu_dropout_forward", N.ptr(x), b, c, hw, N.ptr(mean), N.ptr(invstd), N.ptr(gamma.contiguous()), N.ptr(beta.contiguous()),
               N.ptr(None if noise is None else noise.view(b, c)), N.ptr(out), N.stream())
        ctx.save_for_backward(x, gamma, beta, mean, invstd, noise if noise is not None else mean.new_empty(0))
        ctx.has_noise = noise is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, gamma, beta, mean, invstd, noise = ctx.saved_tensors
        b, c, h, w = x.shape
        hw = h * w
        g = g.contiguous()
        ws = N.workspace.get(x.device, N.lib().awseg_bn_train_workspace(b, c, hw), tag="bntrain")
        dgamma, dbeta = torch.empty_like(mean), torch.empty_like(mean)
        # dx_cl: the gradient leaves as an NCHW tensor over channels-last MEMORY — the layout the producer's backward reads (ops._UpConv3x3)
        dx = torch.empty(b, h, w, c, dtype=x.dtype, device=x.device) if ctx.dx_cl else torch.empty_like(x)
        N.call("awseg_bn_relu_dropout_backward", N.ptr(x), N.ptr(g), b, c, hw, N.ptr(mean), N.ptr(invstd), N.ptr(gamma.contiguous()),
               N.ptr(beta.contiguous()), N.ptr(noise.view(b, c) if ctx.has_noise else None), N.ptr(ws), N.ptr(dgamma), N.ptr(dbeta), N.ptr(dx),
               int(ctx.dx_cl), N.stream())
        if ctx.dx_cl:
            dx = dx.permute(0, 3, 1, 2)
        return dx, dgamma, dbeta, None, None, None, None, None, None


def bn_relu_dropout2d_train_ok(x: torch.Tensor, bn, relu, drop) -> bool:
    """The module triple this Function computes: a training-mode affine BatchNorm2d with running statistics, nn.ReLU, and an
    nn.Dropout2d (or None) in training mode, on a contiguous float32 NCHW map on the GPU whose planes are whole float4s."""
    import torch.nn as nn
    return (BN_TRAIN and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
            and (x.shape[2] * x.shape[3]) % 4 == 0 and isinstance(bn, nn.BatchNorm2d) and bn.training and bn.affine
            and bn.track_running_stats and bn.momentum is not None and isinstance(relu, nn.ReLU)
            and (drop is None or (isinstance(drop, nn.Dropout2d) and drop.training)) and x.shape[0] <= 65535 and x.shape[1] <= 65535)


def bn_relu_dropout2d_train(x: torch.Tensor, bn, drop=None, dx_channels_last: bool = False) -> torch.Tensor:
    """dx_channels_last: hand the input gradient back over channels-last memory (for a producer whose backward reads NHWC)."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BNReLUDropout2d.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, 0.0 if drop is None else float(drop.p),
                                  dx_channels_last)


def bias_act_nhwc_(x_nhwc: torch.Tensor, bias: Optional[torch.Tensor], residual: Optional[torch.Tensor] = None,
                   act: int = 0) -> torch.Tensor:
    """In place: x = act(x + bias[c] (+ residual)) on a contiguous [..., C] float32 tensor."""
    c = x_nhwc.shape[-1]
    N.call("awseg_bias_act_nhwc", N.ptr(x_nhwc), x_nhwc.numel() // c, c, N.ptr(bias), N.ptr(residual), int(act), N.stream())
    return x_nhwc


def winograd_weights(weight: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,3,3] filters (times an optional per-Cout scale) -> U = G g G^T in the kernel's LDS
    image order [Cin/8][16 positions][2][Cout][4]: input channel 8*chunk + 4*(s>>1) + 2*hk + (s&1) at
    [chunk][p][hk][n][s] (include/awseg.h), computed in float64 and rounded once.  Cin % 16 == 0."""
    g = weight.double()
    if scale is not None:
        g = g * scale.double().view(-1, 1, 1, 1)
    cout, cin = weight.shape[0], weight.shape[1]
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=weight.device)
    # channel within a chunk = 4*s_hi + 2*hk + s_lo with s = 2*s_hi + s_lo
    u = torch.einsum("ik,ockl,jl->ijco", G, g, G).reshape(16, cin // 8, 2, 2, 2, cout)   # [p][chunk][s_hi][hk][s_lo][n]
    return u.permute(1, 0, 3, 5, 2, 4).reshape(cin // 8, 16, 2, cout, 4).float().contiguous()   # [chunk][p][hk][n][s]


def conv3x3_winograd(x: torch.Tensor, u: torch.Tensor, shift: torch.Tensor, act: int = 0, dilation: int = 1,
                     residual: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
                     b2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x float32 [B,H,W,Cin] NHWC -> [B,H,W,Cout] (or [B,H,W] with the fused 1x1 + sigmoid head)."""
    x = x.contiguous()
    b, h, w, cin = x.shape
    cout = u.shape[3]
    out = torch.empty((b, h, w) if w2 is not None else (b, h, w, cout), dtype=torch.float32, device=x.device)
    N.call("awseg_conv3x3_winograd_nhwc", N.ptr(x), b, h, w, cin, cout, dilation, N.ptr(u), N.ptr(shift.contiguous()),
           N.ptr(None if residual is None else residual.contiguous()), act, N.ptr(None if w2 is None else w2.contiguous()),
           N.ptr(None if b2 is None else b2.contiguous()), N.ptr(out), N.stream())
    return out


# 3x3 convolutions: 1 = Winograd on split-operand f16 MFMA (csrc/wino_split.hip), 0 = Winograd on float32-input MFMA
WINO_SPLIT = os.environ.get("AWSEG_WINO_SPLIT", "1") != "0"

def winograd_split_weights(weight: torch.Tensor, scale: Optional[torch.Tensor] = None, bf16: bool = False) -> torch.Tensor:
    """[Cout,Cin,3,3] filters (times an optional per-Cout scale) -> the split-operand image of U = G g G^T that
    awseg_conv3x3_winograd_split_nhwc reads (include/awseg.h): f16 high and low parts of U * 2^-eu in the B-fragment
    order [Cin/16][16][Cout/32][hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15][32][8], then 2^eu as one float32.  eu brings
    max|U| into [2^13, 2^14); it is computed on the device (no host synchronisation).  int16 tensor, 16-byte aligned."""
    g = weight.double()
    if scale is not None:
        g = g * scale.double().view(-1, 1, 1, 1)
    cout, cin = weight.shape[0], weight.shape[1]
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=weight.device)
    u = torch.einsum("ik,ockl,jl->ijco", G, g, G).reshape(16, cin, cout)                   # [p][ci][co], float64
    mx = u.abs().max()
    e = torch.where(mx > 0, torch.floor(torch.log2(mx.clamp_min(1e-300))) - 13.0, torch.zeros_like(mx))
    us = u * torch.exp2(-e)
    if bf16:
        hi = us.to(torch.bfloat16).view(torch.int16)
        lo = torch.zeros_like(hi)
    else:
        hi = us.to(torch.float16)
        lo = (us - hi.double()).to(torch.float16).view(torch.int16)
        hi = hi.view(torch.int16)
    nch, ncb = cin // 16, cout // 32

    def frag(t):                                                                          # -> [nch][16][ncb][h][32][8]
        return t.view(16, nch, 2, 8, ncb, 32).permute(1, 0, 4, 2, 5, 3)
    img = torch.stack([frag(hi), frag(lo)], dim=3).reshape(-1).contiguous()               # [nch][16][ncb][hi/lo][h][32][8]
    n = img.numel()
    buf = torch.zeros(n + 8, dtype=torch.int16, device=weight.device)
    buf[:n] = img
    buf[n:n + 2] = torch.exp2(e).to(torch.float32).reshape(1).view(torch.int16)
    return buf


def conv3x3_winograd_split(x: torch.Tensor, u_split: torch.Tensor, cout: int, shift: torch.Tensor, act: int = 0, dilation: int = 1,
                           residual: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
                           b2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv3x3_winograd on the split-operand f16-MFMA kernel: x float32 [B,H,W,Cin] NHWC, u_split = winograd_split_weights(...)."""
    x = x.contiguous()
    b, h, w, cin = x.shape
    need = N.lib().awseg_winograd_split_weight_halfs(cin, cout)
    if need < 0 or u_split.numel() != need + 8:
        raise N.AwsegError(f"u_split does not match Cin {cin}, Cout {cout} (expected {need} + 8 int16)")
    out = torch.empty((b, h, w) if w2 is not None else (b, h, w, cout), dtype=torch.float32, device=x.device)
    N.call("awseg_conv3x3_winograd_split_nhwc", N.ptr(x), b, h, w, cin, cout, dilation, N.ptr(u_split), N.ptr(shift.contiguous()),
           N.ptr(None if residual is None else residual.contiguous()), act, N.ptr(None if w2 is None else w2.contiguous()),
           N.ptr(None if b2 is None else b2.contiguous()), N.ptr(out), N.stream())
    return out


MIXFFN_FUSED = os.environ.get("AWSEG_MIXFFN_FUSED", "1") != "0"  # MiT Mix-FFN (LN -> fc1 -> dw3x3 + GELU -> fc2 + residual) as one tile kernel


def mixffn_split_weights(w: torch.Tensor) -> torch.Tensor:
    """float32 [N,K] -> float16 [2,N,K]: f16(v) and f16(v - f16(v)) of v = w 2^-e, e = floor(log2 max|w|) - 13 (clamped to
    [-126, 1]), so the low parts of small weights are not f16 subnormals — the operand images awseg_mixffn_fused multiplies.
    e rides on the tensor as `_awseg_exp` (awseg_mixffn_fused takes it as an argument); one host synchronisation (callers cache
    the images per parameter version)."""
    w = w.contiguous().float()
    m = float(w.abs().max().item())
    e = 0 if (m == 0.0 or not math.isfinite(m)) else min(1, max(-126, math.frexp(m)[1] - 14))
    v = torch.ldexp(w, torch.tensor(float(-e), device=w.device))
    hi = v.to(torch.float16)
    img = torch.stack([hi, (v - hi.float()).to(torch.float16)]).contiguous()
    img._awseg_exp = e
    return img


def mixffn_fused(tok: torch.Tensor, gamma, beta, eps: float, w1, b1, dw_taps, dw_bias, w2, b2, w1_split=None, w2_split=None,
                 checked: bool = False) -> Optional[torch.Tensor]:
    """tok + fc2(gelu(dwconv3x3(fc1(layernorm(tok))))) on NHWC tokens [B,H,W,C] in one launch (csrc/mixffn.hip); None when the
    kernel does not take the problem (C not 32 / 64, hidden != 4C, weights or LayerNorm parameters beyond the f16 operand range):
    the caller keeps its separate launches.  `checked`: the caller has verified the range conditions (mixffn_operands_ok) —
    otherwise they are checked here, which synchronises the host with the device."""
    b, h, w, c = tok.shape
    if c not in (32, 64) or w1.shape != (4 * c, c) or w2.shape != (c, 4 * c) or dw_taps.shape != (9, 4 * c):
        return None
    if not checked and not mixffn_operands_ok(gamma, beta, w1, w2):
        return None
    tok = tok.contiguous()
    out = torch.empty_like(tok)
    w1s = w1_split if w1_split is not None else mixffn_split_weights(w1)
    w2s = w2_split if w2_split is not None else mixffn_split_weights(w2)
    e1, e2 = getattr(w1s, "_awseg_exp", None), getattr(w2s, "_awseg_exp", None)
    if e1 is None or e2 is None:
        raise N.AwsegError("mixffn weight images without their exponent: pass what mixffn_split_weights returned, not a copy")
    rc = N.try_call("awseg_mixffn_fused", N.ptr(tok), b, h, w, c, N.ptr(gamma.contiguous()), N.ptr(beta.contiguous()), float(eps),
                    N.ptr(w1s), int(e1), N.ptr(b1.contiguous()), N.ptr(dw_taps.contiguous()), N.ptr(dw_bias.contiguous()),
                    N.ptr(w2s), int(e2), N.ptr(w2.contiguous()), N.ptr(b2.contiguous()), N.ptr(out), N.stream())
    return out if rc == 0 else None


def mixffn_operands_ok(gamma, beta, w1, w2) -> bool:
    """The f16 operand range of awseg_mixffn_fused: |w| < 2^15 and the LayerNorm outputs' bound max|gamma| sqrt(C) + max|beta| < 2^15
    (one host synchronisation: callers cache the answer per parameter version)."""
    c = gamma.numel()
    lim = 32768.0
    vals = torch.stack([gamma.abs().max() * (c ** 0.5) + beta.abs().max(), w1.abs().max(), w2.abs().max()])
    return bool(torch.isfinite(vals).all().item()) and bool((vals < lim).all().item())


TWO_STREAMS = os.environ.get("AWSEG_TWO_STREAMS", "1") != "0"    # ensemble eval: DeepLabV3+ on a side stream beside SegFormer (0: one stream)
DEPTH_FUSED = os.environ.get("AWSEG_DEPTH_FUSED", "1") != "0"    # the SegFormer depth head as one full-resolution launch (depthfuse.hip)


def upconv_forms(g9: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """The bilinear forms of relu(shift + conv3x3(interpolate_x32(f))) per frame (csrc/depthfuse.hip): float32 [B, F4 | F2] from
    g9 float32 [B,h,w,9,Cmid] (the per-tap products at the encoder's resolution, BatchNorm scale folded) and the folded shift."""
    g9 = g9.contiguous()
    b, h, w, nine, cmid = g9.shape
    assert nine == 9
    per = N.lib().awseg_upconv_forms_floats(h, w, cmid)
    forms = torch.empty(b, per, dtype=torch.float32, device=g9.device)
    N.call("awseg_upconv_forms", N.ptr(g9), b, cmid, h, w, N.ptr(shift.contiguous()), N.ptr(forms), N.stream())
    return forms


def depth_head_fused(forms: torch.Tensor, h: int, w: int, cmid: int, u_image: torch.Tensor, shift2: torch.Tensor, w2: torch.Tensor,
                     b2: torch.Tensor, bf16: bool = False) -> torch.Tensor:
    """sigmoid(conv1x1(relu(bn(conv3x3(relu(bn(conv3x3(interpolate(f)))))))) at [B, 32h, 32w] in ONE launch from the forms of
    upconv_forms: the hidden map between the two 3x3 convolutions is generated tile by tile inside the Winograd kernel.
    u_image = winograd_split_weights / winograd_bf16_weights of the SECOND 3x3 (Cmid -> 64)."""
    b = forms.shape[0]
    need = N.lib().awseg_winograd_split_weight_halfs(cmid, 64)
    if need < 0 or u_image.numel() != need + 8 or forms.shape[1] != N.lib().awseg_upconv_forms_floats(h, w, cmid):
        raise N.AwsegError(f"depth_head_fused: operands do not match h {h}, w {w}, Cmid {cmid}")
    out = torch.empty(b, 32 * h, 32 * w, dtype=torch.float32, device=forms.device)
    N.call("awseg_depth_head_fused", N.ptr(forms), b, h, w, cmid, N.ptr(u_image), int(bf16), N.ptr(shift2.contiguous()),
           N.ptr(w2.contiguous()), N.ptr(b2.contiguous()), N.ptr(out), N.stream())
    return out


GEMM_WORKSPACE_BYTES = 32 << 20
GEMM_TUNE = os.environ.get("AWSEG_GEMM_TUNE", "0") != "0"      # opt-in: time hipBLASLt's candidates once per new problem shape
# (measured on the bench step: 102.0 vs 101.8 images/s — the library's first-ranked algorithm is already the fastest here)
_gemm_tuned = set()


def gemm_bias_act(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, act: int = 0, residual: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, w_split: Optional[torch.Tensor] = None, split: Optional[bool] = None) -> torch.Tensor:
    """act(x[M,K] @ w[N,K]^T + bias (+ residual[M,N])) in one launch with the epilogue fused; `out` may be `residual`.
    Problems gemm_wants_split() accepts run on the split-operand f16-MFMA kernel (float32-grade, csrc/gemm_split.hip;
    pass `w_split = gemm_split_weights(w)` to reuse the split weights, else they are split on the fly); the rest is one
    hipBLASLt float32 call.  split=True/False overrides the choice.  With AWSEG_GEMM_TUNE=1 the first hipBLASLt call
    of a new (M,N,K,residual,act) times the library's candidate algorithms (synchronising, once)."""
    x, w = x.contiguous(), w.contiguous()
    m, k = x.shape
    n = w.shape[0]
    bias = bias.contiguous()
    if split is None and gemm_wants_bf16(m, n, k):
        wb = w_split if (w_split is not None and getattr(w_split, "_awseg_bf16", False)) else gemm_bf16_weights(w)
        return gemm_bf16_bias_act(x, wb, bias, act, residual=residual, out=out)
    if gemm_wants_split(m, n, k) if split is None else split:
        return gemm_split_bias_act(x, w_split if w_split is not None else gemm_split_weights(w), bias, act, residual=residual, out=out)
    ws = N.workspace.get(x.device, GEMM_WORKSPACE_BYTES, tag="gemm%d" % torch.cuda.current_stream(x.device).cuda_stream)   # one per stream (TWO_STREAMS)
    key = (str(x.device), m, n, k, residual is not None, act)
    if GEMM_TUNE and m > 0 and key not in _gemm_tuned:
        _gemm_tuned.add(key)
        scratch = torch.empty(m, n, dtype=torch.float32, device=x.device)
        rc = N.lib().awseg_gemm_tune(N.ptr(x), N.ptr(w), N.ptr(bias), int(residual is not None), act, N.ptr(scratch), m, n, k,
                                     N.ptr(ws), GEMM_WORKSPACE_BYTES, N.stream())
        if rc < 0:
            N.check(rc, "awseg_gemm_tune")
        del scratch
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    N.call("awseg_gemm_bias_act", N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(residual), act, N.ptr(out), m, n, k,
           N.ptr(ws), GEMM_WORKSPACE_BYTES, N.stream())
    return out


# 1x1 convolutions / Linear layers on the split-operand f16-MFMA GEMM (csrc/gemm_split.hip): faster than hipBLASLt's
# float32 kernels on every ResNet / ASPP / decoder shape measured (tools/kernel_bench.py "gemm"), including the HBM-bound
# ones; narrow outputs (N < 128 = one block tile) stay on the library.  AWSEG_GEMM_SPLIT=0 turns the split path off.
GEMM_SPLIT = os.environ.get("AWSEG_GEMM_SPLIT", "1") != "0"
GEMM_SPLIT_MIN_M, GEMM_SPLIT_MIN_N, GEMM_SPLIT_MIN_K = 128, 128, 64
GEMM_SPLIT_N64 = os.environ.get("AWSEG_GEMM_SPLIT_N64", "1") != "0"


GEMM_SPLIT_NARROW = os.environ.get("AWSEG_GEMM_SPLIT_NARROW", "1") != "0"
STRIDED_UPSAMPLE = os.environ.get("AWSEG_STRIDED_UPSAMPLE", "0") != "0"   # off: see upsample_bilinear
KV_PACKED = os.environ.get("AWSEG_KV_PACKED", "1") != "0"              # key + value projections as one GEMM, packed rows into attention
SMALL_CONV_SPLIT = os.environ.get("AWSEG_SMALL_CONV_SPLIT", "1") != "0"  # gathered-operand GEMM for the small patch convolutions too


def gemm_wants_split(m: int, n: int, k: int) -> bool:
    if not GEMM_SPLIT or k % 8:
        return False
    # N < 64 on 10^6 rows (DeepLabV3+'s 48-channel skip projection and 19-class head, MiT stage 1's 32-channel projections): one
    # masked 64-column tile of the LDS-DMA kernel, 128 rows a block — these launches are bound by reading x once
    if GEMM_SPLIT_NARROW and 8 <= n < 64 and k >= 32 and m >= (1 << 18):
        return True
    if GEMM_SPLIT_NARROW and n % 64 == 0 and k == 32 and m >= (1 << 18):      # MiT stage 1's fc1 (32 -> 128): a single K tile
        return True
    if m < GEMM_SPLIT_MIN_M or k < GEMM_SPLIT_MIN_K:
        return False
    # N = 64 (ResNet layer1 conv1, MiT stage-2 projections): only where the LDS-DMA kernel's 256 x 64 tiles fill the chip
    return n >= GEMM_SPLIT_MIN_N or (n == 64 and GEMM_SPLIT_N64 and ((m + 255) // 256) >= 128)


def gemm_split_weights(w: torch.Tensor) -> torch.Tensor:
    """w float32 [N,K] -> int16 [2,N,K]: f16 bit patterns of the high parts and of the scaled low parts of
    w * 2^-ew (ew normalises max|w| into [2^13, 2^14)).  The returned tensor is a view of a buffer that is 16 bytes
    longer: the trailer holds {max|w| bits, ew} and is read by awseg_gemm_split_bias_act — pass the view on as it is
    (a clone would drop the trailer)."""
    w = w.contiguous()
    n, k = w.shape
    # room for the classic [2][N][K] image, the 16-byte trailer and — K % 32 == 0 — the k-blocked image of gemm_split3.hip
    buf = torch.empty(int(N.lib().awseg_gemm_split_weight_halfs(n, k)), dtype=torch.int16, device=w.device)
    N.call("awseg_gemm_split_weights", N.ptr(w), n, k, N.ptr(buf), N.stream())
    return buf[:2 * n * k].view(2, n, k)


def _split_weights_intact(w_split: torch.Tensor, n: int, k: int) -> bool:
    """the view gemm_split_weights returned still sits in front of its trailer (+ k-blocked image): a clone would drop them"""
    return w_split.untyped_storage().nbytes() - w_split.storage_offset() * 2 >= int(N.lib().awseg_gemm_split_weight_halfs(n, k)) * 2


def gemm_split_bias_act(x: torch.Tensor, w_split: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0,
                        residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x[M,K] @ w[N,K]^T + bias (+ residual[M,N])) with w given as gemm_split_weights(w); `out` may be `residual`."""
    x = x.contiguous()
    m, k = x.shape
    n = w_split.shape[1]
    if not _split_weights_intact(w_split, n, k):
        raise N.AwsegError("w_split lost its 16-byte trailer (weight exponent): pass the tensor gemm_split_weights returned, not a copy")
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    N.call("awseg_gemm_split_bias_act", N.ptr(x), N.ptr(w_split), N.ptr(bias), N.ptr(residual), act, N.ptr(out), m, n, k, N.stream())
    return out


def stem_rows_weights(w: torch.Tensor) -> torch.Tensor:
    """[N, C <= 4, kh, kw <= 8] convolution weights -> the [N, kh * 32] matrix of awseg_conv_rows_gemm_split_bias_act
    (column ky * 32 + kx * 4 + c, zeros elsewhere)."""
    n, c, kh, kw = w.shape
    if c > 4 or kw > 8:
        raise N.AwsegError("stem_rows_weights: at most 4 input channels and 8 kernel columns")
    m = torch.zeros(n, kh, 8, 4, dtype=torch.float32, device=w.device)
    m[:, :, :kw, :c] = w.permute(0, 2, 3, 1)
    return m.view(n, kh * 32)


def conv_rows_gemm_split(x_padded: torch.Tensor, w_split: torch.Tensor, bias: Optional[torch.Tensor], act: int, kernel_h: int,
                         stride: int, pad_y: int, out_width: int) -> Optional[torch.Tensor]:
    """The 7x7 stem as one split-operand GEMM (awseg_conv_rows_gemm_split_bias_act): x_padded float32 [B, H, W + pads, 4] with
    zero padding columns / channel, w_split = gemm_split_weights(stem_rows_weights(w)).  Returns [B, Ho, out_width, N], or None
    when the LDS-DMA kernel does not take the shape (the caller keeps its other path)."""
    b, h, wp, pf = x_padded.shape
    n, k = w_split.shape[1], w_split.shape[2]
    if k != kernel_h * 32 or not x_padded.is_contiguous():
        raise N.AwsegError("conv_rows_gemm_split: weights must be [N, kernel_h * 32] and the image contiguous")
    if not _split_weights_intact(w_split, n, k):
        raise N.AwsegError("w_split lost its 16-byte trailer (weight exponent): pass the tensor gemm_split_weights returned, not a copy")
    ho = (h + 2 * pad_y - kernel_h) // stride + 1
    out = torch.empty(b, ho, out_width, n, dtype=torch.float32, device=x_padded.device)
    rc = N.try_call("awseg_conv_rows_gemm_split_bias_act", N.ptr(x_padded), b, h, wp, pf, kernel_h, stride, pad_y, out_width,
                    N.ptr(w_split), N.ptr(bias), None, act, N.ptr(out), n, N.stream())
    return out if rc == 0 else None


# strided / patch convolutions: gather the A operand inside the split GEMM (default) or write the im2col matrix first (AWSEG_CONV_GATHER=0)
CONV_GATHER = os.environ.get("AWSEG_CONV_GATHER", "1") != "0"


ASPP_PIECES = os.environ.get("AWSEG_ASPP_PIECES", "1") != "0"          # ASPP projection: one GEMM over the four pixel branches
DUAL_TAIL = os.environ.get("AWSEG_DUAL_TAIL", "1") != "0"             # first bottleneck of a ResNet stage: conv3 + downsample branch as one GEMM


def gemm_split_dual(x: torch.Tensor, x2: torch.Tensor, w_split: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0, stride: int = 0,
                    residual: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """act([x | x2] @ w^T + bias (+ residual)) with the A operand in two pieces along K: x [M,k1] rows; x2 [M,k2] rows (stride 0) or an
    NHWC image [B,H,W,k2] whose pixels (b, oy*stride, ox*stride) are the rows (a strided 1x1 convolution folded into the product).
    w_split = gemm_split_weights(w [N,k1+k2]).  Returns None when the LDS-DMA kernel does not take the shape (the caller then runs
    the two products separately)."""
    x, x2 = x.contiguous(), x2.contiguous()
    m, k1 = x.shape
    k2 = x2.shape[-1]
    n = w_split.shape[1]
    if w_split.shape[2] != k1 + k2:
        raise N.AwsegError(f"gemm_split_dual: weights have K = {w_split.shape[2]}, the operands {k1} + {k2}")
    if not _split_weights_intact(w_split, n, k1 + k2):
        raise N.AwsegError("w_split lost its 16-byte trailer (weight exponent): pass the tensor gemm_split_weights returned, not a copy")
    if stride > 0:
        b, h, w = x2.shape[0], x2.shape[1], x2.shape[2]
    else:
        b, h, w = 1, 1, 1
        if x2.numel() != m * k2:
            raise N.AwsegError("gemm_split_dual: x2 has a different row count than x")
    out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    rc = N.try_call("awseg_gemm_split_dual_bias_act", N.ptr(x), k1, N.ptr(x2), k2, b, h, w, int(stride), N.ptr(w_split), N.ptr(bias),
                    N.ptr(residual), act, N.ptr(out), m, n, N.stream())
    return out if rc == 0 else None


def gemm_split_pieces(pieces, w_split: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0, residual: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """act(cat(pieces, dim=1) @ w^T + bias (+ residual)) for 2 .. 4 equally wide row matrices [M,k] without the concatenation (one GEMM
    whose A operand is fetched piece by piece); `out` may be `residual`.  None when the LDS-DMA kernel does not take the shape."""
    import ctypes
    pieces = [p_.contiguous() for p_ in pieces]
    m, kp = pieces[0].shape
    n = w_split.shape[1]
    if any(p_.shape != (m, kp) for p_ in pieces) or w_split.shape[2] != kp * len(pieces):
        raise N.AwsegError("gemm_split_pieces: the pieces must be equally shaped and the weights [N, pieces * k]")
    if not _split_weights_intact(w_split, n, kp * len(pieces)):
        raise N.AwsegError("w_split lost its 16-byte trailer (weight exponent): pass the tensor gemm_split_weights returned, not a copy")
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=pieces[0].device)
    arr = (ctypes.c_void_p * len(pieces))(*[p_.data_ptr() for p_ in pieces])
    rc = N.try_call("awseg_gemm_split_pieces_bias_act", ctypes.cast(arr, ctypes.c_void_p), len(pieces), kp, N.ptr(w_split), N.ptr(bias),
                    N.ptr(residual), act, N.ptr(out), m, n, N.stream())
    return out if rc == 0 else None


def conv_gemm_split(x: torch.Tensor, w_split: torch.Tensor, bias: Optional[torch.Tensor], act: int, kh: int, kw: int, stride: int,
                    pad: int, dilation: int = 1, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv2d on a float32 NHWC tensor [B,H,W,C] (C % 32 == 0) as one split-operand GEMM whose A operand is gathered from x
    while it is staged — the im2col matrix of `im2col_nhwc` is never written.  w_split = gemm_split_weights(w2) with
    w2 [N, kh*kw*C] in (ky, kx, c) column order.  Returns [B,Ho,Wo,N]; bit-identical to im2col_nhwc + gemm_split_bias_act."""
    x = x.contiguous()
    b, h, w, c = x.shape
    n, k = w_split.shape[1], w_split.shape[2]
    if k != kh * kw * c:
        raise N.AwsegError(f"conv_gemm_split: weights have K = {k}, the convolution needs {kh * kw * c}")
    if not _split_weights_intact(w_split, n, k):
        raise N.AwsegError("w_split lost its 16-byte trailer (weight exponent): pass the tensor gemm_split_weights returned, not a copy")
    ho = (h + 2 * pad - dilation * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dilation * (kw - 1) - 1) // stride + 1
    out = torch.empty(b, ho, wo, n, dtype=torch.float32, device=x.device)
    N.call("awseg_conv_gemm_split_bias_act", N.ptr(x), b, h, w, c, kh, kw, stride, pad, dilation, N.ptr(w_split), N.ptr(bias),
           N.ptr(residual), act, N.ptr(out), n, N.stream())
    return out


def im2col_nhwc(x: torch.Tensor, kh: int, kw: int, stride: int, pad: int, dilation: int = 1, k_padded: Optional[int] = None):
    """x float32 [B,H,W,C] -> (cols [B*Ho*Wo, k_padded], Ho, Wo): column (ky*kw + kx)*C + c, zero padded (awseg.h)."""
    x = x.contiguous()
    b, h, w, c = x.shape
    k = kh * kw * c
    kp = k if k_padded is None else int(k_padded)
    ho = (h + 2 * pad - dilation * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dilation * (kw - 1) - 1) // stride + 1
    cols = torch.empty(b * ho * wo, kp, dtype=torch.float32, device=x.device)
    N.call("awseg_im2col_nhwc", N.ptr(x), b, h, w, c, kh, kw, stride, pad, dilation, kp, N.ptr(cols), N.stream())
    return cols, ho, wo


def dwconv3x3_upcat(a: torch.Tensor, hi: torch.Tensor, w9: torch.Tensor) -> torch.Tensor:
    """depthwise3x3(cat(bilinear_up_align_corners(a -> hi's size), hi)) on NHWC tensors: a [B,h,w,Ca], hi [B,H,W,Ch],
    w9 [9,Ca+Ch] -> [B,H,W,Ca+Ch] (DeepLabV3+ decoder, no intermediate tensors)."""
    a, hi = a.contiguous(), hi.contiguous()
    b, h, w, ca = a.shape
    _, H, W, ch = hi.shape
    out = torch.empty(b, H, W, ca + ch, dtype=torch.float32, device=a.device)
    N.call("awseg_dwconv3x3_upcat_nhwc", N.ptr(a), h, w, ca, N.ptr(hi), ch, b, H, W, N.ptr(w9.contiguous()), N.ptr(out), N.stream())
    return out


# default attention kernel: 1 = split-operand f16 MFMA (22-bit operands, float32 accumulation: float32-grade results at
# twice the speed, csrc/attn.hip), 0 = float32-input MFMA
ATTENTION_SPLIT = os.environ.get("AWSEG_ATTN_SPLIT", "1") != "0"


def attention_d32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float,
                  split: Optional[bool] = None) -> torch.Tensor:
    """softmax(q k^T * scale) v for head_dim 32: q [B,Nq,heads*32], k / v [B,Nkv,heads*32] (token-major) -> [B,Nq,heads*32].
    split=True runs the split-operand f16-MFMA kernel (22-bit operands, float32 accumulation), False the float32-MFMA
    kernel; None takes the process default (ATTENTION_SPLIT, env AWSEG_ATTN_SPLIT=0/1)."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    b, nq, c = q.shape
    out = torch.empty_like(q)
    if split is None and PRECISION == "bf16":
        sym = "awseg_attention_d32_bf16"
    else:
        sym = "awseg_attention_d32_split" if (ATTENTION_SPLIT if split is None else split) else "awseg_attention_d32"
    if sym == "awseg_attention_d32_split" and _wants_kv_image(nq, k.shape[1]):
        _attention_split_ws(q, k, v, 0, out, b, heads, nq, k.shape[1], scale)
        return out
    N.call(sym, N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(out), b, heads, nq, k.shape[1], float(scale), N.stream())
    return out


ATTN_KV_IMAGE = os.environ.get("AWSEG_ATTN_KV_IMAGE", "1") != "0"     # split-operand attention: keys / values prepared once per launch


def _wants_kv_image(nq: int, nkv: int) -> bool:
    """The prepared image pays where many query blocks share the keys: MiT stages 1 / 2 at the bench shape (64 / 16 queries per key:
    1.148 -> 1.053 ms for stage 1); at 4 queries per key (stage 3: 0.372 -> 0.376 ms) the preparing kernel costs what it saves."""
    return ATTN_KV_IMAGE and nq >= 8 * nkv


def _attention_split_ws(q, k, v, pitch, out, b, heads, nq, nkv, scale):
    """awseg_attention_d32_split_ws on a per-stream scratch workspace (v may be a view into k's rows: packed keys | values)."""
    nbytes = int(N.lib().awseg_attention_d32_split_workspace(b, heads, nkv))
    ws = N.workspace.get(q.device, nbytes, tag="attn%d" % torch.cuda.current_stream(q.device).cuda_stream)
    N.call("awseg_attention_d32_split_ws", N.ptr(q), N.ptr_strided(k), N.ptr_strided(v), int(pitch), N.ptr(out), b, heads, nq, nkv, float(scale),
           N.ptr(ws), N.stream())


def attention_d32_packed_kv(q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float, split: Optional[bool] = None) -> torch.Tensor:
    """attention_d32 with keys and values packed per token: kv [B,Nkv,2*heads*32] = [key | value], as one GEMM over the stacked key /
    value projection weights writes them.  Same kernels, same values."""
    q, kv = q.contiguous(), kv.contiguous()
    b, nq, c = q.shape
    assert kv.shape[-1] == 2 * c
    out = torch.empty_like(q)
    mode = 2 if (split is None and PRECISION == "bf16") else (1 if (ATTENTION_SPLIT if split is None else split) else 0)
    if mode == 1 and _wants_kv_image(nq, kv.shape[1]):
        _attention_split_ws(q, kv, kv[..., c:], 2 * c, out, b, heads, nq, kv.shape[1], scale)
        return out
    N.call("awseg_attention_d32_packed_kv", N.ptr(q), N.ptr(kv), N.ptr(out), b, heads, nq, kv.shape[1], float(scale), mode, N.stream())
    return out


# Compute precision of the dense contractions (1x1 convolutions / Linear layers, 3x3 Winograd convolutions, attention):
# "f32" = float32-grade results (split-operand f16 MFMA or float32-input MFMA, see set_split), "bf16" = one bf16 MFMA per
# product tile with float32 accumulation (BASELINE config 5).  Models switch it for the duration of their forward.
PRECISION = "f32"


class precision:
    """Context manager: `with ops.precision("bf16"): model(x)`."""

    def __init__(self, dtype: Optional[str]):
        self.dtype = {None: None, "f32": "f32", "fp32": "f32", "float32": "f32", "bf16": "bf16", "bfloat16": "bf16"}[dtype]

    def __enter__(self):
        global PRECISION
        self.prev = PRECISION
        if self.dtype is not None:
            PRECISION = self.dtype
        return self

    def __exit__(self, *exc):
        global PRECISION
        PRECISION = self.prev
        return False


def gemm_wants_bf16(m: int, n: int, k: int) -> bool:
    return PRECISION == "bf16" and m >= 128 and n >= 32 and k >= 16 and k % 8 == 0


def gemm_bf16_weights(w: torch.Tensor) -> torch.Tensor:
    """w float32 [N,K] -> int16 view [2,N,K] of a buffer with a 16-byte trailer (plane 0 = bf16(w), plane 1 unused)."""
    w = w.contiguous()
    n, k = w.shape
    buf = torch.zeros(int(N.lib().awseg_gemm_bf16_weight_halfs(n, k)), dtype=torch.int16, device=w.device)
    N.call("awseg_gemm_bf16_weights", N.ptr(w), n, k, N.ptr(buf), N.stream())
    return buf[:2 * n * k].view(2, n, k)


def gemm_bf16_bias_act(x: torch.Tensor, w_bf16: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0,
                       residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = x.contiguous()
    m, k = x.shape
    n = w_bf16.shape[1]
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    N.call("awseg_gemm_bf16_bias_act", N.ptr(x), N.ptr(w_bf16), N.ptr(bias), N.ptr(residual), act, N.ptr(out), m, n, k, N.stream())
    return out


def winograd_bf16_weights(weight: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The image winograd_split_weights builds, with bf16(U * 2^-eu) in the high slots and zeros in the (unread) low slots."""
    return winograd_split_weights(weight, scale, bf16=True)


def conv3x3_winograd_bf16(x: torch.Tensor, u_bf16: torch.Tensor, cout: int, shift: torch.Tensor, act: int = 0, dilation: int = 1,
                          residual: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
                          b2: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = x.contiguous()
    b, h, w, cin = x.shape
    out = torch.empty((b, h, w) if w2 is not None else (b, h, w, cout), dtype=torch.float32, device=x.device)
    N.call("awseg_conv3x3_winograd_bf16_nhwc", N.ptr(x), b, h, w, cin, cout, dilation, N.ptr(u_bf16), N.ptr(shift.contiguous()),
           N.ptr(None if residual is None else residual.contiguous()), act, N.ptr(None if w2 is None else w2.contiguous()),
           N.ptr(None if b2 is None else b2.contiguous()), N.ptr(out), N.stream())
    return out


def set_split(on: bool) -> None:
    """Process-wide switch between the split-operand f16-MFMA kernels (float32-grade results) and
    their float32-input MFMA counterparts, for every operator that has both."""
    global ATTENTION_SPLIT, GEMM_SPLIT, WINO_SPLIT, HEAD_SPLIT
    ATTENTION_SPLIT = GEMM_SPLIT = WINO_SPLIT = HEAD_SPLIT = bool(on)


def split_state() -> dict:
    return {"attention": ATTENTION_SPLIT, "gemm_1x1": GEMM_SPLIT, "winograd_3x3": WINO_SPLIT, "segformer_head": HEAD_SPLIT}


def restore_split(state: dict) -> None:
    global ATTENTION_SPLIT, GEMM_SPLIT, WINO_SPLIT, HEAD_SPLIT
    ATTENTION_SPLIT, GEMM_SPLIT, WINO_SPLIT = bool(state["attention"]), bool(state["gemm_1x1"]), bool(state["winograd_3x3"])
    HEAD_SPLIT = bool(state.get("segformer_head", HEAD_SPLIT))


def maxpool3x3s2_nhwc(x_nhwc: torch.Tensor, shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.MaxPool2d(3, stride=2, padding=1) on a contiguous float32 [B,H,W,C] tensor -> [B,Ho,Wo,C] (no index tensor); with
    `shift` [C]: relu(pool + shift) in the same pass (the ResNet stem's BatchNorm shift + ReLU moved behind the pooling)."""
    x = x_nhwc.contiguous()
    b, h, w, c = x.shape
    out = torch.empty(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, dtype=torch.float32, device=x.device)
    if shift is not None:
        N.call("awseg_maxpool3x3s2_bias_relu_nhwc", N.ptr(x), b, h, w, c, N.ptr(shift.contiguous()), N.ptr(out), N.stream())
    else:
        N.call("awseg_maxpool3x3s2_nhwc", N.ptr(x), b, h, w, c, N.ptr(out), N.stream())
    return out


def upsample_bilinear(x: torch.Tensor, size, align_corners: bool) -> torch.Tensor:
    """F.interpolate(x, size, mode="bilinear", align_corners=...) / nn.UpsamplingBilinear2d on an NCHW float32 tensor, torch's
    arithmetic (bit-identical), 4 output pixels per lane."""
    b, c, h, w = x.shape
    H, W = int(size[0]), int(size[1])
    # (the 4 x 4-pixels-per-lane kernel can read the small map through its strides — awseg_upsample_bilinear_strided — but lanes that
    # walk NHWC rows 76 bytes apart keep the texture addresser busy for 0.73 ms where the planar map takes 0.32: a planar copy of
    # the small map (57 us at the bench shape) is the cheaper way, measured)
    if not (x.is_contiguous() or (STRIDED_UPSAMPLE and W % 4 == 0 and 3 * w < W and 3 * h < H and all(s_ >= 0 for s_ in x.stride()))):
        x = x.contiguous()
    out = torch.empty(b, c, H, W, dtype=torch.float32, device=x.device)
    # (torch ignores the stride of a size-1 dimension: a [B,1,h,w] channels_last map or a one-image view is_contiguous() with
    # strides the launcher's planar test would reject — what is contiguous is passed with the canonical strides)
    sb, sc, sy, sx = (c * h * w, h * w, w, 1) if x.is_contiguous() else x.stride()
    N.call("awseg_upsample_bilinear_strided", N.ptr_strided(x), b, c, h, w, sb, sc, sy, sx, H, W, int(bool(align_corners)), N.ptr(out), N.stream())
    return out


def stem_image_fill(x: torch.Tensor, image: torch.Tensor) -> None:
    """x [B,C<=4,H,W] (innermost stride 1) -> columns 3.. of the zero-padded NHWC image [B,H,Wp,4] of the 7x7 stems, one pass."""
    b, c, h, w = x.shape
    if x.stride(3) != 1:
        x = x.contiguous()
    N.call("awseg_stem_image", N.ptr_strided(x), b, c, h, w, x.stride(0), x.stride(1), x.stride(2), N.ptr(image), image.shape[2], N.stream())


def rowdot_sigmoid(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], sigmoid: bool = True) -> torch.Tensor:
    """sigmoid(x @ w + bias) for x [rows,k], w [k] -> [rows]: a 1x1 convolution to one channel (+ Sigmoid) on NHWC rows."""
    x, w = x.contiguous(), w.contiguous().view(-1)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    N.call("awseg_rowdot_sigmoid", N.ptr(x), x.shape[0], x.shape[1], N.ptr(w), N.ptr(bias), int(bool(sigmoid)), N.ptr(out), N.stream())
    return out


def aspp_pool_branch(mean: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: Optional[torch.Tensor]) -> torch.Tensor:
    """relu(mean @ w1^T + b1) @ w2^T + b2 for one row per image (the ASPP pooling branch and its slice of the projection)."""
    mean, w1, b1, w2 = mean.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous()
    b, cin = mean.shape
    cmid, cout = w1.shape[0], w2.shape[0]
    ws = torch.empty(int(N.lib().awseg_aspp_pool_branch_workspace(b, cmid)), dtype=torch.uint8, device=mean.device)
    out = torch.empty(b, cout, dtype=torch.float32, device=mean.device)
    N.call("awseg_aspp_pool_branch", N.ptr(mean), b, cin, N.ptr(w1), N.ptr(b1), cmid, N.ptr(w2), N.ptr(None if b2 is None else b2.contiguous()),
           cout, N.ptr(ws), N.ptr(out), N.stream())
    return out


def depth_upsample_combine(d1: torch.Tensor, d2_low: torch.Tensor, weights: Optional[torch.Tensor]):
    """(d2_full, d) with d2_full = bilinear(align_corners=False) upsample of d2_low [B,1,h,w] to d1's size [B,1,H,W] and
    d = weights[0]*d1 + weights[1]*d2_full (mean when weights is None) — PKG/models/model.py:368-371, 471-478."""
    d1, d2_low = d1.contiguous(), d2_low.contiguous()
    b, _, H, W = d1.shape
    h, w = d2_low.shape[-2:]
    d2_full, d = torch.empty_like(d1), torch.empty_like(d1)
    N.call("awseg_depth_upsample_combine", N.ptr(d1), N.ptr(d2_low), b, h, w, H, W, N.ptr(None if weights is None else weights.contiguous()),
           N.ptr(d2_full), N.ptr(d), N.stream())
    return d2_full, d


def layernorm_rows(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """torch.nn.functional.layer_norm over the last dimension for small channel counts (MiT tokens)."""
    x = x.contiguous()
    c = x.shape[-1]
    out = torch.empty_like(x)
    N.call("awseg_layernorm_rows", N.ptr(x), x.numel() // c, c, N.ptr(gamma.contiguous()), N.ptr(beta.contiguous()), float(eps),
           N.ptr(out), N.stream())
    return out
