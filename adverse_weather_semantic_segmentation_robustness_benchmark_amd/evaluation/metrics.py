"""Evaluation metrics with the reference's class / method names (PKG/evaluation/metrics.py),
re-designed so that nothing per-pixel ever leaves the GPU:

* confusion counts accumulate in an int64 device tensor (HIP, A13) — additive across batches,
  images, weather conditions and ranks, so the reference's "concatenate everything on the host,
  count once" (REF/scripts/evaluate.py:203-218) becomes "count as you go, all-reduce 19x19";
* the final IoU arithmetic is done on the HOST with the same torch expressions the reference
  uses (metrics.py:74-83: int64/int64 true-divide -> float32, mean over valid classes), so
  identical counts give a bit-identical mIoU;
* ECE keeps 15 x {count, sum conf, sum correct} per slot on device (HIP, metrics.py:161-194).

The uint8-label quirk of the reference (`targets * num_classes` wraps mod 256 on uint8 tensors,
SURVEY §8 A13) is reproduced by default because the reference's published numbers depend on it;
pass ``wrap_uint8_labels=False`` to get the mathematically intended confusion matrix.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops

logger = logging.getLogger(__name__)


def iou_from_counts(counts: torch.Tensor, num_classes: int) -> Dict[str, Any]:
    """metrics.py:73-89 on a [C*C] or [C,C] int64 count tensor (moved to the host)."""
    cm = counts.detach().to("cpu", torch.int64).view(num_classes, num_classes)
    intersection = torch.diag(cm)
    union = cm.sum(dim=0) + cm.sum(dim=1) - intersection
    valid = union > 0
    per_class = torch.zeros(num_classes)
    per_class[valid] = intersection[valid] / union[valid]
    mean_iou = per_class[valid].mean()
    return {"mean_iou": mean_iou.item(), "per_class_iou": per_class.numpy(), "valid_classes": valid.numpy()}


class ConfusionAccumulator:
    """int64 [n_slots, C*C] on device: slot 0 = overall, slot 1+k = k-th weather condition."""

    def __init__(self, num_classes: int, conditions: Optional[List[str]], device) -> None:
        self.num_classes = num_classes
        self.conditions = list(conditions or [])
        self.counts = ops.new_counts(num_classes, device, 1 + len(self.conditions))
        self.oob = torch.zeros(1, dtype=torch.int64, device=device)

    def cond_ids(self, names) -> torch.Tensor:
        ids = [self.conditions.index(str(n)) if str(n) in self.conditions else -1 for n in names]
        return torch.tensor(ids, dtype=torch.int32).to(self.counts.device, non_blocking=True)

    def all_reduce(self) -> None:
        """Sum counters over ranks (RCCL over xGMI on GPUs; integer sums are order-independent)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM)
            dist.all_reduce(self.oob, op=dist.ReduceOp.SUM)

    def check(self) -> None:
        if int(self.oob.item()):
            raise IndexError("index out of range in confusion accumulation (label outside [0, num_classes))")

    def miou(self, slot: int = 0) -> float:
        return iou_from_counts(self.counts[slot], self.num_classes)["mean_iou"]

    def present(self, slot: int) -> bool:
        return bool(self.counts[slot].sum().item() > 0)


class IoUMetrics:
    """PKG/evaluation/metrics.py:15-123."""

    def __init__(self, num_classes: int, ignore_index: int = 255, wrap_uint8_labels: bool = True) -> None:
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.wrap_uint8_labels = wrap_uint8_labels

    def confusion(self, predictions: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        """int64 [C*C] device counts for one call (HIP).  Logits [B,C,H,W] are arg-maxed on device."""
        device = predictions.device
        counts = ops.new_counts(self.num_classes, device)
        oob = torch.zeros(1, dtype=torch.int64, device=device)
        wrap = self.wrap_uint8_labels and targets.dtype == torch.uint8
        if targets.dtype not in (torch.uint8, torch.int64):
            targets = targets.long()
        if predictions.dim() == 4:                                                   # metrics.py:50-51
            ops.combine_argmax_confusion(predictions.float(), None, 3, want_logits=False, label=targets.contiguous(),
                                         counts=counts, oob=oob, ignore_index=self.ignore_index, wrap_u8=wrap)
        else:
            if predictions.dtype not in (torch.uint8, torch.int64):
                predictions = predictions.long()
            ops.confusion_accumulate(predictions, targets, self.num_classes, counts, oob, self.ignore_index, wrap)
        if int(oob.item()):
            raise IndexError("index out of range in self")                          # what index_add_ raises
        return counts[0]

    def compute_iou(self, predictions: torch.Tensor, targets: torch.Tensor) -> Dict[str, Any]:
        return iou_from_counts(self.confusion(predictions, targets), self.num_classes)

    def compute_pixel_accuracy(self, predictions: torch.Tensor, targets: torch.Tensor) -> float:
        """metrics.py:91-123 — from an UNWRAPPED confusion matrix: correct = trace, total = sum."""
        keep = self.wrap_uint8_labels
        self.wrap_uint8_labels = False
        try:
            cm = self.confusion(predictions, targets).view(self.num_classes, self.num_classes)
        finally:
            self.wrap_uint8_labels = keep
        total = int(cm.sum().item())
        return int(torch.diag(cm).sum().item()) / total if total > 0 else 0.0


class ConfidenceCalibration:
    """PKG/evaluation/metrics.py:126-321."""

    def __init__(self, num_bins: int = 15) -> None:
        self.num_bins = num_bins

    def _bins(self, predictions, targets):
        device = predictions.device
        bins = ops.new_ece_bins(self.num_bins, device)
        edges = torch.linspace(0, 1, self.num_bins + 1).to(device)                   # float32 edges, metrics.py:179
        if targets.dtype not in (torch.uint8, torch.int64):
            targets = targets.long()
        ops.ece_accumulate(predictions.float(), targets, bins, edges)
        return ops.ece_bins_to_numpy(bins)[0], edges.cpu()

    @staticmethod
    def ece_from_bins(b: np.ndarray, edges=None, details: bool = False):
        """metrics.py:183-226 from the accumulators."""
        total = int(b["count"].sum())
        ece, det = 0.0, []
        for k in range(len(b)):
            n = int(b["count"][k])
            lo = float(edges[k]) if edges is not None else 0.0
            hi = float(edges[k + 1]) if edges is not None else 0.0
            if n > 0:
                acc, conf, prop = b["sum_correct"][k] / n, b["sum_conf"][k] / n, n / total
                ece += abs(conf - acc) * prop
                det.append({"bin_lower": lo, "bin_upper": hi, "accuracy": float(acc), "confidence": float(conf),
                            "proportion": float(prop), "error": float(abs(conf - acc))})
            else:
                det.append({"bin_lower": lo, "bin_upper": hi, "accuracy": 0.0, "confidence": 0.0, "proportion": 0.0, "error": 0.0})
        if not details:
            return float(ece)
        return {"ece": float(ece), "bin_details": det,
                "overall_accuracy": float(b["sum_correct"].sum() / total) if total else float("nan"),
                "overall_confidence": float(b["sum_conf"].sum() / total) if total else float("nan")}

    def compute_ece(self, predictions: torch.Tensor, targets: torch.Tensor, return_details: bool = False):
        b, edges = self._bins(predictions, targets)
        return self.ece_from_bins(b, edges, return_details)

    def compute_reliability_diagram_data(self, predictions, targets) -> Dict[str, np.ndarray]:
        det = self.compute_ece(predictions, targets, return_details=True)["bin_details"]
        rows = [d for d in det if d["proportion"] > 0]
        return {"bin_centers": np.array([(d["bin_lower"] + d["bin_upper"]) / 2 for d in rows]),
                "bin_accuracies": np.array([d["accuracy"] for d in rows]),
                "bin_confidences": np.array([d["confidence"] for d in rows]),
                "bin_proportions": np.array([d["proportion"] for d in rows])}

    def temperature_scale(self, logits: torch.Tensor, temperature: float) -> torch.Tensor:
        return logits / temperature

    def optimize_temperature(self, logits: torch.Tensor, targets: torch.Tensor, max_iter: int = 50) -> float:
        """metrics.py:283-321 grid search, including its `view(-1, C)` on NCHW without a permute."""
        best_t, best = 1.0, float("inf")
        flat = logits.reshape(-1, logits.size(1))
        tflat = targets.reshape(-1)
        keep = tflat != 255
        flat, tflat = flat[keep], tflat[keep].long()
        for t in torch.linspace(0.1, 10.0, 100):
            nll = F.cross_entropy(flat / t.item(), tflat).item()
            if nll < best:
                best, best_t = nll, t.item()
        return best_t

    def fit_temperature(self, logits: torch.Tensor, targets: torch.Tensor, temperatures=None, return_details: bool = False):
        """optimize_temperature's grid search as it was meant: the per-pixel NLL over the CLASS dimension of [B,C,H,W] logits,
        every grid point in one device pass (no logit copied, no boolean mask).  Selection rule of the reference: the first
        grid point with the smallest NLL, compared on the exact integer sums.  Raises IndexError on a label outside [0, C)
        other than 255, where F.cross_entropy would."""
        temps = ops.calib_temperatures(ops.DEFAULT_TEMPERATURE_GRID if temperatures is None else temperatures)
        if targets.dtype not in (torch.uint8, torch.int64):
            targets = targets.long()
        device = logits.device
        edges = torch.linspace(0, 1, self.num_bins + 1).to(device)
        stats = ops.new_temperature_grid_stats(len(temps), self.num_bins, device)
        ops.temperature_grid_stats(logits.float(), targets, stats, temps, edges)
        s = ops.temperature_grid_stats_to_numpy(stats)
        if int(s["out_of_range"][0]):
            raise IndexError(f"Target out of bounds: {int(s['out_of_range'][0])} labels outside [0, {logits.size(1)}) other than 255")
        k = first_min_index(s["nll_q"][0], s["count"][0])
        if k is None:
            t = 1.0                                                     # no pixel: the reference's loop keeps its start value
            return {"temperature": t, "index": None, "nll": np.full(len(temps), np.nan), "ece": float("nan"),
                    "temperatures": temps} if return_details else t
        t = float(temps[k])
        if not return_details:
            return t
        return {"temperature": t, "index": k, "temperatures": temps, "nll": mean_nll(s["nll_q"][0], s["count"][0]),
                "ece": self.ece_from_bins(s["bins"][0, k]), "saturated": s["saturated"][0].copy(),
                "nonfinite": s["nonfinite"][0].copy()}           # per grid point, pixels


def mean_nll(nll_q: np.ndarray, count: np.ndarray) -> np.ndarray:
    """Mean per-pixel NLL per grid point from the fixed-point sums (NaN where no pixel counted)."""
    nll_q, count = np.asarray(nll_q), np.asarray(count)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count > 0, nll_q.astype(np.float64) * ops.CALIB_NLL_UNIT / np.maximum(count, 1), np.nan)


def first_min_index(nll_q, count) -> Optional[int]:
    """Index of the first grid point with the smallest mean NLL, compared exactly (nll_q[i] * count[j] vs nll_q[j] * count[i]
    in Python integers); None when no grid point counted a pixel."""
    best = None
    for i, (q, n) in enumerate(zip((int(v) for v in nll_q), (int(v) for v in count))):
        if n <= 0:
            continue
        if best is None or q * best[1] < best[0] * n:
            best = (q, n, i)
    return None if best is None else best[2]


def calibration_from_stats(stats: Dict[str, np.ndarray], temps, conditions, fit_condition: str = "clean") -> Dict[str, float]:
    """Result keys of the streamed temperature calibration from the decoded counters (ops.temperature_grid_stats_to_numpy):
    the temperature is fitted on `fit_condition`'s slot (slot 0 when that condition counted no pixel), the calibrated NLL and
    ECE are reported at it overall and for every condition present, each condition also gets its own optimum.  Host only."""
    temps = np.asarray(temps, dtype=np.float32)
    conditions = list(conditions)
    count, nll_q, bins = stats["count"], stats["nll_q"], stats["bins"]

    def present(slot):
        return int(bins[slot]["count"].sum()) > 0 or int(count[slot].sum()) > 0

    fit = 1 + conditions.index(fit_condition) if fit_condition in conditions else 0
    k = first_min_index(nll_q[fit], count[fit]) if present(fit) else None
    if k is None:
        fit, k = 0, first_min_index(nll_q[0], count[0])
    if k is None:
        return {}
    nll = mean_nll(nll_q, count)
    res = {"calibration_temperature": float(temps[k]), "nll_calibrated": float(nll[0, k]),
           "ece_calibrated": ConfidenceCalibration.ece_from_bins(bins[0, k])}
    for i, name in enumerate(conditions):
        s = 1 + i
        if s >= len(count) or not present(s):
            continue
        res[f"ece_calibrated_{name}"] = ConfidenceCalibration.ece_from_bins(bins[s, k])
        if count[s, k] > 0:
            res[f"nll_calibrated_{name}"] = float(nll[s, k])
        own = first_min_index(nll_q[s], count[s])
        if own is not None:
            res[f"calibration_temperature_{name}"] = float(temps[own])
    # pixels whose NLL was clamped at the cap, at the grid temperature that clamped the most of them (slot 0): a pixel count,
    # not a sum over the grid; non-zero whenever the cap touched any grid point the fit compared
    sat = int(stats["saturated"][0].max()) if stats["saturated"].size else 0
    if sat:
        res["calibration_saturated_pixels"] = float(sat)
    return res


def _agreement(a: np.ndarray) -> Optional[float]:
    total = int(a.sum())
    return None if total == 0 else float(np.trace(a)) / total


def _corruption_error_rate(t: np.ndarray) -> float:
    ref_correct = int(t[0]) + int(t[1])
    return float(int(t[1]) / ref_correct) if ref_correct > 0 else 0.0


def severity_sweep_results(cons: Dict[str, np.ndarray], slots: List[str], kinds, levels: int, intensities: Dict[str, Any],
                           sources: int, mious: Dict[str, float], degradation=None) -> Dict[str, float]:
    """Result keys of the paired severity sweep from the decoded consistency counters (ops.consistency_stats_to_numpy: slot 0 = every
    corrupted frame, slot 1 + k = slots[k]) and the mIoUs already derived from the confusion counters (`mious`: 'clean', each
    '<kind>_s<j>' present).  Host only; every value a float.
      consistency            trace(A) / sum(A): pixel agreement of the corrupted prediction with the clean one
      consistency_miou       mIoU of the corrupted prediction with the clean prediction as the target (iou_from_counts on A)
      corruption_error_rate  labelled pixels the clean prediction gets right and the corrupted one wrong, over those it gets right
    Pooled keys (per kind, over every kind) come from the summed counters, not from means of ratios."""
    degradation = degradation or RobustnessMetrics().compute_robustness_degradation_ratio
    A, T = np.asarray(cons["agreement"], np.int64), np.asarray(cons["transitions"], np.int64)
    C = A.shape[-1]
    res: Dict[str, float] = {"paired_sources": float(sources), "severity_levels": float(levels)}
    for kind in kinds:
        a_kind, t_kind = np.zeros((C, C), np.int64), np.zeros(4, np.int64)
        for j in range(1, levels + 1):
            name = f"{kind}_s{j}"
            s = 1 + slots.index(name)
            res[f"severity_intensity_{name}"] = float(intensities[kind][j - 1])
            if "clean" in mious and name in mious:
                res[f"robustness_degradation_{name}"] = float(degradation(mious["clean"], mious[name]))
            agree = _agreement(A[s])
            if agree is None:
                continue
            a_kind += A[s]
            t_kind += T[s]
            res[f"consistency_{name}"] = agree
            res[f"consistency_miou_{name}"] = float(iou_from_counts(torch.from_numpy(A[s].reshape(-1).copy()), C)["mean_iou"])
            res[f"corruption_error_rate_{name}"] = _corruption_error_rate(T[s])
        agree = _agreement(a_kind)
        if agree is not None:
            res[f"consistency_{kind}"] = agree
    agree = _agreement(A[0])
    if agree is not None:
        res["mean_consistency"] = agree
        res["mean_corruption_error_rate"] = _corruption_error_rate(T[0])
    return res


DEPTH_METRICS = ("mae", "rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "delta1", "delta2", "delta3")
DEPTH_MEMBER_PREFIXES = ("", "segformer_", "deeplabv3plus_")      # series 0 / 1 / 2, the prefixes of the model's own depth keys


def depth_row_metrics(row: np.ndarray) -> Optional[Dict[str, float]]:
    """The depth metrics of one counter row (int64 [AWSEG_DEPTH_ROW], ops.DEPTH_FIELDS order); None when it has no valid pixel.
    Means of the fixed-point sums over the valid count; silog's radicand is clamped at 0 (two separately rounded sums can leave it
    a few units of 2^-20 negative where every pixel has the same log offset)."""
    f = {name: int(row[i]) for i, name in enumerate(ops.DEPTH_FIELDS)}
    n = f["valid"]
    if n <= 0:
        return None
    mean = {k: f[k] * ops.DEPTH_UNIT / n for k in ("sum_abs", "sum_sq", "sum_abs_rel", "sum_sq_rel", "sum_log", "sum_log_sq")}
    return {"mae": mean["sum_abs"], "rmse": float(np.sqrt(mean["sum_sq"])), "abs_rel": mean["sum_abs_rel"], "sq_rel": mean["sum_sq_rel"],
            "rmse_log": float(np.sqrt(mean["sum_log_sq"])),
            "silog": float(np.sqrt(max(mean["sum_log_sq"] - mean["sum_log"] ** 2, 0.0))),
            "delta1": f["delta1"] / n, "delta2": f["delta2"] / n, "delta3": f["delta3"] / n}


def depth_metrics_from_stats(stats, conditions: List[str], kinds=None, levels: int = 0) -> Dict[str, float]:
    """Result keys of the depth error counters (int64 [1 + len(conditions), 3, AWSEG_DEPTH_ROW]; slot 0 = every frame, slot 1 + k =
    conditions[k]).  Host only; every value a float.
      depth_<metric>[_<condition>]                          series 0: the ensemble, or the single model
      segformer_depth_<metric>[_<condition>], deeplabv3plus_depth_<metric>[_<condition>]   the members (three-series counters)
      depth_valid_fraction[_<condition>]                    valid / (valid + masked + non-finite) pixels
      depth_saturated_terms, depth_masked_pixels, depth_nonfinite_pixels                  slot 0, only when non-zero
      depth_degradation_<name> = (abs_rel_<name> - abs_rel_clean) / abs_rel_clean         when 'clean' has abs_rel > 0
    Severity sweep (kinds, levels): conditions are its slots ('clean', '<kind>_s<j>'); each kind also gets keys from the summed
    counters of its slots.  A slot without a valid pixel yields no keys."""
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.ndim != 3 or raw.shape[0] != 1 + len(conditions) or raw.shape[1:] != (len(ops.DEPTH_SERIES), ops.DEPTH_ROW):
        raise ValueError(f"depth stats must be int64 [{1 + len(conditions)}, {len(ops.DEPTH_SERIES)}, {ops.DEPTH_ROW}], got {raw.shape}")
    named = [("", raw[0])] + [("_" + name, raw[1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        idx = [1 + conditions.index(f"{kind}_s{j}") for j in range(1, levels + 1)]
        named.append(("_" + kind, raw[idx].sum(0)))
    res: Dict[str, float] = {}
    for suffix, slot in named:
        got = False
        for prefix, row in zip(DEPTH_MEMBER_PREFIXES, slot):
            m = depth_row_metrics(row)
            if m is None:
                continue
            got = True
            for k in DEPTH_METRICS:
                res[f"{prefix}depth_{k}{suffix}"] = float(m[k])
        if got:
            px = slot[0][:3].astype(np.float64)
            res[f"depth_valid_fraction{suffix}"] = float(px[0] / px.sum())
    i_sat, i_mask, i_bad = (ops.DEPTH_FIELDS.index(k) for k in ("saturated", "masked", "nonfinite"))
    for key, v in (("depth_saturated_terms", int(raw[0, :, i_sat].sum())), ("depth_masked_pixels", int(raw[0, 0, i_mask])),
                   ("depth_nonfinite_pixels", int(raw[0, 0, i_bad]))):
        if v:
            res[key] = float(v)
    base = res.get("depth_abs_rel_clean", 0.0)
    if base > 0:
        for suffix, _ in named[1:]:
            name = suffix[1:]
            if name != "clean" and f"depth_abs_rel_{name}" in res:
                res[f"depth_degradation_{name}"] = float((res[f"depth_abs_rel_{name}"] - base) / base)
    return res


FAILURE_METRICS = ("auroc", "auroc_halfwidth", "aurc", "eaurc")


def failure_metrics_from_hist(right, wrong) -> Dict[str, float]:
    """Failure-detection numbers of one score from its two histograms (counts per bin, bins in ascending score order; `right` /
    `wrong` = pixels whose prediction was right / wrong).  Host only, float64.  Ties inside a bin count as uniformly interleaved.
      auroc            P(score of a wrong pixel > score of a right one) + P(tie)/2 = sum_b wrong_b (right_<b + right_b/2) / (W R);
                       0.5 when there is no wrong or no right pixel
      auroc_halfwidth  sum_b wrong_b right_b / (2 W R): the exact-rank AUROC of the scores that were binned lies within
                       auroc +- halfwidth whatever order the ties really have (0 without a wrong or a right pixel)
      aurc             integral over the coverage c of risk(c) = errors among the c N least uncertain pixels / (c N).  With `a`
                       wrong among the T pixels before a bin that holds w wrong of n, the bin adds w (T = 0) or
                       w + (a - w T / n) ln((T + n) / T); the sum is divided by N
      eaurc            aurc - (e + (1 - e) ln(1 - e)), e = error_rate: the excess over a ranking that puts every error last
      error_rate       W / N (0 without a pixel)"""
    r = np.asarray(right, dtype=np.float64).reshape(-1)
    w = np.asarray(wrong, dtype=np.float64).reshape(-1)
    if r.shape != w.shape:
        raise ValueError(f"the two histograms must have one length, got {r.shape} and {w.shape}")
    R, W = float(r.sum()), float(w.sum())
    total = R + W
    if total == 0:
        return {"auroc": 0.5, "auroc_halfwidth": 0.0, "aurc": 0.0, "eaurc": 0.0, "error_rate": 0.0}
    if W == 0 or R == 0:
        auroc, half = 0.5, 0.0                                                      # metrics.py:430-431
    else:
        below = np.cumsum(r) - r
        auroc = float((w * (below + 0.5 * r)).sum() / (W * R))
        half = float((w * r).sum() / (2.0 * W * R))
    n = r + w
    keep = n > 0
    nk, wk = n[keep], w[keep]
    T = np.cumsum(nk) - nk                                                          # pixels kept before the bin
    a = np.cumsum(wk) - wk                                                          # wrong ones among them
    terms = wk.copy()
    later = T > 0
    terms[later] += (a[later] - wk[later] * T[later] / nk[later]) * np.log1p(nk[later] / T[later])
    aurc = float(terms.sum() / total)
    e = W / total
    best = 1.0 if e >= 1.0 else float(e + (1.0 - e) * np.log1p(-e))
    return {"auroc": auroc, "auroc_halfwidth": half, "aurc": aurc, "eaurc": float(aurc - best), "error_rate": float(e)}


def failure_metrics_from_stats(stats, conditions: List[str], kinds=None, levels: int = 0, single: bool = False) -> Dict[str, float]:
    """Result keys of the failure-detection counters (int64 [1 + len(conditions), AWSEG_FAIL_ROW]; slot 0 = every frame, slot
    1 + k = conditions[k]).  Host only; every value a float.
      failure_<auroc|auroc_halfwidth|aurc|eaurc>_<score>[_<condition>]     score in ops.FAIL_SCORES (single: entropy, msp)
      failure_error_rate[_<condition>]                    of the prediction mIoU scores (row msp: argmax of the combined logits)
      failure_error_rate_mean_probability[_<condition>]   of argmax of the mean probability (rows mi, entropy, variance; not single)
      failure_nonfinite_pixels, failure_out_of_range_labels               slot 0, only when non-zero
    Severity sweep (kinds, levels): conditions are its slots ('clean', '<kind>_s<j>'); each kind also gets keys from the summed
    counters of its slots.  A slot without a counted pixel yields no keys."""
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.ndim != 2 or raw.shape != (1 + len(conditions), ops.FAIL_ROW):
        raise ValueError(f"failure stats must be int64 [{1 + len(conditions)}, {ops.FAIL_ROW}], got {raw.shape}")
    dec = ops.failure_stats_to_numpy(raw)
    named = [("", dec["hist"][0], int(dec["pixels"][0]))]
    named += [("_" + name, dec["hist"][1 + k], int(dec["pixels"][1 + k])) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        idx = [1 + conditions.index(f"{kind}_s{j}") for j in range(1, levels + 1)]
        named.append(("_" + kind, dec["hist"][idx].sum(0), int(dec["pixels"][idx].sum())))
    scores = [(i, s) for i, s in enumerate(ops.FAIL_SCORES) if not single or s in ("entropy", "msp")]
    res: Dict[str, float] = {}
    for suffix, hist, pixels in named:
        if pixels <= 0:
            continue
        for i, score in scores:
            m = failure_metrics_from_hist(hist[i, 0], hist[i, 1])
            for k in FAILURE_METRICS:
                res[f"failure_{k}_{score}{suffix}"] = float(m[k])
            if score == "msp":
                res[f"failure_error_rate{suffix}"] = float(m["error_rate"])
            elif score == "entropy" and not single:
                res[f"failure_error_rate_mean_probability{suffix}"] = float(m["error_rate"])
    for key, v in (("failure_nonfinite_pixels", int(dec["nonfinite"][0])), ("failure_out_of_range_labels", int(dec["out_of_range"][0]))):
        if v:
            res[key] = float(v)
    return res


def boundary_metrics_from_stats(stats, widths, conditions: List[str], num_classes: int, kinds=None, levels: int = 0,
                                degradation=None) -> Dict[str, float]:
    """Result keys of the boundary-band counters (int64 [1 + len(conditions), len(widths) + 1, C*C + 2 C], include/awseg.h; slot 0 =
    every frame, slot 1 + k = conditions[k]).  Host only; every value a float.  Per width d (the band: labelled pixels within
    Chebyshev distance d of a class boundary, the rings 0 .. k of the counters summed) and suffix ('' | _<condition>):
      boundary_miou_w<d>       iou_from_counts on the band's confusion matrix (trimap mIoU; band of the label map)
      boundary_accuracy_w<d>   trace / total of it (trimap accuracy)
      boundary_iou_w<d>        mean over the classes with a non-empty union of inter / (gt + pr - inter): gt[c] the band's labelled
                               pixels of class c (label band), pr[c] those predicted c within the prediction's band, inter[c] those
                               where both hold and the classes agree (Boundary IoU, Cheng et al. 2021, over the labelled pixels)
      boundary_fraction_w<d>   share of the labelled pixels inside the label band
    and per suffix interior_miou (iou_from_counts on the last ring: farther than the widest band from any label boundary).  A band
    without a pixel yields its fraction only; a slot without a labelled pixel yields no keys.
    Severity sweep (kinds, levels): conditions are its slots ('clean', '<kind>_s<j>'); each kind also gets keys from the summed
    counters of its slots.  With 'clean' present, for every adverse kind (without a sweep: every other condition)
      boundary_degradation_w<d>_<kind> = degradation(boundary_iou_w<d>_clean, boundary_iou_w<d>_<kind>)
      interior_degradation_<kind>      = degradation(interior_miou_clean, interior_miou_<kind>)
    degradation: RobustnessMetrics.compute_robustness_degradation_ratio unless given."""
    w = [int(d) for d in ops.boundary_widths(widths)]
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    C = int(num_classes)
    if raw.ndim != 3 or raw.shape != (1 + len(conditions), len(w) + 1, C * (C + 2)):
        raise ValueError(f"boundary stats must be int64 [{1 + len(conditions)}, {len(w) + 1}, {C * (C + 2)}], got {raw.shape}")
    if degradation is None:
        degradation = RobustnessMetrics(C).compute_robustness_degradation_ratio
    named = [("", raw[0])] + [("_" + name, raw[1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        idx = [1 + conditions.index(f"{kind}_s{j}") for j in range(1, levels + 1)]
        named.append(("_" + kind, raw[idx].sum(0)))
    res: Dict[str, float] = {}
    for suffix, slot in named:
        dec = ops.boundary_stats_to_numpy(slot, C)
        total = int(dec["conf"].sum())
        if total <= 0:
            continue
        conf, inter, pr = (np.cumsum(dec[k], axis=0) for k in ("conf", "inter", "pr"))
        for k, d in enumerate(w):
            band = int(conf[k].sum())
            res[f"boundary_fraction_w{d}{suffix}"] = float(band / total)
            if band <= 0:
                continue
            res[f"boundary_miou_w{d}{suffix}"] = float(iou_from_counts(torch.from_numpy(conf[k].reshape(-1).copy()), C)["mean_iou"])
            res[f"boundary_accuracy_w{d}{suffix}"] = float(np.trace(conf[k]) / band)
            union = conf[k].sum(axis=1) + pr[k] - inter[k]
            seen = union > 0
            res[f"boundary_iou_w{d}{suffix}"] = float((inter[k][seen] / union[seen].astype(np.float64)).mean())
        last = dec["conf"][len(w)]
        if int(last.sum()) > 0:
            res[f"interior_miou{suffix}"] = float(iou_from_counts(torch.from_numpy(last.reshape(-1).copy()), C)["mean_iou"])
    adverse = list(kinds) if kinds else [name for name in conditions if name != "clean"]
    for kind in adverse:
        for d in w:
            a, b = f"boundary_iou_w{d}_clean", f"boundary_iou_w{d}_{kind}"
            if a in res and b in res:
                res[f"boundary_degradation_w{d}_{kind}"] = float(degradation(res[a], res[b]))
        if "interior_miou_clean" in res and f"interior_miou_{kind}" in res:
            res[f"interior_degradation_{kind}"] = float(degradation(res["interior_miou_clean"], res[f"interior_miou_{kind}"]))
    return res


SEGMENT_THRESHOLDS = {0.25: 1, 0.5: 2, 0.75: 3, 1.0: 4}              # h / A >= j / 4  <=>  cov >= j + 1 (include/awseg.h)
SEGMENT_SIZE_GROUPS = (("small", 0, 5), ("medium", 5, 7), ("large", 7, 11))     # buckets [lo, hi): area < 1024, < 16384, the rest


def segment_options(threshold=0.5, min_area=16):
    """(j, first bucket) of a coverage threshold in {0.25, 0.5, 0.75, 1.0} and a smallest counted area that is a power of 4 in
    [1, 4^10]; ValueError for anything else."""
    ok = isinstance(threshold, (int, float, np.integer, np.floating)) and not isinstance(threshold, (bool, np.bool_))
    if not ok or float(threshold) not in SEGMENT_THRESHOLDS:
        raise ValueError(f"the segment coverage threshold is one of {sorted(SEGMENT_THRESHOLDS)}, got {threshold!r}")
    ok = isinstance(min_area, (int, np.integer)) and not isinstance(min_area, (bool, np.bool_))
    areas = [4 ** k for k in range(11)]
    if not ok or int(min_area) not in areas:
        raise ValueError(f"the smallest counted segment area is a power of 4 in [1, 4^10], got {min_area!r}")
    return SEGMENT_THRESHOLDS[float(threshold)], areas.index(int(min_area))


def segment_metrics_from_stats(stats, conditions: List[str], num_classes: int, threshold=0.5, min_area=16, kinds=None,
                               levels: int = 0) -> Dict[str, float]:
    """Result keys of the segment-level counters (int64 [1 + len(conditions), C, 11, 48], include/awseg.h; slot 0 = every frame, slot
    1 + k = conditions[k]).  Host only; every value a float.  A label segment is DETECTED when at least `threshold` of its pixels are
    predicted as its class (cov >= j + 1), a prediction segment is TRUE when at least `threshold` of its pixels carry its class as
    label; segments below `min_area` pixels are not counted.  Per suffix ('' | _<condition>), with per class N label segments, TP
    detected ones, FN = N - TP, M prediction segments, FP the ones that are not true:
      segment_recall           mean over the classes with N > 0 of TP / N
      segment_precision        mean over the classes with M > 0 of (M - FP) / M
      segment_f1               mean over the classes with 2 TP + FN + FP > 0 of 2 TP / (2 TP + FN + FP)
      segment_miss_rate        share of the label segments of which not one pixel is found (cov == 0)
      segment_false_rate       share of the prediction segments without one pixel of their class in the label
      segment_count, segment_pred_count
      segment_recall_<g>, segment_miss_rate_<g>, segment_f1_<g>    for the size groups g = small (area < 1024), medium (< 16384), large
      segment_recall_class<c>  TP / N of class c
    With 'clean' present, for every adverse kind (without a sweep: every other condition)
      segment_recall_drop_<kind> = segment_recall_clean - segment_recall_<kind>, segment_miss_rate_rise_<kind> the reverse difference.
    Severity sweep (kinds, levels): conditions are its slots ('clean', '<kind>_s<j>'); each kind also gets keys from the summed
    counters of its slots, and per '<kind>_s<j>' and '<kind>'
      segment_lost_<n>         of the label segments the clean twin's map detects, the share this frame's map does not
      segment_recovered_<n>    of those the clean twin's map does not detect, the share this frame's map does
    A key whose denominator is 0 is absent."""
    j, k0 = segment_options(threshold, min_area)
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    C = int(num_classes)
    if raw.shape != (1 + len(conditions), C, ops.SEGMENT_BUCKETS, ops.SEGMENT_CELLS):
        raise ValueError(f"segment stats must be int64 [{1 + len(conditions)}, {C}, {ops.SEGMENT_BUCKETS}, {ops.SEGMENT_CELLS}], "
                         f"got {raw.shape}")
    named = [("", raw[0])] + [("_" + name, raw[1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        idx = [1 + conditions.index(f"{kind}_s{lv}") for lv in range(1, levels + 1)]
        named.append(("_" + kind, raw[idx].sum(0)))
    res: Dict[str, float] = {}

    def rates(slot, lo, hi):
        """slot [C, 11, 48], buckets [max(lo, k0), hi) -> per class N, TP, M, FP and the two cov == 0 counts."""
        part = slot[:, max(lo, k0):hi].sum(axis=1)
        lab, prd = part[:, :42].reshape(C, 6, 7), part[:, 42:]
        return (lab.sum(axis=(1, 2)), lab[:, j + 1:].sum(axis=(1, 2)), prd.sum(axis=1), prd[:, :j + 1].sum(axis=1),
                int(lab[:, 0].sum()), int(prd[:, 0].sum()), lab)

    def put(key, num, den):
        if den > 0:
            res[key] = float(num / den)

    def class_mean(key, num, den):
        seen = den > 0
        if seen.any():
            res[key] = float((num[seen] / den[seen].astype(np.float64)).mean())

    for suffix, slot in named:
        n, tp, m, fp, miss, false, lab = rates(slot, 0, ops.SEGMENT_BUCKETS)
        if int(n.sum()) + int(m.sum()) <= 0:
            continue
        class_mean("segment_recall" + suffix, tp, n)
        class_mean("segment_precision" + suffix, m - fp, m)
        class_mean("segment_f1" + suffix, 2 * tp, 2 * tp + (n - tp) + fp)
        put("segment_miss_rate" + suffix, miss, int(n.sum()))
        put("segment_false_rate" + suffix, false, int(m.sum()))
        res["segment_count" + suffix] = float(n.sum())
        res["segment_pred_count" + suffix] = float(m.sum())
        for c in range(C):
            put(f"segment_recall_class{c}{suffix}", int(tp[c]), int(n[c]))
        for group, lo, hi in SEGMENT_SIZE_GROUPS:
            gn, gtp, gm, gfp, gmiss, _, _ = rates(slot, lo, hi)
            class_mean(f"segment_recall_{group}{suffix}", gtp, gn)
            put(f"segment_miss_rate_{group}{suffix}", gmiss, int(gn.sum()))
            class_mean(f"segment_f1_{group}{suffix}", 2 * gtp, 2 * gtp + (gn - gtp) + gfp)
        if suffix and suffix != "_clean":
            # rc < 6: the frame had a reference; rows cov, columns rc
            ref_hit, ref_miss = lab[:, :, j + 1:6], lab[:, :, :j + 1]
            put("segment_lost" + suffix, int(ref_hit[:, :j + 1].sum()), int(ref_hit.sum()))
            put("segment_recovered" + suffix, int(ref_miss[:, j + 1:].sum()), int(ref_miss.sum()))
    adverse = list(kinds) if kinds else [name for name in conditions if name != "clean"]
    for kind in adverse:
        for key, out, sign in (("segment_recall", "segment_recall_drop", 1.0), ("segment_miss_rate", "segment_miss_rate_rise", -1.0)):
            a, b = f"{key}_clean", f"{key}_{kind}"
            if a in res and b in res:
                res[f"{out}_{kind}"] = float(sign * (res[a] - res[b]))
    return res


def change_metrics_from_stats(stats, edges, slots: List[str], kinds, levels: int, num_classes: int) -> Dict[str, float]:
    """Result keys of the change-strata counters (int64 [1 + len(slots), K + 1, C*C + 6], include/awseg.h; slot 0 = every corrupted
    frame, slot 1 + k = slots[k]; K = len(edges) + 1 strata, row K the unmeasured pixels).  Host only; every value a float.  Stratum
    k holds the pixels whose input change lies in [edges[k - 1], edges[k]) (stratum 0: below edges[0], stratum K - 1: from the last
    edge up).  Pooling as severity_sweep_results: per '<kind>_s<j>', per '<kind>' from the summed counters of its levels, and over
    slot 0 under the prefix 'mean_'.  With <n> the name and k = 0 .. K - 1 (the mean_ keys carry no name: mean_miou_chg0):
      change_fraction_<n>_chg<k>           pixels[k] / all pixels, the unmeasured row included
      miou_<n>_chg<k>                      iou_from_counts on conf[k]; absent without a labelled pixel
      accuracy_<n>_chg<k>                  trace / total of conf[k]; absent without a labelled pixel
      consistency_<n>_chg<k>               agree[k] / pixels[k]; absent without a pixel
      corruption_error_rate_<n>_chg<k>     cw / (cc + cw): of the labelled pixels the clean prediction gets right, those the
                                           corrupted one gets wrong; absent when the clean prediction gets none right
      corruption_error_share_<n>_chg<k>    cw[k] / sum of cw over every row (the unmeasured one included): the share of the newly
                                           introduced errors that sit in stratum k; absent when there is no such error
    and change_edge_<k> (k = 0 .. K - 2) plus change_unmeasured_pixels (slot 0, when non-zero).  A name without a pixel yields no
    keys.  Known limit: these counters never wrap uint8 labels, the pooled confusion counters do at C = 19 (as the reference does),
    so there miou_*_chg<k> describes the unwrapped confusion matrix and the strata need not recombine to the pooled miou_<n>."""
    e = ops.change_edges(list(edges))
    K, C = int(e.size) + 1, int(num_classes)
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.ndim != 3 or raw.shape != (1 + len(slots), K + 1, C * C + 6):
        raise ValueError(f"change-strata stats must be int64 [{1 + len(slots)}, {K + 1}, {C * C + 6}], got {raw.shape}")
    named = []
    for kind in kinds:
        idx = [1 + slots.index(f"{kind}_s{j}") for j in range(1, levels + 1)]
        named += [(f"_{kind}_s{j}", raw[i]) for j, i in zip(range(1, levels + 1), idx)]
        named.append((f"_{kind}", raw[idx].sum(0)))
    named.append((None, raw[0]))
    res: Dict[str, float] = {f"change_edge_{k}": float(e[k]) for k in range(K - 1)}
    for name, slot in named:
        dec = ops.strata_stats_to_numpy(slot, C)
        total = int(dec["pixels"].sum())
        if total <= 0:
            continue
        new_errors = int(dec["transitions"][:, 1].sum())

        def key(metric, k, name=name):
            return f"mean_{metric}_chg{k}" if name is None else f"{metric}{name}_chg{k}"
        for k in range(K):
            px, conf, t = int(dec["pixels"][k]), dec["conf"][k], dec["transitions"][k]
            res[key("change_fraction", k)] = float(px / total)
            labelled = int(conf.sum())
            if labelled > 0:
                res[key("miou", k)] = float(iou_from_counts(torch.from_numpy(conf.reshape(-1).copy()), C)["mean_iou"])
                res[key("accuracy", k)] = float(int(np.trace(conf)) / labelled)
            if px > 0:
                res[key("consistency", k)] = float(int(dec["agree"][k]) / px)
            clean_right = int(t[0]) + int(t[1])
            if clean_right > 0:
                res[key("corruption_error_rate", k)] = float(int(t[1]) / clean_right)
            if new_errors > 0:
                res[key("corruption_error_share", k)] = float(int(t[1]) / new_errors)
    unmeasured = int(raw[0, K, C * C + 5])
    if unmeasured:
        res["change_unmeasured_pixels"] = float(unmeasured)
    return res


IQ_SLOPE_MIN_DAMAGE = 1e-6                                          # miou_drop_per_ssim needs 1 - ssim at least this


def quality_metrics_from_stats(stats, slots: List[str], kinds, levels: int, results: Dict[str, Any], targets=(0.9, 0.75, 0.5),
                               degradation=None) -> Dict[str, float]:
    """Result keys of the image-quality counters (int64 [1 + len(slots), AWSEG_IQ_ROW], include/awseg.h; slot 0 = every corrupted
    frame, slot 1 + k = slots[k]; the clean slot stays empty: a clean frame has no twin) and, with the sweep's mIoU keys in
    `results` (miou_clean, miou_<kind>_s<j>), the mIoU at equal SSIM.  Host only, float64 on exact integer sums; every value a float.
    Pooling as severity_sweep_results: per '<kind>_s<j>', per '<kind>' from the summed counters of its levels, and over slot 0 under
    the prefix 'mean_' (mean_psnr, mean_ssim).  With <n> the name:
      mse_<n>                  sum of squared differences / error terms, on the [0, 1] scale; present when terms were measured
      psnr_<n>                 10 log10(1 / mse) in dB; absent when mse == 0
      mean_abs_change_<n>      mean absolute difference in 8-bit grey levels (x 255)
      ssim_<n>, ssim_luminance_<n>, ssim_contrast_<n>   means over the measured windows of s, l and cs; present when windows were
                               measured.  The accuracy of these numbers is that of the float32 window arithmetic
    and quality_unmeasured_terms, quality_unmeasured_windows (slot 0, when non-zero).
    Matched damage, per kind: the points (1, miou_clean), (ssim_<kind>_s<j>, miou_<kind>_s<j>) for j = 1 .. levels must all be
    there and SSIM must strictly decrease with j, else the kind gets none of the following and ssim_not_monotonic_<kind> = 1.0.
    For every target t in `targets` within [ssim_<kind>_s<levels>, 1] (no extrapolation), TT = round(100 t):
      miou_at_ssim<TT>_<kind>                        piecewise linear in SSIM between the points
      robustness_degradation_at_ssim<TT>_<kind>      degradation(miou_clean, that)
      mean_miou_at_ssim<TT>                          mean over the kinds, only when every kind has the value
    and per level miou_drop_per_ssim_<kind>_s<j> = (miou_clean - miou_<kind>_s<j>) / (1 - ssim_<kind>_s<j>), absent when the
    denominator is below 1e-6.  degradation: RobustnessMetrics.compute_robustness_degradation_ratio unless given."""
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.ndim != 2 or raw.shape != (1 + len(slots), ops.IQ_ROW):
        raise ValueError(f"image-quality stats must be int64 [{1 + len(slots)}, {ops.IQ_ROW}], got {raw.shape}")
    degradation = degradation or RobustnessMetrics().compute_robustness_degradation_ratio
    kinds, levels = list(kinds), int(levels)
    named = []
    for kind in kinds:
        idx = [1 + slots.index(f"{kind}_s{j}") for j in range(1, levels + 1)]
        named += [(f"{kind}_s{j}", raw[i]) for j, i in zip(range(1, levels + 1), idx)]
        named.append((kind, raw[idx].sum(0)))
    named.append((None, raw[0]))
    res: Dict[str, float] = {}
    for name, row in named:
        dec = {f: int(v) for f, v in ops.image_quality_to_numpy(row).items()}

        def key(metric, name=name):
            return f"mean_{metric}" if name is None else f"{metric}_{name}"
        if dec["error_terms"] > 0:
            mse = dec["sum_sq"] * ops.IQ_UNIT / dec["error_terms"]
            res[key("mse")] = float(mse)
            if mse > 0:
                res[key("psnr")] = float(10.0 * np.log10(1.0 / mse))
            res[key("mean_abs_change")] = float(255.0 * dec["sum_abs"] * ops.IQ_UNIT / dec["error_terms"])
        if dec["windows"] > 0:
            res[key("ssim")] = float(dec["sum_ssim"] * ops.IQ_UNIT / dec["windows"])
            res[key("ssim_luminance")] = float(dec["sum_luminance"] * ops.IQ_UNIT / dec["windows"])
            res[key("ssim_contrast")] = float(dec["sum_contrast"] * ops.IQ_UNIT / dec["windows"])
    for k, field in (("quality_unmeasured_terms", "error_terms_unmeasured"), ("quality_unmeasured_windows", "windows_unmeasured")):
        v = int(ops.image_quality_to_numpy(raw[0])[field])
        if v:
            res[k] = float(v)
    clean = results.get("miou_clean")
    at = {}                                                                 # TT -> {kind: interpolated mIoU}
    for kind in kinds:
        pts = [(1.0, clean)] + [(res.get(f"ssim_{kind}_s{j}"), results.get(f"miou_{kind}_s{j}")) for j in range(1, levels + 1)]
        if clean is not None:
            for j in range(1, levels + 1):
                q, m = pts[j]
                if q is not None and m is not None and 1.0 - q >= IQ_SLOPE_MIN_DAMAGE:
                    res[f"miou_drop_per_ssim_{kind}_s{j}"] = float((float(clean) - float(m)) / (1.0 - q))
        if any(q is None or m is None for q, m in pts) or any(not pts[j + 1][0] < pts[j][0] for j in range(levels)):
            res[f"ssim_not_monotonic_{kind}"] = 1.0
            continue
        qs = np.array([q for q, _ in pts][::-1], dtype=np.float64)          # ascending for np.interp
        ms = np.array([float(m) for _, m in pts][::-1], dtype=np.float64)
        for t in targets:
            t = float(t)
            if not qs[0] <= t <= 1.0:
                continue
            tt = int(round(100.0 * t))
            v = float(np.interp(t, qs, ms))
            res[f"miou_at_ssim{tt}_{kind}"] = v
            res[f"robustness_degradation_at_ssim{tt}_{kind}"] = float(degradation(float(clean), v))
            at.setdefault(tt, {})[kind] = v
    for tt, per in at.items():
        if kinds and all(k in per for k in kinds):
            res[f"mean_miou_at_ssim{tt}"] = float(np.mean([per[k] for k in kinds]))
    return res


def restoration_metrics_from_stats(restored, plain, stats, conditions: List[str], num_classes: int, kinds=None, levels: int = 0,
                                   degradation=None) -> Dict[str, float]:
    """Result keys of the dehazing front-end.  `restored`, `plain`: the confusion counters int64
    [1 + len(conditions), C * C] of the forward on the restored frames and of the ordinary one; `stats`: the dehazing counters int64
    [1 + len(conditions), AWSEG_DEHAZE_ROW] (include/awseg_restore.h); slot 0 = every restored frame, slot 1 + k = conditions[k].
    Host only, float64 on exact integer sums; every value a float.  With <n> a condition (under a severity sweep its slots
    'clean', '<kind>_s<j>', and each '<kind>' from the summed counters of its levels), for every <n> with restored frames:
      miou_<n>_restored                         mIoU of the restored frames, as miou_<n> is of the plain ones
      restoration_gain_<n>                      miou_<n>_restored - miou_<n> on the same frames; not clamped: a loss is negative
      airlight_<n>                              the mean over the three channels of the frames' mean airlight
      transmission_mean_<n>                     the mean transmission t over the restored pixels
    over slot 0: overall_miou_restored, mean_restoration_gain (against the plain counters summed over the conditions that have
    restored frames: the same frames when every frame carries a condition of the list), mean_airlight, mean_transmission;
      restoration_clean_cost                    miou_clean - miou_clean_restored: what the front-end costs where nothing was wrong
      robustness_degradation_<n>_restored       degradation(plain miou_clean, miou_<n>_restored), <n> != clean
      restoration_nonfinite_values, restoration_airlight_floored_frames    slot 0, only when non-zero
    A ratio without a denominator is absent, not 0: no restored frame, no key.  degradation:
    RobustnessMetrics.compute_robustness_degradation_ratio unless given."""
    conditions, C = list(conditions), int(num_classes)
    n = 1 + len(conditions)
    conf = {}
    for what, a in (("restored", restored), ("plain", plain)):
        a = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.int64)
        if a.shape != (n, C * C):
            raise ValueError(f"{what} confusion counters must be int64 [{n}, {C * C}], got {a.shape}")
        conf[what] = a
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.shape != (n, ops.DEHAZE_ROW):
        raise ValueError(f"dehaze stats must be int64 [{n}, {ops.DEHAZE_ROW}], got {raw.shape}")
    degradation = degradation or RobustnessMetrics().compute_robustness_degradation_ratio

    def miou(counts) -> Optional[float]:
        return float(iou_from_counts(torch.from_numpy(counts.copy()), C)["mean_iou"]) if counts.sum() > 0 else None

    named = [(name, [1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        named.append((kind, [1 + conditions.index(f"{kind}_s{j}") for j in range(1, int(levels) + 1)]))
    res: Dict[str, float] = {}
    clean_plain = miou(conf["plain"][1 + conditions.index("clean")]) if "clean" in conditions else None
    same_frames = np.zeros(C * C, dtype=np.int64)                           # plain counters of the conditions that were restored
    rows = [(None, conf["restored"][0], None, raw[0])]
    for name, idx in named:
        rows.append((name, conf["restored"][idx].sum(0), conf["plain"][idx].sum(0), raw[idx].sum(0)))
        if len(idx) == 1 and conf["restored"][idx[0]].sum() > 0:
            same_frames += conf["plain"][idx[0]]
    for name, r_counts, p_counts, row in rows:
        dec = {f: int(v) for f, v in ops.dehaze_stats_to_numpy(row).items()}

        def key(metric, name=name):
            return f"mean_{metric}" if name is None else f"{metric}_{name}"
        r = miou(r_counts)
        if r is not None:
            res["overall_miou_restored" if name is None else f"miou_{name}_restored"] = r
            p = miou(same_frames if name is None else p_counts)
            if p is not None:
                res[key("restoration_gain")] = r - p
            if name is not None and name != "clean" and clean_plain is not None:
                res[f"robustness_degradation_{name}_restored"] = float(degradation(clean_plain, r))
        if dec["frames"] > 0:
            res[key("airlight")] = float(sum(dec[f"sum_airlight_{c}"] for c in range(3)) * ops.DEHAZE_UNIT / (3.0 * dec["frames"]))
        if dec["pixels"] > 0:
            res["mean_transmission" if name is None else f"transmission_mean_{name}"] = float(dec["sum_transmission"] * ops.DEHAZE_UNIT
                                                                                              / dec["pixels"])
    if clean_plain is not None and "miou_clean_restored" in res:
        res["restoration_clean_cost"] = clean_plain - res["miou_clean_restored"]
    for k, field in (("restoration_nonfinite_values", "nonfinite_values"), ("restoration_airlight_floored_frames", "airlight_floored_frames")):
        v = int(ops.dehaze_stats_to_numpy(raw[0])[field])
        if v:
            res[k] = float(v)
    return res


def tta_metrics_from_stats(tta_counts, plain_counts, consistency, conditions: List[str], num_classes: int, kinds=None, levels: int = 0,
                           degradation=None, views=None, scales=None, flip=None) -> Dict[str, Any]:
    """Result keys of the test-time augmentation.  `tta_counts`, `plain_counts`: the confusion counters int64
    [1 + len(conditions), C * C] of the view-averaged prediction and of the plain one; `consistency`: int64 [1 + len(conditions),
    C * C + 4] (ops.new_consistency_stats), the agreement matrix A[plain class, TTA class] over all pixels and the four transition
    counts over the labelled ones (both right, plain right + TTA wrong, plain wrong + TTA right, both wrong); slot 0 = every frame,
    slot 1 + k = conditions[k].  Host only, float64 on exact integer sums.  With <n> a condition (under a severity sweep its slots
    'clean', '<kind>_s<j>', and each '<kind>' from the summed counters of its levels), for every <n> with frames:
      miou_<n>_tta                       mIoU of the averaged prediction, as miou_<n> is of the plain one
      tta_gain_<n>                       miou_<n>_tta - miou_<n> on the same frames; not clamped: a loss is negative
      robustness_degradation_<n>_tta     degradation(miou_clean_tta, miou_<n>_tta), <n> != clean
      tta_changed_fraction_<n>           1 - trace(A) / sum(A): the share of the pixels whose class the averaging changed
      tta_fixed_fraction_<n>             plain wrong and TTA right, over the labelled pixels
      tta_broken_fraction_<n>            plain right and TTA wrong, over the labelled pixels
    over slot 0: overall_miou_tta, mean_tta_gain (against the plain counters summed over the conditions that have frames),
    mean_tta_changed_fraction; and, when given, tta_views (float), tta_scales (a list of floats), tta_flip (1.0 or 0.0).
    A ratio without a denominator is absent, not 0.  degradation: RobustnessMetrics.compute_robustness_degradation_ratio unless
    given."""
    conditions, C = list(conditions), int(num_classes)
    n = 1 + len(conditions)
    arrays = {}
    for what, a, width in (("tta", tta_counts, C * C), ("plain", plain_counts, C * C), ("consistency", consistency, C * C + 4)):
        a = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.int64)
        if a.shape != (n, width):
            raise ValueError(f"{what} counters must be int64 [{n}, {width}], got {a.shape}")
        arrays[what] = a
    degradation = degradation or RobustnessMetrics().compute_robustness_degradation_ratio

    def miou(counts) -> Optional[float]:
        return float(iou_from_counts(torch.from_numpy(counts.copy()), C)["mean_iou"]) if counts.sum() > 0 else None

    named = [(name, [1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        named.append((kind, [1 + conditions.index(f"{kind}_s{j}") for j in range(1, int(levels) + 1)]))
    res: Dict[str, Any] = {}
    same_frames = np.zeros(C * C, dtype=np.int64)                           # plain counters of the conditions that have TTA frames
    rows = [(None, arrays["tta"][0], None, arrays["consistency"][0])]
    for name, idx in named:
        rows.append((name, arrays["tta"][idx].sum(0), arrays["plain"][idx].sum(0), arrays["consistency"][idx].sum(0)))
        if len(idx) == 1 and arrays["tta"][idx[0]].sum() > 0:
            same_frames += arrays["plain"][idx[0]]
    mious = {}
    for name, t_counts, p_counts, row in rows:
        t = miou(t_counts)
        if t is not None:
            mious[name] = t
            res["overall_miou_tta" if name is None else f"miou_{name}_tta"] = t
            p = miou(same_frames if name is None else p_counts)
            if p is not None:
                res["mean_tta_gain" if name is None else f"tta_gain_{name}"] = t - p
        agreement, transitions = row[:C * C].reshape(C, C), row[C * C:]
        pixels, labelled = int(agreement.sum()), int(transitions.sum())
        if pixels > 0:
            res["mean_tta_changed_fraction" if name is None else f"tta_changed_fraction_{name}"] = 1.0 - float(np.trace(agreement)) / pixels
        if labelled > 0 and name is not None:
            res[f"tta_fixed_fraction_{name}"] = float(transitions[2]) / labelled
            res[f"tta_broken_fraction_{name}"] = float(transitions[1]) / labelled
    for name, t in mious.items():
        if name is not None and name != "clean" and "clean" in mious:
            res[f"robustness_degradation_{name}_tta"] = float(degradation(mious["clean"], t))
    if views is not None:
        res["tta_views"] = float(views)
    if scales is not None:
        res["tta_scales"] = [float(s) for s in scales]
    if flip is not None:
        res["tta_flip"] = float(bool(flip))
    return res


def guided_metrics_from_stats(stats, conditions: List[str], kinds=None, levels: int = 0) -> Dict[str, float]:
    """Result keys of the guided-filter refinement from its counters int64 [1 + len(conditions),
    AWSEG_GUIDED_ROW] (include/awseg_restore.h; slot 0 = every restored frame, slot 1 + k = conditions[k]).  Host only, float64 on
    exact integer sums; every value a float.  With <n> a condition (under a sweep its slots and each '<kind>' from the summed counters
    of its levels), for every <n> with restored pixels:
      transmission_refinement_<n>        mean |t - t_patch|: how far the filter moved the patch transmission fmaxf(p, t_min)
      transmission_clamped_fraction_<n>  share of the pixels whose filter output q was above 1 or below t_min
    and over slot 0 mean_transmission_refinement, mean_transmission_clamped_fraction.  No pixel, no key."""
    conditions = list(conditions)
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.shape != (1 + len(conditions), ops.GUIDED_ROW):
        raise ValueError(f"guided stats must be int64 [{1 + len(conditions)}, {ops.GUIDED_ROW}], got {raw.shape}")
    named = [(None, raw[0])] + [(name, raw[1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        named.append((kind, raw[[1 + conditions.index(f"{kind}_s{j}") for j in range(1, int(levels) + 1)]].sum(0)))
    res: Dict[str, float] = {}
    for name, row in named:
        dec = {f: int(v) for f, v in ops.guided_stats_to_numpy(row).items()}
        if dec["pixels"] <= 0:
            continue
        moved = float(dec["sum_transmission_moved"] * ops.DEHAZE_UNIT / dec["pixels"])
        clamped = float((dec["above_one_pixels"] + dec["below_floor_pixels"]) / dec["pixels"])
        res["mean_transmission_refinement" if name is None else f"transmission_refinement_{name}"] = moved
        res["mean_transmission_clamped_fraction" if name is None else f"transmission_clamped_fraction_{name}"] = clamped
    return res


def relight_metrics_from_stats(stats, conditions: List[str], kinds=None, levels: int = 0) -> Dict[str, Any]:
    """Result keys of the night relighting (evaluation.restoration with method: clahe) from its counters int64
    [1 + len(conditions), AWSEG_RELIGHT_ROW] (include/awseg_restore.h; slot 0 = every restored frame, slot 1 + k = conditions[k]).
    Host only, float64 on exact integer sums; every value a float but restoration_method.  With <n> a condition (under a sweep its
    slots and each '<kind>' from the summed counters of its levels; slot 0 under the prefix mean_ instead of the suffix):
      luma_<n>, luma_<n>_restored        mean luma of the frames as they came and as they were restored (pixels > 0)
      relight_gain_<n>                   their ratio, restored / plain (plain luma > 0)
      white_balance_gain_{r,g,b}_<n>     the frames' mean grey-world gains (frames > 0)
      relight_capped_fraction_<n>        share of the pixels whose luma gain was held at max_gain
      relight_saturated_fraction_<n>     share of the channel values (3 per pixel) that left [0, 1] upwards and were clipped
    and restoration_method = 'clahe'; restoration_nonfinite_values (slot 0) only when non-zero.  A ratio without a denominator is
    absent, not 0."""
    conditions = list(conditions)
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.shape != (1 + len(conditions), ops.RELIGHT_ROW):
        raise ValueError(f"relight stats must be int64 [{1 + len(conditions)}, {ops.RELIGHT_ROW}], got {raw.shape}")
    named = [(None, raw[0])] + [(name, raw[1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        named.append((kind, raw[[1 + conditions.index(f"{kind}_s{j}") for j in range(1, int(levels) + 1)]].sum(0)))
    res: Dict[str, Any] = {"restoration_method": "clahe"}
    for name, row in named:
        dec = {f: int(v) for f, v in ops.relight_stats_to_numpy(row).items()}

        def key(metric, tail="", name=name):
            return f"mean_{metric}{tail}" if name is None else f"{metric}_{name}{tail}"
        if dec["frames"] > 0:
            for c, ch in enumerate("rgb"):
                res[key(f"white_balance_gain_{ch}")] = float(dec[f"sum_gain_{c}"] * ops.RELIGHT_UNIT / dec["frames"])
        if dec["pixels"] > 0:
            res[key("luma")] = float(dec["sum_luma"] * ops.RELIGHT_UNIT / dec["pixels"])
            res[key("luma", "_restored")] = float(dec["sum_luma_restored"] * ops.RELIGHT_UNIT / dec["pixels"])
            if dec["sum_luma"] > 0:
                res[key("relight_gain")] = float(dec["sum_luma_restored"] / dec["sum_luma"])
            res[key("relight_capped_fraction")] = float(dec["capped_pixels"] / dec["pixels"])
            res[key("relight_saturated_fraction")] = float(dec["saturated_values"] / (3.0 * dec["pixels"]))
    nonfinite = int(ops.relight_stats_to_numpy(raw[0])["nonfinite_values"])
    if nonfinite:
        res["restoration_nonfinite_values"] = float(nonfinite)
    return res


def deocclude_metrics_from_stats(stats, conditions: List[str], kinds=None, levels: int = 0) -> Dict[str, Any]:
    """Result keys of the rain and snow removal (evaluation.restoration with method: tophat) from its counters int64
    [1 + len(conditions), AWSEG_DEOCCLUDE_ROW] (include/awseg_restore.h; slot 0 = every restored frame, slot 1 + k = conditions[k]).
    Host only, float64 on exact integer sums; every value a float but restoration_method.  With <n> a condition (under a sweep its
    slots and each '<kind>' from the summed counters of its levels; slot 0 under the prefix mean_ instead of the suffix):
      occluder_fraction_<n>              masked pixels / pixels
      occluder_seed_fraction_<n>         seed pixels (before the dilation) / pixels
      occluder_unfilled_fraction_<n>     masked pixels without an unmasked neighbour in their window / masked pixels
      occluder_change_<n>                mean absolute change per masked channel value (3 per masked pixel), in [0, 1]
    and restoration_method = 'tophat'; restoration_nonfinite_values (slot 0) only when non-zero.  A ratio without a denominator is
    absent, not 0."""
    conditions = list(conditions)
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.shape != (1 + len(conditions), ops.DEOCCLUDE_ROW):
        raise ValueError(f"deocclude stats must be int64 [{1 + len(conditions)}, {ops.DEOCCLUDE_ROW}], got {raw.shape}")
    named = [(None, raw[0])] + [(name, raw[1 + k]) for k, name in enumerate(conditions)]
    for kind in (kinds or []):
        named.append((kind, raw[[1 + conditions.index(f"{kind}_s{j}") for j in range(1, int(levels) + 1)]].sum(0)))
    res: Dict[str, Any] = {"restoration_method": "tophat"}
    for name, row in named:
        dec = {f: int(v) for f, v in ops.deocclude_stats_to_numpy(row).items()}

        def key(metric, name=name):
            return f"mean_{metric}" if name is None else f"{metric}_{name}"
        if dec["pixels"] > 0:
            res[key("occluder_fraction")] = float(dec["masked_pixels"] / dec["pixels"])
            res[key("occluder_seed_fraction")] = float(dec["seed_pixels"] / dec["pixels"])
        if dec["masked_pixels"] > 0:
            res[key("occluder_unfilled_fraction")] = float(dec["unfilled_pixels"] / dec["masked_pixels"])
            res[key("occluder_change")] = float(dec["sum_change"] * ops.DEOCCLUDE_UNIT / (3.0 * dec["masked_pixels"]))
    nonfinite = int(ops.deocclude_stats_to_numpy(raw[0])["nonfinite_values"])
    if nonfinite:
        res["restoration_nonfinite_values"] = float(nonfinite)
    return res


def estimate_metrics_from_stats(stats, conditions: List[str], kinds=None, levels: int = 0, route: str = "estimated") -> Dict[str, Any]:
    """Result keys of the blind routing (evaluation.restoration with method: auto) from the counters of the weather
    estimate, int64 [1 + len(conditions), AWSEG_ESTIMATE_ROW] (include/awseg_restore.h; slot 0 = every selected frame, slot 1 + k =
    conditions[k]).  Host only, float64 on exact integer sums; every value a float but restoration_method and restoration_route.
    With <n> a condition (under a sweep its slots and each '<kind>' from the summed counters of its levels; slot 0 under the prefix
    mean_ instead of the suffix), for every <n> with frames:
      route_{none,dark_channel,clahe,tophat}_fraction_<n>   share of the frames the ESTIMATE sent to that method: the rows of the
                                         confusion table of estimated against true condition (under route: oracle the routes
                                         applied are ops.ESTIMATE_EXPECTED_ROUTE's, these stay the estimate's)
      route_accuracy_<n>                 share of the frames sent where ops.ESTIMATE_EXPECTED_ROUTE sends <n> ('<kind>_s<j>' counts as
                                         its kind); only for the conditions the map names
      route_accuracy                     the same pooled over the condition slots the map names
      estimate_dark_channel_<n>, estimate_luma_<n>          mean dark channel and mean luma over the pixels
      estimate_cast_<n>                  red over blue: the ratio of the channel sums 0 and 2 (absent when channel 2 sums to 0)
      estimate_seed_fraction_<n>         top-hat seeds / pixels
    and restoration_method = 'auto', restoration_route = `route`; restoration_nonfinite_values (slot 0) only when non-zero.  A ratio
    without a denominator is absent, not 0."""
    conditions = list(conditions)
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    if raw.shape != (1 + len(conditions), ops.ESTIMATE_ROW):
        raise ValueError(f"estimate stats must be int64 [{1 + len(conditions)}, {ops.ESTIMATE_ROW}], got {raw.shape}")
    if route not in ("estimated", "oracle"):
        raise ValueError(f"route is 'estimated' or 'oracle', got {route!r}")
    kinds, levels = list(kinds or []), int(levels)

    def expected(name):
        """The route the map names for a condition, a sweep's slot or a kind; None when it names none."""
        base = name.rsplit("_s", 1)[0] if kinds and name not in ops.ESTIMATE_EXPECTED_ROUTE and name.rsplit("_s", 1)[0] in kinds else name
        return ops.ESTIMATE_EXPECTED_ROUTE.get(base)
    named = [(None, raw[0])] + [(name, raw[1 + k]) for k, name in enumerate(conditions)]
    for kind in kinds:
        named.append((kind, raw[[1 + conditions.index(f"{kind}_s{j}") for j in range(1, levels + 1)]].sum(0)))
    res: Dict[str, Any] = {"restoration_method": "auto", "restoration_route": route}
    for name, row in named:
        dec = {f: int(v) for f, v in ops.estimate_stats_to_numpy(row).items()}

        def key(metric, name=name):
            return f"mean_{metric}" if name is None else f"{metric}_{name}"
        if dec["frames"] > 0:
            for r in ops.ESTIMATE_ROUTES:
                res[key(f"route_{r}_fraction")] = float(dec[f"routed_{r}"] / dec["frames"])
            want = None if name is None else expected(name)
            if want is not None:
                res[f"route_accuracy_{name}"] = float(dec[f"routed_{want}"] / dec["frames"])
        if dec["pixels"] > 0:
            res[key("estimate_dark_channel")] = float(dec["sum_dark"] * ops.ESTIMATE_UNIT / dec["pixels"])
            res[key("estimate_luma")] = float(dec["sum_luma"] * ops.ESTIMATE_UNIT / dec["pixels"])
            res[key("estimate_seed_fraction")] = float(dec["seed_pixels"] / dec["pixels"])
        if dec["sum_channel_2"] > 0:
            res[key("estimate_cast")] = float(dec["sum_channel_0"] / dec["sum_channel_2"])
    right = frames = 0
    for k, name in enumerate(conditions):                                  # the slots themselves: a kind's sum would count them twice
        want = expected(name)
        if want is not None:
            dec = ops.estimate_stats_to_numpy(raw[1 + k])
            right, frames = right + int(dec[f"routed_{want}"]), frames + int(dec["frames"])
    if frames > 0:
        res["route_accuracy"] = float(right / frames)
    nonfinite = int(ops.estimate_stats_to_numpy(raw[0])["nonfinite_values"])
    if nonfinite:
        res["restoration_nonfinite_values"] = float(nonfinite)
    return res


IQ_PLAIN_STEMS = ("mse", "psnr", "mean_abs_change", "ssim", "ssim_luminance", "ssim_contrast")


def restored_quality_metrics_from_stats(restored, plain, slots: List[str], kinds, levels: int) -> Dict[str, float]:
    """Fidelity of the restored frames: `restored`, `plain` image-quality counters int64 [1 + len(slots), AWSEG_IQ_ROW] of the
    restored frames and of the corrupted ones against the same clean twins.  The clean slot of `restored` holds the restored clean
    frames against themselves-before (the clean slot of `plain` is empty).  Host only; every value a float.  With <stem> one of
    IQ_PLAIN_STEMS and <n> a '<kind>_s<j>' or a '<kind>' (summed counters of its levels), from quality_metrics_from_stats:
      <stem>_<n>_restored                   that key of the restored counters
      restoration_psnr_gain_<n>, restoration_ssim_gain_<n>     restored - plain on the same frames
      mean_<stem>_restored, mean_restoration_psnr_gain, mean_restoration_ssim_gain     pooled over the corrupted frames that were
                                            restored (the clean ones left out; the plain side over the same slots)
      psnr_clean_restored, ssim_clean_restored                 what the front-end does to a frame that needed nothing
    The mIoU-at-equal-SSIM interpolation is not repeated.  A ratio without a denominator is absent, not 0."""
    slots, kinds, levels = list(slots), list(kinds), int(levels)
    r = np.asarray(restored.cpu().numpy() if isinstance(restored, torch.Tensor) else restored, dtype=np.int64).copy()
    p = np.asarray(plain.cpu().numpy() if isinstance(plain, torch.Tensor) else plain, dtype=np.int64).copy()
    for what, a in (("restored", r), ("plain", p)):
        if a.shape != (1 + len(slots), ops.IQ_ROW):
            raise ValueError(f"{what} image-quality stats must be int64 [{1 + len(slots)}, {ops.IQ_ROW}], got {a.shape}")
    res: Dict[str, float] = {}
    if "clean" in slots:
        row = r[1 + slots.index("clean")]
        own = quality_metrics_from_stats(np.stack([row, row]), ["clean_s1"], ["clean"], 1, {})
        res.update({f"{stem}_clean_restored": own[f"{stem}_clean"] for stem in ("psnr", "ssim") if f"{stem}_clean" in own})
    level_slots = [1 + slots.index(f"{kind}_s{j}") for kind in kinds for j in range(1, levels + 1)]
    done = [i for i in level_slots if r[i].any()]
    r[0], p[0] = r[done].sum(0), p[done].sum(0)                              # pooled: the corrupted frames that were restored
    after, before = quality_metrics_from_stats(r, slots, kinds, levels, {}), quality_metrics_from_stats(p, slots, kinds, levels, {})
    names = [f"{kind}_s{j}" for kind in kinds for j in range(1, levels + 1)] + kinds
    for stem in IQ_PLAIN_STEMS:
        for key in [f"{stem}_{n}" for n in names] + [f"mean_{stem}"]:
            if key in after:
                res[f"{key}_restored"] = after[key]
    for stem in ("psnr", "ssim"):
        for n in names + [None]:
            key = f"mean_{stem}" if n is None else f"{stem}_{n}"
            if key in after and key in before:
                res[f"mean_restoration_{stem}_gain" if n is None else f"restoration_{stem}_gain_{n}"] = after[key] - before[key]
    return res


def weight_grid_row_miou(inter, lab, prd) -> Optional[float]:
    """mIoU from the marginals of one grid point (int64 [C] each: hits, labelled, predicted): iou_from_counts' expressions (int64 /
    int64 true-divide to float32, mean over the classes with a non-empty union), so the configured point reproduces the pooled
    mIoU of the confusion matrix bit for bit.  None when no class has a union."""
    i, l, p = (torch.as_tensor(np.ascontiguousarray(v), dtype=torch.int64) for v in (inter, lab, prd))
    union = l + p - i
    valid = union > 0
    if not bool(valid.any()):
        return None
    return float((i[valid] / union[valid]).mean().item())


def weight_grid_metrics_from_stats(stats, conditions: List[str], num_classes: int, grid, configured_index: int,
                                   calibration_condition: str = "clean", kinds=None, levels=None) -> Dict[str, Any]:
    """Result keys of the ensemble weight sweep (int64 [1 + len(conditions), G + 3, 2 C], include/awseg.h; slot 0 = every frame, slot
    1 + k = conditions[k]).  grid: the G float32 pairs the counters were filled with; the SegFormer share of a point is its first
    weight.  configured_index: the point that holds the model's own softmax(ensemble_weights).  Host only.  Per suffix
    ('' | _<condition>), for every slot with a labelled pixel:
      ensemble_weight_best      the share of the point with the highest mIoU of the slot; ties go to the point nearest the configured
                                share, then to the lower index           miou_best_weight        the mIoU there
      miou_configured_weight    the mIoU at the configured point
      miou_fitted_weight        the mIoU at the fitted point: the best point of slot `calibration_condition` (ensemble_weight_fitted)
      miou_weight_gain          fitted minus configured
      miou_weight_regret_<s>    named slots only: the slot's own best minus its fitted value (what a clean-fitted weighting loses there)
      segformer_miou, deeplabv3plus_miou      the grid's ends (1, 0) and (0, 1), when the grid has them
      member_both_right, member_only_segformer, member_only_deeplabv3plus, member_neither_right, member_oracle_accuracy (1 - neither),
      member_disagreement       shares of the labelled pixels, from the members' own argmax
      ensemble_weight_miou_curve               the list of mIoUs, one per point
    and ensemble_weight_grid (the list of shares), weight_grid_out_of_range_labels / weight_grid_nan_pixels (slot 0, when non-zero).
    Severity sweep (kinds, levels): conditions are its slots ('clean', '<kind>_s<j>'); each kind gets ensemble_weight_best_<kind> and
    miou_weight_regret_<kind> from the summed counters of its slots.  All-zero stats give {}."""
    raw = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    C = int(num_classes)
    pairs = np.asarray(grid, dtype=np.float32)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1:
        raise ValueError(f"the weight grid is float32 [G, 2], got {pairs.shape}")
    G = pairs.shape[0]
    if raw.ndim != 3 or raw.shape != (1 + len(conditions), G + 3, 2 * C):
        raise ValueError(f"weight grid stats must be int64 [{1 + len(conditions)}, {G + 3}, {2 * C}], got {raw.shape}")
    if isinstance(configured_index, (bool, np.bool_)) or not 0 <= int(configured_index) < G:
        raise ValueError(f"configured_index is a grid point in [0, {G}), got {configured_index!r}")
    cfg = int(configured_index)
    if not raw.any():
        return {}
    shares = [float(v) for v in pairs[:, 0]]

    def curve(slot):
        return [weight_grid_row_miou(slot[g, :C], slot[G, :C], slot[g, C:]) for g in range(G)]

    def best(miou):
        top = max(miou)
        return min((g for g in range(G) if miou[g] == top), key=lambda g: (abs(shares[g] - shares[cfg]), g))

    def present(slot):
        return int(slot[G, :C].sum()) > 0

    fitted = None
    if calibration_condition in conditions and present(raw[1 + conditions.index(calibration_condition)]):
        fitted = best(curve(raw[1 + conditions.index(calibration_condition)]))
    ends = {"segformer": [g for g in range(G) if pairs[g, 0] == 1.0 and pairs[g, 1] == 0.0],
            "deeplabv3plus": [g for g in range(G) if pairs[g, 0] == 0.0 and pairs[g, 1] == 1.0]}
    res: Dict[str, Any] = {"ensemble_weight_grid": shares}
    if fitted is not None:
        res["ensemble_weight_fitted"] = shares[fitted]
    named = [("", raw[0])] + [("_" + name, raw[1 + k]) for k, name in enumerate(conditions)]
    for suffix, slot in named:
        if not present(slot):
            continue
        miou = curve(slot)
        b = best(miou)
        res[f"ensemble_weight_best{suffix}"] = shares[b]
        res[f"miou_best_weight{suffix}"] = miou[b]
        res[f"miou_configured_weight{suffix}"] = miou[cfg]
        if fitted is not None:
            res[f"miou_fitted_weight{suffix}"] = miou[fitted]
            res[f"miou_weight_gain{suffix}"] = miou[fitted] - miou[cfg]
            if suffix:
                res[f"miou_weight_regret{suffix}"] = miou[b] - miou[fitted]
        for member, at in ends.items():
            if at:
                res[f"{member}_miou{suffix}"] = miou[at[0]]
        labelled = int(slot[G, :C].sum())
        both, only1, only2 = int(slot[G, C:].sum()), int(slot[G + 1, :C].sum()), int(slot[G + 1, C:].sum())
        neither = labelled - both - only1 - only2
        res[f"member_both_right{suffix}"] = both / labelled
        res[f"member_only_segformer{suffix}"] = only1 / labelled
        res[f"member_only_deeplabv3plus{suffix}"] = only2 / labelled
        res[f"member_neither_right{suffix}"] = neither / labelled
        res[f"member_oracle_accuracy{suffix}"] = 1.0 - neither / labelled
        res[f"member_disagreement{suffix}"] = int(slot[G + 2, 2]) / labelled
        res[f"ensemble_weight_miou_curve{suffix}"] = miou
    for kind in (kinds or []):
        idx = [1 + conditions.index(f"{kind}_s{j}") for j in range(1, int(levels or 0) + 1)]
        slot = raw[idx].sum(0) if idx else None
        if slot is None or not present(slot):
            continue
        miou = curve(slot)
        b = best(miou)
        res[f"ensemble_weight_best_{kind}"] = shares[b]
        if fitted is not None:
            res[f"miou_weight_regret_{kind}"] = miou[b] - miou[fitted]
    for key, v in (("weight_grid_out_of_range_labels", int(raw[0, G + 2, 0])), ("weight_grid_nan_pixels", int(raw[0, G + 2, 1]))):
        if v:
            res[key] = float(v)
    return res


ADVERSE_KINDS = ("fog", "rain", "snow", "night")                    # the kinds finalize() reports a degradation for


def replicate_miou(counts, num_classes: int):
    """mIoU of every row of int64 [..., 3 C] counters (C intersection | C label count | C prediction count): iou_from_counts'
    float32 expressions (int64 / int64 true-divide, mean over the classes with a non-empty union) on the marginals instead of the
    confusion matrix.  -> (miou float64 [...], NaN where no class has a union; present bool [...]: some labelled pixel)."""
    t = torch.as_tensor(np.ascontiguousarray(counts), dtype=torch.int64)
    c = int(num_classes)
    if t.shape[-1] != 3 * c:
        raise ValueError(f"frame count rows hold 3 x {c} counters, got {t.shape[-1]}")
    inter, lab, prd = t[..., :c], t[..., c:2 * c], t[..., 2 * c:]
    union = lab + prd - inter
    valid = union > 0
    per = torch.where(valid, inter / union.clamp(min=1), torch.zeros((), dtype=torch.float32))
    miou = per.sum(-1) / valid.sum(-1).to(torch.float32)
    return miou.to(torch.float64).numpy(), (lab.sum(-1) > 0).numpy()


def bootstrap_metrics_from_replicates(replicates, conditions: List[str], num_classes: int, point: Dict[str, Any],
                                      confidence: float = 0.95, seed: int = 0, kinds=None, levels: int = 0,
                                      degradation=None) -> Dict[str, float]:
    """Interval keys of the frame bootstrap from the replicate sums int64 [R, 1 + len(conditions), 3 C] (ops.bootstrap_counts: slot 0
    = every frame, slot 1 + k = conditions[k]) and the pooled point estimates `point` (the results so far: a quantity gets an
    interval when its point estimate is there).  Host only.  Per quantity Q
      Q_ci_low, Q_ci_high   percentile interval: np.quantile(method='linear') of the valid replicates at (1 -+ confidence) / 2
      Q_se                  their standard deviation (ddof = 1; NaN below two)
    for Q = overall_miou, miou_<slot>, miou_<kind> (sweep: the kind's severity slots summed per replicate),
    robustness_degradation_<kind>[_s<j>] (`degradation` on the replicate's clean and adverse mIoU: the reference's clamp at 0 stays,
    so an interval can sit on 0), robustness_degradation_ratio (mean over kinds per replicate) and the unclamped
    miou_drop_<kind>[_s<j>] = clean - adverse, whose point value is a new key and which also gets miou_drop_*_p_nonpositive: the share
    of valid replicates with a drop <= 0 (the paired one-sided bootstrap p-value of 'this kind costs nothing').  A replicate in which
    a slot drew no labelled pixel is left out of every quantity that needs that slot (bootstrap_empty_replicates_<slot> counts them,
    when there are any)."""
    degradation = degradation or RobustnessMetrics().compute_robustness_degradation_ratio
    rep = replicates.cpu().numpy() if isinstance(replicates, torch.Tensor) else np.asarray(replicates, dtype=np.int64)
    if rep.ndim != 3 or rep.shape[1] != 1 + len(conditions) or rep.shape[2] != 3 * num_classes or rep.shape[0] < 1:
        raise ValueError(f"replicate sums must be int64 [R, {1 + len(conditions)}, {3 * num_classes}], got {rep.shape}")
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"confidence lies in (0, 1), got {confidence!r}")
    R = rep.shape[0]
    res: Dict[str, float] = {"bootstrap_replicates": float(R), "bootstrap_confidence": float(confidence), "bootstrap_seed": float(seed)}
    miou, present = replicate_miou(rep, num_classes)
    series: Dict[str, Any] = {}                                       # name in the mIoU namespace -> (values [R], valid [R])
    if "overall_miou" in point:
        series["overall"] = (miou[:, 0], present[:, 0])
    for k, name in enumerate(conditions):
        if f"miou_{name}" in point:
            series[name] = (miou[:, 1 + k], present[:, 1 + k])
    for kind in (kinds or []):
        idx = [1 + conditions.index(f"{kind}_s{j}") for j in range(1, levels + 1)]
        if f"miou_{kind}" in point:
            series[kind] = replicate_miou(rep[:, idx].sum(axis=1), num_classes)
    lo_q, hi_q = (1.0 - float(confidence)) / 2.0, (1.0 + float(confidence)) / 2.0

    def summarise(key, values, valid):
        v = np.asarray(values, dtype=np.float64)[valid]
        low, high = (np.quantile(v, [lo_q, hi_q], method="linear") if v.size else (np.nan, np.nan))
        res[f"{key}_ci_low"], res[f"{key}_ci_high"] = float(low), float(high)
        res[f"{key}_se"] = float(np.std(v, ddof=1)) if v.size >= 2 else float("nan")
        return v

    for name, (values, valid) in series.items():
        summarise("overall_miou" if name == "overall" else f"miou_{name}", values, valid)
        empty = int(R - valid.sum())
        if empty and name not in (kinds or []):
            res[f"bootstrap_empty_replicates_{name}"] = float(empty)
    if "clean" in series:
        clean, clean_ok = series["clean"]
        degs = {}
        for name, (values, valid) in series.items():
            if f"robustness_degradation_{name}" not in point:
                continue
            ok = clean_ok & valid
            deg = np.array([degradation(float(a), float(b)) if o else np.nan for a, b, o in zip(clean, values, ok)], dtype=np.float64)
            summarise(f"robustness_degradation_{name}", deg, ok)
            if name in ADVERSE_KINDS:
                degs[name] = (deg, ok)
            res[f"miou_drop_{name}"] = float(point["miou_clean"] - point[f"miou_{name}"])
            drop = summarise(f"miou_drop_{name}", clean - values, ok)
            res[f"miou_drop_{name}_p_nonpositive"] = float(np.mean(drop <= 0)) if drop.size else float("nan")
        if degs and "robustness_degradation_ratio" in point:
            ok = np.logical_and.reduce([o for _, o in degs.values()])
            summarise("robustness_degradation_ratio", np.mean([d for d, _ in degs.values()], axis=0), ok)
    return res


class EnsembleDisagreementMetrics:
    """PKG/evaluation/metrics.py:324-467 — torch ops on whatever device the logits live on."""

    def compute_disagreement_map(self, predictions_list: List[torch.Tensor]) -> torch.Tensor:
        if len(predictions_list) < 2:
            raise ValueError("Need at least 2 predictions for disagreement computation")
        probs = torch.stack([F.softmax(p, dim=1) for p in predictions_list], dim=0)
        mean_probs = probs.mean(dim=0)
        mean_entropy = -torch.sum(mean_probs * torch.log(mean_probs + 1e-8), dim=1)
        individual = -torch.sum(probs * torch.log(probs + 1e-8), dim=2)
        return mean_entropy - individual.mean(dim=0)

    def compute_variance_map(self, predictions_list: List[torch.Tensor]) -> torch.Tensor:
        return torch.var(torch.stack([F.softmax(p, dim=1) for p in predictions_list], dim=0), dim=0)

    def compute_disagreement_auroc(self, predictions_list, targets, error_threshold: float = 0.5) -> float:
        """metrics.py:393-438.  AUROC = rank statistic; computed from a device sort (Mann-Whitney
        with average ranks for ties), no sklearn round trip."""
        dis = self.compute_disagreement_map(predictions_list)
        mean_probs = torch.stack([F.softmax(p, dim=1) for p in predictions_list], dim=0).mean(dim=0)
        errors = (mean_probs.argmax(dim=1) != targets).reshape(-1)
        valid = targets.reshape(-1) != 255
        s, e = dis.reshape(-1)[valid].double(), errors[valid]
        n_pos, n_neg = int(e.sum().item()), int((~e).sum().item())
        if n_pos == 0 or n_neg == 0:
            return 0.5
        vals, inv, cnt = torch.unique(s, sorted=True, return_inverse=True, return_counts=True)
        end = torch.cumsum(cnt, 0).double()
        avg_rank = end - (cnt.double() - 1) / 2                                     # 1-based average rank per distinct value
        rank_sum_pos = avg_rank[inv][e].sum().item()
        return float((rank_sum_pos - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))

    def compute_jensen_shannon_divergence(self, pred1, pred2) -> torch.Tensor:
        p1, p2 = F.softmax(pred1, dim=1), F.softmax(pred2, dim=1)
        m = (p1 + p2) / 2
        kl1 = F.kl_div(p1.log(), m, reduction="none").sum(dim=1)
        kl2 = F.kl_div(p2.log(), m, reduction="none").sum(dim=1)
        return (kl1 + kl2) / 2


class RobustnessMetrics:
    """PKG/evaluation/metrics.py:470-651."""

    def __init__(self, num_classes: int = 19, weather_conditions: List[str] = None) -> None:
        self.num_classes = num_classes
        self.weather_conditions = weather_conditions or ["clean", "fog", "rain", "snow", "night"]
        self.iou_metrics = IoUMetrics(num_classes)
        self.calibration_metrics = ConfidenceCalibration()
        self.ensemble_metrics = EnsembleDisagreementMetrics()

    def new_accumulator(self, device) -> ConfusionAccumulator:
        return ConfusionAccumulator(self.num_classes, self.weather_conditions, device)

    def compute_miou(self, predictions: torch.Tensor, targets: torch.Tensor) -> float:
        return self.iou_metrics.compute_iou(predictions, targets)["mean_iou"]

    def compute_weather_specific_metrics(self, predictions_dict, targets_dict) -> Dict[str, float]:
        out = {}
        for weather in self.weather_conditions:
            if weather in predictions_dict and weather in targets_dict:
                p, t = predictions_dict[weather], targets_dict[weather]
                if len(p) > 0 and len(t) > 0:
                    out[f"miou_{weather}"] = self.compute_miou(p, t)
        return out

    def compute_robustness_degradation_ratio(self, clean_miou: float, adverse_miou: float) -> float:
        if clean_miou == 0:                                                          # metrics.py:559-563
            return 1.0
        return max(0.0, (clean_miou - adverse_miou) / clean_miou)

    def compute_comprehensive_metrics(self, predictions, targets, ensemble_predictions=None,
                                      weather_condition: str = "clean") -> Dict[str, float]:
        m = {"mean_iou": self.iou_metrics.compute_iou(predictions, targets)["mean_iou"],
             "pixel_accuracy": self.iou_metrics.compute_pixel_accuracy(predictions, targets),
             "expected_calibration_error": self.calibration_metrics.compute_ece(predictions, targets)}
        if ensemble_predictions and len(ensemble_predictions) >= 2:
            m["ensemble_disagreement_auroc"] = self.ensemble_metrics.compute_disagreement_auroc(ensemble_predictions, targets)
        m[f"miou_{weather_condition}"] = m["mean_iou"]
        return m

    def create_robustness_summary(self, weather_metrics: Dict[str, Dict[str, float]]) -> Dict[str, float]:
        summary = {}
        clean = weather_metrics.get("clean", {}).get("mean_iou", 0.0)
        for w in ("fog", "rain", "snow", "night"):
            if w in weather_metrics:
                summary[f"robustness_degradation_{w}"] = self.compute_robustness_degradation_ratio(
                    clean, weather_metrics[w].get("mean_iou", 0.0))
        degs = [summary[k] for k in (f"robustness_degradation_{w}" for w in ("fog", "rain", "snow", "night")) if k in summary]
        if degs:
            summary["robustness_degradation_ratio"] = np.mean(degs)
        eces = [m.get("expected_calibration_error", 0.0) for m in weather_metrics.values()]
        if eces:
            summary["expected_calibration_error"] = np.mean(eces)
        aur = [m.get("ensemble_disagreement_auroc", 0.5) for m in weather_metrics.values()]
        if aur:
            summary["ensemble_disagreement_auroc"] = np.mean(aur)
        return summary
