"""`evaluate_model` — the evaluation hot loop of REF/scripts/evaluate.py:134-274, same arguments
and result keys, with every per-pixel quantity kept on the GPU.

Reference: forward -> argmax -> `.cpu()` of predictions, labels, the FULL logits and both member
logits per batch, `torch.cat` on the host (9.5 GB for 20 frames at 1024x2048), then metrics
once at the end.  Here each batch updates additive device counters and nothing else survives it:

  * confusion  int64[1+K, C*C]   slot 0 overall, slot 1+k weather condition k  (HIP, fused with
                                  combine / temperature / argmax)
  * ECE bins   [1+K, 15] x {count, sum conf, sum correct}                      (HIP)
  * AUROC      int64[2, 2^13] histogram of the disagreement score by error/non-error

Counters are SUM-all-reduced over ranks once (RCCL), then rank-agnostic host math finishes:
the 19-element IoU divide/mean uses the reference's own torch expressions, so identical counts
give bit-identical mIoU at any GPU count.
"""
from __future__ import annotations

import logging
from typing import Any, Dict

import numpy as np
import os

import torch
import torch.nn.functional as F

from .. import _native as N
from .. import ops, parallel
from ..data.loader import resolve_severities, slot_name
from .metrics import (ConfidenceCalibration, ConfusionAccumulator, RobustnessMetrics, bootstrap_metrics_from_replicates,
                      boundary_metrics_from_stats, calibration_from_stats, change_metrics_from_stats, deocclude_metrics_from_stats, estimate_metrics_from_stats,
                      depth_metrics_from_stats,
                      failure_metrics_from_stats, iou_from_counts, guided_metrics_from_stats, quality_metrics_from_stats,
                      relight_metrics_from_stats, restoration_metrics_from_stats, restored_quality_metrics_from_stats,
                      segment_metrics_from_stats, segment_options, severity_sweep_results, tta_metrics_from_stats,
                      weight_grid_metrics_from_stats)

logger = logging.getLogger(__name__)

AUROC_BINS = 1 << 13                      # per-block LDS histogram (2 x 8192 x 4 B = 64 KB)
AUROC_LO, AUROC_HI = -1e-3, 0.70          # mutual information of two members lies in [0, ln 2]
# The device AUROC is the rank statistic of a 2^13-bin histogram of the disagreement score (ties inside a bin count half), not
# sklearn's exact ranks (metrics.py:434): asserted within AUROC_TOLERANCE of sklearn end to end (tests/test_gpu_models.py) —
# 30x looser than every other gate of the path, so the results dict says how the number was made.
AUROC_TOLERANCE = 3e-3


def _cfg(config, key, default):
    try:
        v = config.get(key, default)
    except Exception:  # noqa: BLE001
        v = default
    return default if v is None else v


def _flag(config, key) -> bool:
    on = _cfg(config, key, False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"{key} is true or false, got {on!r}")
    return bool(on)


def _needs_sweep(config, key, why) -> None:
    if _cfg(config, "evaluation.severities", None) is None:
        raise ValueError(f"{key} needs a severity sweep (evaluation.severities): without one {why}")


def check_frames(option, images) -> None:
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise ValueError(f"evaluation.{option}: the frames are float32 [B, 3, H, W], got {images.dtype} {tuple(images.shape)}")


def _check_budget(count: int, budget: int, what: str) -> None:
    """The fixed-point counters are int64 sums of per-term values (include/awseg.h): raise before they could wrap.  `what`: the
    counters and the unit `budget` is in."""
    if count > budget:
        raise OverflowError(f"{what.format(budget)} (summed over ranks); {count} would exceed that")


def _warn_wrapped_index(opt, labels, num_classes: int, text: str) -> None:
    """Once per run: uint8 labels make the pooled confusion counters reproduce the reference's wrapped index, `opt`'s never wrap."""
    if labels.dtype == torch.uint8 and num_classes * (num_classes - 1) > 255 and not opt.get("warned"):
        opt["warned"] = True
        logger.warning(text, num_classes)


def temperature_grid(spec):
    """`evaluation.temperature_grid`: a list of temperatures, or {min, max, steps} = torch.linspace(min, max, steps) in float32
    (the reference's grid is {min: 0.1, max: 10.0, steps: 100}).  None / absent: calibration off."""
    if spec is None:
        return None
    if isinstance(spec, dict):
        return torch.linspace(float(spec["min"]), float(spec["max"]), int(spec["steps"])).numpy()
    return ops.calib_temperatures(list(spec))


def check_calibration_budget(pixels: int) -> None:
    """The NLL counters are int64 sums of per-pixel values up to 2^31."""
    _check_budget(pixels, ops.CALIB_PIXEL_BUDGET, "temperature calibration counters hold {} pixels")


def depth_options(config):
    """`evaluation.depth_metrics` (bool, default off), `evaluation.depth_min` (finite, > 0, default 1e-3: the target is a [0, 1] map
    that can touch 0, so the relative errors need a floor) and `evaluation.depth_target` ('frame': the loader's target, estimated
    from the frame as rendered; 'clean': under a severity sweep every variant is scored against its clean frame's target).
    -> None when off, else {'min': float, 'target': str}."""
    on = _flag(config, "evaluation.depth_metrics")
    target = _cfg(config, "evaluation.depth_target", "frame")
    if target not in ("frame", "clean"):
        raise ValueError(f"evaluation.depth_target is 'frame' or 'clean', got {target!r}")
    md = _cfg(config, "evaluation.depth_min", 1e-3)
    if isinstance(md, (bool, str)) or not isinstance(md, (int, float, np.floating, np.integer)) or not (np.isfinite(md) and md > 0):
        raise ValueError(f"evaluation.depth_min must be a finite number > 0, got {md!r}")
    if not on:
        return None
    if target == "clean":
        _needs_sweep(config, "evaluation.depth_target: clean", "a frame has no clean counterpart")
    return {"min": float(md), "target": str(target)}


def failure_option(config) -> bool:
    """`evaluation.failure_detection` (bool, default off): per-condition failure-detection counters (AUROC / AURC of four
    uncertainty scores against the prediction's errors)."""
    return _flag(config, "evaluation.failure_detection")


def boundary_option(config):
    """`evaluation.boundary_widths` (default off): 1 .. 4 strictly increasing integer band widths within [1, 16] for the
    boundary-band counters (trimap mIoU / Boundary IoU per condition).  -> None when absent, else the list."""
    spec = _cfg(config, "evaluation.boundary_widths", None)
    if spec is None:
        return None
    try:
        if isinstance(spec, (bool, str, bytes, dict, int, float, np.number, np.bool_)):
            raise ValueError("not a list")
        return [int(d) for d in ops.boundary_widths(list(spec))]
    except (ValueError, TypeError) as e:
        raise ValueError(f"evaluation.boundary_widths is a list of 1 .. {ops.BOUNDARY_MAX_WIDTHS} strictly increasing integers within "
                         f"[1, {ops.BOUNDARY_MAX_RADIUS}], got {spec!r} ({e})") from None


def segment_option(config):
    """`evaluation.segment_metrics` (bool, default off): segment-level counters (which label segments the prediction finds, loses and
    invents per condition).  `evaluation.segment_threshold`: the share of a segment that must be covered, one of
    0.25 / 0.5 / 0.75 / 1.0 (default 0.5); `evaluation.segment_min_area`: the smallest segment counted, a power of 4 in [1, 4^10]
    (default 16); both checked also when the option is off.  -> None when off, else {'threshold': float, 'min_area': int}."""
    on = _flag(config, "evaluation.segment_metrics")
    threshold = _cfg(config, "evaluation.segment_threshold", 0.5)
    min_area = _cfg(config, "evaluation.segment_min_area", 16)
    try:
        segment_options(threshold, min_area)
    except ValueError as e:
        raise ValueError(f"evaluation.segment_threshold / evaluation.segment_min_area: {e}") from None
    if not on:
        return None
    return {"threshold": float(threshold), "min_area": int(min_area)}


WEIGHT_GRID_MAX_SHARES = ops.WGRID_MAX_POINTS - 1        # the model's own pair is always the last point


def weight_grid_shares(spec):
    """The SegFormer shares of `evaluation.ensemble_weight_grid`: an integer n in [2, 63] = n equally spaced shares k / (n - 1), or
    a list of 1 .. 63 strictly increasing numbers in [0, 1]; 0 and 1 are added when missing (within the 63).  -> list of floats."""
    what = (f"evaluation.ensemble_weight_grid is an integer in [2, {WEIGHT_GRID_MAX_SHARES}] (equally spaced SegFormer shares) or a "
            f"list of 1 .. {WEIGHT_GRID_MAX_SHARES} strictly increasing shares in [0, 1] (0 and 1 are added when missing, within "
            f"the {WEIGHT_GRID_MAX_SHARES}), got {spec!r}")
    if isinstance(spec, (bool, np.bool_, str, bytes, dict, float, np.floating)):
        raise ValueError(what)
    if isinstance(spec, (int, np.integer)):
        n = int(spec)
        if not 2 <= n <= WEIGHT_GRID_MAX_SHARES:
            raise ValueError(what)
        return [k / (n - 1) for k in range(n)]
    try:
        shares = list(spec)
    except TypeError:
        raise ValueError(what) from None
    if not shares or any(isinstance(a, (bool, np.bool_, str, bytes)) or not isinstance(a, (int, float, np.integer, np.floating))
                         or not 0.0 <= float(a) <= 1.0 for a in shares):                  # (a NaN fails the comparison)
        raise ValueError(what)
    shares = [float(a) for a in shares]
    if any(b <= a for a, b in zip(shares, shares[1:])):
        raise ValueError(what)
    shares = ([0.0] if shares[0] != 0.0 else []) + shares + ([1.0] if shares[-1] != 1.0 else [])
    if len(shares) > WEIGHT_GRID_MAX_SHARES:
        raise ValueError(what)
    return shares


def weight_grid_pairs(shares, configured) -> np.ndarray:
    """float32 [len(shares) + 1, 2]: (float32(a), float32(1) - float32(a)) per share, then the model's own pair `configured`."""
    a = np.asarray(shares, dtype=np.float32)
    own = np.asarray(configured, dtype=np.float32).reshape(1, 2)
    return np.ascontiguousarray(np.concatenate([np.stack([a, np.float32(1) - a], axis=1), own], axis=0))


def weight_grid_option(config, model=None):
    """`evaluation.ensemble_weight_grid` (default off): the ensemble weight sweep -- the mIoU of every condition at
    every member weighting of a grid (weight_grid_shares) plus the model's own softmax(ensemble_weights) as the last point, and how
    the members' own predictions split the labelled pixels.  `evaluation.weight_grid_condition` (default 'clean'): the evaluated
    condition the fitted weighting is chosen on.  `model`, when given, must be the two-member ensemble combining by
    weighted_average; its pair closes the grid.  -> None when off, else {'shares', 'condition'} and, with a model, 'pairs' (float32
    [G, 2]) and 'configured_index' (G - 1)."""
    spec = _cfg(config, "evaluation.ensemble_weight_grid", None)
    condition = _cfg(config, "evaluation.weight_grid_condition", "clean")
    if not isinstance(condition, str) or not condition:
        raise ValueError(f"evaluation.weight_grid_condition is the name of an evaluated condition, got {condition!r}")
    if spec is None:
        return None
    opt = {"shares": weight_grid_shares(spec), "condition": condition}
    sweep = _cfg(config, "evaluation.severities", None) is not None
    evaluated = list(_cfg(config, "data.weather_conditions", []))
    if not sweep and condition not in evaluated:
        raise ValueError(f"evaluation.weight_grid_condition {condition!r} is not among the evaluated conditions {evaluated} "
                         "(data.weather_conditions)")
    if model is not None:
        if not (hasattr(model, "segformer") and hasattr(model, "deeplabv3plus") and hasattr(model, "ensemble_weights")):
            raise ValueError("evaluation.ensemble_weight_grid sweeps the weights of the SegFormer + DeepLabV3+ ensemble: the model is "
                             f"a {type(model).__name__}, which has no two members to weigh")
        strategy = getattr(model, "ensemble_strategy", "weighted_average")
        if strategy != "weighted_average":
            raise ValueError("evaluation.ensemble_weight_grid sweeps the weights of model.ensemble_strategy weighted_average; the "
                             f"model combines by {strategy!r}")
        own = F.softmax(model.ensemble_weights.detach().float(), dim=0).cpu().numpy()     # the pair the forward pass combines with
        opt["pairs"] = weight_grid_pairs(opt["shares"], own)
        opt["configured_index"] = len(opt["shares"])
    return opt


def change_option(config, images=None):
    """`evaluation.change_strata` (default off): the edges of the change strata, a list of 1 .. 7 strictly increasing finite numbers
    >= 0 in 8-bit grey levels of the loader's normalisation, or 'default' = [0.5, 4.5, 16.5, 64.5].  The errors of
    every corrupted frame are then split by how much the corruption changed each input pixel against the clean frame, so the option
    needs a severity sweep (evaluation.severities).  `images`, when given, is a batch of frames: they must be float32 [B, 3, H, W].
    -> None when absent, else the list of edges."""
    spec = _cfg(config, "evaluation.change_strata", None)
    if spec is None:
        return None
    try:
        edges = [float(v) for v in ops.change_edges(spec)]
    except (ValueError, TypeError) as e:
        raise ValueError(f"evaluation.change_strata is 'default' or a list of 1 .. {ops.MAX_STRATA - 1} strictly increasing finite "
                         f"numbers >= 0, got {spec!r} ({e})") from None
    _needs_sweep(config, "evaluation.change_strata", "a corrupted frame has no clean twin to measure the change against")
    if images is not None:
        check_frames("change_strata", images)
    return edges


IQ_DEFAULT_TARGETS = (0.9, 0.75, 0.5)
IQ_MAX_TARGETS = 8


def quality_options(config, images=None):
    """`evaluation.image_quality` (bool, default off): PSNR and SSIM (with its luminance and contrast-structure factors) of every
    corrupted frame against its clean frame, and the mIoU of every kind at equal SSIM; needs a severity sweep
    (evaluation.severities).  `evaluation.image_quality_targets`: the SSIM values the mIoU is interpolated at, a list of 1 .. 8
    numbers in (0, 1), default [0.9, 0.75, 0.5]; checked also when the option is off.  `images`, when given, is a batch of frames:
    they must be float32 [B, 3, H, W].  -> None when off, else {'targets': [...]}."""
    on = _flag(config, "evaluation.image_quality")
    spec = _cfg(config, "evaluation.image_quality_targets", list(IQ_DEFAULT_TARGETS))
    bad = isinstance(spec, (bool, str, bytes, dict, int, float, np.number, np.bool_))
    try:
        targets = [] if bad else list(spec)
    except TypeError:
        bad, targets = True, []
    if bad or not 1 <= len(targets) <= IQ_MAX_TARGETS or any(
            isinstance(t, (bool, np.bool_, str, bytes)) or not isinstance(t, (int, float, np.integer, np.floating))
            or not 0.0 < float(t) < 1.0 for t in targets):
        raise ValueError(f"evaluation.image_quality_targets is a list of 1 .. {IQ_MAX_TARGETS} numbers in (0, 1), got {spec!r}")
    if not on:
        return None
    _needs_sweep(config, "evaluation.image_quality", "a corrupted frame has no clean twin to measure the image quality against")
    if images is not None:
        check_frames("image_quality", images)
    return {"targets": [float(t) for t in targets]}


def check_quality_budget(terms: int) -> None:
    """The image-quality counters are int64 sums of per-term values up to 2^26."""
    _check_budget(terms, ops.IQ_TERM_BUDGET, "image-quality counters hold {} pixel-channels")


# `evaluation.restoration`: one entry per method, in the order of the routes, of the refusals and of the result keys.  'keys': its
# config keys (`radius` is the dark channel's and the top-hat's and belongs to the method named); 'maps': the keys given by name
# and what the names stand for (the first is the default); 'parameters': ops' check of them; 'new_stats': what makes its counters;
# 'attr': the EvalState attribute they live in; 'run': (images, counters..., cond, **parameters) -> (restored frames, ...);
# 'metrics': counters -> result keys (None: the dehazer's go through restoration_metrics_from_stats with the second confusion).
RESTORATION = {
    "dark_channel": {                                                  # awseg_dehaze, DESIGN.md 10n: also what no `method` means
        "keys": ("radius", "omega", "t_min", "airlight_min", "refine"), "maps": {"refine": {"opening": 1, "none": 0}},
        "parameters": ops.dehaze_parameters, "new_stats": ops.new_dehaze_stats, "attr": "restoration", "run": ops.dehaze, "metrics": None},
    "clahe": {                                                         # awseg_relight, DESIGN.md 10o
        "keys": ("grid", "clip_limit", "max_gain", "white_balance"), "maps": {"white_balance": {"gray_world": True, "none": False}},
        "parameters": ops.relight_parameters, "new_stats": ops.new_relight_stats, "attr": "restoration_relight", "run": ops.relight,
        "metrics": relight_metrics_from_stats},
    "tophat": {                                                        # awseg_deocclude, DESIGN.md 10p
        "keys": ("radius", "threshold", "bright_min", "dilate"), "maps": {},
        "parameters": ops.deocclude_parameters, "new_stats": ops.new_deocclude_stats, "attr": "restoration_deocclude",
        "run": ops.deocclude, "metrics": deocclude_metrics_from_stats},
}
# the dark channel under refine: guided (awseg_dehaze_guided): what runs in its place, the filter's counters
# beside the dehazer's
RESTORATION_GUIDED = {"keys": ("radius", "omega", "t_min", "airlight_min", "guided_radius", "guided_eps"),
                      "parameters": ops.dehaze_guided_parameters, "new_stats": ops.new_guided_stats, "attr": "restoration_guided",
                      "run": ops.dehaze_guided, "metrics": guided_metrics_from_stats}
RESTORATION_METHODS = tuple(RESTORATION)
RESTORATION_KEYS = RESTORATION["dark_channel"]["keys"]
RESTORATION_REFINE = RESTORATION["dark_channel"]["maps"]["refine"]
RESTORATION_GUIDED_KEYS = RESTORATION_GUIDED["keys"][4:]               # only under refine: guided
RESTORATION_RELIGHT_KEYS = RESTORATION["clahe"]["keys"]
RESTORATION_WHITE_BALANCE = RESTORATION["clahe"]["maps"]["white_balance"]
RESTORATION_DEOCCLUDE_KEYS = RESTORATION["tophat"]["keys"]
# under method: auto (awseg_weather_estimate) the three methods above are chosen per frame: the keys of that level,
# the keys of `estimator`, and the route a rule that knew the weather would take (names outside the map: none)
RESTORATION_AUTO_KEYS = ("route", "estimator") + RESTORATION_METHODS
RESTORATION_ROUTES = ("estimated", "oracle")
RESTORATION_ESTIMATOR_KEYS = tuple(ops.ESTIMATE_DEFAULTS)


def _method_keys(method: str) -> tuple:
    """Every config key of a method."""
    return RESTORATION[method]["keys"] + (RESTORATION_GUIDED_KEYS if method == "dark_channel" else ())



def _method_option(method: str, spec) -> dict:
    """`evaluation.restoration` under one method of the table (without 'method') -> the checked option, without 'conditions'."""
    entry, own = RESTORATION[method], set(_method_keys(method))
    for other in RESTORATION if isinstance(spec, dict) else ():
        foreign = sorted(set(spec) & (set(_method_keys(other)) - own))
        if foreign:
            raise ValueError(f"evaluation.restoration: {foreign} belong to method: {other}, got method: {method}")
    if not isinstance(spec, dict) or set(spec) - own:
        if method != "dark_channel":
            raise ValueError(f"evaluation.restoration with method: {method} is a dict with keys among {list(entry['keys'])}, got {spec!r}")
        raise ValueError(f"evaluation.restoration is 'dark_channel', 'clahe', 'tophat' or a dict with keys among "
                         f"{list(_method_keys(method))} (method: clahe: {list(RESTORATION_RELIGHT_KEYS)}; method: "
                         f"tophat: {list(RESTORATION_DEOCCLUDE_KEYS)}), got {spec!r}")
    kw = dict(spec)
    for key, values in entry["maps"].items():
        names = list(values) + ["guided"] * (key == "refine")
        given = kw.get(key, names[0])
        if not isinstance(given, str) or given not in names:
            raise ValueError(f"evaluation.restoration.{key} is {', '.join(map(repr, names[:-1]))} or {names[-1]!r}, got {given!r}")
        if key in kw and given in values:
            kw[key] = values[given]
    guided = kw.get("refine") == "guided"
    if not guided and set(kw) & set(RESTORATION_GUIDED_KEYS):
        raise ValueError(f"evaluation.restoration: {sorted(set(kw) & set(RESTORATION_GUIDED_KEYS))} belong to refine: guided, got "
                         f"refine: {spec.get('refine', 'opening')}")
    try:
        if guided:
            opt = {**RESTORATION_GUIDED["parameters"](**{k: v for k, v in kw.items() if k != "refine"}), "refine": "guided"}
        else:
            opt = entry["parameters"](**kw)
    except ValueError as e:
        raise ValueError(f"evaluation.restoration: {e}") from None
    return opt if method == "dark_channel" else {"method": method, **opt}      # no `method`, no 'method' key


def _auto_option(spec: dict) -> dict:
    """The dict of `evaluation.restoration` under method: auto (without 'method') -> the checked option, without 'conditions':
    {'method': 'auto', 'route', 'estimator', 'dark_channel', 'clahe', 'tophat'}, the last three what restoration_option gives for
    that method alone (without 'conditions')."""
    levels = {**{method: _method_keys(method) for method in RESTORATION}, "estimator": RESTORATION_ESTIMATOR_KEYS}
    for key in sorted(set(spec) - set(RESTORATION_AUTO_KEYS)):
        homes = [name for name, keys in levels.items() if key in keys]
        if homes:
            raise ValueError(f"evaluation.restoration: {key!r} belongs under {' or '.join(repr(h) for h in homes)} with method: auto, "
                             "not beside them")
        raise ValueError(f"evaluation.restoration with method: auto is a dict with keys among {list(RESTORATION_AUTO_KEYS)}, got {spec!r}")
    route = spec.get("route", "estimated")
    if not isinstance(route, str) or route not in RESTORATION_ROUTES:
        raise ValueError(f"evaluation.restoration.route is 'estimated' or 'oracle', got {route!r}")
    opt = {"method": "auto", "route": route}
    est = spec.get("estimator", {})
    if not isinstance(est, dict) or set(est) - set(RESTORATION_ESTIMATOR_KEYS):
        raise ValueError(f"evaluation.restoration.estimator is a dict with keys among {list(RESTORATION_ESTIMATOR_KEYS)}, got {est!r}")
    try:
        opt["estimator"] = ops.weather_estimate_parameters(**est)
    except ValueError as e:
        raise ValueError(f"evaluation.restoration.estimator: {e}") from None
    for method in RESTORATION_METHODS:
        sub = spec.get(method, {})
        if not isinstance(sub, dict) or set(sub) & ({"method"} | set(RESTORATION_AUTO_KEYS)):
            raise ValueError(f"evaluation.restoration.{method} is a dict of that method's parameters, got {sub!r}")
        if method == "dark_channel" and sub.get("refine") == "guided":
            raise ValueError("evaluation.restoration.dark_channel: refine: guided is not available under method: auto")
        try:
            one = restoration_option({"evaluation.restoration": {"method": method, **sub}})
        except ValueError as e:
            raise ValueError(str(e).replace("evaluation.restoration", f"evaluation.restoration.{method}", 1)) from None
        opt[method] = {k: v for k, v in one.items() if k not in ("method", "conditions")}
    return opt


def restoration_option(config, images=None):
    """`evaluation.restoration` (default off): 'dark_channel', or a dict with any of `radius` (an integer in [1, 15], default 7),
    `omega`, `t_min`, `airlight_min` (numbers in (0, 1], defaults 0.95, 0.1, 0.1) and `refine` ('opening', the default, 'none', or
    'guided': the guided-filter refinement of DESIGN.md 10n-bis, which alone takes `guided_radius`, an integer in [1, 32], default
    min(4 radius, 32), and `guided_eps`, a number in [1e-4, 1], default 1e-3):
    every selected frame is dehazed by the dark-channel prior and scored a second time.
    `evaluation.restoration_conditions`: the weather conditions whose frames are restored, a list of names; absent: all of them,
    'clean' included (a blind front-end does not know the weather); checked also when the option is off.  `images`, when given, is
    a batch of frames: they must be float32 [B, 3, H, W].
    Or 'clahe', or a dict with `method: clahe` and any of `grid` (n or [tiles_y, tiles_x], integers in [1, 16], default 8),
    `clip_limit`, `max_gain` (numbers in [1, 64], defaults 2 and 8) and `white_balance` ('gray_world', the default, or 'none'):
    every selected frame is relit by CLAHE on the luma with a grey-world white balance instead.
    Or 'tophat', or a dict with `method: tophat` and any of `radius` (an integer in [1, 15], default 9), `threshold` (a number in
    (0, 1], default 0.06), `bright_min` (a number in [0, 1], default 0.5) and `dilate` (an integer in [0, 2], default 1): the bright
    occluders of rain and snow are masked by the white top-hat and filled from their neighbours instead.  `method:
    dark_channel` means what the absence of `method` means; the keys of one method are refused under another (`radius` belongs to
    the method named).
    -> None when absent, else {'radius', 'omega', 't_min', 'airlight_min', 'refine' (0 / 1), 'conditions' (a list, or None = all)};
    under 'guided': {'radius', 'omega', 't_min', 'airlight_min', 'guided_radius', 'guided_eps', 'refine': 'guided', 'conditions'};
    under 'clahe': {'method': 'clahe', 'grid' (ty, tx), 'clip_limit', 'max_gain', 'white_balance' (a bool), 'conditions'};
    under 'tophat': {'method': 'tophat', 'radius', 'threshold', 'bright_min', 'dilate', 'conditions'}.  Only the last two carry a
    'method' key, and 'auto':
    'auto', or a dict with `method: auto` and any of `route` ('estimated', the default: every selected frame goes to the method the
    weather estimate of DESIGN.md 10q names for it, or to none; 'oracle': to the method ops.ESTIMATE_EXPECTED_ROUTE names for its true
    condition, the upper bound), `estimator` (a dict of the estimate's parameters: `radius`, `threshold`, `bright_min`, `cast_max`, `luma_max`,
    `dark_min`, `seed_min`; ops.ESTIMATE_DEFAULTS) and `dark_channel`, `clahe`, `tophat` (each a dict of that method's parameters as
    above, its defaults when absent; `refine: guided` is refused).  A key of one level is refused at another.
    -> {'method': 'auto', 'route', 'estimator', 'dark_channel', 'clahe', 'tophat', 'conditions'}."""
    names = _cfg(config, "evaluation.restoration_conditions", None)
    if names is not None:
        if isinstance(names, (str, bytes, dict)) or not isinstance(names, (list, tuple)) or not names \
                or any(not isinstance(n, str) or not n for n in names):
            raise ValueError(f"evaluation.restoration_conditions is a non-empty list of condition names, got {names!r}")
        names = [str(n) for n in names]
    spec = _cfg(config, "evaluation.restoration", None)
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec not in RESTORATION_METHODS and spec != "auto":
            raise ValueError(f"evaluation.restoration is 'dark_channel', 'clahe', 'tophat', 'auto' or a dict of a method's parameters, "
                             f"got {spec!r}")
        spec = {"method": spec}
    method = RESTORATION_METHODS[0]
    if isinstance(spec, dict) and "method" in spec:
        method = spec["method"]
        if not isinstance(method, str) or (method not in RESTORATION_METHODS and method != "auto"):
            raise ValueError(f"evaluation.restoration.method is 'dark_channel', 'clahe', 'tophat' or 'auto', got {method!r}")
        spec = {k: v for k, v in spec.items() if k != "method"}
    opt = _auto_option(spec) if method == "auto" else _method_option(method, spec)
    if images is not None:
        check_frames("restoration", images)
    opt["conditions"] = names
    return opt


TTA_PRESETS = {"flip": {"scales": [1.0], "flip": True}, "ms_flip": {"scales": [0.5, 0.75, 1.0, 1.25, 1.5], "flip": True}}
TTA_KEYS = ("scales", "flip")
TTA_MAX_SCALES = 8
TTA_SCALE_RANGE = (0.25, 2.0)
TTA_GRID = 32                                  # a rescaled view's sides are multiples of this, at least two of them


def tta_option(config):
    """`evaluation.tta` (default off): test-time augmentation -- the members' logits averaged over mirrored and
    rescaled views of every frame, scored a second time.  'flip': scales [1.0] with the mirrored view; 'ms_flip': scales 0.5, 0.75,
    1.0, 1.25, 1.5, each also mirrored; or a dict with `scales` (1 .. 8 strictly increasing numbers in [0.25, 2]; 1.0 is added when
    absent; default [1.0]) and `flip` (true or false, default true).  Any other key is refused by name.
    -> None when absent, else {'scales': [...], 'flip': bool}."""
    spec = _cfg(config, "evaluation.tta", None)
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec not in TTA_PRESETS:
            raise ValueError(f"evaluation.tta is {', '.join(map(repr, TTA_PRESETS))} or a dict with keys among {list(TTA_KEYS)}, got {spec!r}")
        spec = TTA_PRESETS[spec]
    if not isinstance(spec, dict):
        raise ValueError(f"evaluation.tta is {', '.join(map(repr, TTA_PRESETS))} or a dict with keys among {list(TTA_KEYS)}, got {spec!r}")
    unknown = sorted(str(k) for k in set(spec) - set(TTA_KEYS))
    if unknown:
        raise ValueError(f"evaluation.tta: unknown key{'s' if unknown[1:] else ''} {', '.join(map(repr, unknown))}; the keys are "
                         f"{list(TTA_KEYS)}")
    flip = spec.get("flip", True)
    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError(f"evaluation.tta.flip is true or false, got {flip!r}")
    scales = spec.get("scales", [1.0])
    lo, hi = TTA_SCALE_RANGE
    what = (f"evaluation.tta.scales is a list of 1 .. {TTA_MAX_SCALES} strictly increasing numbers in [{lo}, {hi}] (1.0 is added when "
            f"absent), got {scales!r}")
    if isinstance(scales, (bool, np.bool_, str, bytes, dict, int, float, np.number)):
        raise ValueError(what)
    try:
        scales = list(scales)
    except TypeError:
        raise ValueError(what) from None
    if not 1 <= len(scales) <= TTA_MAX_SCALES or any(
            isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating))
            or not lo <= float(v) <= hi for v in scales):                                  # (a NaN fails the comparison)
        raise ValueError(what)
    scales = [float(v) for v in scales]
    if any(b <= a for a, b in zip(scales, scales[1:])):
        raise ValueError(what)
    if 1.0 not in scales:
        scales = sorted(scales + [1.0])
    if len(scales) == 1 and not flip:
        raise ValueError("evaluation.tta: scales [1.0] without flip is the plain forward alone: nothing to average")
    return {"scales": scales, "flip": bool(flip)}


def tta_views(option) -> list:
    """The extra views of an option in the order they run, [(scale, flip)]: ascending scale, unflipped before flipped.  View 0, the
    plain forward (scale 1, no flip), is not among them: there are 1 + len(...) views in all."""
    return [(s, f) for s in option["scales"] for f in ((False, True) if option["flip"] else (False,)) if not (s == 1.0 and not f)]


def tta_view_size(height: int, width: int, scale: float) -> tuple:
    """The size of a view: the frame's own at scale 1, else both sides 32 max(2, floor(side scale / 32 + 0.5))."""
    if scale == 1.0:
        return int(height), int(width)
    return tuple(TTA_GRID * max(2, int(np.floor(side * scale / TTA_GRID + 0.5))) for side in (int(height), int(width)))


def tta_view_sizes(option, height: int, width: int) -> list:
    """[(scale, flip, (h, w))] of the extra views for frames of height x width.  Two scales that give one size are refused."""
    by_size = {}
    for s in option["scales"]:
        size = tta_view_size(height, width, s)
        if size in by_size:
            raise ValueError(f"evaluation.tta: scales {by_size[size]} and {s} both give views of {size[0]} x {size[1]} pixels from "
                             f"frames of {height} x {width}")
        by_size[size] = s
    return [(s, f, tta_view_size(height, width, s)) for s, f in tta_views(option)]


BOOTSTRAP_MAX_REPLICATES = 65536


def bootstrap_options(config, num_sources=None):
    """`evaluation.bootstrap_replicates` (default absent = off: an integer in [1, 65536]), `evaluation.bootstrap_confidence` (a
    float in (0, 1), default 0.95) and `evaluation.bootstrap_seed` (an integer in [0, 2^63), default 0): the paired frame bootstrap
    of the per-condition mIoU.  -> None when off, else {'replicates', 'confidence', 'seed', 'sources'} with
    'sources' = num_sources (the number of source frames of the evaluation set: the resampling unit)."""
    def integer(key, v, lo, hi):
        if isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"evaluation.{key} is an integer in [{lo}, {hi}], got {v!r}")
        return int(v)
    conf = _cfg(config, "evaluation.bootstrap_confidence", 0.95)
    if isinstance(conf, (bool, np.bool_, str, bytes)) or not isinstance(conf, (int, float, np.floating, np.integer)) \
            or not 0.0 < float(conf) < 1.0:
        raise ValueError(f"evaluation.bootstrap_confidence is a number in (0, 1), got {conf!r}")
    seed = integer("bootstrap_seed", _cfg(config, "evaluation.bootstrap_seed", 0), 0, 2 ** 63 - 1)
    reps = _cfg(config, "evaluation.bootstrap_replicates", None)
    if reps is None:
        return None
    reps = integer("bootstrap_replicates", reps, 1, BOOTSTRAP_MAX_REPLICATES)
    if num_sources is not None and (isinstance(num_sources, bool) or not isinstance(num_sources, (int, np.integer)) or num_sources < 1):
        raise ValueError(f"the frame bootstrap resamples the source frames of a sized dataset, got {num_sources!r} of them")
    return {"replicates": reps, "confidence": float(conf), "seed": seed, "sources": None if num_sources is None else int(num_sources)}


def bootstrap_resampling_set(table: torch.Tensor, seen: torch.Tensor, slot: torch.Tensor, oob: torch.Tensor):
    """The summed tables of the frame bootstrap (EvalState.bootstrap, after the all-reduce) -> (table [n, V, 3 C], slots int32
    [n, V], the n kept source indices): the sources of which no frame came (drop_last, a short shard) leave the resampling set, the
    rest are compacted where they are.  ValueError when a (source, variant) came more than once (its row would hold two frames and
    its slot entry a sum), IndexError when the per-frame pass met a value outside the classes."""
    twice = (seen > 1).any(dim=1).nonzero()
    if twice.numel():
        raise ValueError(f"source {int(twice[0, 0])}: a frame came more than once; the frame bootstrap needs every "
                         "(source, variant) at most once")
    if int(oob.item()):
        raise IndexError("prediction map or label value outside [0, num_classes) in the per-frame counters")
    keep = (seen.sum(dim=1) > 0).nonzero().view(-1)
    if keep.numel() == 0:
        raise ValueError("the frame bootstrap saw no frame")
    return table.index_select(0, keep), slot.index_select(0, keep).to(torch.int32), keep


def check_depth_budget(pixels: int) -> None:
    """The depth counters are int64 sums of per-pixel terms up to 2^31."""
    _check_budget(pixels, ops.DEPTH_PIXEL_BUDGET, "depth error counters hold {} pixels")


# The optional counters of EvalState in the order they join the all-reduce (the same on every rank).  Per option: the attribute that
# holds its dict (None when off), the keys whose tensors are summed, the host count that travels behind them with the check of its
# budget on the SUMMED count, and what finalize raises when the summed 'oob' word is not zero (the bootstrap's is checked where its
# tables are read: bootstrap_resampling_set).
COUNTERS = (
    ("calib", ("stats",), "pixels", check_calibration_budget, None),
    ("depth", ("stats",), "pixels", check_depth_budget, None),
    ("failure", ("stats",), None, None, None),
    ("boundary", ("stats", "oob"), None, None, "prediction map value outside [0, num_classes) in the boundary counters"),
    ("change", ("stats", "oob"), None, None, "prediction map value outside [0, num_classes), or a clean-frame row outside the buffer, "
                                             "in the change-strata counters"),
    ("quality", ("stats", "oob"), "terms", check_quality_budget, "a clean-frame row outside the buffer in the image-quality counters"),
    ("segments", ("stats", "oob"), None, None, "prediction map value outside [0, num_classes) in the segment counters"),
    ("weight_grid", ("stats",), None, None, None),
    ("restoration", ("counts", "oob", "stats"), None, None, "label outside [0, num_classes) in the confusion counters of the restored frames"),
    ("restoration_guided", ("stats",), None, None, None),
    ("restoration_relight", ("stats",), None, None, None),
    ("restoration_deocclude", ("stats",), None, None, None),
    ("restoration_estimate", ("stats",), None, None, None),
    ("restored_quality", ("stats", "oob"), "terms", check_quality_budget, "a clean-frame row outside the buffer in the image-quality "
                                                                          "counters of the restored frames"),
    ("tta", ("counts", "oob", "stats"), None, None, "label or prediction map value outside [0, num_classes) in the counters of the "
                                                    "test-time augmentation"),
    ("bootstrap", ("table", "seen", "slot", "oob"), None, None, None),     # ranks fill disjoint rows: the sum is the union
    ("paired", ("stats", "oob", "sources"), None, None, "prediction map value outside [0, num_classes) in the consistency counters"),
)


def _grown(buf, numel: int, device):
    """A flat uint8 buffer of at least numel elements: `buf` when it is large enough (grow-only, contents not kept)."""
    return buf if buf is not None and buf.numel() >= numel else torch.empty(numel, dtype=torch.uint8, device=device)


def _keep_rows(store, n_rows: int, data, idx, fill: bool):
    """store['rows']: float32 [rows, width] of per-source clean data at the row indices of the clean prediction maps, grown to their
    n_rows with the old rows kept.  `data` [B, ...] is this batch's, `idx` (EvalState.frame_ref) its sources' rows: a clean batch
    (fill) leaves its data there.  -> the buffer."""
    rows, width = store["rows"], data[0].numel()
    if rows is not None and rows.shape[1] != width:
        raise ValueError("every frame of a severity sweep must have the same size")
    if rows is None or rows.shape[0] < n_rows:
        store["rows"] = torch.empty(n_rows, width, dtype=torch.float32, device=data.device)
        if rows is not None:
            store["rows"][:rows.shape[0]].copy_(rows)
        rows = store["rows"]
    if fill:
        rows.index_copy_(0, idx.long(), data.reshape(data.shape[0], width))
    return rows


class EvalState:
    """All cross-batch state of one evaluation run (device resident, additive)."""

    def __init__(self, metrics: RobustnessMetrics, conditions, device, num_bins: int = 15, ensemble: bool = False, *,
                 temperature_grid=None, calibration_condition: str = "clean", sweep=None, depth=None, failure: bool = False,
                 boundary=None, bootstrap=None, change=None, quality=None, segments=None, weight_grid=None, restoration=None,
                 tta=None):
        # paired severity sweep (data.loader.SeveritySweep): the condition slots are 'clean' and '<kind>_s<j>' instead of the
        # weather conditions; every counter below uses that one slot list
        self.sweep = sweep
        if sweep is not None:
            conditions = sweep.slots()
        self.acc = metrics.new_accumulator(device)
        self.acc.conditions = list(conditions)
        self.acc.counts = ops.new_counts(metrics.num_classes, device, 1 + len(conditions))
        self.ece = ops.new_ece_bins(num_bins, device, 1 + len(conditions))
        self.edges = torch.linspace(0, 1, num_bins + 1).to(device)
        self.auroc = torch.zeros(2, AUROC_BINS, dtype=torch.int64, device=device) if ensemble else None
        self.samples = 0
        # the uint8 prediction map of the batch in flight, for whichever counters read one (pred_map); clean maps of a sweep are kept
        # in self.paired instead
        self.pred_scratch = None
        # streamed temperature calibration (off unless a grid is given): NLL + ECE bins per (slot, grid temperature)
        self.calib = None
        if temperature_grid is not None:
            temps = ops.calib_temperatures(temperature_grid)
            self.calib = {"temps": temps, "condition": calibration_condition, "pixels": 0,
                          "stats": ops.new_temperature_grid_stats(len(temps), num_bins, device, 1 + len(conditions))}
        # depth error sums (off unless depth = depth_options(config)): int64 [slot, series, AWSEG_DEPTH_ROW]
        self.depth = None
        if depth is not None:
            if depth["target"] == "clean" and sweep is None:
                raise ValueError("depth_target 'clean' needs a severity sweep")
            # 'rows': under depth_target 'clean', the clean frames' targets (_keep_rows)
            self.depth = {"stats": ops.new_depth_eval_stats(device, 1 + len(conditions)), "min": float(depth["min"]),
                          "target": depth["target"], "pixels": 0, "rows": None}
        # failure-detection counters (off unless failure = failure_option(config)): int64 [slot, AWSEG_FAIL_ROW] over this run's slots
        self.failure = None
        if failure:
            self.failure = {"stats": ops.new_failure_stats(device, 1 + len(conditions)), "conditions": list(conditions),
                            "single": not ensemble}
        # boundary-band counters (off unless boundary = boundary_option(config)): int64 [slot, ring, C*C + 2 C]
        self.boundary = None
        if boundary is not None:
            widths = [int(d) for d in ops.boundary_widths(boundary)]
            self.boundary = {"widths": widths, "stats": ops.new_boundary_stats(metrics.num_classes, len(widths), device, 1 + len(conditions)),
                             "oob": torch.zeros(1, dtype=torch.int64, device=device)}
        # frame bootstrap (off unless bootstrap = bootstrap_options(config, num_sources)): per-frame IoU counters int64
        # [source, variant, 3 C], how often each (source, variant) came, and 1 + its condition slot; variant 0 is the only one
        # without a sweep, under a sweep variant = the frame's slot index (0 clean, 1 + k S + j - 1 for kind k at level j)
        self.bootstrap = None
        if bootstrap is not None:
            if bootstrap.get("sources") is None:
                raise ValueError("the frame bootstrap needs the number of source frames (a loader with a sized dataset)")
            n_src, variants = int(bootstrap["sources"]), len(conditions) if sweep is not None else 1
            self.bootstrap = {"replicates": int(bootstrap["replicates"]), "confidence": float(bootstrap["confidence"]),
                              "seed": int(bootstrap["seed"]), "sources": n_src, "variants": variants,
                              "table": ops.new_frame_counts(n_src * variants, metrics.num_classes, device).view(n_src, variants, -1),
                              "seen": torch.zeros(n_src, variants, dtype=torch.int64, device=device),
                              "slot": torch.zeros(n_src, variants, dtype=torch.int64, device=device),
                              "oob": torch.zeros(1, dtype=torch.int64, device=device)}
        # the clean frames as the model saw them (kept when the change strata or the image-quality counters are on): 'rows' of 3 hw,
        # filled once per clean batch (keep_clean_frames, _keep_rows)
        self.clean_frames = None
        # change strata (off unless change = change_option(config)): int64 [slot, stratum, C*C + 6] over the sweep's slots.  'rows':
        # the buffer of self.clean_frames; 'scratch': the uint8 stratum map of a variant batch (live next to its prediction map)
        self.change = None
        if change is not None:
            if sweep is None:
                raise ValueError("change strata need a severity sweep")
            edges = ops.change_edges(change)
            self.change = {"edges": [float(v) for v in edges],
                           "stats": ops.new_strata_stats(metrics.num_classes, len(edges) + 1, device, 1 + len(conditions)),
                           "oob": torch.zeros(1, dtype=torch.int64, device=device), "rows": None, "scratch": None}
            self.clean_frames = {"rows": None}
        # image-quality counters (off unless quality = quality_options(config)): int64 [slot, AWSEG_IQ_ROW] over the sweep's slots;
        # 'terms': the pixel-channels counted so far, against the fixed-point budget of the sums
        self.quality = None
        if quality is not None:
            if sweep is None:
                raise ValueError("image-quality counters need a severity sweep")
            self.quality = {"targets": [float(t) for t in quality["targets"]], "terms": 0,
                            "stats": ops.new_image_quality_stats(device, 1 + len(conditions)),
                            "oob": torch.zeros(1, dtype=torch.int64, device=device)}
            self.clean_frames = {"rows": None}
        # segment-level counters (off unless segments = segment_option(config)): int64 [slot, C, 11, 48].  Under a sweep the clean
        # maps of self.paired are the references
        self.segments = None
        if segments is not None:
            segment_options(segments["threshold"], segments["min_area"])
            self.segments = {"threshold": float(segments["threshold"]), "min_area": int(segments["min_area"]),
                             "stats": ops.new_segment_stats(metrics.num_classes, device, 1 + len(conditions)),
                             "oob": torch.zeros(1, dtype=torch.int64, device=device)}
        # ensemble weight sweep (off unless weight_grid = weight_grid_option(config, model)): int64 [slot, G + 3, 2 C]
        self.weight_grid = None
        if weight_grid is not None:
            if not ensemble or weight_grid.get("pairs") is None:
                raise ValueError("the ensemble weight sweep needs the two-member ensemble (weight_grid_option(config, model))")
            if weight_grid["condition"] not in conditions:              # (under a sweep: its slots, known only here)
                raise ValueError(f"evaluation.weight_grid_condition {weight_grid['condition']!r} is not among the evaluated conditions "
                                 f"{list(conditions)}")
            pairs = ops.check_weight_grid(weight_grid["pairs"])
            self.weight_grid = {"pairs": pairs, "configured_index": int(weight_grid["configured_index"]),
                                "condition": weight_grid["condition"],
                                "stats": ops.new_weight_grid_stats(1 + len(conditions), pairs.shape[0], metrics.num_classes, device)}
        # restored frames (off unless restoration = restoration_option(config)): a SECOND confusion accumulator over this run's slots
        # for the forward on the dehazed frames, and the dehazing counters int64 [slot, AWSEG_DEHAZE_ROW].  'conditions': the weather
        # conditions whose frames are restored (None: all); 'oob' is the second accumulator's
        # Every entry of RESTORATION keeps its counters, int64 [slot, row], in its own attribute ({'stats'}, None while it does not
        # run): `restoration` the dehazer's (AWSEG_DEHAZE_ROW), `restoration_guided` the filter's under refine: guided,
        # `restoration_relight` and `restoration_deocclude` those of method: clahe and method: tophat, whose frames go through the
        # dehazer's second pass all the same; their masks and gains are not kept.  Without dehazing counters `restoration['stats']`
        # has no rows (the reduce and the result keys see nothing).  Under method: auto all three methods' counters
        # are allocated and each sees the frames routed to it
        for entry in (*RESTORATION.values(), RESTORATION_GUIDED):
            setattr(self, entry["attr"], None)
        self.restoration_estimate = None
        self._restoration_method = None if restoration is None else restoration.get("method", RESTORATION_METHODS[0])
        if restoration is not None:
            auto, slots = self._restoration_method == "auto", 1 + len(conditions)
            options = {m: restoration[m] for m in RESTORATION} if auto else {self._restoration_method: restoration}
            params = {}
            for method, opt in options.items():
                entries = [RESTORATION[method]] + [RESTORATION_GUIDED] * (opt.get("refine") == "guided")      # the last runs
                params[method] = entries[-1]["parameters"](**{k: opt[k] for k in entries[-1]["keys"]})
                for entry in entries:
                    setattr(self, entry["attr"], {"stats": entry["new_stats"](device, slots)})
            acc = ConfusionAccumulator(metrics.num_classes, list(conditions), device)
            own = self.restoration or {"stats": torch.zeros(0, ops.DEHAZE_ROW, dtype=torch.int64, device=device)}
            self.restoration = {"params": None if auto else params[self._restoration_method], "acc": acc, "counts": acc.counts,
                                "oob": acc.oob, "stats": own["stats"],
                                "conditions": None if restoration.get("conditions") is None else {str(c) for c in restoration["conditions"]}}
            # the counters of the weather estimate, int64 [slot, AWSEG_ESTIMATE_ROW], see every selected frame.  'route': 'estimated'
            # or 'oracle'; 'params': the estimator's and each method's; 'host', 'event': the pinned buffer the routes are copied to and
            # the event behind that copy (estimated only); 'pending': the estimate of the batch in flight; 'readbacks': how many
            # batches' routes the host has waited for
            if auto:
                self.restoration_estimate = {"stats": ops.new_estimate_stats(device, slots), "route": restoration["route"],
                                             "params": {"estimator": ops.weather_estimate_parameters(**restoration["estimator"]), **params},
                                             "host": None, "event": None, "pending": None, "readbacks": 0}
        # fidelity of the restored frames (only when the sweep, the image-quality counters and the restoration are all on): a SECOND
        # image-quality tensor, the restored frames against the same kept clean frames; the clean batch against its own kept rows
        self.restored_quality = None
        if restoration is not None and self.quality is not None:
            self.restored_quality = {"terms": 0, "stats": ops.new_image_quality_stats(device, 1 + len(conditions)),
                                     "oob": torch.zeros(1, dtype=torch.int64, device=device)}
        # test-time augmentation (off unless tta = tta_option(config)): a SECOND confusion accumulator over this run's
        # slots for the view-averaged logits ('oob' is its word, and the consistency pass's), the consistency counters of the averaged
        # prediction against the plain one (ops.new_consistency_stats), and one more uint8 prediction map ('pred', grow-only).
        # 'sizes': the views of the frame size seen last
        self.tta = None
        if tta is not None:
            acc = ConfusionAccumulator(metrics.num_classes, list(conditions), device)
            self.tta = {"scales": [float(v) for v in tta["scales"]], "flip": bool(tta["flip"]), "views": 1 + len(tta_views(tta)),
                        "acc": acc, "counts": acc.counts, "oob": acc.oob,
                        "stats": ops.new_consistency_stats(metrics.num_classes, device, 1 + len(conditions)), "pred": None, "sizes": None}
        self.paired = None
        if sweep is not None:
            # clean prediction maps, one uint8 row per source whose clean frame has been seen and whose K x S variants have not all
            # been counted yet; rows are reused once a source is done
            self.paired = {"stats": ops.new_consistency_stats(metrics.num_classes, device, 1 + len(conditions)),
                           "oob": torch.zeros(1, dtype=torch.int64, device=device), "rows": None, "free": [], "live": {},
                           "done": set(), "variants": len(sweep.kinds) * sweep.levels,
                           "sources": torch.zeros(1, dtype=torch.int64, device=device)}

    def _ref_rows(self, n: int, shape, device):
        """n consecutive free rows of the clean-map buffer (grown when no run of n is free): the clean batch writes its maps there
        directly."""
        pd = self.paired
        hw = int(np.prod(shape))
        if pd["rows"] is not None and pd["rows"].shape[1] != hw:
            raise ValueError("every frame of a severity sweep must have the same size")
        free = sorted(pd["free"])
        for i in range(len(free) - n + 1):
            if free[i + n - 1] - free[i] == n - 1:
                run = free[i:i + n]
                pd["free"] = [r for r in pd["free"] if r not in run]
                return run[0]
        old = 0 if pd["rows"] is None else pd["rows"].shape[0]
        new = torch.empty(max(2 * old, old + n), hw, dtype=torch.uint8, device=device)
        if old:
            new[:old].copy_(pd["rows"])
        pd["free"] += list(range(old, new.shape[0]))
        pd["rows"] = new
        return self._ref_rows(n, shape, device)

    def paired_pred_out(self, sources, severity, shape, device):
        """Where this batch's prediction map goes: clean frames straight into fresh rows of the clean-map buffer, variants into
        scratch.  Checks the order: a variant needs its source's clean frame first, and a clean frame comes once."""
        pd, n = self.paired, len(sources)
        if severity == 0:
            for s in sources:
                if s in pd["live"] or s in pd["done"]:
                    raise ValueError(f"source {s}: its clean frame came twice")
            r0 = self._ref_rows(n, shape, device)
            for i, s in enumerate(sources):
                pd["live"][s] = [r0 + i, pd["variants"]]
            return pd["rows"][r0:r0 + n].view((n,) + tuple(shape))
        for s in sources:
            if s not in pd["live"]:
                raise ValueError(f"source {s}: a corrupted frame came before its clean frame" if s not in pd["done"] else
                                 f"source {s}: more corrupted frames than the sweep's {pd['variants']}")
        return self.pred_map((n,) + tuple(shape), device)

    def pred_map(self, shape, device):
        """The reused uint8 [B, H, W] map the statistics pass writes this batch's prediction into, for every counter that reads it."""
        numel = int(np.prod(shape))
        self.pred_scratch = _grown(self.pred_scratch, numel, device)
        return self.pred_scratch[:numel].view(tuple(shape))

    def frame_ref(self, sources, severity, device):
        """The rows of this batch's sources in the clean-map buffer (and in every row store kept in step with it) as an int32
        device tensor: made once per batch, after paired_pred_out, for every update that reads those rows.  None on a clean batch
        with no row store to fill: nothing reads them."""
        if severity == 0 and self.clean_frames is None and (self.depth is None or self.depth["target"] != "clean"):
            return None
        rows = [self.paired["live"][s][0] for s in sources]
        return torch.tensor(rows, dtype=torch.int32).to(device, non_blocking=True)

    def update_segments(self, pred, labels, frame_ref, cond, num_classes: int) -> None:
        """Segment counters of this batch; a variant batch of a sweep (frame_ref: its sources' rows) is also counted against their
        clean maps (the rows the paired pass keeps: no map of its own).  Runs before update_consistency releases the rows."""
        sg = self.segments
        ref_maps = None if frame_ref is None else self.paired["rows"].view((-1,) + tuple(pred.shape[1:]))
        ops.segment_stats(pred, labels.reshape(pred.shape), num_classes, sg["stats"], sg["oob"], cond, ref_maps=ref_maps,
                          frame_ref=frame_ref)

    def update_bootstrap(self, pred, labels, sources, cond_ids, num_classes: int) -> None:
        """Per-frame IoU counters of this batch into rows (source, variant); cond_ids: the host list cond was made from."""
        bs = self.bootstrap
        if any(c < 0 for c in cond_ids):
            raise ValueError("the frame bootstrap needs every frame's condition among the counter slots "
                             f"{self.acc.conditions} (data.weather_conditions)")
        bad = [s for s in sources if not 0 <= s < bs["sources"]]
        if bad:
            raise ValueError(f"source {bad[0]} is outside the evaluation set's {bs['sources']} source frames")
        _warn_wrapped_index(bs, labels, num_classes,
                            "frame bootstrap: with uint8 labels and %d classes the pooled confusion counters reproduce the reference's "
                            "wrapped index, the per-frame counters never wrap: the intervals describe the unwrapped mIoU and need not "
                            "contain the pooled point estimates (DESIGN.md 10g)")
        v = bs["variants"]
        rows = [s * v + (c if v > 1 else 0) for s, c in zip(sources, cond_ids)]
        # one host-to-device copy: the rows, and 1 + slot of each
        host = torch.tensor([rows, [1 + c for c in cond_ids]], dtype=torch.int64).to(pred.device, non_blocking=True)
        ops.frame_iou_counts(pred, labels, num_classes, host[0].to(torch.int32), bs["table"], bs["oob"])
        bs["seen"].view(-1).index_add_(0, host[0], torch.ones_like(host[0]))
        bs["slot"].view(-1).index_add_(0, host[0], host[1])           # a frame that comes twice is caught by 'seen' after the reduce

    def bootstrap_replicates(self):
        """After all_reduce: check the tables, drop the sources no rank saw, resample.  -> (int64 [R, slots, 3 C] on the host,
        number of sources resampled)."""
        bs = self.bootstrap
        table, slots, keep = bootstrap_resampling_set(bs["table"], bs["seen"], bs["slot"], bs["oob"])
        oob = torch.zeros(1, dtype=torch.int64, device=table.device)
        rep = ops.bootstrap_counts(table, slots, 1 + len(self.acc.conditions), bs["seed"], bs["replicates"], oob)
        if int(oob.item()):
            raise IndexError("slot outside the counter slots in the frame bootstrap's slot table")
        return rep.cpu().numpy(), int(keep.numel())

    def keep_clean_frames(self, images, frame_ref, severity) -> None:
        """The clean-frame buffer in step with the clean-map buffer; a clean batch (after paired_pred_out gave its sources their
        rows) leaves its frames there.  Once per batch, for the change strata and the image-quality counters alike."""
        rows = _keep_rows(self.clean_frames, self.paired["rows"].shape[0], images, frame_ref, severity == 0)
        if self.change is not None:
            self.change["rows"] = rows

    def update_quality(self, images, rows, cond) -> None:
        """A variant batch's image-quality counters against its sources' clean frames (rows: frame_ref's tensor, or the list it is
        made from).  Raises before the fixed-point budget of the sums would be exceeded."""
        q = self.quality
        check_quality_budget(q["terms"] + images.numel())
        q["terms"] += images.numel()
        if not torch.is_tensor(rows):
            rows = torch.tensor(rows, dtype=torch.int32).to(images.device, non_blocking=True)
        twins = self.clean_frames["rows"].view((-1,) + tuple(images.shape[1:]))
        ops.image_quality(images, twins, rows, q["stats"], cond=cond, oob=q["oob"])

    def check_relight_grid(self, images) -> None:
        """Under method: clahe a tile is never empty: the grid may not have more tiles than the frames have rows or columns."""
        if self.restoration_relight is not None and images.dim() == 4:
            auto = self.restoration_estimate
            ty, tx = (self.restoration["params"] if auto is None else auto["params"]["clahe"])["grid"]
            if ty > images.shape[2] or tx > images.shape[3]:
                raise ValueError(f"evaluation.restoration: a grid of {ty} x {tx} tiles does not fit frames of {images.shape[2]} x "
                                 f"{images.shape[3]} pixels")

    def _selected(self, kinds):
        """The batch's frames of the selected weather conditions: their indices."""
        rs = self.restoration
        return [i for i, k in enumerate(kinds) if rs["conditions"] is None or str(k) in rs["conditions"]]

    def begin_estimate(self, images, kinds, cond) -> None:
        """Under method: auto, at the top of the batch and before its forward is enqueued: the weather estimate of the selected
        frames into its counters.  With route: estimated the routes start on their way to a pinned host buffer and an event is
        recorded behind the copy; update_restoration waits for that event, after the plain forward has been enqueued, so the host
        waits for the estimator and not for the forward.  With route: oracle nothing is read back."""
        es = self.restoration_estimate
        check_frames("restoration", images)
        keep = self._selected(kinds)
        es["pending"] = None
        if not keep:
            return
        if len(keep) < images.shape[0]:
            idx = torch.tensor(keep, dtype=torch.int64).to(images.device, non_blocking=True)
            images, cond = images.index_select(0, idx), cond.index_select(0, idx)
        route, _ = ops.weather_estimate(images, es["stats"], cond, **es["params"]["estimator"])
        es["pending"] = {"frames": len(keep)}
        if es["route"] == "estimated":
            if es["host"] is None or es["host"].numel() < len(keep):
                es["host"] = torch.empty(len(keep), dtype=torch.int32).pin_memory()
                es["event"] = torch.cuda.Event()
            es["host"][:len(keep)].copy_(route, non_blocking=True)
            es["event"].record()

    def _routes(self, kinds) -> list:
        """The route (an index into ops.ESTIMATE_ROUTES) of every selected frame of the batch in flight: the estimate's, read back
        here (the one host synchronisation the option adds: on the estimator's event), or under route: oracle the one
        ops.ESTIMATE_EXPECTED_ROUTE names for the frame's true condition."""
        es = self.restoration_estimate
        pending, es["pending"] = es["pending"], None
        if pending is None or pending["frames"] != len(kinds):
            raise ValueError("evaluation.restoration: method: auto needs the batch's weather estimate (begin_estimate) before its routes")
        if es["route"] == "oracle":
            return [ops.ESTIMATE_ROUTES.index(ops.ESTIMATE_EXPECTED_ROUTE.get(str(k), "none")) for k in kinds]
        es["event"].synchronize()
        es["readbacks"] += 1
        return [int(r) for r in es["host"][:len(kinds)].tolist()]

    def _restore(self, method, images, cond, params):
        """The frames through one method of the table (the guided dehazer where its counters are allocated) into its counters."""
        entries = [RESTORATION[method]] + [RESTORATION_GUIDED] * (method == "dark_channel" and self.restoration_guided is not None)
        return entries[-1]["run"](images, *(getattr(self, e["attr"])["stats"] for e in entries), cond, **params)[0]

    def _restore_by_route(self, images, cond, routes):
        """The frames grouped by route, each group through its method into that method's own counters, written back into one batch;
        the frames routed to none are copied as they are."""
        es, n = self.restoration_estimate, images.shape[0]
        run = lambda name, x, c: self._restore(name, x, c, es["params"][name])      # noqa: E731
        restored = None
        for r, name in enumerate(ops.ESTIMATE_ROUTES):
            members = [i for i, v in enumerate(routes) if v == r]
            if not members:
                continue
            if len(members) == n:                                     # the whole batch takes one route
                return images if name == "none" else run(name, images, cond)
            if restored is None:
                restored = torch.empty_like(images)
            idx = torch.tensor(members, dtype=torch.int64).to(images.device, non_blocking=True)
            group = images.index_select(0, idx)
            restored.index_copy_(0, idx, group if name == "none" else run(name, group, cond.index_select(0, idx)))
        return restored

    def update_restoration(self, model, images, labels, kinds, cond, rows=None) -> None:
        """The batch's frames of the selected weather conditions (`kinds`: the loader's names, before a sweep's slot names), dehazed,
        through one more forward into the second confusion accumulator.  Nothing else sees the restored frames, but the second
        image-quality tensor when it is on (`rows`: frame_ref's rows of the batch's sources in the kept clean frames)."""
        rs = self.restoration
        check_frames("restoration", images)
        keep = self._selected(kinds)
        if not keep:
            return
        if len(keep) < images.shape[0]:
            idx = torch.tensor(keep, dtype=torch.int64).to(images.device, non_blocking=True)
            images, labels, cond = images.index_select(0, idx), labels.index_select(0, idx), cond.index_select(0, idx)
            if rows is not None:
                rows = rows.index_select(0, idx) if torch.is_tensor(rows) else [rows[i] for i in keep]
        self.check_relight_grid(images)
        if self.restoration_estimate is not None:
            restored = self._restore_by_route(images, cond, self._routes([kinds[i] for i in keep]))
        else:
            restored = self._restore(self._restoration_method, images, cond, rs["params"])
        if self.restored_quality is not None:
            # (the rows a last variant batch has just released still hold their frames: nothing writes them before the next batch)
            rq = self.restored_quality
            check_quality_budget(rq["terms"] + restored.numel())
            rq["terms"] += restored.numel()
            if not torch.is_tensor(rows):
                rows = torch.tensor(rows, dtype=torch.int32).to(images.device, non_blocking=True)
            twins = self.clean_frames["rows"].view((-1,) + tuple(images.shape[1:]))
            ops.image_quality(restored, twins, rows, rq["stats"], cond=cond, oob=rq["oob"])
        if self.auroc is not None:                                    # the ensemble
            model.forward_eval(restored, labels, rs["counts"], rs["oob"], cond, want_logits=False, want_pred=False, stats=None)
        else:
            logits = model(restored)["segmentation"].float().contiguous()
            ops.combine_argmax_confusion(logits, None, 3, want_logits=False, label=labels.contiguous(), counts=rs["counts"],
                                         oob=rs["oob"], cond=cond)

    def update_tta(self, model, images, labels, cond, members, plain_pred, num_classes: int) -> None:
        """Test-time augmentation of this batch.  `members`: the plain forward's member logits (one map for a single
        model), fresh tensors nothing reads any more: they are the accumulators, the first extra view folded in with
        TTA_SCALE_ADD and the others with TTA_ADD, every view weighing float32(1) / float32(views).  The averaged logits go through
        the model's own combine into the second accumulator and the TTA prediction map, which is counted against `plain_pred`."""
        t = self.tta
        check_frames("tta", images)
        h, w = int(images.shape[2]), int(images.shape[3])
        if t["sizes"] is None or t["sizes"][0] != (h, w):
            t["sizes"] = ((h, w), tta_view_sizes(t, h, w))
        weight = np.float32(1) / np.float32(t["views"])
        members = [m if m.is_contiguous() else m.contiguous() for m in members]
        images = images.contiguous()
        ensemble = len(members) == 2
        for i, (_, flip, size) in enumerate(t["sizes"][1]):
            view = ops.tta_view(images, size, flip)
            if ensemble:
                out = model.forward_eval(view, want_logits=False, want_pred=False, want_depth=False, combine=False)
                logits = [out["segformer_seg"], out["deeplabv3plus_seg"]]
            else:
                logits = [model(view)["segmentation"].float()]
            for l, acc in zip(logits, members):
                ops.tta_accumulate(l.contiguous(), acc, flip, weight, ops.TTA_SCALE_ADD if i == 0 else ops.TTA_ADD)
        t["pred"] = _grown(t["pred"], plain_pred.numel(), images.device)
        pred = t["pred"][:plain_pred.numel()].view(plain_pred.shape)
        if ensemble:
            mode, w_, T = model.combine_arguments()
            ops.combine_argmax_confusion(members[0], members[1], mode, w_, T, want_logits=False, label=labels.contiguous(),
                                         counts=t["counts"], oob=t["oob"], cond=cond, pred_out=pred)
        else:
            ops.combine_argmax_confusion(members[0], None, 3, want_logits=False, label=labels.contiguous(), counts=t["counts"],
                                         oob=t["oob"], cond=cond, pred_out=pred)
        rows = torch.arange(images.shape[0], dtype=torch.int32, device=images.device)
        ops.prediction_consistency(pred, plain_pred, rows, labels, num_classes, t["stats"], t["oob"], cond)

    def update_change(self, images, pred, labels, frame_ref, cond, num_classes: int) -> None:
        """A variant batch is split into change strata against its sources' clean frames and counted against their clean maps.
        Runs before update_consistency releases the rows."""
        ch = self.change
        _warn_wrapped_index(ch, labels, num_classes,
                            "change strata: with uint8 labels and %d classes the pooled confusion counters reproduce the reference's "
                            "wrapped index, the stratified counters never wrap: miou_*_chg<k> describes the unwrapped confusion matrix "
                            "and the strata need not recombine to the pooled mIoU (DESIGN.md 10h)")
        ch["scratch"] = _grown(ch["scratch"], pred.numel(), images.device)
        strata = ch["scratch"][:pred.numel()].view(pred.shape)
        ops.change_strata(images, ch["rows"], frame_ref, ch["edges"], out=strata, oob=ch["oob"])
        ops.stratified_stats(pred, labels, strata, len(ch["edges"]) + 1, num_classes, ch["stats"], ch["oob"],
                             ref_maps=self.paired["rows"], frame_ref=frame_ref, cond=cond)

    def update_consistency(self, pred, labels, sources, frame_ref, cond, num_classes: int) -> None:
        """Count a variant batch's maps against its sources' clean maps (slot 0 + its condition slot); free the rows of sources whose
        sweep is complete."""
        pd = self.paired
        ops.prediction_consistency(pred, pd["rows"], frame_ref, labels, num_classes, pd["stats"], pd["oob"], cond)
        for s in sources:
            ent = pd["live"][s]
            ent[1] -= 1
            if ent[1] == 0:
                del pd["live"][s]
                pd["free"].append(ent[0])
                pd["done"].add(s)

    def depth_target(self, target: torch.Tensor, frame_ref, severity) -> torch.Tensor:
        """The target this batch's depth maps are scored against, and the pixel budget check.  depth_target 'clean': a clean batch
        (after paired_pred_out gave its sources their rows: frame_ref) leaves its targets in those rows, a variant batch gathers its
        sources'."""
        d = self.depth
        if target.dim() != 3 or target.dtype != torch.float32:
            raise ValueError(f"the depth target is float32 [B, H, W], got {target.dtype} {tuple(target.shape)}")
        check_depth_budget(d["pixels"] + target.numel())
        d["pixels"] += target.numel()
        if d["target"] != "clean":
            return target
        rows = _keep_rows(d, self.paired["rows"].shape[0], target, frame_ref, severity == 0)
        return target if severity == 0 else rows.index_select(0, frame_ref.long()).view(target.shape)

    def update_calibration(self, labels: torch.Tensor, cond, logits=None, members=None) -> None:
        """Grid NLL / ECE of this batch: from the two member maps (members = (seg1, seg2, mode, weights, T)) or materialised
        logits.  Raises before the fixed-point pixel budget of the counters would be exceeded."""
        c = self.calib
        check_calibration_budget(c["pixels"] + labels.numel())
        c["pixels"] += labels.numel()
        if members is not None:
            s1, s2, mode, w, T = members
            ops.ensemble_temperature_grid_stats(s1, s2, mode, w, T, labels, c["stats"], c["temps"], self.edges, cond)
        else:
            ops.temperature_grid_stats(logits, labels, c["stats"], c["temps"], self.edges, cond)

    def update_weight_grid(self, labels: torch.Tensor, cond, members) -> None:
        """The weight sweep's counters of this batch from the two member maps (members = (seg1, seg2, ...) as update_calibration
        receives them): every grid point's mIoU counters and the members' own predictions in one pass."""
        wg = self.weight_grid
        ops.ensemble_weight_grid_stats(members[0], members[1], wg["pairs"], labels, cond, wg["stats"])

    def update_auroc(self, seg1, seg2, labels):
        """Disagreement = mutual information (metrics.py:353-367); error = argmax of the MEAN
        PROBABILITY != label (metrics.py:414-419); pixels with label 255 dropped (:426)."""
        p1, p2 = F.softmax(seg1, dim=1), F.softmax(seg2, dim=1)
        m = (p1 + p2) / 2
        h_mean = -(m * torch.log(m + 1e-8)).sum(dim=1)
        h_ind = (-(p1 * torch.log(p1 + 1e-8)).sum(dim=1) - (p2 * torch.log(p2 + 1e-8)).sum(dim=1)) / 2
        dis = (h_mean - h_ind).reshape(-1)
        lab = labels.reshape(-1).long()
        err = (m.argmax(dim=1).reshape(-1) != lab)
        valid = lab != 255
        b = ((dis - AUROC_LO) * (AUROC_BINS / (AUROC_HI - AUROC_LO))).long().clamp_(0, AUROC_BINS - 1)
        idx = b + err.long() * AUROC_BINS
        # no boolean indexing / bincount here: both would synchronise the host with the device every batch
        self.auroc.view(-1).index_add_(0, idx, valid.to(torch.int64))

    def all_reduce(self):
        """ONE SUM all-reduce of every counter — all int64 (confusion, ECE bins with fixed-point confidence sums, AUROC
        histogram): integer sums are order-independent, so the results are bit-identical at any rank count."""
        ts = [self.acc.counts, self.acc.oob, self.ece]
        if self.auroc is not None:
            ts.append(self.auroc)
        pd = self.paired
        if pd is not None:
            if pd["live"]:
                raise ValueError(f"severity sweep incomplete: {len(pd['live'])} source(s) lack corrupted frames, "
                                 f"e.g. source {min(pd['live'])}")
            pd["sources"].fill_(len(pd["done"]))
        summed = []
        for name, keys, count, check, _ in COUNTERS:
            opt = getattr(self, name)
            if opt is None:
                continue
            ts += [opt[k] for k in keys]
            if count is not None:
                # the ranks' counts travel in the same message: the budget is that of the SUMMED counters
                ts.append(torch.tensor([opt[count]], dtype=torch.int64, device=opt["stats"].device))
                summed.append((check, ts[-1]))
        parallel.all_reduce_sum_(ts)
        for check, total in summed:
            check(int(total.item()))

    def check_oob(self) -> None:
        """After all_reduce: raise when a counter pass met a value outside its range on any rank."""
        for name, _, _, _, message in COUNTERS:
            opt = getattr(self, name)
            if opt is not None and message is not None and int(opt["oob"].item()):
                raise IndexError(message)

    def auroc_value(self) -> float:
        neg, pos = self.auroc[0].double(), self.auroc[1].double()
        P, Nn = pos.sum().item(), neg.sum().item()
        if P == 0 or Nn == 0:
            return 0.5                                                             # metrics.py:430-431
        below = torch.cumsum(neg, 0) - neg
        return float((pos * (below + 0.5 * neg)).sum().item() / (P * Nn))


# confusion + calibration + disagreement statistics in one pass over the member logits (AWSEG_STATS_ONE_PASS=0: two passes)
STATS_ONE_PASS = os.environ.get("AWSEG_STATS_ONE_PASS", "1") != "0"


def _combine_args(model, strategy):
    """(mode, softmaxed weights, temperature) of r = combine(seg1, seg2)/T: one definition for every kernel that forms r from the
    member maps (calibration grid, ECE + disagreement, failure detection), so that they describe the same logits."""
    mode = N.COMBINE_WEIGHTED if strategy == "weighted_average" else N.COMBINE_MEAN
    w = F.softmax(model.ensemble_weights, dim=0) if mode == N.COMBINE_WEIGHTED else None
    T = model.temperature if getattr(model, "temperature_scaling", False) else None
    return mode, w, T


@torch.no_grad()
def eval_batch(model, st: EvalState, images: torch.Tensor, labels: torch.Tensor, conds, metrics: RobustnessMetrics,
               with_stats: bool = True, *, sources=None, severity=None, depth=None) -> None:
    """One batch of the evaluation loop (evaluate.py:166-200 + the per-batch share of :203-255): forward, argmax,
    confusion per condition, and (with_stats) the ECE bins and the disagreement histogram — all into `st`'s
    device counters.  Nothing per-pixel survives the call.
    Severity sweep (st.sweep): `sources` (global indices) and `severity` (0 clean, 1..S) of the batch; conds are its kinds.  The
    batch's prediction map is kept (clean) or compared with its sources' clean maps (variants).
    Depth metrics (st.depth): `depth` is the batch's target float32 [B, H, W]; the depth maps are scored in one pass and not kept."""
    pred_out = rows = None                                            # rows: st.frame_ref of a sweep's batch
    kinds = conds                                                     # the loader's names (a sweep renames conds to its slots)
    if st.sweep is not None:
        if sources is None or severity is None:
            raise ValueError("a severity sweep needs the paired loader's 'source' and 'severity' for every batch")
        severity = int(severity[0] if isinstance(severity, (list, tuple)) else severity)
        sources = [int(s) for s in sources]
        conds = [slot_name(c, severity) for c in conds]
        unknown = sorted({c for c in conds if c not in st.acc.conditions})
        if unknown:
            raise ValueError(f"batch conditions {unknown} are not slots of the severity sweep")
        pred_out = st.paired_pred_out(sources, severity, tuple(images.shape[2:]), images.device)
        rows = st.frame_ref(sources, severity, images.device)
    variant = st.sweep is not None and severity != 0
    if st.change is not None:
        check_frames("change_strata", images)
    if st.quality is not None:
        check_frames("image_quality", images)
    st.check_relight_grid(images)                                     # before the forward: the first batch is refused as it comes
    bd, bs, sg = st.boundary, st.bootstrap, st.segments
    if bs is not None:
        if sources is None:
            raise ValueError("the frame bootstrap needs the loader's 'source' (global sample indices) for every batch")
        sources = [int(s) for s in sources]
        if len(sources) != images.shape[0]:
            raise ValueError(f"{len(sources)} sources for a batch of {images.shape[0]} frames")
    if pred_out is None and (bd is not None or bs is not None or sg is not None or st.tta is not None):
        pred_out = st.pred_map((images.shape[0],) + tuple(images.shape[2:]), images.device)
    cond = st.acc.cond_ids(conds)
    depth_kw = {}
    if st.depth is not None:
        if depth is None:
            raise ValueError("evaluation.depth_metrics: the loader gives no depth target (batch['depth']; data.include_depth)")
        if not getattr(model, "include_depth", True):
            raise ValueError("evaluation.depth_metrics: the model has no depth head (model.include_depth)")
        depth = st.depth_target(depth, rows, severity)
        # the ensemble scores its three series in one pass and writes neither the upsampled nor the combined map
        depth_kw = {"depth_stats": (depth, cond, st.depth["stats"], st.depth["min"]), "want_depth": False}
    if labels.dtype not in (torch.uint8, torch.int64):
        labels = labels.long()
    if st.weight_grid is not None:                                    # before anything of the batch is counted
        if st.auroc is None:
            raise ValueError("the ensemble weight sweep needs the two-member ensemble")
        if getattr(model, "ensemble_strategy", "weighted_average") != "weighted_average":
            raise ValueError("the ensemble weight sweep needs model.ensemble_strategy weighted_average, got "
                             f"{model.ensemble_strategy!r}")
    if st.restoration_estimate is not None:                           # method: auto: the weather estimate, behind every check of the
        st.begin_estimate(images, kinds, cond)                        # batch and ahead of its forward
    if st.auroc is not None:
        strategy = getattr(model, "ensemble_strategy", "weighted_average")
        fused_stats = metrics.num_classes == 19 and strategy != "max_confidence" and images[0, 0].numel() % 4 == 0
        need_logits = (with_stats or st.calib is not None) and not fused_stats
        if st.failure is not None and strategy == "max_confidence":
            need_logits = True                                    # the msp row reads the combined logits: the kernel does not know the rule
        one_pass = (st.edges, st.ece, st.auroc, AUROC_LO, AUROC_HI) if (with_stats and fused_stats and STATS_ONE_PASS) else None
        res = model.forward_eval(images, labels, st.acc.counts, st.acc.oob, cond, want_logits=need_logits, want_pred=False, stats=one_pass,
                                 pred_out=pred_out, **depth_kw)
        if st.calib is not None:
            if fused_stats:                                       # grid statistics of combine(s1, s2)/T from the two member maps
                mode, w, T = _combine_args(model, strategy)
                st.update_calibration(labels, cond, members=(res["segformer_seg"], res["deeplabv3plus_seg"], mode, w, T))
            else:
                st.update_calibration(labels, cond, logits=res["segmentation"])
        if st.weight_grid is not None:                              # (its strategy was checked above)
            st.update_weight_grid(labels, cond, members=(res["segformer_seg"], res["deeplabv3plus_seg"]))
        if st.failure is not None:
            # max_confidence hands over its combined logits: the kernel does not know that rule
            mode, w, T = _combine_args(model, strategy)
            ops.ensemble_failure_stats(res["segformer_seg"], res["deeplabv3plus_seg"], mode, w, T, labels, st.failure["stats"], cond,
                                       combined=res["segmentation"] if strategy == "max_confidence" else None)
        if one_pass is not None and getattr(model, "_stats_fused", False):
            pass                                                  # confusion, ECE bins and the disagreement histogram came out of ONE pass
        elif with_stats and fused_stats:
            # ECE of the combined logits + disagreement histogram in ONE pass over the member logits:
            # the ensemble logits are never materialised
            mode, w, T = _combine_args(model, strategy)
            ops.ensemble_eval_stats(res["segformer_seg"], res["deeplabv3plus_seg"], mode, w, T, labels, cond, st.edges, st.ece,
                                    st.auroc, AUROC_LO, AUROC_HI)
        elif with_stats:
            st.update_auroc(res["segformer_seg"], res["deeplabv3plus_seg"], labels)
            ops.ece_accumulate(res["segmentation"], labels, st.ece, st.edges, cond)
    else:
        out = model(images)
        logits = out["segmentation"].float().contiguous()
        if st.depth is not None:
            if "depth" not in out:
                raise ValueError("evaluation.depth_metrics: the model has no depth head (no 'depth' in its output)")
            ops.depth_eval_stats(out["depth"].float(), None, None, depth, st.depth["stats"], st.depth["min"], cond)
        ops.combine_argmax_confusion(logits, None, 3, want_logits=False, label=labels.contiguous(), counts=st.acc.counts,
                                     oob=st.acc.oob, cond=cond, pred_out=pred_out)
        if with_stats:
            ops.ece_accumulate(logits, labels, st.ece, st.edges, cond)
        if st.calib is not None:
            st.update_calibration(labels, cond, logits=logits)
        if st.failure is not None:
            ops.failure_stats(logits, labels, st.failure["stats"], cond)
    if bd is not None:
        ops.boundary_stats(pred_out, labels.reshape(pred_out.shape), bd["widths"], metrics.num_classes, bd["stats"], bd["oob"], cond)
    if sg is not None:
        st.update_segments(pred_out, labels, rows if variant else None, cond, metrics.num_classes)
    if bs is not None:
        ids = [st.acc.conditions.index(str(c)) if str(c) in st.acc.conditions else -1 for c in conds]      # cond_ids' rule
        st.update_bootstrap(pred_out, labels, sources, ids, metrics.num_classes)
    if st.clean_frames is not None:
        st.keep_clean_frames(images, rows, severity)
    if variant:                                                       # against the clean frames and maps; the last one releases the rows
        if st.quality is not None:
            st.update_quality(images, rows, cond)
        if st.change is not None:
            st.update_change(images, pred_out, labels, rows, cond, metrics.num_classes)
        st.update_consistency(pred_out, labels, sources, rows, cond, metrics.num_classes)
    if st.restoration is not None:                                    # after everything above: one more forward, on the dehazed frames
        st.update_restoration(model, images, labels, kinds, cond, rows)
    if st.tta is not None:                                            # last: the plain member logits become the accumulators
        members = [res["segformer_seg"], res["deeplabv3plus_seg"]] if st.auroc is not None else [logits]
        st.update_tta(model, images, labels, cond, members, pred_out, metrics.num_classes)
    st.samples += images.size(0)


@torch.no_grad()
def evaluate_model(model: torch.nn.Module, test_loader, metrics: RobustnessMetrics, device, config) -> Dict[str, Any]:
    model.eval()
    conditions = list(_cfg(config, "data.weather_conditions", []))
    num_bins = int(_cfg(config, "evaluation.num_bins", 15))
    is_ensemble = hasattr(model, "segformer") and hasattr(model, "deeplabv3plus")
    spec = _cfg(config, "evaluation.severities", None)
    sweep = None
    if spec is not None:
        ds = getattr(test_loader, "dataset", None)
        rng = getattr(getattr(ds, "weather_transforms", None), "rng", "philox")
        sweep = resolve_severities(spec, conditions, rng)
    bootstrap = bootstrap_options(config)
    if bootstrap is not None:
        try:
            bootstrap["sources"] = len(test_loader.dataset)
        except (AttributeError, TypeError):
            raise ValueError("evaluation.bootstrap_replicates: the frame bootstrap resamples source frames and needs a loader with a "
                             "sized dataset (len(test_loader.dataset))") from None
    st = EvalState(metrics, conditions, device, num_bins, ensemble=is_ensemble,
                   temperature_grid=temperature_grid(_cfg(config, "evaluation.temperature_grid", None)),
                   calibration_condition=str(_cfg(config, "evaluation.calibration_condition", "clean")), sweep=sweep,
                   depth=depth_options(config), failure=failure_option(config),
                   boundary=boundary_option(config), bootstrap=bootstrap, change=change_option(config),
                   quality=quality_options(config), segments=segment_option(config),
                   weight_grid=weight_grid_option(config, model), restoration=restoration_option(config),
                   tta=tta_option(config))
    for batch in test_loader:
        images = batch["image"].to(device)
        labels = batch["label"].to(device)
        extra = {"sources": batch.get("source"), "severity": batch.get("severity")} if sweep is not None else {}
        if st.bootstrap is not None:
            extra["sources"] = batch.get("source")
        if st.depth is not None:
            extra["depth"] = None if batch.get("depth") is None else batch["depth"].to(device)
        eval_batch(model, st, images, labels, batch.get("weather_condition", ["clean"] * images.size(0)), metrics, **extra)
    return finalize(st, metrics)


def finalize(st: EvalState, metrics: RobustnessMetrics) -> Dict[str, Any]:
    """All-reduce the counters, then the scalar host math of evaluate.py:214-271."""
    st.all_reduce()
    st.acc.check()
    st.check_oob()
    sweep_kw = {"kinds": st.sweep.kinds if st.sweep is not None else None, "levels": st.sweep.levels if st.sweep is not None else 0}
    results: Dict[str, Any] = {"overall_miou": st.acc.miou(0)}
    weather_mious = {}
    for k, name in enumerate(st.acc.conditions):
        if st.acc.present(1 + k):
            weather_mious[name] = st.acc.miou(1 + k)
            results[f"miou_{name}"] = weather_mious[name]
    bins = ops.ece_bins_to_numpy(st.ece)
    results["expected_calibration_error"] = ConfidenceCalibration.ece_from_bins(bins[0])
    for k, name in enumerate(st.acc.conditions):
        if bins[1 + k]["count"].sum() > 0:
            results[f"ece_{name}"] = ConfidenceCalibration.ece_from_bins(bins[1 + k])
    if st.calib is not None:
        results.update(calibration_from_stats(ops.temperature_grid_stats_to_numpy(st.calib["stats"]), st.calib["temps"],
                                              st.acc.conditions, st.calib["condition"]))
    if st.auroc is not None:
        results["ensemble_disagreement_auroc"] = st.auroc_value()
        results["ensemble_disagreement_auroc_bins"] = float(AUROC_BINS)             # rank histogram, not exact ranks:
        results["ensemble_disagreement_auroc_tolerance"] = AUROC_TOLERANCE           # |device - sklearn| bound the tests assert
    if st.sweep is not None:
        # per kind: its severity slots summed (the counters are additive), so miou_<kind> / ece_<kind> / robustness_degradation_<kind>
        # keep their meaning over the kind's frames
        pd = st.paired
        slots = st.acc.conditions
        for kind in st.sweep.kinds:
            idx = [1 + slots.index(slot_name(kind, j)) for j in range(1, st.sweep.levels + 1)]
            cnt = st.acc.counts[idx].sum(0)
            if int(cnt.sum().item()) > 0:
                weather_mious[kind] = iou_from_counts(cnt, metrics.num_classes)["mean_iou"]
                results[f"miou_{kind}"] = weather_mious[kind]
            kb = bins[idx[0]].copy()
            for i in idx[1:]:
                for f in ("count", "sum_conf", "sum_correct"):
                    kb[f] += bins[i][f]
            if kb["count"].sum() > 0:
                results[f"ece_{kind}"] = ConfidenceCalibration.ece_from_bins(kb)
        results.update(severity_sweep_results(ops.consistency_stats_to_numpy(pd["stats"], metrics.num_classes), slots,
                                              st.sweep.kinds, st.sweep.levels, st.sweep.intensities, int(pd["sources"].item()),
                                              weather_mious, metrics.compute_robustness_degradation_ratio))
    if st.depth is not None:
        results.update(depth_metrics_from_stats(st.depth["stats"].cpu().numpy(), st.acc.conditions, **sweep_kw))
    if st.failure is not None:
        results.update(failure_metrics_from_stats(st.failure["stats"].cpu().numpy(), st.failure["conditions"], **sweep_kw,
                                                  single=st.failure["single"]))
    bd, sg, wg, ch, q, bs = st.boundary, st.segments, st.weight_grid, st.change, st.quality, st.bootstrap
    if bd is not None:
        results.update(boundary_metrics_from_stats(bd["stats"].cpu().numpy(), bd["widths"], st.acc.conditions, metrics.num_classes,
                                                   **sweep_kw, degradation=metrics.compute_robustness_degradation_ratio))
    if sg is not None:
        results.update(segment_metrics_from_stats(sg["stats"].cpu().numpy(), st.acc.conditions, metrics.num_classes,
                                                  threshold=sg["threshold"], min_area=sg["min_area"], **sweep_kw))
    if wg is not None:
        results.update(weight_grid_metrics_from_stats(wg["stats"].cpu().numpy(), st.acc.conditions, metrics.num_classes, wg["pairs"],
                                                      wg["configured_index"], calibration_condition=wg["condition"], **sweep_kw))
    if ch is not None:
        results.update(change_metrics_from_stats(ch["stats"].cpu().numpy(), ch["edges"], st.acc.conditions, st.sweep.kinds,
                                                 st.sweep.levels, metrics.num_classes))
    if q is not None:
        # after the sweep results: the matched-damage keys read miou_clean and miou_<kind>_s<j>
        results.update(quality_metrics_from_stats(q["stats"].cpu().numpy(), st.acc.conditions, st.sweep.kinds, st.sweep.levels, results,
                                                  q["targets"], metrics.compute_robustness_degradation_ratio))
    if st.restoration is not None:
        rs = st.restoration
        # without dehazing counters (method: clahe, method: tophat) all-zero rows give no dehazing key
        dehaze_stats = rs["stats"].cpu().numpy() if rs["stats"].shape[0] else np.zeros((1 + len(st.acc.conditions), ops.DEHAZE_ROW), np.int64)
        results.update(restoration_metrics_from_stats(rs["counts"].cpu().numpy(), st.acc.counts.cpu().numpy(), dehaze_stats,
                                                      st.acc.conditions, metrics.num_classes, **sweep_kw,
                                                      degradation=metrics.compute_robustness_degradation_ratio))
        for entry in (*RESTORATION.values(), RESTORATION_GUIDED):   # in the table's order: later keys overwrite earlier ones
            held = getattr(st, entry["attr"])
            if held is not None and entry["metrics"] is not None:
                results.update(entry["metrics"](held["stats"].cpu().numpy(), st.acc.conditions, **sweep_kw))
        if st.restoration_guided is not None:
            results["restoration_refine"] = "guided"
        if st.restoration_estimate is not None:                    # last: restoration_method and the non-finite count are the estimate's
            results.update(estimate_metrics_from_stats(st.restoration_estimate["stats"].cpu().numpy(), st.acc.conditions, **sweep_kw,
                                                       route=st.restoration_estimate["route"]))
        if st.restored_quality is not None:
            results.update(restored_quality_metrics_from_stats(st.restored_quality["stats"].cpu().numpy(), q["stats"].cpu().numpy(),
                                                               st.acc.conditions, st.sweep.kinds, st.sweep.levels))
    if st.tta is not None:
        t = st.tta
        results.update(tta_metrics_from_stats(t["counts"].cpu().numpy(), st.acc.counts.cpu().numpy(), t["stats"].cpu().numpy(),
                                              st.acc.conditions, metrics.num_classes, **sweep_kw,
                                              degradation=metrics.compute_robustness_degradation_ratio, views=t["views"],
                                              scales=t["scales"], flip=t["flip"]))
    if "clean" in weather_mious:
        for w in ("fog", "rain", "snow", "night"):
            if w in weather_mious:
                results[f"robustness_degradation_{w}"] = metrics.compute_robustness_degradation_ratio(
                    weather_mious["clean"], weather_mious[w])
        degs = [results[f"robustness_degradation_{w}"] for w in ("fog", "rain", "snow", "night")
                if f"robustness_degradation_{w}" in results]
        if degs:
            results["robustness_degradation_ratio"] = np.mean(degs)
    if bs is not None:
        # last: a quantity gets an interval when its point estimate is above.  The point estimates stay the pooled ones.
        rep, n_sources = st.bootstrap_replicates()
        results.update(bootstrap_metrics_from_replicates(rep, st.acc.conditions, metrics.num_classes, results, bs["confidence"],
                                                         bs["seed"], **sweep_kw, degradation=metrics.compute_robustness_degradation_ratio))
        results["bootstrap_sources"] = float(n_sources)
    return results
