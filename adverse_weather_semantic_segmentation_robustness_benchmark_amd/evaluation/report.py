"""Evaluation report files of REF/scripts/evaluate.py:277-392: the raw
`evaluation_results.json` and the markdown `evaluation_report.md` with the same sections, row
formats (three decimals) and pass marks, so downstream tooling that parses the reference's report
reads this one."""
from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Any, Dict, Optional

# target values the reference compares against when none are given (evaluate.py:303-311)
DEFAULT_TARGETS = {"miou_clean": 0.78, "miou_fog": 0.65, "miou_rain": 0.62, "robustness_degradation_ratio": 0.18,
                   "expected_calibration_error": 0.05, "ensemble_disagreement_auroc": 0.85}
ADVERSE = ("fog", "rain", "snow", "night")


def _ci(results: Dict[str, Any], key: str) -> str:
    """' [low, high]' of the frame bootstrap's percentile interval of `key`, or '' when the run had none."""
    if f"{key}_ci_low" not in results:
        return ""
    return f" [{results[f'{key}_ci_low']:.3f}, {results[f'{key}_ci_high']:.3f}]"


def report_markdown(results: Dict[str, Any], target_metrics: Optional[Dict[str, float]] = None) -> str:
    targets = DEFAULT_TARGETS if target_metrics is None else target_metrics
    lines = ["# Adverse Weather Semantic Segmentation Evaluation Report", "", "## Summary Metrics", "",
             "| Metric | Target | Actual | Status |", "|--------|--------|--------|--------|"]
    for name, want in targets.items():
        got = results.get(name, 0.0)
        lines.append(f"| {name} | {want:.3f} | {got:.3f} | {'✓' if got >= want else '✗'} |")    # `>=` for every row, :315
    lines += ["", "## Weather-Specific Performance", ""]
    lines += [f"- **{c.title()}**: mIoU = {results[f'miou_{c}']:.3f}{_ci(results, f'miou_{c}')}" for c in ("clean",) + ADVERSE if f"miou_{c}" in results]
    lines += ["", "## Robustness Analysis", ""]
    if "robustness_degradation_ratio" in results:
        lines.append(f"- **Overall Degradation Ratio**: {results['robustness_degradation_ratio']:.3f}"
                     f"{_ci(results, 'robustness_degradation_ratio')}")
    lines += [f"- **{c.title()} Degradation**: {results[f'robustness_degradation_{c}']:.3f}{_ci(results, f'robustness_degradation_{c}')}"
              for c in ADVERSE
              if f"robustness_degradation_{c}" in results]
    if "expected_calibration_error" in results:
        lines += ["", "## Confidence Calibration", "", f"- **Expected Calibration Error**: {results['expected_calibration_error']:.3f}"]
    if "ensemble_disagreement_auroc" in results:
        lines += ["", "## Ensemble Performance", "", f"- **Disagreement AUROC**: {results['ensemble_disagreement_auroc']:.3f}"]
    if "severity_levels" in results:
        lines += severity_section(results)
    if any(k.startswith("depth_abs_rel") for k in results):
        lines += depth_section(results)
    if any(k.startswith("failure_auroc_") for k in results):
        lines += failure_section(results)
    if any(k.startswith("boundary_iou_") for k in results):
        lines += boundary_section(results)
    if any(k.startswith("segment_count") for k in results):
        lines += segment_section(results)
    if "ensemble_weight_grid" in results:
        lines += weight_grid_section(results)
    if any(k.startswith("change_fraction_") for k in results):
        lines += change_section(results)
    if any(re.match(r"mse_.+_s\d+$", k) for k in results):
        lines += quality_section(results)
    if "overall_miou_restored" in results:
        lines += restoration_section(results)
    if "overall_miou_tta" in results:
        lines += tta_section(results)
    if "bootstrap_replicates" in results:
        lines += bootstrap_section(results)
    return "\n".join(lines)


def tta_section(results: Dict[str, Any]) -> list:
    """Test-time augmentation (evaluation.tta): one line per condition with the mIoU of the plain forward, of the logits averaged
    over the views, the difference, the share of the pixels whose class the averaging changed, and the shares of the labelled
    pixels it set right and set wrong."""
    names = [m.group(1) for k in results for m in [re.match(r"miou_(.+)_tta$", k)] if m]

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    scales = results.get("tta_scales")
    how = f"{int(results['tta_views'])} views" if "tta_views" in results else "several views"
    if scales is not None:
        how += " (scales " + ", ".join(f"{s:g}" for s in scales) + (", each also mirrored left to right" if results.get("tta_flip") else "") + ")"
    lines = ["", "## Test-Time Augmentation", "",
             f"Every member's logits averaged over {how} of the same frame, mirrored back and resampled to the frame, then combined "
             "and scored again (DESIGN.md 10r).  Gain: TTA - plain mIoU on the same frames (negative: the views cost accuracy); "
             "changed: share of the pixels whose class the averaging changed; fixed / broken: share of the labelled pixels it set "
             "right / set wrong.", "",
             "| Condition | Plain mIoU | TTA mIoU | Gain | Changed | Fixed | Broken |", "|---|---|---|---|---|---|---|"]
    for n in names:
        lines.append(f"| {n} | {cell(f'miou_{n}')} | {cell(f'miou_{n}_tta')} | {cell(f'tta_gain_{n}')} | "
                     f"{cell(f'tta_changed_fraction_{n}')} | {cell(f'tta_fixed_fraction_{n}')} | {cell(f'tta_broken_fraction_{n}')} |")
    lines.append(f"| all | {cell('overall_miou')} | {cell('overall_miou_tta')} | {cell('mean_tta_gain')} | "
                 f"{cell('mean_tta_changed_fraction')} | - | - |")
    return lines


def restoration_section(results: Dict[str, Any]) -> list:
    """Input restoration (evaluation.restoration): one line per condition with the mIoU of the frames as they came, of the same
    frames dehazed by the dark-channel prior, the difference, and the mean transmission the front-end estimated.  Under method:
    clahe (restoration_method in the results) the frames were relit instead and the luma gain stands where the mean transmission
    does, the share of gain-capped pixels where the airlight does; under method: tophat the occluders of rain and snow were masked
    and filled, and the masked share of the pixels and the mean change of a masked value stand in those two columns.  Under method:
    auto each frame went to one of the three or to none: the two columns are the share of the frames routed where the condition's
    name says they belong and the share routed to none, and a second table is the confusion table of the weather estimate."""
    names = [m.group(1) for k in results for m in [re.match(r"miou_(.+)_restored$", k)] if m]

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    relit = results.get("restoration_method") == "clahe"
    tophat = results.get("restoration_method") == "tophat"
    auto = results.get("restoration_method") == "auto"
    lines = ["", "## Input Restoration", ""]
    if auto:
        how = ("the method a weather estimate of its own pixels names (the mean dark channel, the red-to-blue ratio of the channel "
               "means with the mean luma, the share of top-hat seeds; DESIGN.md 10q)"
               if results.get("restoration_route") != "oracle" else
               "the method its true condition names (route: oracle, the upper bound of the routing; the estimate is only counted)")
        lines += [f"Method: auto, route: {results.get('restoration_route', 'estimated')}.  Every selected frame was sent to {how}: "
                  "dark_channel, clahe, tophat or none, restored by it in front of the model, and scored again.  Gain: restored - "
                  "plain mIoU on the same frames (negative: the front-end costs accuracy); routed right: share of the frames the "
                  "estimate sent where the condition's name says they belong; to none: share it left as they came.", ""]
    elif tophat:
        lines += ["Method: tophat.  In every selected frame the bright occluders of rain and snow were masked by the white top-hat of "
                  "all three channels and filled from their unmasked neighbours in front of the model, and the frame scored again.  "
                  "Gain: restored - plain mIoU on the same frames (negative: the front-end costs accuracy); occluders: share of the "
                  "pixels that were masked; change: mean absolute change of a masked channel value.", ""]
    elif relit:
        lines += ["Method: clahe.  Every selected frame relit by contrast-limited adaptive histogram equalisation of the luma with a "
                  "grey-world white balance in front of the model and scored again.  Gain: restored - plain mIoU on the same frames "
                  "(negative: the front-end costs accuracy); luma gain: mean luma of the restored frames over that of the frames as "
                  "they came; capped: share of the pixels whose gain was held at the limit.", ""]
    else:
        lines += ["Method: dark_channel.  Every selected frame dehazed by the dark-channel prior in front of the model and scored "
                  "again.  Gain: restored - plain mIoU on the same frames (negative: the front-end costs accuracy); mean t: the mean "
                  "estimated transmission (1 = nothing removed).", ""]
    # under refine: guided two more cells per line (how far the filter moved the patch transmission, the share of clamped pixels);
    # with the image-quality counters two more (PSNR and SSIM of the restored frames against the clean twins, with the gain over
    # the corrupted ones)
    guided = any(k.startswith("transmission_refinement_") for k in results)
    fidelity = any(re.match(r"(psnr|ssim)_.+_restored$", k) for k in results)
    head = ["Condition", "Plain mIoU", "Restored mIoU", "Gain"] \
        + (["Routed right", "To none"] if auto else ["Occluders", "Change"] if tophat else ["Luma gain", "Capped"] if relit
           else ["Mean t", "Airlight"]) + ["Degradation restored"]
    fifth, sixth = (("route_accuracy", "route_none_fraction") if auto else ("occluder_fraction", "occluder_change") if tophat
                    else ("relight_gain", "relight_capped_fraction") if relit else ("transmission_mean", "airlight"))
    head += ["Refinement", "Clamped"] * guided + ["PSNR restored (gain)", "SSIM restored (gain)"] * fidelity
    if "restoration_refine" in results:
        lines += [f"Transmission refinement: {results['restoration_refine']} filter (DESIGN.md 10n-bis).", ""]
    lines += ["| " + " | ".join(head) + " |", "|---" * len(head) + "|"]

    def more(n):
        cells = []
        if guided:
            cells += [cell("mean_transmission_refinement" if n is None else f"transmission_refinement_{n}"),
                      cell("mean_transmission_clamped_fraction" if n is None else f"transmission_clamped_fraction_{n}")]
        if fidelity:
            for stem, fmt in (("psnr", ".2f"), ("ssim", ".3f")):
                key = f"mean_{stem}_restored" if n is None else f"{stem}_{n}_restored"
                gain = f"mean_restoration_{stem}_gain" if n is None else f"restoration_{stem}_gain_{n}"
                cells.append(format(results[key], fmt) + (f" ({results[gain]:+{fmt}})" if gain in results else "") if key in results else "-")
        return "".join(f" {c} |" for c in cells)
    for n in names:
        lines.append(f"| {n} | {cell('miou_' + n)} | {cell('miou_' + n + '_restored')} | {cell('restoration_gain_' + n)} | "
                     f"{cell(fifth + '_' + n)} | {cell(sixth + '_' + n)} | {cell('robustness_degradation_' + n + '_restored')} |"
                     + more(n))
    lines.append(f"| all | - | {cell('overall_miou_restored')} | {cell('mean_restoration_gain')} | "
                 f"{cell('route_accuracy' if auto else 'mean_' + fifth if relit or tophat else 'mean_transmission')} | "
                 f"{cell('mean_' + sixth)} | - |" + more(None))
    if auto:
        routes = ("none", "dark_channel", "clahe", "tophat")
        seen = [m.group(1) for k in results for m in [re.match(r"route_none_fraction_(.+)$", k)] if m]
        lines += ["", "Estimated route against true condition (shares of the condition's frames), with the statistics the estimate "
                  "decides on:", "", "| Condition | " + " | ".join(routes) + " | Dark channel | Luma | Red / blue | Seeds |",
                  "|---" * 9 + "|"]
        for n in seen:
            lines.append(f"| {n} | " + " | ".join(cell(f"route_{r}_fraction_{n}") for r in routes)
                         + f" | {cell('estimate_dark_channel_' + n)} | {cell('estimate_luma_' + n)} | {cell('estimate_cast_' + n)} | "
                         + (f"{results['estimate_seed_fraction_' + n]:.5f}" if 'estimate_seed_fraction_' + n in results else "-") + " |")
    if relit:
        gains = [f"{results[k]:.3f}" for k in ("mean_white_balance_gain_r", "mean_white_balance_gain_g", "mean_white_balance_gain_b")
                 if k in results]
        if len(gains) == 3:
            lines += ["", f"- **Mean white-balance gains** (r / g / b): {' / '.join(gains)}"]
    if tophat and "mean_occluder_unfilled_fraction" in results:
        lines += ["", f"- **Masked pixels left unfilled** (no unmasked pixel in their window): {results['mean_occluder_unfilled_fraction']:.3f}"]
    extra = [f"- **Clean cost** (plain - restored mIoU of the clean frames): {results['restoration_clean_cost']:.3f}"] \
        if "restoration_clean_cost" in results else []
    extra += [f"- **{title}**: {int(results[key])}" for key, title in (("restoration_nonfinite_values", "Input values that are not finite"),
                                                                      ("restoration_airlight_floored_frames", "Frames whose airlight hit the floor"))
              if key in results]
    return lines + ([""] + extra if extra else [])


def quality_section(results: Dict[str, Any]) -> list:
    """Image quality (evaluation.image_quality): one line per kind and level with what the rendering did to the image (PSNR, SSIM
    and its luminance and contrast-structure factors) next to the mIoU, then the mIoU of every kind at equal SSIM."""
    names = list(dict.fromkeys(m.group(1) for k in results for m in [re.match(r"mse_(.+_s\d+)$", k)] if m))
    kinds = list(dict.fromkeys(n.rsplit("_s", 1)[0] for n in names))

    def cell(key, fmt=".3f"):
        return format(results[key], fmt) if key in results else "-"
    lines = ["", "## Image Quality", "", "Every corrupted frame against its clean frame, on the [0, 1] scale: PSNR in dB, SSIM over "
             "whole 11 x 11 Gaussian windows and its two factors (luminance; contrast and structure).", "",
             "| Kind | Level | PSNR | SSIM | Luminance | Contrast | mIoU | mIoU drop per SSIM |", "|---" * 8 + "|"]
    for n in names:
        kind, level = n.rsplit("_s", 1)
        lines.append(f"| {kind} | {level} | {cell('psnr_' + n, '.2f')} | {cell('ssim_' + n)} | {cell('ssim_luminance_' + n)} | "
                     f"{cell('ssim_contrast_' + n)} | {cell('miou_' + n)} | {cell('miou_drop_per_ssim_' + n)} |")
    if "mean_ssim" in results:
        lines.append(f"| all | - | {cell('mean_psnr', '.2f')} | {cell('mean_ssim')} | {cell('mean_ssim_luminance')} | "
                     f"{cell('mean_ssim_contrast')} | - | - |")
    targets = sorted({int(m.group(1)) for k in results for m in [re.match(r"(?:mean_)?miou_at_ssim(\d+)(?:_|$)", k)] if m}, reverse=True)
    if targets:
        lines += ["", "mIoU at equal SSIM (piecewise linear between the levels, never extrapolated) / degradation against clean:", "",
                  "| Kind | " + " | ".join(f"SSIM {t / 100:g}" for t in targets) + " |", "|---" * (len(targets) + 1) + "|"]
        for kind in kinds:
            lines.append(f"| {kind} | " + " | ".join(
                f"{cell(f'miou_at_ssim{t}_{kind}')} / {cell(f'robustness_degradation_at_ssim{t}_{kind}')}" for t in targets) + " |")
        lines.append("| mean | " + " | ".join(cell(f"mean_miou_at_ssim{t}") for t in targets) + " |")
    extra = [f"- **SSIM does not decrease with the level for {k[len('ssim_not_monotonic_'):]}**: no mIoU at equal SSIM"
             for k in results if k.startswith("ssim_not_monotonic_")]
    extra += [f"- **{title}**: {int(results[key])}" for key, title in (("quality_unmeasured_terms", "Error terms not measured"),
                                                                      ("quality_unmeasured_windows", "Windows not measured")) if key in results]
    return lines + ([""] + extra if extra else [])


def segment_section(results: Dict[str, Any]) -> list:
    """Segments (evaluation.segment_metrics): one line per condition with how many label segments the prediction finds, misses
    entirely and invents, overall and by size group; under a severity sweep the share of the clean twin's detections each kind and
    level loses."""
    names = [""] + [k[len("segment_count_"):] for k in results if k.startswith("segment_count_")]

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    lines = ["", "## Segments", "", "8-connected segments of one class: recall, precision and F1 over segments (class means), the share "
             "of label segments of which no pixel is found (miss rate) and of prediction segments without a pixel of their class "
             "(false rate); small: below 1024 pixels, medium: below 16384.", "",
             "| Condition | Segments | Recall | Precision | F1 | Miss rate | False rate | Recall small / medium / large | "
             "Miss rate small / medium / large |", "|---" * 9 + "|"]
    for n in names:
        sfx = "_" + n if n else ""
        groups = lambda key: " / ".join(cell(f"{key}_{g}{sfx}") for g in ("small", "medium", "large"))      # noqa: E731
        lines.append(f"| {n or 'all'} | {int(results.get('segment_count' + sfx, 0))} | {cell('segment_recall' + sfx)} | "
                     f"{cell('segment_precision' + sfx)} | {cell('segment_f1' + sfx)} | {cell('segment_miss_rate' + sfx)} | "
                     f"{cell('segment_false_rate' + sfx)} | {groups('segment_recall')} | {groups('segment_miss_rate')} |")
    lost = [k[len("segment_lost_"):] for k in results if k.startswith("segment_lost_")]
    if lost:
        lines += ["", "Of the label segments the clean frame's prediction detects, the share the corrupted frame's loses; of those it "
                  "does not detect, the share the corrupted frame's recovers:", "", "| Kind | Lost | Recovered |", "|---|---|---|"]
        lines += [f"| {n} | {cell('segment_lost_' + n)} | {cell('segment_recovered_' + n)} |" for n in lost]
    return lines


def weight_grid_section(results: Dict[str, Any]) -> list:
    """Ensemble weights (evaluation.ensemble_weight_grid): one line per condition with the mIoU at the configured, the fitted and the
    condition's own best weighting, that best SegFormer share, both members' mIoU and the oracle accuracy."""
    names = [""] + [k[len("miou_best_weight_"):] for k in results if k.startswith("miou_best_weight_")]

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    head = "Ensemble mIoU at every SegFormer share of a grid"
    if "ensemble_weight_fitted" in results:
        head += f"; the fitted share {results['ensemble_weight_fitted']:.3f} is the best one on the calibration condition"
    lines = ["", "## Ensemble Weights", "", head + ".  Oracle accuracy: the share of labelled pixels at least one member gets right.", "",
             "| Condition | Configured mIoU | Fitted mIoU | Best mIoU | Best share | SegFormer mIoU | DeepLabV3+ mIoU | Oracle accuracy |",
             "|---" * 8 + "|"]
    for n in names:
        sfx = "_" + n if n else ""
        lines.append(f"| {n or 'all'} | {cell('miou_configured_weight' + sfx)} | {cell('miou_fitted_weight' + sfx)} | {cell('miou_best_weight' + sfx)} | "
                     f"{cell('ensemble_weight_best' + sfx)} | {cell('segformer_miou' + sfx)} | {cell('deeplabv3plus_miou' + sfx)} | "
                     f"{cell('member_oracle_accuracy' + sfx)} |")
    extra = [f"- **{title}**: {int(results[key])}" for key, title in (("weight_grid_out_of_range_labels", "Labels out of range"),
                                                                      ("weight_grid_nan_pixels", "Labelled pixels with a NaN logit"))
             if key in results]
    return lines + ([""] + extra if extra else [])


def change_section(results: Dict[str, Any]) -> list:
    """Change strata (evaluation.change_strata): one line per kind and stratum of the input change against the clean frame."""
    edges = []
    while f"change_edge_{len(edges)}" in results:
        edges.append(results[f"change_edge_{len(edges)}"])
    K = len(edges) + 1
    bounds = [f"< {edges[0]:g}"] + [f"[{a:g}, {b:g})" for a, b in zip(edges, edges[1:])] + [f">= {edges[-1]:g}"]
    names = list(dict.fromkeys(m.group(1) for k in results for m in [re.match(r"change_fraction_(.+)_chg\d+$", k)]
                               if m and not re.search(r"_s\d+$", m.group(1))))

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    lines = ["", "## Change Strata", "", "Pixels split by how much the corruption changed the input against the clean frame (largest "
             "channel difference, 8-bit grey levels).  Error share: the part of the errors the corruption introduced (clean right, "
             "corrupted wrong) that falls into the stratum.", "",
             "| Kind | Change | Pixel share | mIoU | Accuracy | Consistency | Corruption error rate | Error share |", "|---" * 8 + "|"]
    for n in names + [None]:
        for k in range(K):
            key = (lambda m, n=n, k=k: f"mean_{m}_chg{k}" if n is None else f"{m}_{n}_chg{k}")
            if key("change_fraction") not in results:
                continue
            lines.append(f"| {n or 'all'} | {bounds[k]} | {cell(key('change_fraction'))} | {cell(key('miou'))} | {cell(key('accuracy'))} | "
                         f"{cell(key('consistency'))} | {cell(key('corruption_error_rate'))} | {cell(key('corruption_error_share'))} |")
    if "change_unmeasured_pixels" in results:
        lines += ["", f"- **Pixels without a measured change**: {int(results['change_unmeasured_pixels'])}"]
    return lines


def bootstrap_section(results: Dict[str, Any]) -> list:
    """Frame bootstrap (evaluation.bootstrap_replicates): every quantity with an interval, its pooled point estimate, the
    percentile interval, the standard error and, for the unclamped mIoU drops, the share of replicates with no drop."""
    names = [k[:-len("_ci_low")] for k in results if k.endswith("_ci_low")]
    conf = 100.0 * float(results.get("bootstrap_confidence", 0.95))
    lines = ["", "## Bootstrap Intervals", "",
             f"{int(results['bootstrap_replicates'])} paired bootstrap replicates over {int(results.get('bootstrap_sources', 0))} source "
             f"frames (all variants of a source drawn together), seed {int(results.get('bootstrap_seed', 0))}; {conf:g} % percentile "
             "intervals.  Degradations are clamped at 0 as their point estimates are; the mIoU drops are not.", "",
             "| Quantity | Point | Low | High | SE | P(drop <= 0) |", "|---|---|---|---|---|---|"]

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    for n in names:
        lines.append(f"| {n} | {cell(n)} | {cell(n + '_ci_low')} | {cell(n + '_ci_high')} | {cell(n + '_se')} | "
                     f"{cell(n + '_p_nonpositive')} |")
    empty = [f"- **Replicates without a labelled pixel of {k[len('bootstrap_empty_replicates_'):]}**: {int(results[k])}"
             for k in results if k.startswith("bootstrap_empty_replicates_")]
    return lines + ([""] + empty if empty else [])


def boundary_section(results: Dict[str, Any]) -> list:
    """Boundary bands (evaluation.boundary_widths): condition x width Boundary IoU, the interior mIoU, and what each adverse kind
    loses at the boundary (widest band) against what it loses in the interior."""
    import re
    widths = sorted({int(m.group(1)) for k in results for m in [re.match(r"boundary_fraction_w(\d+)$", k)] if m})
    first = f"boundary_fraction_w{widths[0]}_"
    names = [""] + [k[len(first):] for k in results if k.startswith(first)]

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    lines = ["", "## Boundary Bands", "", "Boundary IoU over the labelled pixels within w pixels (Chebyshev) of a class boundary; "
             "interior: mIoU beyond the widest band.", "",
             "| Condition | " + " | ".join(f"w = {d}" for d in widths) + f" | Band share (w = {widths[-1]}) | Interior mIoU | "
             f"Boundary degradation (w = {widths[-1]}) | Interior degradation |", "|---" * (len(widths) + 5) + "|"]
    for n in names:
        sfx = "_" + n if n else ""
        lines.append(f"| {n or 'all'} | " + " | ".join(cell(f"boundary_iou_w{d}{sfx}") for d in widths) +
                     f" | {cell(f'boundary_fraction_w{widths[-1]}{sfx}')} | {cell('interior_miou' + sfx)} | "
                     f"{cell(f'boundary_degradation_w{widths[-1]}{sfx}') if n else '-'} | {cell('interior_degradation' + sfx) if n else '-'} |")
    return lines


FAILURE_SCORES = ("mi", "entropy", "variance", "msp")


def failure_section(results: Dict[str, Any]) -> list:
    """Failure detection (evaluation.failure_detection): condition x score, AUROC +- its halfwidth and the excess AURC."""
    scores = [s for s in FAILURE_SCORES if f"failure_auroc_{s}" in results]
    first = f"failure_auroc_{scores[0]}_"
    names = [""] + [k[len(first):] for k in results if k.startswith(first)]

    def cell(score, sfx):
        if f"failure_auroc_{score}{sfx}" not in results:
            return "-"
        return (f"{results[f'failure_auroc_{score}{sfx}']:.3f} ± {results[f'failure_auroc_halfwidth_{score}{sfx}']:.3f} / "
                f"{results[f'failure_eaurc_{score}{sfx}']:.3f}")
    lines = ["", "## Failure Detection", "", "AUROC ± halfwidth / E-AURC of each uncertainty score against the prediction's errors.", "",
             "| Condition | " + " | ".join(scores) + " | Error rate |", "|---" * (len(scores) + 2) + "|"]
    for n in names:
        sfx = "_" + n if n else ""
        err = f"{results['failure_error_rate' + sfx]:.3f}" if "failure_error_rate" + sfx in results else "-"
        lines.append(f"| {n or 'all'} | " + " | ".join(cell(s, sfx) for s in scores) + f" | {err} |")
    extra = [f"- **{title}**: {int(results[key])}" for key, title in (("failure_nonfinite_pixels", "Non-finite pixels"),
                                                                     ("failure_out_of_range_labels", "Out-of-range labels")) if key in results]
    return lines + ([""] + extra if extra else [])


def depth_section(results: Dict[str, Any]) -> list:
    """Depth metrics (evaluation.depth_metrics): condition x metric for the ensemble (or the single model), one line per member."""
    cols = ("abs_rel", "sq_rel", "mae", "rmse", "rmse_log", "silog", "delta1", "delta2", "delta3")
    names = [""] + [k[len("depth_abs_rel_"):] for k in results if k.startswith("depth_abs_rel_")]

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    lines = ["", "## Depth", "", "| Condition | " + " | ".join(cols) + " | Valid | Degradation |", "|---" * (len(cols) + 3) + "|"]
    for n in names:
        sfx = "_" + n if n else ""
        lines.append(f"| {n or 'all'} | " + " | ".join(cell(f"depth_{c}{sfx}") for c in cols) +
                     f" | {cell('depth_valid_fraction' + sfx)} | {cell('depth_degradation' + sfx) if n else '-'} |")
    lines.append("")
    for prefix, title in (("segformer_", "SegFormer"), ("deeplabv3plus_", "DeepLabV3+")):
        if f"{prefix}depth_abs_rel" in results:
            lines.append(f"- **{title}**: " + ", ".join(f"{c} = {results[f'{prefix}depth_{c}']:.3f}" for c in cols
                                                        if f"{prefix}depth_{c}" in results))
    for key, title in (("depth_masked_pixels", "Masked pixels (target below the floor)"), ("depth_nonfinite_pixels", "Non-finite pixels"),
                       ("depth_saturated_terms", "Saturated terms")):
        if key in results:
            lines.append(f"- **{title}**: {int(results[key])}")
    return lines


def severity_section(results: Dict[str, Any]) -> list:
    """The paired severity sweep (evaluation.severities): one table per adverse kind, one row per level."""
    levels = int(results["severity_levels"])
    kinds = [k for k in dict.fromkeys(key[len("severity_intensity_"):].rsplit("_s", 1)[0] for key in results
                                      if key.startswith("severity_intensity_"))]
    lines = ["", "## Severity Sweep", "", f"{int(results.get('paired_sources', 0))} source frames, each also rendered under every "
             f"kind at {levels} severity levels; consistency and corruption error rate compare with the clean frame's prediction."]
    if "mean_consistency" in results:
        lines.append(f"- **Mean Consistency**: {results['mean_consistency']:.3f}")
    if "mean_corruption_error_rate" in results:
        lines.append(f"- **Mean Corruption Error Rate**: {results['mean_corruption_error_rate']:.3f}")

    def cell(key):
        return f"{results[key]:.3f}" if key in results else "-"
    for kind in kinds:
        lines += ["", f"### {kind.title()}", "", "| Level | Intensity | mIoU | Degradation | Consistency | Corruption Error Rate |",
                  "|-------|-----------|------|-------------|-------------|-----------------------|"]
        for j in range(1, levels + 1):
            n = f"{kind}_s{j}"
            lines.append(f"| {j} | {cell('severity_intensity_' + n)} | {cell('miou_' + n)}{_ci(results, 'miou_' + n)} | "
                         f"{cell('robustness_degradation_' + n)}{_ci(results, 'robustness_degradation_' + n)} | "
                         f"{cell('consistency_' + n)} | {cell('corruption_error_rate_' + n)} |")
    return lines


def generate_evaluation_report(results: Dict[str, Any], output_dir, target_metrics: Optional[Dict[str, float]] = None) -> None:
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / "evaluation_results.json").write_text(json.dumps(results, indent=2))
    (out / "evaluation_report.md").write_text(report_markdown(results, target_metrics))
