#!/usr/bin/env python3
"""Evaluation entry point — counterpart of REF/scripts/evaluate.py (same positional/flag CLI:
`evaluate.py <checkpoint> [--config C] [--output-dir D] [--device DEV]`, same result keys, same
evaluation_results.json).  Under `torch.distributed.run` every rank evaluates its own shard of the
test set and the counters are all-reduced over RCCL.

    python scripts/evaluate.py checkpoints/best.pth --config configs/default.yaml
    python scripts/evaluate.py none --config configs/default.yaml        # random-init model (no checkpoint)
"""
import argparse
import json
import logging
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch

from adverse_weather_semantic_segmentation_robustness_benchmark_amd import parallel
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import CityscapesKITTIDataset, create_dataloader
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.harness import evaluate_model
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import RobustnessMetrics
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import generate_evaluation_report, restoration_section
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.utils.checkpoint import load_model_state
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.models.model import DeepLabV3PlusModel, EnsembleModel, SegFormerModel
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.utils.config import (create_default_config, get_device_config, load_config,
                                                                                    setup_logging)

logger = logging.getLogger("evaluate")


def load_model(config, checkpoint_path, device):
    """REF/scripts/evaluate.py:42-86."""
    kind = config.get("model.type", "ensemble")
    nc, depth = config.get("model.num_classes", 19), config.get("model.include_depth", True)
    if kind == "segformer":
        model = SegFormerModel(num_classes=nc, include_depth=depth)
    elif kind == "deeplabv3plus":
        model = DeepLabV3PlusModel(num_classes=nc, include_depth=depth)
    elif kind == "ensemble":
        model = EnsembleModel(num_classes=nc, include_depth=depth, ensemble_strategy=config.get("model.ensemble_strategy", "weighted_average"),
                              temperature_scaling=config.get("model.temperature_scaling", True))
    else:
        raise ValueError(f"Unknown model type: {kind}")
    if checkpoint_path and str(checkpoint_path).lower() != "none":
        ckpt = torch.load(checkpoint_path, map_location=device, weights_only=False)
        load_model_state(model, ckpt)            # incl. the transformers-version key translation
    return model.to(device).eval()


def parse_severities(text: str):
    """--severities: 'reference' or '0.3,0.6,0.9' (validated with the configuration by the dataset)."""
    text = text.strip()
    if text == "reference":
        return text
    try:
        return [float(v) for v in text.split(",") if v.strip()]
    except ValueError:
        raise ValueError(f"--severities takes 'reference' or comma-separated intensities, got {text!r}") from None


def parse_boundary_widths(text: str):
    """--boundary-widths: comma-separated integers (the harness checks their range and order)."""
    try:
        return [int(x) for x in text.split(",")]
    except ValueError:
        raise ValueError(f"--boundary-widths takes comma-separated integers such as 1,2,4,8, got {text!r}") from None


def parse_change_strata(text: str):
    """--change-strata: 'default' or comma-separated numbers (the harness checks their range and order)."""
    if text.strip() == "default":
        return "default"
    try:
        return [float(x) for x in text.split(",")]
    except ValueError:
        raise ValueError(f"--change-strata takes 'default' or comma-separated numbers such as 0.5,4.5,16.5, got {text!r}") from None


def parse_weight_grid(text: str):
    """--ensemble-weight-grid: an integer n (n equally spaced SegFormer shares) or comma-separated shares (the harness checks their
    number, range and order)."""
    try:
        return [float(x) for x in text.split(",")] if "," in text or "." in text else int(text)
    except ValueError:
        raise ValueError(f"--ensemble-weight-grid takes an integer such as 11 or comma-separated shares such as 0.25,0.5,0.75, got "
                         f"{text!r}") from None


def parse_image_quality_targets(text: str):
    """--image-quality-targets: comma-separated SSIM values (the harness checks their number and range)."""
    try:
        return [float(x) for x in text.split(",")]
    except ValueError:
        raise ValueError(f"--image-quality-targets takes comma-separated numbers such as 0.9,0.75,0.5, got {text!r}") from None


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Evaluate adverse-weather segmentation model (MI355X-native path)")
    ap.add_argument("checkpoint", type=str)
    ap.add_argument("--config", type=str, default=None)
    ap.add_argument("--output-dir", type=str, default="evaluation_results")
    ap.add_argument("--device", type=str, default="auto")
    ap.add_argument("--severities", type=str, default=None,
                    help="paired severity sweep: 'reference' or comma-separated intensities (overrides evaluation.severities)")
    ap.add_argument("--depth-metrics", action="store_true",
                    help="score the depth heads against the loader's depth target, per condition (sets evaluation.depth_metrics)")
    ap.add_argument("--failure-detection", action="store_true",
                    help="AUROC / AURC of four uncertainty scores against the prediction's errors, per condition "
                         "(sets evaluation.failure_detection)")
    ap.add_argument("--boundary-widths", type=str, default=None,
                    help="boundary-band metrics (trimap mIoU, Boundary IoU) per condition: 1-4 comma-separated increasing band widths in "
                         "pixels, each within [1, 16], e.g. 1,2,4,8 (sets evaluation.boundary_widths)")
    ap.add_argument("--segment-metrics", action="store_true",
                    help="segment-level metrics per condition: which 8-connected label segments the prediction finds, loses "
                         "entirely and invents (sets evaluation.segment_metrics)")
    ap.add_argument("--segment-threshold", type=float, default=None, metavar="T",
                    help="share of a segment that must be covered for it to count as found: 0.25, 0.5, 0.75 or 1.0 (default 0.5; "
                         "sets evaluation.segment_threshold)")
    ap.add_argument("--segment-min-area", type=int, default=None, metavar="A",
                    help="smallest segment counted, in pixels: a power of 4 (default 16; sets evaluation.segment_min_area)")
    ap.add_argument("--ensemble-weight-grid", type=str, default=None, metavar="N|A,B,C",
                    help="ensemble weight sweep: the mIoU of every condition at every member weighting of a grid, and which member is "
                         "right where: an integer n in [2, 63] (n equally spaced SegFormer shares) or 1-63 comma-separated increasing "
                         "shares in [0, 1] (sets evaluation.ensemble_weight_grid)")
    ap.add_argument("--change-strata", type=str, default=None, metavar="EDGES",
                    help="split every corrupted frame's errors by how much the corruption changed each input pixel against the clean "
                         "frame: 'default' (0.5,4.5,16.5,64.5) or 1-7 comma-separated increasing edges in 8-bit grey levels; needs "
                         "--severities (sets evaluation.change_strata)")
    ap.add_argument("--image-quality", action="store_true",
                    help="PSNR and SSIM (with its luminance and contrast factors) of every corrupted frame against its clean frame, "
                         "and the mIoU of every kind at equal SSIM; needs --severities (sets evaluation.image_quality)")
    ap.add_argument("--image-quality-targets", type=str, default=None, metavar="SSIM",
                    help="the SSIM values the mIoU is interpolated at: 1-8 comma-separated numbers in (0, 1), default 0.9,0.75,0.5 "
                         "(sets evaluation.image_quality_targets)")
    ap.add_argument("--tta", type=str, default=None, choices=("flip", "ms_flip"),
                    help="test-time augmentation: score the logits averaged over views of every frame a second time; flip: the "
                         "mirrored view, ms_flip: scales 0.5, 0.75, 1, 1.25, 1.5, each also mirrored (sets evaluation.tta)")
    ap.add_argument("--tta-scales", type=str, default=None, metavar="A,B,C",
                    help="the scales of the views, 1 .. 8 increasing numbers in [0.25, 2]; 1 is added when absent (sets "
                         "evaluation.tta.scales)")
    ap.add_argument("--tta-no-flip", action="store_true", help="no mirrored views (sets evaluation.tta.flip: false)")
    ap.add_argument("--restoration", type=str, default=None, choices=("dark_channel", "clahe", "tophat", "auto"),
                    help="restore every frame in front of the model and score it a second time: plain and restored mIoU and the gain "
                         "per condition.  dark_channel: dehazing by the dark-channel prior (with the mean transmission); clahe: night "
                         "relighting by CLAHE on the luma with a grey-world white balance (with the luma gain); tophat: rain "
                         "and snow removal, the bright occluders masked by the white top-hat and filled from their neighbours (with "
                         "the masked share of the pixels); auto: one of the three, or none, per frame, chosen by a weather estimate "
                         "from the frame's pixels alone (with the confusion table of the estimate).  Sets evaluation.restoration")
    ap.add_argument("--restoration-route", type=str, default=None, choices=("estimated", "oracle"),
                    help="what routes the frames under --restoration auto: the weather estimate (default), or oracle: the true "
                         "condition, the upper bound (sets evaluation.restoration.route)")
    ap.add_argument("--restoration-seed-min", type=float, default=None, metavar="X",
                    help="share of top-hat seed pixels above which a frame goes to tophat, 0 .. 1 (default 0.001, chosen at 256 x 512 "
                         "and above: it depends on the resolution; needs --restoration auto; sets "
                         "evaluation.restoration.estimator.seed_min)")
    ap.add_argument("--restoration-dark-min", type=float, default=None, metavar="X",
                    help="mean dark channel above which a frame goes to dark_channel, 0 .. 1 (default 0.47; needs --restoration auto; "
                         "sets evaluation.restoration.estimator.dark_min)")
    ap.add_argument("--restoration-cast-max", type=float, default=None, metavar="X",
                    help="red-to-blue ratio of the channel means below which a dark frame goes to clahe, 0 .. 4 (default 0.65; needs "
                         "--restoration auto; sets evaluation.restoration.estimator.cast_max)")
    ap.add_argument("--restoration-conditions", type=str, default=None, metavar="A,B",
                    help="restore only the frames of these comma-separated weather conditions (default: all, clean included; sets "
                         "evaluation.restoration_conditions)")
    ap.add_argument("--restoration-refine", type=str, default=None, choices=("opening", "none", "guided"),
                    help="transmission from the morphological opening of the normalised dark channel (default), from He's plain "
                         "patch minimum, or from the guided filter of the patch transmission (sets evaluation.restoration.refine)")
    ap.add_argument("--restoration-guided-radius", type=int, default=None, metavar="R",
                    help="window radius of the guided filter, 1 .. 32 (default min(4 radius, 32); needs --restoration-refine guided; "
                         "sets evaluation.restoration.guided_radius)")
    ap.add_argument("--restoration-guided-eps", type=float, default=None, metavar="EPS",
                    help="regularisation of the guided filter, 1e-4 .. 1 (default 1e-3; needs --restoration-refine guided; sets "
                         "evaluation.restoration.guided_eps)")
    ap.add_argument("--restoration-grid", type=str, default=None, metavar="N|TYxTX",
                    help="tiles of the CLAHE grid, 8 or 8x8, 1 .. 16 each way (default 8; needs --restoration clahe; sets "
                         "evaluation.restoration.grid)")
    ap.add_argument("--restoration-clip-limit", type=float, default=None, metavar="C",
                    help="clip limit of the tile histograms in multiples of the mean bin, 1 .. 64 (default 2; needs --restoration "
                         "clahe; sets evaluation.restoration.clip_limit)")
    ap.add_argument("--restoration-max-gain", type=float, default=None, metavar="G",
                    help="largest luma gain of a pixel, 1 .. 64 (default 8; needs --restoration clahe; sets "
                         "evaluation.restoration.max_gain)")
    ap.add_argument("--restoration-white-balance", type=str, default=None, choices=("gray_world", "none"),
                    help="white balance of the relit frames (default gray_world; needs --restoration clahe; sets "
                         "evaluation.restoration.white_balance)")
    ap.add_argument("--restoration-radius", type=int, default=None, metavar="R",
                    help="window radius, 1 .. 15: of the top-hat and the fill under --restoration tophat (default 9), of the dark "
                         "channel under --restoration dark_channel (default 7); sets evaluation.restoration.radius")
    ap.add_argument("--restoration-threshold", type=float, default=None, metavar="T",
                    help="smallest top-hat of all three channels that makes a pixel an occluder, in (0, 1] (default 0.06; needs "
                         "--restoration tophat; sets evaluation.restoration.threshold)")
    ap.add_argument("--restoration-bright-min", type=float, default=None, metavar="B",
                    help="smallest value of the darkest channel of an occluder, 0 .. 1 (default 0.5; needs --restoration tophat; sets "
                         "evaluation.restoration.bright_min)")
    ap.add_argument("--restoration-dilate", type=int, default=None, metavar="D",
                    help="pixels the occluder mask is grown by to cover the blurred rim, 0 .. 2 (default 1; needs --restoration "
                         "tophat; sets evaluation.restoration.dilate)")
    ap.add_argument("--bootstrap", type=int, default=None, metavar="N",
                    help="paired frame bootstrap with N replicates (1 .. 65536): percentile intervals and standard errors of every "
                         "mIoU and degradation (sets evaluation.bootstrap_replicates)")
    ap.add_argument("--bootstrap-confidence", type=float, default=None, metavar="C",
                    help="confidence level of the intervals, in (0, 1) (sets evaluation.bootstrap_confidence; default 0.95)")
    ap.add_argument("--bootstrap-seed", type=int, default=None, metavar="S",
                    help="seed of the resampling draws (sets evaluation.bootstrap_seed; default 0)")
    return ap


def apply_bootstrap_options(args, config) -> None:
    """--bootstrap / --bootstrap-confidence / --bootstrap-seed into the configuration (the harness checks their ranges)."""
    for flag, key in (("bootstrap", "evaluation.bootstrap_replicates"), ("bootstrap_confidence", "evaluation.bootstrap_confidence"),
                      ("bootstrap_seed", "evaluation.bootstrap_seed")):
        if getattr(args, flag) is not None:
            config.set(key, getattr(args, flag))


def parse_restoration_grid(text: str):
    """'8' -> 8, '8x4' -> [8, 4] (tile rows x tile columns); ValueError otherwise.  The harness checks the range."""
    parts = text.lower().split("x")
    if len(parts) not in (1, 2) or not all(p.strip().isdigit() for p in parts):
        raise ValueError(f"--restoration-grid is N or TYxTX (integers), got {text!r}")
    values = [int(p) for p in parts]
    return values[0] if len(values) == 1 else values


# --restoration-<flag> -> (the --restoration values it needs, its key under evaluation.restoration, what reads its text), in the order
# the messages name them.  The guided filter's flags pass without --restoration: what they need first is --restoration-refine guided
RESTORATION_FLAGS = {
    "route": (("auto",), "route", None), "seed_min": (("auto",), "estimator.seed_min", None),
    "dark_min": (("auto",), "estimator.dark_min", None), "cast_max": (("auto",), "estimator.cast_max", None),
    "refine": (("dark_channel",), "refine", None),
    "guided_radius": (("dark_channel", None), "guided_radius", None), "guided_eps": (("dark_channel", None), "guided_eps", None),
    "grid": (("clahe",), "grid", parse_restoration_grid), "clip_limit": (("clahe",), "clip_limit", None),
    "max_gain": (("clahe",), "max_gain", None), "white_balance": (("clahe",), "white_balance", None),
    "radius": (("tophat", "dark_channel"), "radius", None),
    "threshold": (("tophat",), "threshold", None), "bright_min": (("tophat",), "bright_min", None), "dilate": (("tophat",), "dilate", None),
}


def parse_tta_scales(text: str):
    """--tta-scales: comma-separated numbers (the harness checks their range and order)."""
    try:
        return [float(v) for v in text.split(",")]
    except ValueError:
        raise ValueError(f"--tta-scales takes comma-separated numbers such as 0.5,1,1.5, got {text!r}") from None


def apply_tta_options(args, config) -> None:
    """--tta, --tta-scales and --tta-no-flip into `evaluation.tta` (the harness checks it)."""
    if args.tta is None and args.tta_scales is None:
        if args.tta_no_flip:
            raise ValueError("--tta-no-flip needs --tta-scales: without the mirrored view and without other scales nothing is averaged")
        return
    if args.tta is not None and args.tta_scales is None and not args.tta_no_flip:
        config.set("evaluation.tta", args.tta)
        return
    if args.tta == "flip" and args.tta_no_flip:
        raise ValueError("--tta flip with --tta-no-flip: nothing is averaged")
    spec = {"flip": not args.tta_no_flip}
    if args.tta_scales is not None:
        spec["scales"] = parse_tta_scales(args.tta_scales)
    elif args.tta == "ms_flip":
        spec["scales"] = [0.5, 0.75, 1.0, 1.25, 1.5]
    config.set("evaluation.tta", spec)


def apply_restoration_options(args, config) -> None:
    """--restoration / --restoration-conditions and the flags of RESTORATION_FLAGS into the configuration (the harness checks them)."""
    method, option = args.restoration, lambda flag: f"--restoration-{flag.replace('_', '-')}"      # noqa: E731
    given = {f: getattr(args, f"restoration_{f}") for f in RESTORATION_FLAGS if getattr(args, f"restoration_{f}") is not None}
    for flag in given:
        owners = RESTORATION_FLAGS[flag][0]
        if method in owners:
            continue
        if method == "auto":
            raise ValueError(f"{', '.join(option(f) for f in given if 'auto' not in RESTORATION_FLAGS[f][0])}: under --restoration auto "
                             "the methods' parameters are configuration only (evaluation.restoration.dark_channel / .clahe / .tophat)")
        if owners[0] == "dark_channel" and method is not None:
            raise ValueError(f"--restoration-refine and --restoration-guided-* belong to --restoration dark_channel, not to {method}")
        names = [option(f) for f, (o, _, _) in RESTORATION_FLAGS.items() if o == owners]
        raise ValueError(f"{', '.join(names[:-1])}{' and ' if names[1:] else ''}{names[-1]} need{'' if names[1:] else 's'} "
                         f"{' or '.join('--restoration ' + o for o in owners)}")
    if given.keys() & {"guided_radius", "guided_eps"} and args.restoration_refine != "guided":
        raise ValueError("--restoration-guided-radius and --restoration-guided-eps need --restoration-refine guided")
    if method is not None:
        spec = {}
        for flag, value in given.items():
            _, key, read = RESTORATION_FLAGS[flag]
            *outer, key = key.split(".")
            level = spec
            for name in outer:
                level = level.setdefault(name, {})
            level[key] = value if read is None else read(value)
        if method != "dark_channel":                                   # the dark channel's dict carries no 'method' key
            spec = {"method": method, **spec}
        config.set("evaluation.restoration", spec if set(spec) - {"method"} else method)
    if args.restoration_conditions is not None:
        config.set("evaluation.restoration_conditions", [c.strip() for c in args.restoration_conditions.split(",") if c.strip()])


def main():
    args = build_parser().parse_args()
    try:
        config = load_config(args.config) if args.config else create_default_config()
        setup_logging(config)
        rank, local, world = parallel.init_from_env()
        dev = get_device_config(args.device if args.device != "auto" else config.get("device", "auto"))
        device = torch.device(dev, local) if dev.startswith("cuda") and ":" not in dev else torch.device(dev)
        model = load_model(config, args.checkpoint, device)
        if args.severities is not None:
            config.set("evaluation.severities", parse_severities(args.severities))
        if args.depth_metrics:
            config.set("evaluation.depth_metrics", True)
        if args.failure_detection:
            config.set("evaluation.failure_detection", True)
        if args.boundary_widths is not None:
            config.set("evaluation.boundary_widths", parse_boundary_widths(args.boundary_widths))
        if args.segment_metrics:
            config.set("evaluation.segment_metrics", True)
        if args.segment_threshold is not None:
            config.set("evaluation.segment_threshold", args.segment_threshold)
        if args.segment_min_area is not None:
            config.set("evaluation.segment_min_area", args.segment_min_area)
        if args.ensemble_weight_grid is not None:
            config.set("evaluation.ensemble_weight_grid", parse_weight_grid(args.ensemble_weight_grid))
        if args.change_strata is not None:
            config.set("evaluation.change_strata", parse_change_strata(args.change_strata))
        if args.image_quality:
            config.set("evaluation.image_quality", True)
        if args.image_quality_targets is not None:
            config.set("evaluation.image_quality_targets", parse_image_quality_targets(args.image_quality_targets))
        apply_bootstrap_options(args, config)
        apply_restoration_options(args, config)
        apply_tta_options(args, config)
        sev = config.get("evaluation.severities")
        paired = {"weather_schedule": "paired", "severities": sev} if sev is not None else {}
        ds = CityscapesKITTIDataset(data_root=config.get("data.data_root", "data"), split="test",
                                    image_size=tuple(config.get("data.image_size", [512, 1024])),
                                    weather_conditions=config.get("data.weather_conditions"), apply_augmentation=False,
                                    include_depth=config.get("data.include_depth", True), device=device, **paired)
        loader = create_dataloader(ds, batch_size=config.get("training.batch_size", 8), shuffle=False, rank=rank, world_size=world)
        metrics = RobustnessMetrics(num_classes=config.get("model.num_classes", 19), weather_conditions=config.get("data.weather_conditions"))
        results = evaluate_model(model, loader, metrics, device, config)
        if rank == 0:
            # (the weight sweep's grid and curves are lists of floats; every other value is a scalar)
            # and restoration_refine, which names the refinement)
            plain = {k: [float(x) for x in v] if isinstance(v, (list, tuple)) else v if isinstance(v, str) else float(v)
                     for k, v in results.items()}
            generate_evaluation_report(plain, Path(args.output_dir))   # json + markdown, :277-392
            for k, v in plain.items():
                if isinstance(v, list):
                    logger.info("%s: %s", k, " ".join(f"{x:.4f}" for x in v))
                elif isinstance(v, str):
                    logger.info("%s: %s", k, v)
                else:
                    logger.info("%s: %.4f", k, v)
            if "overall_miou_restored" in plain:                       # --restoration: plain / restored / gain / mean t per condition
                for line in restoration_section(plain):
                    if line:
                        logger.info("%s", line)
    except Exception as e:  # noqa: BLE001 - the reference converts failures to exit code 1 (evaluate.py:506-508)
        logger.error("Evaluation failed: %s", e)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
