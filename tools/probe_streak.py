"""Where the rain kernel's time goes: the same 8 frames with (a) the drawn drops, (b) thin drops only, (c) no drops.
    python tools/probe_streak.py"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops                      # noqa: E402
from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import preprocessing as P  # noqa: E402


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]))


def main():
    B, H, W = 8, 1024, 2048
    np.random.seed(0)
    imgs = torch.randint(0, 255, (B, H, W, 3), dtype=torch.uint8, device="cuda")
    norm = torch.empty(B, 3, H, W, device="cuda")
    idx = list(range(B))
    rd = [P.draw_rain(H, W, 0.5) for _ in range(B)]
    variants = {"drawn drops": [d[1] for d in rd]}
    thin = [d[1].copy() for d in rd]
    for t in thin:
        t[:, 4] = 1
    variants["thin drops only"] = thin
    variants["no drops"] = [d[1][:0] for d in rd]
    for name, drops in variants.items():
        rj, rp = ops.prim_jobs(idx, [d[0] for d in rd], drops)
        ms = timed(lambda: ops.rain(imgs, rj, rp, norm_out=norm))
        print(f"rain, {name:18s} {ms * 1e3:8.1f} us   {15 * H * W * B / ms / 1e6:8.1f} GB/s")
    sd = [P.draw_snow(H, W, 0.5) for _ in range(B)]
    for name, fl in (("drawn flakes", [d[1] for d in sd]), ("no flakes", [d[1][:0] for d in sd])):
        for ks in (3, 7):
            sj, sp = ops.prim_jobs(idx, [d[0] for d in sd], fl, [ks] * B)
            ms = timed(lambda: ops.snow(imgs, sj, sp, norm_out=norm))
            print(f"snow k{ks}, {name:14s} {ms * 1e3:8.1f} us   {15 * H * W * B / ms / 1e6:8.1f} GB/s")


if __name__ == "__main__":
    main()
