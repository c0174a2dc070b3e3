#!/usr/bin/env python3
"""How often the stale-maximum loop of csrc/attn.hip takes its rescale path, counted on the CPU.

A numpy emulation of the tile loop's control flow (32-key tiles, one query per lane, 32 queries per wave, the branch taken by the
whole wave when any of its queries has a tile maximum more than tau above its stale integer maximum, every query of the wave then
moving to max(m, ceil(tile maximum))), on
  * the inputs of the attention tests (standard normal q, k at the tests' shapes, plain and x 8; the flat-softmax case), and
  * the q / k that the bench model (EnsembleModel, seed 42, random weights, a uniform random uint8 frame) hands its stage-1 and
    stage-2 attention, taken with forward hooks from the as-written transformers module on the CPU at a reduced frame.
Printed per input and tau: the share of (wave, tile) pairs behind the first tile that rescale, the same per query, and the largest
number of bits the stale maximum sat above / below the exact running maximum.

    python tools/attention_stale_rate.py [--height 512] [--width 1024] [--taus 2,3,4,6,8]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LOG2E = 1.4426950408889634


def emulate(q, k, scale, tau):
    """q [nq, 32], k [nkv, 32] of one (image, head).  Returns (wave-tiles behind the first, rescaling ones, query-tiles, rescaling
    ones, max of m - running max, max of running max - m)."""
    s = (q.astype(np.float64) * (scale * LOG2E)) @ k.astype(np.float64).T
    nq, nkv = s.shape
    T = nkv // 32
    pad = (-nq) % 32
    tm = s.reshape(nq, T, 32).max(-1)
    if pad:
        tm = np.concatenate([tm, np.repeat(tm[-1:], pad, 0)], 0)          # the kernel clamps the ragged wave's queries to the last one
    tm = tm.reshape(-1, 32, T)                                            # [wave, lane, tile]
    m = np.ceil(tm[:, :, 0])
    run = tm[:, :, 0].copy()
    wt = wr = qt = qr = 0
    above = below = 0.0
    for t in range(1, T):
        trig = tm[:, :, t] - m > tau
        wave = trig.any(1)
        wt += wave.size; wr += int(wave.sum()); qt += trig.size; qr += int(trig.sum())
        new = np.maximum(m, np.ceil(tm[:, :, t]))
        m = np.where(wave[:, None], new, m)
        run = np.maximum(run, tm[:, :, t])
        above = max(above, float((m - run).max())); below = max(below, float((run - m).max()))
    return wt, wr, qt, qr, above, below


def report(name, cases, taus):
    for tau in taus:
        tot = np.zeros(4)
        above = below = 0.0
        for q, k, scale in cases:
            r = emulate(q, k, scale, tau)
            tot += r[:4]; above = max(above, r[4]); below = max(below, r[5])
        print(f"{name:58s} tau {tau:2d}: wave-tiles rescaling {100 * tot[1] / max(tot[0], 1):6.2f} %  query-tiles {100 * tot[3] / max(tot[2], 1):7.3f} %"
              f"   m - max <= {above:.2f}, max - m <= {below:.2f} bits", flush=True)


def heads_of(q, k, nh):
    """[B, n, nh*32] -> list of per-(image, head) (q, k)"""
    out = []
    for b in range(q.shape[0]):
        for h in range(nh):
            out.append((q[b, :, 32 * h:32 * h + 32], k[b, :, 32 * h:32 * h + 32]))
    return out


def test_inputs():
    rs = np.random.RandomState(0)
    cases = {}
    for B, nh, nq, nkv in ((2, 5, 300, 2048), (2, 1, 200, 64), (1, 8, 64, 96), (2, 2, 2100, 256)):
        q, k = rs.randn(B, nq, nh * 32).astype(np.float32), rs.randn(B, nkv, nh * 32).astype(np.float32)
        for mult in (1.0, 8.0):
            cases[f"tests: randn q, k x{mult:g}  B{B} h{nh} {nq} q x {nkv} k"] = [(a * mult, b * mult, 32 ** -0.5) for a, b in heads_of(q, k, nh)]
    q = (rs.randn(1, 256, 32) * 0.01).astype(np.float32); k = rs.randn(1, 2048, 32).astype(np.float32); k[:, 5] *= 400.0
    cases["tests: flat softmax, one dominant key  256 q x 2048 k"] = [(q[0], k[0], 32 ** -0.5)]
    return cases


def model_inputs(height, width):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.models.model import EnsembleModel
    torch.manual_seed(42); np.random.seed(42)
    model = EnsembleModel(num_classes=19, include_depth=True, pretrained=False).eval()
    seg = model.segformer.segformer
    grabbed = {}
    hooks = []
    for si, st in enumerate(list(seg.encoder.block) if hasattr(seg, "encoder") else [s.blocks for s in seg.stages]):
        for bi, blk in enumerate(st):
            att = blk.attention
            att = getattr(att, "self", att)
            qm = getattr(att, "query", None) or att.q_proj
            km = getattr(att, "key", None) or att.k_proj
            nh = att.num_attention_heads
            for tag, mod in (("q", qm), ("k", km)):
                hooks.append(mod.register_forward_hook(lambda _m, _i, o, key=(si, bi, tag, nh): grabbed.__setitem__(key, o.detach().float().numpy())))
    g = torch.Generator().manual_seed(42 * 1000003)
    img = torch.randint(0, 255, (1, height, width, 3), dtype=torch.uint8, generator=g)
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    x = ((img.float() / 255.0 - mean) / std).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        seg(x)
    for h_ in hooks:
        h_.remove()
    cases = {}
    for (si, bi, tag, nh), arr in sorted(grabbed.items()):
        if tag != "q" or si > 1:
            continue
        q = arr.reshape(1, -1, nh * 32); k = grabbed[(si, bi, "k", nh)].reshape(1, -1, nh * 32)
        if k.shape[1] % 32:
            continue
        cases[f"bench model stage {si + 1} block {bi}: {q.shape[1]} q x {k.shape[1]} k, {nh} head(s)"] = [(a, b, 32 ** -0.5) for a, b in heads_of(q, k, nh)]
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--taus", type=str, default="2,3,4,6,8")
    a = ap.parse_args()
    taus = [int(t) for t in a.taus.split(",")]
    for name, cases in test_inputs().items():
        report(name, cases, taus)
    for name, cases in model_inputs(a.height, a.width).items():
        report(name, cases, taus)


if __name__ == "__main__":
    main()
