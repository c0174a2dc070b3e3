"""Float64 model of the depth error counters (csrc/deptheval.hip, ops.depth_eval_stats) and of their host math.

`depth_stats` computes what the device accumulates — per condition slot and prediction series the valid / masked / non-finite
pixel counts, the six clamped error sums, the three threshold counts and the saturated terms — from the same float32 input
values, in float64 (`ft=np.float64`) or, as the yardstick of the tests' gate, with every per-pixel operation rounded to float32
and only the sums in float64 (`ft=np.float32`, the "twin").  It also counts, per threshold, the valid pixels whose ratio lies
within relative 2^-20 of the threshold (`near`): the only pixels a float32 computation may legitimately put on the other side.
"""
from __future__ import annotations

import numpy as np

UNIT = 2.0 ** -20
CAP = 2048.0
THRESHOLDS = (1.25, 1.5625, 1.953125)
FIELDS = ("valid", "masked", "nonfinite", "sum_abs", "sum_sq", "sum_abs_rel", "sum_sq_rel", "sum_log", "sum_log_sq",
          "delta1", "delta2", "delta3", "saturated")
SUMS = FIELDS[3:9]
MEANS = ("mae", "mse", "abs_rel", "sq_rel", "mean_log", "mean_log_sq")


def upsample(lo, H: int, W: int, ft=np.float64) -> np.ndarray:
    """Bilinear upsample [B,h,w] -> [B,H,W], torch's align_corners=False rule: scale = (float32)in / out, source index
    max(scale * (dst + 0.5) - 0.5, 0), the second texel clamped to the last; the expression order of the device kernel."""
    lo = np.asarray(lo)
    _, h, w = lo.shape

    def axis(n_in, n_out):
        s = ft(np.float32(n_in) / np.float32(n_out))
        f = np.maximum(s * (np.arange(n_out).astype(ft) + ft(0.5)) - ft(0.5), ft(0))
        i0 = np.minimum(f.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = (f - i0.astype(ft)).astype(ft)
        return i0, i1, (ft(1) - l1).astype(ft), l1
    y0, y1, ly0, ly1 = axis(h, H)
    x0, x1, lx0, lx1 = axis(w, W)
    L = lo.astype(ft)
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        top = lx0 * L[:, y0][:, :, x0] + lx1 * L[:, y0][:, :, x1]
        bot = lx0 * L[:, y1][:, :, x0] + lx1 * L[:, y1][:, :, x1]
        return (ly0 * top + ly1 * bot).astype(ft)


def series_maps(d1, d2_low, weights, ft=np.float64) -> list:
    """[d1] or [ensemble, d1, upsampled d2]: combine = weights[0]*d1 + weights[1]*d2, or (d1 + d2)/2 when weights is None."""
    a = np.asarray(d1, np.float32).astype(ft)
    a = a.reshape((-1,) + a.shape[-2:])
    if d2_low is None:
        return [a]
    lo = np.asarray(d2_low, np.float32)
    v = upsample(lo.reshape((-1,) + lo.shape[-2:]), a.shape[1], a.shape[2], ft)
    with np.errstate(invalid="ignore", over="ignore"):
        if weights is None:
            m = (a + v) / ft(2)
        else:
            w = np.asarray(weights, np.float32).astype(ft)
            m = w[0] * a + w[1] * v
    return [m.astype(ft), a, v]


def depth_stats(d1, d2_low, weights, target, min_depth: float = 1e-3, cond=None, n_slots: int = 1, ft=np.float64) -> dict:
    """-> valid / masked / nonfinite [S]; sums [S, NS, 6] (clamped terms, float64 sums, SUMS order), qsums [S, NS, 6] (the terms
    rounded to nearest in units of 2^-20, int64), delta / near [S, NS, 3], saturated [S, NS]."""
    maps = series_maps(d1, d2_low, weights, ft)
    t = np.asarray(target, np.float32).astype(ft).reshape(maps[0].shape)
    md = ft(np.float32(min_depth))
    B, NS = t.shape[0], len(maps)
    fin = np.isfinite(t)
    for p in maps:
        fin &= np.isfinite(p)
    masked = fin & (t < md)
    valid = fin & ~masked
    out = {"valid": np.zeros(n_slots, np.int64), "masked": np.zeros(n_slots, np.int64), "nonfinite": np.zeros(n_slots, np.int64),
           "sums": np.zeros((n_slots, NS, 6)), "qsums": np.zeros((n_slots, NS, 6), np.int64),
           "delta": np.zeros((n_slots, NS, 3), np.int64), "near": np.zeros((n_slots, NS, 3), np.int64),
           "saturated": np.zeros((n_slots, NS), np.int64)}
    for b in range(B):
        slots = [0]
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            slots.append(1 + int(cond[b]))
        ok = valid[b]
        tt = t[b][ok]
        per = {"valid": int(ok.sum()), "masked": int(masked[b].sum()), "nonfinite": int((~fin[b]).sum())}
        for s in slots:
            for k, v in per.items():
                out[k][s] += v
        for i, p in enumerate(maps):
            pp = p[b][ok]
            e = (pp - tt).astype(ft)
            ae, se = np.abs(e), (e * e).astype(ft)
            q = np.maximum(pp, md)
            g = (np.log(q).astype(ft) - np.log(tt).astype(ft)).astype(ft)
            r = np.maximum((q / tt).astype(ft), (tt / q).astype(ft))
            terms = [ae, se, (ae / tt).astype(ft), (se / tt).astype(ft), g, (g * g).astype(ft)]
            sat, sums, qs = 0, [], []
            for x in terms:
                x = x.astype(np.float64)
                over = np.abs(x) > CAP
                sat += int(over.sum())
                x = np.where(over, np.copysign(CAP, x), x)
                sums.append(float(x.sum()))
                qs.append(int(np.rint(x * 2.0 ** 20).astype(np.int64).sum()))
            r64 = r.astype(np.float64)
            dl = [int((r64 < th).sum()) for th in THRESHOLDS]
            nr = [int((np.abs(r64 / th - 1.0) <= 2.0 ** -20).sum()) for th in THRESHOLDS]
            for s in slots:
                out["sums"][s, i] += sums
                out["qsums"][s, i] += qs
                out["delta"][s, i] += dl
                out["near"][s, i] += nr
                out["saturated"][s, i] += sat
    return out


def rows(st: dict) -> np.ndarray:
    """The model's counters in the device layout: int64 [S, 3, 13] (unused series rows zero)."""
    S, NS = st["saturated"].shape
    raw = np.zeros((S, 3, len(FIELDS)), np.int64)
    for i in range(NS):
        raw[:, i, 0], raw[:, i, 1], raw[:, i, 2] = st["valid"], st["masked"], st["nonfinite"]
        raw[:, i, 3:9] = st["qsums"][:, i]
        raw[:, i, 9:12] = st["delta"][:, i]
        raw[:, i, 12] = st["saturated"][:, i]
    return raw


def means(st: dict) -> np.ndarray:
    """sums / valid count, [S, NS, 6] (MEANS order); NaN where a slot has no valid pixel."""
    n = st["valid"].astype(np.float64)[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return st["sums"] / n


def device_means(raw: np.ndarray) -> np.ndarray:
    """The same means from device counters int64 [S, 3, 13]."""
    raw = np.asarray(raw, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return raw[..., 3:9].astype(np.float64) * UNIT / raw[..., 0:1].astype(np.float64)


def metrics(valid: int, sums, delta) -> dict:
    """The host math on float64 sums: the nine metrics of one slot and series."""
    m = np.asarray(sums, np.float64) / valid
    return {"mae": m[0], "rmse": np.sqrt(m[1]), "abs_rel": m[2], "sq_rel": m[3], "rmse_log": np.sqrt(m[5]),
            "silog": np.sqrt(max(m[5] - m[4] ** 2, 0.0)), "delta1": delta[0] / valid, "delta2": delta[1] / valid,
            "delta3": delta[2] / valid}
