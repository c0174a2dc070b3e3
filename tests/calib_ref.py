"""Float64 models of the streamed temperature calibration (csrc/calib.hip, ops.temperature_grid_stats).

`grid_stats_f64` computes, for logits r (the float32 values the ECE sees) and every grid temperature, what the device
accumulates — per slot and temperature the pixel count, the per-pixel NLL (clamped at the cap, saturations counted) and
the ECE bins {count, sum conf, sum correct} — in float64, and marks the pixels whose float64 confidence lies within
`edge_ulps` float32 ulps of a bin edge (the only pixels whose bin a float32 computation may legitimately change).
"""
from __future__ import annotations

import numpy as np

NLL_CAP = 2048.0
NLL_UNIT = 2.0 ** -20


def ulp32(x) -> np.ndarray:
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def _flat(r, y, cond, n_slots):
    r = np.asarray(r)
    b, c = r.shape[:2]
    rr = r.reshape(b, c, -1).transpose(0, 2, 1).reshape(-1, c)                      # [pixels, C]
    yy = np.asarray(y).reshape(b, -1).astype(np.int64).reshape(-1)
    img = np.repeat(np.arange(b), rr.shape[0] // b)
    slot = np.full(b, -1) if cond is None else np.array([1 + int(v) if 0 <= int(v) < n_slots - 1 else -1 for v in cond])
    return rr, yy, img, slot[img]


def grid_stats_f64(r, y, temps, edges, cond=None, n_slots: int = 1, edge_ulps: float = 8.0) -> dict:
    """r [B,C,H,W] (float32 values), y [B,H,W]; returns count/nll_sum/nll_exact/saturated [S,K], bins count/sum_conf/correct
    [S,K,nb], near_edge [S,K], out_of_range [S].  nll_sum is the clamped float64 sum, nll_exact the unclamped one."""
    rr, yy, img, pslot = _flat(r, y, cond, n_slots)
    edges = np.asarray(edges, np.float32).astype(np.float64)
    nb = len(edges) - 1
    temps = np.asarray(temps, np.float32).astype(np.float64)
    K, C = len(temps), rr.shape[1]
    valid = yy != 255
    nll_ok = valid & (yy >= 0) & (yy < C)
    pred = rr.argmax(axis=1)                                     # first maximum of the float32 values
    correct = pred == yy
    r64 = rr.astype(np.float64)
    out = {k: np.zeros((n_slots, K)) for k in ("count", "nll_sum", "nll_exact", "saturated", "near_edge")}
    out.update({k: np.zeros((n_slots, K, nb)) for k in ("bin_count", "bin_conf", "bin_correct")})
    out["out_of_range"] = np.zeros(n_slots)
    slots = [np.ones_like(valid)] + [pslot == s for s in range(1, n_slots)]
    for s, in_s in enumerate(slots):
        out["out_of_range"][s] = np.sum(in_s & valid & ~nll_ok)
    for k, t in enumerate(temps):
        z = r64 / t
        zm = z.max(axis=1, keepdims=True)
        e = np.exp(z - zm)
        se = e.sum(axis=1)
        conf = 1.0 / se
        zy = np.take_along_axis(z - zm, np.clip(yy, 0, C - 1)[:, None], axis=1)[:, 0]
        nll = np.log(se) - zy
        b = np.searchsorted(edges, conf, side="left") - 1             # edges[b] < conf <= edges[b+1]
        inb = valid & (b >= 0) & (b < nb)
        gap = np.min(np.abs(conf[:, None] - edges[None, :]) / ulp32(edges)[None, :].clip(min=2.0 ** -149), axis=1)
        near = gap <= edge_ulps
        for s, in_s in enumerate(slots):
            m = in_s & nll_ok
            out["count"][s, k] = m.sum()
            out["nll_exact"][s, k] = nll[m].sum()
            out["nll_sum"][s, k] = np.minimum(nll[m], NLL_CAP).sum()
            out["saturated"][s, k] = np.sum(nll[m] > NLL_CAP)
            mb = in_s & inb
            out["bin_count"][s, k] = np.bincount(b[mb], minlength=nb)
            out["bin_conf"][s, k] = np.bincount(b[mb], weights=conf[mb], minlength=nb)
            out["bin_correct"][s, k] = np.bincount(b[mb], weights=correct[mb].astype(np.float64), minlength=nb)
            out["near_edge"][s, k] = np.sum(in_s & valid & near)
    return out


def mean_nll(ref: dict) -> np.ndarray:
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ref["count"] > 0, ref["nll_sum"] / np.maximum(ref["count"], 1), np.nan)


def ece_f64(ref: dict, s: int, k: int) -> float:
    n = ref["bin_count"][s, k]
    tot = n.sum()
    if tot == 0:
        return 0.0
    nz = n > 0
    return float(np.sum(np.abs(ref["bin_conf"][s, k][nz] / n[nz] - ref["bin_correct"][s, k][nz] / n[nz]) * n[nz] / tot))


def nll_gate(e_twin32: float) -> float:
    """|device - f64| bound of a grid point's mean NLL: 4x what float32 torch makes of the same quantity, plus one
    fixed-point unit."""
    return 4.0 * e_twin32 + NLL_UNIT
