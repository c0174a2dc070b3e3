"""numpy model of the boundary-band counters (include/awseg.h, awseg_boundary_stats).

Two independent formulations of the ring of a pixel's edge distance, plus a third where scipy imports:
  rings_direct     for every offset of the (2 d_n + 1)^2 window a shifted comparison; the edge distance is the smallest Chebyshev
                   length of an offset whose pixel is valid and differs
  rings_separable  per width, the window min and max over the valid values (rows, then columns) against the pixel's own value
  rings_scipy      the same min / max through scipy.ndimage on neutral-filled maps
All take maps [B, H, W] with a validity mask and return int [B, H, W]: ring k < n when d_(k-1) < e <= d_k, n for the interior (only
meaningful where the pixel itself is valid).
"""
from __future__ import annotations

import numpy as np

BIG = 1 << 14            # neutral for min; -1 is neutral for max (classes are 0 .. 31)


def label_valid(label: np.ndarray, num_classes: int, ignore_index: int = 255) -> np.ndarray:
    l = label.astype(np.int64)
    return (l != ignore_index) & (l >= 0) & (l < num_classes)


def pred_valid(pred: np.ndarray, num_classes: int) -> np.ndarray:
    return pred.astype(np.int64) < num_classes


def rings_direct(m: np.ndarray, valid: np.ndarray, widths) -> np.ndarray:
    widths = [int(d) for d in widths]
    B, H, W = m.shape
    m = m.astype(np.int64)
    R = widths[-1]
    e = np.full((B, H, W), R + 1, dtype=np.int64)                     # R + 1 stands for "beyond the widest band"
    for dy in range(-R, R + 1):
        ys, yd = slice(max(0, dy), min(H, H + dy)), slice(max(0, -dy), min(H, H - dy))       # q = p + (dy, dx): q in ys, p in yd
        if ys.start >= ys.stop:
            continue
        for dx in range(-R, R + 1):
            xs, xd = slice(max(0, dx), min(W, W + dx)), slice(max(0, -dx), min(W, W - dx))
            if xs.start >= xs.stop or (dy == 0 and dx == 0):
                continue
            diff = valid[:, ys, xs] & (m[:, ys, xs] != m[:, yd, xd])
            view = e[:, yd, xd]
            np.minimum(view, np.where(diff, max(abs(dy), abs(dx)), R + 1), out=view)
    return np.searchsorted(np.asarray(widths), e, side="left")        # smallest k with e <= d_k; n when e > d_n


def _window(a: np.ndarray, d: int, axis: int, fn, fill: int) -> np.ndarray:
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (d, d)
    p = np.pad(a, pad, constant_values=fill)
    out = None
    for s in range(2 * d + 1):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(s, s + n)
        out = p[tuple(sl)].copy() if out is None else fn(out, p[tuple(sl)], out=out)
    return out


def rings_separable(m: np.ndarray, valid: np.ndarray, widths) -> np.ndarray:
    widths = [int(d) for d in widths]
    v = m.astype(np.int16)
    lo, hi = np.where(valid, v, np.int16(BIG)), np.where(valid, v, np.int16(-1))
    ring = np.full(m.shape, len(widths), dtype=np.int64)
    for d in widths:
        mn = _window(_window(lo, d, 2, np.minimum, BIG), d, 1, np.minimum, BIG)
        mx = _window(_window(hi, d, 2, np.maximum, -1), d, 1, np.maximum, -1)
        ring -= ((mn < v) | (mx > v))
    return ring


def rings_scipy(m: np.ndarray, valid: np.ndarray, widths) -> np.ndarray:
    from scipy import ndimage
    widths = [int(d) for d in widths]
    v = m.astype(np.int32)
    lo, hi = np.where(valid, v, BIG), np.where(valid, v, -1)
    ring = np.full(m.shape, len(widths), dtype=np.int64)
    for d in widths:
        size = (1, 2 * d + 1, 2 * d + 1)                              # frames never see each other
        mn = ndimage.minimum_filter(lo, size=size, mode="constant", cval=BIG)
        mx = ndimage.maximum_filter(hi, size=size, mode="constant", cval=-1)
        ring -= ((mn < v) | (mx > v))
    return ring


def boundary_counters(pred: np.ndarray, label: np.ndarray, widths, num_classes: int, cond=None, n_slots: int = 1,
                      ignore_index: int = 255, rings=rings_separable):
    """-> (stats int64 [n_slots, n + 1, C*C + 2 C], oob): the counters awseg_boundary_stats adds for these maps."""
    C, n = int(num_classes), len(widths)
    lv, pv = label_valid(label, C, ignore_index), pred_valid(pred, C)
    t = np.where(lv, label.astype(np.int64), 0)
    p = np.where(pv, pred.astype(np.int64), 0)
    rl, rp = rings(t, lv, widths), rings(p, pv, widths)
    row = C * C + 2 * C
    stats = np.zeros((n_slots, n + 1, row), dtype=np.int64)
    oob = int((lv & ~pv).sum())
    for b in range(pred.shape[0]):
        k = lv[b] & pv[b]
        tb, pb, rlb, rpb = t[b][k], p[b][k], rl[b][k], rp[b][k]
        one = np.zeros((n + 1) * row, dtype=np.int64)
        np.add.at(one, rlb * row + tb * C + pb, 1)
        np.add.at(one, rpb * row + C * C + C + pb, 1)
        eq = tb == pb
        np.add.at(one, np.maximum(rlb, rpb)[eq] * row + C * C + tb[eq], 1)
        one = one.reshape(n + 1, row)
        stats[0] += one
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            stats[1 + int(cond[b])] += one
    return stats, oob


def band_mask(m: np.ndarray, valid: np.ndarray, d: int, rings=rings_separable) -> np.ndarray:
    """Valid pixels with edge distance <= d."""
    return valid & (rings(m, valid, [d]) == 0)


def metrics_from_masks(pred: np.ndarray, label: np.ndarray, widths, num_classes: int, ignore_index: int = 255) -> dict:
    """boundary_miou / accuracy / iou / fraction per width and interior_miou straight from band masks (no counters)."""
    C = int(num_classes)
    lv, pv = label_valid(label, C, ignore_index), pred_valid(pred, C)
    assert not (lv & ~pv).any()
    t, p = np.where(lv, label.astype(np.int64), 0), np.where(pv, pred.astype(np.int64), 0)

    def miou(mask):
        ious = []
        for c in range(C):
            union = (mask & ((t == c) | (p == c))).sum()
            if union:
                ious.append((mask & (t == c) & (p == c)).sum() / union)
        return float(np.mean(ious))
    res = {}
    for d in widths:
        gb, pb = band_mask(t, lv, d, rings_direct), band_mask(p, pv, d, rings_direct) & lv
        res[f"boundary_fraction_w{d}"] = float(gb.sum() / lv.sum())
        res[f"boundary_miou_w{d}"] = miou(gb)
        res[f"boundary_accuracy_w{d}"] = float((gb & (t == p)).sum() / gb.sum())
        ious = []
        for c in range(C):
            g, q = gb & (t == c), pb & (p == c)
            if (g | q).sum():
                ious.append((g & q).sum() / (g | q).sum())
        res[f"boundary_iou_w{d}"] = float(np.mean(ious))
    inner = lv & ~band_mask(t, lv, widths[-1], rings_direct)
    if inner.any():
        res["interior_miou"] = miou(inner)
    return res
