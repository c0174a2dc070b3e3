"""numpy model of the change strata: the stratum map awseg_change_strata writes, the counters
awseg_stratified_stats accumulates, and the host math the harness derives from them.  Written from include/awseg.h, not from the HIP
code.  Device-agnostic: plain arrays in, plain arrays out.  Helpers only."""
from __future__ import annotations

import numpy as np

NONE = 255
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
DEFAULT_SCALE = (np.float32(255.0) * IMAGENET_STD).astype(np.float32)


def change_map(image, ref, scale):
    """(change float32 [hw], nan bool [hw]) of one frame: image, ref float32 [Ch, hw]; max over channels of |image - ref| * scale
    in float32, one rounding per operation."""
    image, ref = np.asarray(image, np.float32), np.asarray(ref, np.float32)
    scale = np.asarray(scale, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = image - ref                                               # float32 - float32 -> float32
        nan = np.isnan(d).any(axis=0)
        v = np.abs(d) * scale[:, None]
    v = np.where(np.isnan(v), np.float32(0), v)                       # (only where `nan` is set)
    return v.max(axis=0).astype(np.float32), nan


def change_strata(image, refs, frame_ref, edges, scale=None):
    """(uint8 [B, hw], oob): the vectorised formulation.  image float32 [B, Ch, hw], refs float32 [R, Ch, hw]."""
    image, refs = np.asarray(image, np.float32), np.asarray(refs, np.float32)
    edges = np.asarray(edges, np.float32)
    scale = DEFAULT_SCALE if scale is None else np.asarray(scale, np.float32)
    B, _, hw = image.shape
    out = np.full((B, hw), NONE, np.uint8)
    oob = 0
    for b in range(B):
        r = int(frame_ref[b])
        if r < 0:
            continue
        if r >= refs.shape[0]:
            oob += hw
            continue
        m, nan = change_map(image[b], refs[r], scale)
        s = (m[:, None] >= edges[None, :]).sum(axis=1).astype(np.uint8)
        out[b] = np.where(nan, NONE, s)
    return out, oob


def change_strata_loop(image, refs, frame_ref, edges, scale=None):
    """The same, one pixel at a time with scalar float32 arithmetic."""
    image, refs = np.asarray(image, np.float32), np.asarray(refs, np.float32)
    scale = DEFAULT_SCALE if scale is None else np.asarray(scale, np.float32)
    B, Ch, hw = image.shape
    out = np.full((B, hw), NONE, np.uint8)
    oob = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            r = int(frame_ref[b])
            if r < 0:
                continue
            if r >= refs.shape[0]:
                oob += hw
                continue
            for p in range(hw):
                m, nan = np.float32(0), False
                for c in range(Ch):
                    d = np.float32(image[b, c, p]) - np.float32(refs[r, c, p])
                    if d != d:
                        nan = True
                        continue
                    v = np.float32(abs(d)) * np.float32(scale[c])
                    if v > m:
                        m = v
                out[b, p] = NONE if nan else sum(1 for e in edges if m >= np.float32(e))
    return out, oob


def row_len(C):
    return C * C + 6


def stratified_counts(pred, label, stratum, K, C, ref=None, ignore_index=255):
    """(int64 [K + 1, C*C + 6], oob) of one set of pixels (any shape, flattened together): the vectorised formulation.  ref None:
    the paired cells and `agree` stay 0."""
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    t = np.asarray(label).reshape(-1).astype(np.int64)
    s = np.minimum(np.asarray(stratum).reshape(-1).astype(np.int64), K)
    ok = p < C
    r = None
    if ref is not None:
        r = np.asarray(ref).reshape(-1).astype(np.int64)
        ok &= r < C
    rows = np.zeros((K + 1, row_len(C)), np.int64)
    lab = ok & (t != ignore_index) & (t >= 0) & (t < C)
    rows[:, :C * C] = np.bincount((s[lab] * C + t[lab]) * C + p[lab], minlength=(K + 1) * C * C).reshape(K + 1, C * C)
    rows[:, C * C + 5] = np.bincount(s[ok], minlength=K + 1)
    if r is not None:
        code = 2 * (r[lab] != t[lab]) + (p[lab] != t[lab])            # both correct, ref correct + variant wrong, ...
        rows[:, C * C:C * C + 4] = np.bincount(s[lab] * 4 + code, minlength=(K + 1) * 4).reshape(K + 1, 4)
        rows[:, C * C + 4] = np.bincount(s[ok & (p == r)], minlength=K + 1)
    return rows, int((~ok).sum())


def stratified_counts_loop(pred, label, stratum, K, C, ref=None, ignore_index=255):
    """The same, one pixel at a time."""
    p, t, s = (np.asarray(a).reshape(-1) for a in (pred, label, stratum))
    r = None if ref is None else np.asarray(ref).reshape(-1)
    rows = np.zeros((K + 1, row_len(C)), np.int64)
    oob = 0
    for i in range(p.size):
        pi, ti, k = int(p[i]), int(t[i]), min(int(s[i]), K)
        if pi >= C or (r is not None and int(r[i]) >= C):
            oob += 1
            continue
        rows[k, C * C + 5] += 1
        if r is not None and int(r[i]) == pi:
            rows[k, C * C + 4] += 1
        if ti == ignore_index or ti < 0 or ti >= C:
            continue
        rows[k, ti * C + pi] += 1
        if r is not None:
            rows[k, C * C + (0 if int(r[i]) == ti else 2) + (0 if pi == ti else 1)] += 1
    return rows, oob


def stratified_stats(preds, labels, strata, K, C, refs=None, frame_ref=None, cond=None, n_slots=1, ignore_index=255, counts=stratified_counts):
    """int64 [n_slots, K + 1, C*C + 6] and oob for a batch: frame b against row frame_ref[b] of refs (< 0: skipped; >= len(refs): not
    counted, its pixels added to oob; refs None: every frame counted unpaired), into slot 0 and slot 1 + cond[b] when in range."""
    stats = np.zeros((n_slots, K + 1, row_len(C)), np.int64)
    oob = 0
    for b in range(len(preds)):
        ref = None
        if refs is not None:
            r = int(frame_ref[b])
            if r < 0:
                continue
            if r >= len(refs):
                oob += int(np.asarray(preds[b]).size)
                continue
            ref = refs[r]
        rows, bad = counts(preds[b], labels[b], strata[b], K, C, ref=ref, ignore_index=ignore_index)
        oob += bad
        stats[0] += rows
        if cond is not None and 0 <= cond[b] and cond[b] + 1 < n_slots:
            stats[1 + cond[b]] += rows
    return stats, oob


def _miou64(conf):
    """mIoU of a confusion matrix in float64 over the classes with a non-empty union."""
    conf = np.asarray(conf, np.float64)
    inter = np.diag(conf)
    union = conf.sum(0) + conf.sum(1) - inter
    seen = union > 0
    return float((inter[seen] / union[seen]).mean())


def metrics_from_masks(pred, label, stratum, ref, K, C, ignore_index=255):
    """The per-stratum quantities straight from the maps (no counters, no oob values expected): {metric: {k: value}}, float64."""
    p, t, s, r = (np.asarray(a).reshape(-1).astype(np.int64) for a in (pred, label, stratum, ref))
    s = np.minimum(s, K)
    lab = (t != ignore_index) & (t >= 0) & (t < C)
    new_err = lab & (r == t) & (p != t)
    out = {m: {} for m in ("change_fraction", "miou", "accuracy", "consistency", "corruption_error_rate", "corruption_error_share")}
    for k in range(K):
        sel = s == k
        out["change_fraction"][k] = sel.sum() / p.size
        sl = sel & lab
        if sl.any():
            conf = np.zeros((C, C))
            np.add.at(conf, (t[sl], p[sl]), 1)
            out["miou"][k] = _miou64(conf)
            out["accuracy"][k] = (p[sl] == t[sl]).mean()
        if sel.any():
            out["consistency"][k] = (p[sel] == r[sel]).mean()
        right = sl & (r == t)
        if right.any():
            out["corruption_error_rate"][k] = (p[right] != t[right]).mean()
        if new_err.any():
            out["corruption_error_share"][k] = (new_err & sel).sum() / new_err.sum()
    return out
