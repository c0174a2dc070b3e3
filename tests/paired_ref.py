"""numpy model of the paired severity sweep: the consistency counters awseg_prediction_consistency accumulates,
and the host math the harness derives from them.  Device-agnostic: plain arrays in, plain arrays out."""
from __future__ import annotations

import numpy as np


def consistency_counts(pred, ref, label, num_classes: int, ignore_index: int = 255):
    """(row int64 [C*C + 4], oob) of one set of frames: pred / ref uint8 maps, label the matching label map (any shape, flattened
    together).  A[r*C + p] over every pixel whose two map values are < C; the four transitions (both correct, ref correct + variant
    wrong, ref wrong + variant correct, both wrong) over those pixels whose label is neither ignore_index nor outside [0, C)."""
    C = num_classes
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    r = np.asarray(ref).reshape(-1).astype(np.int64)
    t = np.asarray(label).reshape(-1).astype(np.int64)
    ok = (p < C) & (r < C)
    row = np.zeros(C * C + 4, np.int64)
    row[:C * C] = np.bincount(r[ok] * C + p[ok], minlength=C * C)
    lab = ok & (t != ignore_index) & (t >= 0) & (t < C)
    rc, vc = r[lab] == t[lab], p[lab] == t[lab]
    row[C * C:] = [np.sum(rc & vc), np.sum(rc & ~vc), np.sum(~rc & vc), np.sum(~rc & ~vc)]
    return row, int((~ok).sum())


def consistency_stats(preds, refs, labels, num_classes: int, cond=None, n_slots: int = 1, ignore_index: int = 255, skip=()):
    """int64 [n_slots, C*C + 4] and oob for a batch: frame b into slot 0 and slot 1 + cond[b] (when in range); frames in `skip` are
    left out."""
    stats = np.zeros((n_slots, num_classes * num_classes + 4), np.int64)
    oob = 0
    for b in range(len(preds)):
        if b in skip:
            continue
        row, bad = consistency_counts(preds[b], refs[b], labels[b], num_classes, ignore_index)
        oob += bad
        stats[0] += row
        if cond is not None and 0 <= cond[b] and cond[b] + 1 < n_slots:
            stats[1 + cond[b]] += row
    return stats, oob


def confusion(pred, label, num_classes: int, ignore_index: int = 255, wrap_u8: bool = True):
    """The confusion counters' rule (metrics.py:54-71 with the uint8 index wrap on uint8 labels), flattened [C*C]."""
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    lab = np.asarray(label)
    t = lab.reshape(-1).astype(np.int64)
    keep = t != ignore_index
    base = ((t * num_classes) & 0xFF) if (wrap_u8 and lab.dtype == np.uint8) else t * num_classes
    idx = (base + p)[keep]
    return np.bincount(idx, minlength=num_classes * num_classes)[:num_classes * num_classes].astype(np.int64)
