"""numpy model of the segment-level counters (include/awseg.h, awseg_segment_stats).

The components come from a union-find over the pairs of 8-adjacent pixels of one class, in two independent forms:
  components         numpy: the pairs as index arrays, then rounds of "compress every path, hook the larger root of every pair under
                     the smaller" until no pair has two roots
  components_python  a per-pixel Python union-find with path halving (small maps only)
Both make the smaller index the parent, so a component's root is its first pixel in raster order: the canonical id y * W + x.
Everything else (areas, hits, coverage cells, size buckets, slots) is integer bookkeeping on those ids.
"""
from __future__ import annotations

import numpy as np

BUCKETS, CELLS = 11, 48


def live_mask(label: np.ndarray, num_classes: int, ignore_index: int = 255) -> np.ndarray:
    l = label.astype(np.int64)
    return (l != ignore_index) & (l >= 0) & (l < num_classes)


def components(cls: np.ndarray) -> np.ndarray:
    """cls int [H, W], < 0 = in no segment -> int32 [H, W]: the canonical id of every pixel's 8-connected component, -1 for none."""
    H, W = cls.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    a_list, b_list = [], []
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        ys, yd = slice(0, H - dy), slice(dy, H)
        xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        same = (cls[ys, xs] == cls[yd, xd]) & (cls[ys, xs] >= 0)
        a_list.append(idx[ys, xs][same])
        b_list.append(idx[yd, xd][same])
    a, b = np.concatenate(a_list), np.concatenate(b_list)
    parent = np.arange(H * W, dtype=np.int64)
    while True:
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        ra, rb = parent[a], parent[b]
        two = ra != rb
        if not two.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[two], np.minimum(ra, rb)[two])
    return np.where(cls >= 0, parent.reshape(H, W), -1).astype(np.int32)


def components_python(cls: np.ndarray) -> np.ndarray:
    H, W = cls.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for y in range(H):
        for x in range(W):
            c = cls[y, x]
            if c < 0:
                continue
            for dy, dx in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and cls[yy, xx] == c:
                    ra, rb = find(y * W + x), find(yy * W + xx)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
    out = np.full((H, W), -1, dtype=np.int32)
    for y in range(H):
        for x in range(W):
            if cls[y, x] >= 0:
                out[y, x] = find(y * W + x)
    return out


def cov(h, area):
    """Coverage cell: 0 when h == 0, else 1 + floor(4 h / A).  Integers or integer arrays."""
    h, area = np.asarray(h, dtype=np.int64), np.asarray(area, dtype=np.int64)
    return np.where(h == 0, 0, 1 + (4 * h) // np.maximum(area, 1))


def bucket(area):
    """Size bucket min(10, floor(log2 A) / 2): bucket k is [4^k, 4^(k+1)), the last one everything from 2^20."""
    area = np.asarray(area, dtype=np.int64)
    s = np.zeros(area.shape, dtype=np.int64)
    for k in range(1, BUCKETS):
        s += area >= 4 ** k
    return s


def _segments(ids: np.ndarray, cls: np.ndarray, *hit_masks):
    """-> (roots, class, area, hits per mask) of the segments of one frame's id map."""
    flat = ids.reshape(-1)
    inside = flat >= 0
    n = flat.size
    area = np.bincount(flat[inside], minlength=n)
    roots = np.nonzero(area)[0]
    hits = [np.bincount(flat[inside], weights=m.reshape(-1)[inside].astype(np.float64), minlength=n).astype(np.int64)[roots] for m in hit_masks]
    return roots, cls.reshape(-1)[roots], area[roots], hits


def segment_counters(pred: np.ndarray, label: np.ndarray, num_classes: int, cond=None, n_slots: int = 1, ref_maps=None, frame_ref=None,
                     ignore_index: int = 255, labeller=components):
    """-> (stats int64 [n_slots, C, 11, 48], oob, label_ids int32 [B, H, W], pred_ids int32 [B, H, W]): what awseg_segment_stats adds
    and writes for these maps."""
    C = int(num_classes)
    B, H, W = pred.shape
    stats = np.zeros((n_slots, C, BUCKETS, CELLS), dtype=np.int64)
    label_ids, pred_ids = np.empty((B, H, W), dtype=np.int32), np.empty((B, H, W), dtype=np.int32)
    oob = 0
    for b in range(B):
        live = live_mask(label[b], C, ignore_index)
        t = np.where(live, label[b].astype(np.int64), -1)
        p = pred[b].astype(np.int64)
        oob += int((live & (p >= C)).sum())
        ref = None
        if ref_maps is not None and frame_ref is not None:
            r = int(frame_ref[b])
            if r >= len(ref_maps):
                oob += H * W
            elif r >= 0:
                ref = ref_maps[r].astype(np.int64)
                oob += int((live & (ref >= C)).sum())
        pc = np.where(live & (p < C), p, -1)
        label_ids[b], pred_ids[b] = labeller(t), labeller(pc)
        one = np.zeros((C, BUCKETS, CELLS), dtype=np.int64)
        hit = live & (p == t)
        masks = (hit,) if ref is None else (hit, live & (ref == t))
        _, cl, area, hits = _segments(label_ids[b], t, *masks)
        rc = 6 if ref is None else cov(hits[1], area)
        np.add.at(one, (cl, bucket(area), cov(hits[0], area) * 7 + rc), 1)
        _, cl, area, hits = _segments(pred_ids[b], pc, hit)
        np.add.at(one, (cl, bucket(area), 42 + cov(hits[0], area)), 1)
        stats[0] += one
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            stats[1 + int(cond[b])] += one
    return stats, oob, label_ids, pred_ids
