"""Numpy model of the frame bootstrap (include/awseg.h): per-frame IoU counters, the Philox draw rule and the
replicate sums, written from the header's text and independent of the package's code.  Everything is an integer: the device must
equal it exactly."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM = 0x0B07
MASK = 0xFFFFFFFF


def philox4x32_7(seed, ctr, stream=STREAM):
    """Philox4x32 with 7 rounds on counter words (ctr lo, ctr hi, stream, 0x9E3779B9) and key (seed lo, seed hi) -> uint32 [..., 4].
    `ctr` may be an array of uint64 counters."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0 = ctr & np.uint64(MASK)
    c1 = ctr >> np.uint64(32)
    c2 = np.full_like(c0, stream)
    c3 = np.full_like(c0, W0)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(7):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                 # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def draws(seed, q, n):
    """The n source indices of replicate q: draw j = (word j % 4 of call q * ceil(n / 4) + j // 4) * n >> 32."""
    n4 = (n + 3) // 4
    ctr = (np.uint64(q) * np.uint64(n4) + np.arange(n4, dtype=np.uint64)) if n4 else np.zeros(0, np.uint64)
    u = philox4x32_7(seed, ctr).reshape(-1)[:n].astype(np.uint64)
    return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def frame_counts(pred, label, num_classes, frame_row, n_rows, ignore_index=255, table=None):
    """-> (table int64 [n_rows, 3 C], oob).  pred uint8 [B, ...], label integer [B, ...]."""
    c = int(num_classes)
    table = np.zeros((n_rows, 3 * c), np.int64) if table is None else table.copy()
    oob = 0
    for b in range(pred.shape[0]):
        p = pred[b].reshape(-1).astype(np.int64)
        t = label[b].reshape(-1).astype(np.int64)
        r = int(frame_row[b])
        if r < 0:
            continue
        if r >= n_rows:
            oob += p.size
            continue
        labelled = (t != ignore_index) & (t >= 0) & (t < c)
        oob += int((p >= c).sum()) + int((~labelled & (t != ignore_index)).sum())
        keep = labelled & (p < c)
        p, t = p[keep], t[keep]
        table[r, :c] += np.bincount(t[p == t], minlength=c)
        table[r, c:2 * c] += np.bincount(t, minlength=c)
        table[r, 2 * c:] += np.bincount(p, minlength=c)
    return table, oob


def slot_oob(slots, n_slots):
    s = np.asarray(slots)
    return int(((s < 0) | (s >= n_slots)).sum())


def replicate_sums_loop(table, slots, n_slots, seed, r0, R):
    """The definition, draw by draw: int64 [R, n_slots, W]."""
    table, slots = np.asarray(table, np.int64), np.asarray(slots)
    n, V, W = table.shape
    out = np.zeros((R, n_slots, W), np.int64)
    for r in range(R):
        for i in draws(seed, r0 + r, n):
            for v in range(V):
                s = int(slots[i, v])
                if 1 <= s < n_slots:
                    out[r, 0] += table[i, v]
                    out[r, s] += table[i, v]
    return out


def replicate_sums(table, slots, n_slots, seed, r0, R):
    """The same through multiplicities: per-source slot sums [n, n_slots, W], then (times each source was drawn) . sums.  Python
    integers would be exact at any size; int64 is what the device holds, and the tests stay far below 2^63."""
    table, slots = np.asarray(table, np.int64), np.asarray(slots)
    n, V, W = table.shape
    per = np.zeros((n, n_slots, W), np.int64)
    for v in range(V):
        s = slots[:, v].astype(np.int64)
        ok = (s >= 1) & (s < n_slots)
        idx = np.nonzero(ok)[0]
        np.add.at(per, (idx, s[idx]), table[idx, v])
        per[idx, 0] += table[idx, v]
    out = np.zeros((R, n_slots, W), np.int64)
    for r in range(R):
        mult = np.bincount(draws(seed, r0 + r, n), minlength=n).astype(np.int64)
        out[r] = np.tensordot(mult, per, axes=(0, 0))
    return out


def confusion(pred, label, num_classes, ignore_index=255):
    """An independent C x C confusion matrix (rows: label) of the labelled pixels with a prediction < C."""
    c = int(num_classes)
    cm = np.zeros((c, c), np.int64)
    p, t = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(label).reshape(-1).astype(np.int64)
    for a, b in zip(t, p):
        if a != ignore_index and 0 <= a < c and b < c:
            cm[a, b] += 1
    return cm
