"""Reference model of the ensemble weight sweep's counters (include/awseg.h) in numpy: the weighted combine as two
float32 products and one float32 sum evaluated elementwise, torch's argmax rule written out class by class, and every counter of
every slot.  No code of the package is used for the model itself."""
import numpy as np

C19 = 19


def argmax_rule(v) -> np.ndarray:
    """torch's argmax along axis 1 written out: walk the classes in order and take v[c] when it is greater than the best so far,
    or when it is a NaN and the best is not -- the first maximum, a NaN wins (and the first NaN stays)."""
    v = np.asarray(v)
    best = v[:, 0].copy()
    arg = np.zeros(best.shape, dtype=np.int64)
    for c in range(1, v.shape[1]):
        with np.errstate(invalid="ignore"):
            take = ~(v[:, c] <= best) & ~np.isnan(best)
        best = np.where(take, v[:, c], best)
        arg = np.where(take, c, arg)
    return arg


def combine(s1, s2, w0, w1) -> np.ndarray:
    """w0 * s1 + w1 * s2 in float32, every product and the sum rounded on its own (0 * inf is NaN, as on the device)."""
    s1, s2 = np.asarray(s1, np.float32), np.asarray(s2, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (np.float32(w0) * s1).astype(np.float32)
        q = (np.float32(w1) * s2).astype(np.float32)
        return (u + q).astype(np.float32)


def slot_masks(B, cond, n_slots) -> np.ndarray:
    """[n_slots, B] bool: slot 0 holds every frame, slot 1 + cond[b] frame b when 0 <= cond[b] < n_slots - 1."""
    m = np.zeros((n_slots, B), dtype=bool)
    m[0] = True
    for b, c in enumerate(cond if cond is not None else []):
        if 0 <= c < n_slots - 1:
            m[1 + c, b] = True
    return m


def counters(s1, s2, weights, label, cond=None, n_slots=1, ignore_index=255) -> np.ndarray:
    """int64 [n_slots, G + 3, 2 C] for members [B, C, ...] float32, weights [G, 2] float32 and labels [B, ...] of any integer type."""
    s1, s2 = np.asarray(s1, np.float32), np.asarray(s2, np.float32)
    B, C = s1.shape[:2]
    s1, s2 = s1.reshape(B, C, -1), s2.reshape(B, C, -1)
    w = np.asarray(weights, np.float32).reshape(-1, 2)
    G = w.shape[0]
    lab = np.asarray(label).astype(np.int64).reshape(B, -1)
    in_range = (lab >= 0) & (lab < C)
    labelled = in_range & (lab != ignore_index)
    stray = ~in_range & (lab != ignore_index)
    m1, m2 = argmax_rule(s1), argmax_rule(s2)
    nan = np.isnan(s1).any(axis=1) | np.isnan(s2).any(axis=1)
    preds = [argmax_rule(combine(s1, s2, w[g, 0], w[g, 1])) for g in range(G)]
    out = np.zeros((n_slots, G + 3, 2 * C), dtype=np.int64)

    def per_class(mask):
        return np.bincount(lab[mask], minlength=C)[:C]
    for s, frames in enumerate(slot_masks(B, cond, n_slots)):
        sel = labelled & frames[:, None]
        for g in range(G):
            out[s, g, :C] = per_class(sel & (preds[g] == lab))
            out[s, g, C:] = np.bincount(preds[g][sel], minlength=C)
        r1, r2 = m1 == lab, m2 == lab
        out[s, G, :C] = per_class(sel)
        out[s, G, C:] = per_class(sel & r1 & r2)
        out[s, G + 1, :C] = per_class(sel & r1 & ~r2)
        out[s, G + 1, C:] = per_class(sel & ~r1 & r2)
        out[s, G + 2, 0] = (stray & frames[:, None]).sum()
        out[s, G + 2, 1] = (sel & nan).sum()
        out[s, G + 2, 2] = (sel & (m1 != m2)).sum()
    return out


def miou(inter, lab, prd) -> float:
    """The mean over the classes with a non-empty union of I / (L + P - I), in the float32 arithmetic that yields the pooled mIoU
    from a confusion matrix: int64 operands converted to float32, divided, and averaged in float32."""
    i, l, p = (np.asarray(v, dtype=np.int64) for v in (inter, lab, prd))
    union = l + p - i
    valid = union > 0
    per = i[valid].astype(np.float32) / union[valid].astype(np.float32)
    return float(per.mean(dtype=np.float32))


def eighths_case(seed, B, hw, dtype=np.uint8, C=C19, specials=True):
    """Members drawn as multiples of 1/8 in [-2, 2] (exact ties between classes and between members are frequent), labels uniform
    with about 5 % 255 and a few out-of-range values (19, 200; -1 for int64), and, with `specials`, a few pixels that carry a NaN,
    +inf or -inf in one member or both (among them +inf in one member against -inf in the other at the same class)."""
    rs = np.random.RandomState(seed)
    s1 = (rs.randint(-16, 17, (B, C, hw)) / 8.0).astype(np.float32)
    s2 = (rs.randint(-16, 17, (B, C, hw)) / 8.0).astype(np.float32)
    label = rs.randint(0, C, (B, hw)).astype(dtype)
    label[rs.rand(B, hw) < 0.05] = 255
    stray = [19, 200] + ([-1] if dtype == np.int64 else [])
    for k, v in enumerate(stray):
        label[(k * 3) % B, (5 * k + 1) % hw] = v
    if specials:
        # (value in SegFormer, value in DeepLab, same class?) per special pixel; None: the member keeps its draw.  The first four
        # already hold NaN, +inf and -inf in both members, so a 4-pixel frame carries them all
        patterns = [(np.inf, -np.inf, True), (np.nan, np.inf, False), (-np.inf, np.nan, False), (np.inf, None, False),
                    (None, np.inf, False), (np.nan, None, False), (None, -np.inf, False), (-np.inf, np.inf, True),
                    (np.inf, np.inf, True), (None, np.nan, False), (-np.inf, None, False), (np.nan, np.nan, True)]
        for k in range(min(len(patterns), hw)):
            v1, v2, same_class = patterns[k]
            b, c, p = k % B, (7 * k) % C, (k * 11 + 2) % hw
            if v1 is not None:
                s1[b, c, p] = v1
            if v2 is not None:
                s2[b, c if same_class else (c + k + 1) % C, p] = v2
    return s1, s2, label
