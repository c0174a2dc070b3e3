"""Reference model of the failure-detection counters (include/awseg.h): the four uncertainty scores with the
reference's own expressions in torch float64 (and their float32 twin), the bin rule from arithmetic instead of bit patterns, the
histograms per slot, and the monotone sandwich the GPU tests gate on.  No code of the package is used for the model itself."""
import math

import numpy as np
import torch

SCORES = ("mi", "entropy", "variance", "msp")
BINS = 3072
# lower edge of bin b: 2^(-22 + b // 128) * (1 + (b % 128) / 128), exact in float64 (and in float32)
EDGES = np.array([math.ldexp(1.0 + (b % 128) / 128.0, -22 + b // 128) for b in range(BINS)], dtype=np.float64)
# The sandwich is a statement about real numbers; the host function evaluates both of its sides and the device's value as float64
# sums of at most 2 x 3072 terms of magnitude <= 1, each good to 2^-53: 7e-13 in all.  The bounds are compared with that slack.
HOST_EPS = 1e-12
TIE = 1e-4          # top-two margin under which the device may flag a pixel the other way (such pixels are relabelled 255)


def bin_index(values) -> np.ndarray:
    """Bin of real-valued scores: the largest b with EDGES[b] <= s, 0 below the first edge, BINS - 1 from 4.0 up."""
    v = np.asarray(values, dtype=np.float64)
    return np.clip(np.searchsorted(EDGES, v, side="right") - 1, 0, BINS - 1)


# ----------------------------------------------------------------------------- inputs
def random_case(seed, B, C, H, W, scale=2.0):
    """Both members randn * scale, uniform labels, 5 % of them 255."""
    rs = np.random.RandomState(seed)
    s1 = (rs.randn(B, C, H, W) * scale).astype(np.float32)
    s2 = (rs.randn(B, C, H, W) * scale).astype(np.float32)
    label = rs.randint(0, C, (B, H, W)).astype(np.uint8)
    label[rs.rand(B, H, W) < 0.05] = 255
    return s1, s2, label


def trained_like_case(seed, B, C, H, W):
    """A shared one-hot evidence for a class that is the label 85 % of the time, its margin log-uniform over 1..20 (shrunk where
    the class is wrong), plus independent member noise; 5 % of the labels 255.  The scores spread over many octaves and the
    error rate is near 0.2."""
    rs = np.random.RandomState(seed)
    label = rs.randint(0, C, (B, H, W))
    right = rs.rand(B, H, W) < 0.85
    cls = np.where(right, label, (label + rs.randint(1, C, (B, H, W))) % C)
    margin = np.exp(rs.uniform(0.0, np.log(20.0), (B, H, W)))
    margin = np.where(right, margin, 1.0 + 0.3 * (margin - 1.0))
    base = np.zeros((B, C, H, W), dtype=np.float64)
    np.put_along_axis(base, cls[:, None], margin[:, None], axis=1)
    s1 = (base + 0.7 * rs.randn(B, C, H, W)).astype(np.float32)
    s2 = (base + 0.7 * rs.randn(B, C, H, W)).astype(np.float32)
    label = label.astype(np.uint8)
    label[rs.rand(B, H, W) < 0.05] = 255
    return s1, s2, label


def combine(s1, s2, mode, weights=None, temperature=None) -> np.ndarray:
    """r = combine(seg1, seg2)/T in float32, one rounding per operation, as awseg_ensemble_eval_stats forms it.
    mode 'weighted' (weights float32[2]) or 'mean'."""
    s1, s2 = np.asarray(s1, np.float32), np.asarray(s2, np.float32)
    if mode == "weighted":
        w = np.asarray(weights, np.float32)
        r = (w[0] * s1).astype(np.float32) + (w[1] * s2).astype(np.float32)
    else:
        r = (s1 + s2) / np.float32(2)
    if temperature is not None:
        r = r / np.float32(temperature)
    return r.astype(np.float32)


# ----------------------------------------------------------------------------- scores
def _entropy(p):
    return -(p * torch.log(p + 1e-8)).sum(1)


def _top2_margin(v, scale):
    top = torch.topk(v, 2, dim=1).values
    return ((top[:, 0] - top[:, 1]) / scale(top, v)).numpy()


def ensemble_scores(s1, s2, r, dt=torch.float64):
    """The four scores [B, H, W] of the reference's expressions evaluated in `dt`, the two error-free predictions and the relative
    top-two margins of m and r (float64 only)."""
    a, b, rr = (torch.from_numpy(np.ascontiguousarray(x)).to(dt) for x in (s1, s2, r))
    p1, p2 = torch.softmax(a, 1), torch.softmax(b, 1)
    m = (p1 + p2) / 2
    hm = _entropy(m)
    out = {"mi": hm - (_entropy(p1) + _entropy(p2)) / 2, "entropy": hm, "variance": ((p1 - p2) ** 2).sum(1) / 2,
           "msp": 1 - torch.softmax(rr, 1).max(1).values}
    out = {k: v.numpy() for k, v in out.items()}
    out["pred_mean"], out["pred_r"] = m.argmax(1).numpy(), rr.argmax(1).numpy()
    if dt == torch.float64:
        out["margin_mean"] = _top2_margin(m, lambda top, v: top[:, 0])
        out["margin_r"] = _top2_margin(rr, lambda top, v: v.abs().amax(1).clamp_min(1e-300))
    return out


def single_scores(logits, dt=torch.float64):
    x = torch.from_numpy(np.ascontiguousarray(logits)).to(dt)
    p = torch.softmax(x, 1)
    out = {"entropy": _entropy(p).numpy(), "msp": (1 - p.max(1).values).numpy()}
    out["pred_mean"] = out["pred_r"] = x.argmax(1).numpy()
    if dt == torch.float64:
        out["margin_mean"] = out["margin_r"] = _top2_margin(x, lambda top, v: v.abs().amax(1).clamp_min(1e-300))
    return out


def drop_flag_ties(label, sc, limit=1e-3, tie_margin=TIE):
    """Label 255 for pixels whose top two values of m or of r lie within `tie_margin` (relative): the device may flag those the
    other way.  Returns the new label map and the share of pixels removed, which must stay under `limit`."""
    tie = (sc["margin_mean"] <= tie_margin) | (sc["margin_r"] <= tie_margin)
    tie &= label != 255
    out = label.copy()
    out[tie] = 255
    share = float(tie.mean())
    assert share <= limit, f"{share:.4%} of the pixels are flag ties (limit {limit:.2%})"
    return out, share


def share_top_class(s1, s2):
    """s2 with, per pixel, its values at argmax(s2) and at argmax(s1) exchanged: the members keep their own random values and
    margins but name the same class.  For saturated members (logit scale 30), which otherwise give m the value 0.5 twice wherever
    they disagree, with an argmax decided below float32."""
    out = s2.copy()
    a1, a2 = s1.argmax(1)[:, None], s2.argmax(1)[:, None]
    v1, v2 = np.take_along_axis(s2, a1, 1), np.take_along_axis(s2, a2, 1)
    np.put_along_axis(out, a1, v2, 1)
    np.put_along_axis(out, a2, np.where(a1 == a2, v2, v1), 1)
    return out


def deltas(sc64, sc32, label, C, names=SCORES):
    """delta per score: 4 x the largest |float32 twin - float64| over the pixels that count."""
    ok = np.asarray(label).astype(np.int64) < C
    return {k: 4.0 * float(np.abs(sc32[k].astype(np.float64) - sc64[k])[ok].max()) if ok.any() else 0.0 for k in names if k in sc64}


# ----------------------------------------------------------------------------- histograms
def flags(sc, label):
    """error flags [B, H, W] of rows 0-2 (mean probability) and of row 3 (combined logits)."""
    lab = np.asarray(label).astype(np.int64)
    return sc["pred_mean"] != lab, sc["pred_r"] != lab


def slot_masks(B, cond, n_slots):
    """[n_slots, B] bool: which frames a slot holds."""
    m = np.zeros((n_slots, B), dtype=bool)
    m[0] = True
    for b, c in enumerate(cond if cond is not None else []):
        if 0 <= c < n_slots - 1:
            m[1 + c, b] = True
    return m


def model_stats(sc, label, C, cond=None, n_slots=1, finite=None, names=SCORES):
    """{'hist' [slots, 4, 2, BINS], 'pixels', 'nonfinite', 'out_of_range' [slots]} of float64 scores."""
    lab = np.asarray(label).astype(np.int64)
    B = lab.shape[0]
    finite = np.ones(lab.shape, dtype=bool) if finite is None else finite
    in_range = (lab >= 0) & (lab < C)
    counted = in_range & finite
    e_mean, e_r = flags(sc, lab)
    hist = np.zeros((n_slots, len(SCORES), 2, BINS), dtype=np.int64)
    out = {"pixels": np.zeros(n_slots, np.int64), "nonfinite": np.zeros(n_slots, np.int64), "out_of_range": np.zeros(n_slots, np.int64)}
    for s, frames in enumerate(slot_masks(B, cond, n_slots)):
        sel = counted & frames[:, None, None]
        out["pixels"][s] = sel.sum()
        out["nonfinite"][s] = (in_range & ~finite & frames[:, None, None]).sum()
        out["out_of_range"][s] = (~in_range & (lab != 255) & frames[:, None, None]).sum()
        for i, name in enumerate(SCORES):
            if name not in names or name not in sc:
                continue
            err = (e_r if name == "msp" else e_mean)[sel]
            b = bin_index(sc[name][sel])
            for f in (0, 1):
                hist[s, i, f] = np.bincount(b[err == bool(f)], minlength=BINS)
    out["hist"] = hist
    return out


def count_below(values, thresholds) -> np.ndarray:
    """how many of `values` are < each threshold."""
    return np.searchsorted(np.sort(np.asarray(values, dtype=np.float64)), np.asarray(thresholds, dtype=np.float64), side="left")


def hist_of(score, wrong):
    """[2, BINS] of real-valued scores and their error flags."""
    b = bin_index(score)
    return np.stack([np.bincount(b[~wrong], minlength=BINS), np.bincount(b[wrong], minlength=BINS)])


def sandwich(score, wrong, delta, metrics_from_hist):
    """Binning is monotone; auroc cannot fall when a wrong pixel's score rises or a right pixel's falls, and aurc cannot rise.
    -> {'auroc': (lo, hi), 'aurc': (lo, hi)} over every score field within +-delta of `score`."""
    sign = np.where(wrong, 1.0, -1.0)
    up = metrics_from_hist(*hist_of(score + delta * sign, wrong))        # errors look as uncertain as they can
    dn = metrics_from_hist(*hist_of(score - delta * sign, wrong))
    return {"auroc": (dn["auroc"], up["auroc"]), "aurc": (up["aurc"], dn["aurc"])}


def exact_aurc(score, wrong) -> float:
    """The mean of the running risk over the pixels kept in ascending score order (stable sort)."""
    order = np.argsort(score, kind="stable")
    w = wrong[order].astype(np.float64)
    return float((np.cumsum(w) / np.arange(1, w.size + 1)).mean())
