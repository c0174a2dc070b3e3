"""numpy model of awseg_dehaze_guided (include/awseg_restore.h), built on tests/restore_ref.py for v, A and the
patch minimum e.  The box sums are explicit shifted-slice additions over a zero-padded array, in the header's order (left to right,
then top to bottom): with dtype float32 the kernel has to reproduce every bit.  dtype float64 is the same model in double precision,
for the accuracy comparison.  Importing this file needs no GPU."""
from __future__ import annotations

import numpy as np

from tests import restore_ref as R

ROW = 4
ABOVE_ONE, BELOW_FLOOR, SUM_MOVED, PIXELS = range(ROW)
MAX_RADIUS = 32


def default_guided_radius(radius: int) -> int:
    return min(4 * radius, MAX_RADIUS)


def box_sum(x: np.ndarray, R_: int) -> np.ndarray:
    """S(x): h = ((x[.., x-R] + x[.., x-R+1]) + ...) + x[.., x+R], then S = ((h[y-R] + h[y-R+1]) + ...) + h[y+R]; positions outside the
    frame are +0."""
    h, w = x.shape
    pad = np.zeros((h + 2 * R_, w + 2 * R_), dtype=x.dtype)
    pad[R_:R_ + h, R_:R_ + w] = x
    rows = pad[:, 0:w].copy()
    for k in range(1, 2 * R_ + 1):
        rows = rows + pad[:, k:k + w]
    out = rows[0:h].copy()
    for k in range(1, 2 * R_ + 1):
        out = out + rows[k:k + h]
    return out


def window_count(h: int, w: int, R_: int, dtype) -> np.ndarray:
    """N: (rows of the window inside the frame) * (columns of it inside the frame), exact in float32."""
    y, x = np.arange(h), np.arange(w)
    ny = np.minimum(y + R_, h - 1) - np.maximum(y - R_, 0) + 1
    nx = np.minimum(x + R_, w - 1) - np.maximum(x - R_, 0) + 1
    return (ny[:, None] * nx[None, :]).astype(dtype)


def box_mean(x: np.ndarray, R_: int) -> np.ndarray:
    return box_sum(x, R_) / window_count(*x.shape, R_, x.dtype)


def guided_transmission(v, p, guided_radius, guided_eps, t_min, dtype=np.float32) -> dict:
    """The filter alone, from v [3, H, W] and the raw patch transmission p [H, W] (float32 values, computed on in `dtype`)
    -> {'g', 'var', 'cov', 'a', 'b', 'q', 't'}."""
    c = lambda z: dtype(np.float32(z))                                   # noqa: E731  (a float32 constant, carried in dtype)
    v, p = v.astype(dtype), p.astype(dtype)
    g = (c(0.299) * v[0] + c(0.587) * v[1]) + c(0.114) * v[2]
    mg, mp, mgg, mgp = box_mean(g, guided_radius), box_mean(p, guided_radius), box_mean(g * g, guided_radius), box_mean(g * p, guided_radius)
    var = mgg - mg * mg
    cov = mgp - mg * mp
    a = cov / (var + c(guided_eps))
    b = mp - a * mg
    q = box_mean(a, guided_radius) * g + box_mean(b, guided_radius)
    t = np.fmax(np.fmin(q, dtype(1.0)), c(t_min))
    return {"g": g, "var": var, "cov": cov, "a": a, "b": b, "q": q, "t": t}


def dehaze_guided_frame(frame, mean, std, radius=7, omega=0.95, t_min=0.1, airlight_min=0.1, guided_radius=None, guided_eps=1e-3,
                        dtype=np.float32) -> dict:
    """One frame [3, H, W] -> {'restored', 'airlight', 'row' int64 [8] (the row of restore_ref with the refined t), 'guided_row'
    int64 [ROW], and the intermediates 'v', 'e', 'p', 'g', 'var', 'cov', 'a', 'b', 'q', 't', 't_patch', 'J'}.  v, A and e are float32
    whatever `dtype` is; everything after them is computed in `dtype`."""
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    base = R.dehaze_frame(frame, mean, std, radius=radius, omega=omega, t_min=t_min, airlight_min=airlight_min, refine=0)
    if guided_radius is None:
        guided_radius = default_guided_radius(radius)
    v, A, e = base["v"], base["airlight"], base["e"]
    p = dtype(1.0) - dtype(np.float32(omega)) * e.astype(dtype)
    f = guided_transmission(v, p, guided_radius, guided_eps, t_min, dtype)
    t, q = f["t"], f["q"]
    tm = dtype(np.float32(t_min))
    t_patch = np.fmax(p, tm)
    vd, Ad = v.astype(dtype), A.astype(dtype)
    J = np.stack([np.fmin(np.fmax((vd[c] - Ad[c]) / t + Ad[c], dtype(0)), dtype(1)) for c in range(3)])
    restored = np.stack([(J[c] - dtype(mean[c])) / dtype(std[c]) for c in range(3)])
    row = base["row"].copy()
    row[R.SUM_T] = int(np.rint(t * dtype(65536.0)).astype(np.int64).sum())
    guided_row = np.array([int((q > dtype(1.0)).sum()), int((q < tm).sum()),
                           int(np.rint(np.abs(t - t_patch) * dtype(65536.0)).astype(np.int64).sum()), t.size], dtype=np.int64)
    return {"restored": restored, "airlight": A, "row": row, "guided_row": guided_row, "v": v, "e": e, "p": p, "t_patch": t_patch,
            "J": J, **f}


def dehaze_guided(image, mean=None, std=None, cond=None, n_slots=1, **params):
    """image [B, 3, H, W] -> (restored [B, 3, H, W], airlight [B, 3], t [B, H, W], stats int64 [n_slots, 8], guided_stats int64
    [n_slots, ROW]), float32: frame b into slot 0 and slot 1 + cond[b] when that is a slot."""
    image = np.asarray(image, dtype=np.float32)
    mean = R.IMAGENET_MEAN if mean is None else mean
    std = R.IMAGENET_STD if std is None else std
    restored, airlight = np.empty_like(image), np.empty((image.shape[0], 3), dtype=np.float32)
    t = np.empty((image.shape[0],) + image.shape[2:], dtype=np.float32)
    stats, guided = np.zeros((n_slots, R.ROW), dtype=np.int64), np.zeros((n_slots, ROW), dtype=np.int64)
    for b in range(image.shape[0]):
        f = dehaze_guided_frame(image[b], mean, std, **params)
        restored[b], airlight[b], t[b] = f["restored"], f["airlight"], f["t"]
        slots = [0] + ([1 + int(cond[b])] if cond is not None and 0 <= int(cond[b]) < n_slots - 1 else [])
        for s in slots:
            stats[s] += f["row"]
            guided[s] += f["guided_row"]
    return restored, airlight, t, stats, guided


def depth_step_scene(seed=0, h=64, w=96, spacing=4, airlight=(0.86, 0.88, 0.9), near=0.85, far=0.3):
    """A textured scene J with a zero every `spacing` pixels (the prior holds), and a transmission with a depth step in the middle:
    `near` on the left half, `far` on the right.  -> (I, J, t_true, A), [3, H, W] values in [0, 1] (t_true [H, W])."""
    rng = np.random.default_rng(seed)
    J = (0.15 + 0.6 * rng.random((3, h, w))).astype(np.float32)
    J[:, ::spacing, ::spacing] = 0.0
    t = np.full((h, w), near, dtype=np.float32)
    t[:, w // 2:] = far
    A = np.asarray(airlight, dtype=np.float32)
    I = (J * t + A[:, None, None] * (1.0 - t)).astype(np.float32)
    return I, J, t, A
