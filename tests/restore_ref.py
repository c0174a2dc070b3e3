"""numpy float32 model of awseg_dehaze (include/awseg_restore.h), written without the kernel's tiling: every window
is taken directly over its (2r+1)^2 positions, clipped to the frame.  One float32 operation per step in the header's order, so the
kernel has to reproduce every bit.  Importing this file needs no GPU."""
from __future__ import annotations

import numpy as np

ROW = 8
FRAMES, SUM_A0, SUM_A1, SUM_A2, PIXELS, SUM_T, NONFINITE, FLOORED = range(ROW)
UNIT = 2.0 ** -16
Q16 = np.float32(65536.0)
ZERO, ONE = np.float32(0.0), np.float32(1.0)
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def window(a: np.ndarray, r: int, op, outside) -> np.ndarray:
    """op (np.fmin / np.fmax) over the (2r+1)^2 window of every position of the last two axes; positions outside the frame hold
    `outside`, the value that takes part in nothing."""
    h, w = a.shape[-2:]
    pad = np.full(a.shape[:-2] + (h + 2 * r, w + 2 * r), outside, dtype=np.float32)
    pad[..., r:r + h, r:r + w] = a
    out = a.astype(np.float32, copy=True)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = op(out, pad[..., dy:dy + h, dx:dx + w])
    return out


def erode(a, r):
    return window(a, r, np.fmin, np.float32(np.inf))


def dilate(a, r):
    return window(a, r, np.fmax, np.float32(-np.inf))


def opening(a, r):
    return dilate(erode(a, r), r)


def n_top(hw: int) -> int:
    return (int(hw) + 999) // 1000


def b_star(hist, top: int) -> int:
    """The largest bin whose suffix sum reaches `top`."""
    suffix = np.cumsum(np.asarray(hist, dtype=np.int64)[::-1])[::-1]
    return int(np.nonzero(suffix >= top)[0].max())


def unit(frame, mean, std):
    """v = fmin(fmax(x * std + mean, 0), 1) per channel: [3, H, W] float32; NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = frame.astype(np.float32) * std[:, None, None]
        x = x + mean[:, None, None]
    return np.fmin(np.fmax(x, ZERO), ONE)


def dehaze_frame(frame, mean, std, radius=7, omega=0.95, t_min=0.1, airlight_min=0.1, refine=1) -> dict:
    """One frame [3, H, W] -> {'restored' [3, H, W], 'airlight' [3], 'row' int64 [ROW] (frames = 1), and the intermediates 'v',
    'dark', 'bins', 'b_star', 'selected', 'n', 'e', 'o', 't', 'J'}."""
    frame = np.asarray(frame, dtype=np.float32)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    omega, t_min, a_min = np.float32(omega), np.float32(t_min), np.float32(airlight_min)
    _, h, w = frame.shape
    v = unit(frame, mean, std)
    m = np.fmin(np.fmin(v[0], v[1]), v[2])
    dark = erode(m, radius)
    bins = (dark * np.float32(255.0)).astype(np.int32)
    hist = np.bincount(bins.ravel(), minlength=256)
    bs = b_star(hist, n_top(h * w))
    sel = bins >= bs
    count = int(sel.sum())
    a_raw = np.empty(3, dtype=np.float32)
    for c in range(3):
        s = int(np.rint(v[c][sel] * Q16).astype(np.int64).sum())
        a_raw[c] = np.float32(np.float64(s) / (np.float64(count) * 65536.0))
    A = np.fmax(a_raw, a_min)
    n = np.fmin(np.fmin(v[0] / A[0], v[1] / A[1]), v[2] / A[2])
    e = erode(n, radius)
    o = dilate(e, radius) if refine else e
    t = np.fmax(ONE - omega * o, t_min)
    J = np.stack([np.fmin(np.fmax((v[c] - A[c]) / t + A[c], ZERO), ONE) for c in range(3)])
    restored = np.stack([(J[c] - mean[c]) / std[c] for c in range(3)]).astype(np.float32)
    row = np.zeros(ROW, dtype=np.int64)
    row[FRAMES] = 1
    row[SUM_A0:SUM_A2 + 1] = np.rint(A * Q16).astype(np.int64)
    row[PIXELS] = h * w
    row[SUM_T] = int(np.rint(t * Q16).astype(np.int64).sum())
    row[NONFINITE] = int((~np.isfinite(frame)).sum())
    row[FLOORED] = int((a_raw < a_min).any())
    return {"restored": restored, "airlight": A, "row": row, "v": v, "dark": dark, "bins": bins, "b_star": bs, "selected": count,
            "n": n, "e": e, "o": o, "t": t, "J": J}


def dehaze(image, mean=None, std=None, cond=None, n_slots=1, **params):
    """image [B, 3, H, W] -> (restored [B, 3, H, W], airlight [B, 3], stats int64 [n_slots, ROW]): frame b into slot 0 and slot
    1 + cond[b] when that is a slot."""
    image = np.asarray(image, dtype=np.float32)
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    restored, airlight = np.empty_like(image), np.empty((image.shape[0], 3), dtype=np.float32)
    stats = np.zeros((n_slots, ROW), dtype=np.int64)
    for b in range(image.shape[0]):
        f = dehaze_frame(image[b], mean, std, **params)
        restored[b], airlight[b] = f["restored"], f["airlight"]
        stats[0] += f["row"]
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            stats[1 + int(cond[b])] += f["row"]
    return restored, airlight, stats


def normalise(v, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[..., 3, H, W] values in [0, 1] -> the loader's float32 frames."""
    return ((np.asarray(v, dtype=np.float32) - mean[:, None, None]) / std[:, None, None]).astype(np.float32)


def hazy_scene(seed=0, h=48, w=80, spacing=4, airlight=(0.86, 0.88, 0.9)):
    """A scene J with a black pixel in every window (a lattice of zeros every `spacing` pixels, so the dark channel of J is zero as
    the prior assumes), haze of a smooth transmission t(x) falling from 0.9 on the left to 0.25 on the right and the airlight A:
    I = J t + A (1 - t); the right edge is the bright, hazy region the airlight estimate has to find.  -> (I, J, t, A), [3, H, W]
    values in [0, 1] (t [H, W])."""
    rng = np.random.default_rng(seed)
    J = (0.15 + 0.6 * rng.random((3, h, w))).astype(np.float32)
    J[:, ::spacing, ::spacing] = 0.0
    t = np.broadcast_to(np.linspace(0.9, 0.25, w, dtype=np.float32), (h, w)).copy()
    A = np.asarray(airlight, dtype=np.float32)
    I = (J * t + A[:, None, None] * (1.0 - t)).astype(np.float32)
    return I, J, t, A
