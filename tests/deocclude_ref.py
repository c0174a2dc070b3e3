"""numpy model of awseg_deocclude (include/awseg_restore.h): bright occluders narrower than a window found by the
white top-hat of every channel and filled from their unmasked neighbours, written without the kernels' tiles, halos and packed
words: every window pass is 2r + 1 shifted views of a padded frame.  One float32 operation per step in the header's order (integers
and float64 where the header says so), so the kernels have to reproduce every bit.  Importing this file needs no GPU.

The float32 / float64 fill bound.  J_c = float32(S_c / (N * 65536)) is ONE rounding of an exact quotient of integers (the float64
division and the float64 -> float32 conversion: S_c < 2^26 and N * 65536 < 2^26 are exact in float64, the quotient is rounded to
53 bits and then to 24).  The float64 variant keeps the 53-bit quotient.  Both lie in [0, 1], so they differ by at most half a
float32 ulp of a value <= 1 plus the double rounding, FILL_F32_BOUND = 2^-24 (1 + 2^-28).

Launch geometry the GPU tests have to cross (csrc/deocclude.hip): both kernels run on 32 x 64 tiles; the detection kernel stages a
halo of 2 r + d (32 = the tile height at r = 15, d = 2), the fill kernel one of r; the 16-byte path needs W % 4 == 0 and aligned
tensors."""
from __future__ import annotations

import numpy as np

ROW = 7
FRAMES, PIXELS, SEEDS, MASKED, UNFILLED, CHANGE, NONFINITE = range(ROW)
MAX_RADIUS, MAX_DILATE = 15, 2
TILE_H, TILE_W = 32, 64
Q16 = np.float32(65536.0)
ZERO, ONE = np.float32(0.0), np.float32(1.0)
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
DEFAULTS = {"radius": 9, "threshold": 0.06, "bright_min": 0.5, "dilate": 1}
FILL_F32_BOUND = 2.0 ** -24 * (1.0 + 2.0 ** -28)
RAIN_COLOUR = np.array([0.8, 0.9, 1.0], dtype=np.float32)          # the renderer's streaks (awseg_rain_apply)


def unit(frame, mean, std):
    """v = fmin(fmax(x * std + mean, 0), 1) per channel: [3, H, W] float32; NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = frame.astype(np.float32) * std[:, None, None]
        x = x + mean[:, None, None]
    return np.fmin(np.fmax(x, ZERO), ONE)


def window(a, r: int, op, outside):
    """(2r+1)^2 window `op` (np.minimum / np.maximum / np.add) of a [..., H, W], clipped to the frame: positions outside hold
    `outside`, the neutral element.  Separable; exact for the three operations on the types they are used with."""
    r = int(r)
    if r == 0:
        return a.copy()
    h, w = a.shape[-2:]
    pad = [(0, 0)] * (a.ndim - 2)
    p = np.pad(a, pad + [(0, 0), (r, r)], constant_values=outside)
    rows = p[..., :, 0:w].copy()
    for k in range(1, 2 * r + 1):
        rows = op(rows, p[..., :, k:k + w])
    p = np.pad(rows, pad + [(r, r), (0, 0)], constant_values=outside)
    out = p[..., 0:h, :].copy()
    for k in range(1, 2 * r + 1):
        out = op(out, p[..., k:k + h, :])
    return out


def opening(v, r: int):
    """e = window minimum, o = window maximum of e; positions outside the frame take part in neither.  o <= v."""
    e = window(v, r, np.minimum, np.float32(np.inf))
    return window(e, r, np.maximum, np.float32(-np.inf))


def detect(v, radius, threshold, bright_min, dilate) -> dict:
    """v [3, H, W] -> {'o', 'h', 'b', 'seed' (bool), 'mask' (uint8)}."""
    o = opening(v, radius)
    t = v - o
    h = np.fmin(np.fmin(t[0], t[1]), t[2])
    b = np.fmin(np.fmin(v[0], v[1]), v[2])
    seed = (h > np.float32(threshold)) & (b >= np.float32(bright_min))
    mask = window(seed.astype(np.uint8), dilate, np.maximum, np.uint8(0))
    return {"o": o, "h": h, "b": b, "seed": seed, "mask": mask}


def fill(v, mask, radius, float64: bool = False) -> dict:
    """v [3, H, W], mask uint8 [H, W] -> {'J' [3, H, W] (float32, or float64 with `float64`), 'q', 'S', 'N', 'unfilled' (bool)}."""
    q = np.rint(v * Q16).astype(np.int32)
    keep = (mask == 0)
    n = window(keep.astype(np.int64), radius, np.add, np.int64(0))
    s = window(np.where(keep[None], q, 0).astype(np.int64), radius, np.add, np.int64(0))
    masked = mask != 0
    filled = masked & (n > 0)
    quotient = s.astype(np.float64) / (np.maximum(n, 1).astype(np.float64) * 65536.0)[None]
    if float64:
        J = np.where(filled[None], quotient, v.astype(np.float64))
    else:
        J = np.where(filled[None], quotient.astype(np.float32), v).astype(np.float32)
    return {"J": J, "q": q, "S": s, "N": n, "unfilled": masked & (n == 0)}


def deocclude_frame(frame, mean, std, radius=9, threshold=0.06, bright_min=0.5, dilate=1) -> dict:
    """One frame [3, H, W] -> {'restored' [3, H, W], 'mask' uint8 [H, W], 'row' int64 [ROW] (frames = 1) and the intermediates 'v',
    'o', 'h', 'b', 'seed', 'J', 'S', 'N', 'unfilled'}."""
    frame = np.asarray(frame, dtype=np.float32)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    assert 1 <= int(radius) <= MAX_RADIUS and 0 <= int(dilate) <= MAX_DILATE
    _, h, w = frame.shape
    v = unit(frame, mean, std)
    det = detect(v, radius, threshold, bright_min, dilate)
    fl = fill(v, det["mask"], radius)
    J = fl["J"]
    restored = np.stack([(J[c] - mean[c]) / std[c] for c in range(3)]).astype(np.float32)
    masked = det["mask"] != 0
    moved = np.abs(np.rint(J * Q16).astype(np.int64) - fl["q"].astype(np.int64))
    row = np.zeros(ROW, dtype=np.int64)
    row[FRAMES] = 1
    row[PIXELS] = h * w
    row[SEEDS] = int(det["seed"].sum())
    row[MASKED] = int(masked.sum())
    row[UNFILLED] = int(fl["unfilled"].sum())
    row[CHANGE] = int(moved[:, masked].sum())
    row[NONFINITE] = int((~np.isfinite(frame)).sum())
    return {"restored": restored, "mask": det["mask"], "row": row, "v": v, **{k: det[k] for k in ("o", "h", "b", "seed")},
            **{k: fl[k] for k in ("J", "S", "N", "unfilled")}}


def deocclude(image, mean=None, std=None, cond=None, n_slots=1, **params):
    """image [B, 3, H, W] -> (restored [B, 3, H, W], mask uint8 [B, H, W], stats int64 [n_slots, ROW]): frame b into slot 0 and
    slot 1 + cond[b] when that is a slot."""
    image = np.asarray(image, dtype=np.float32)
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    restored = np.empty_like(image)
    mask = np.empty((image.shape[0],) + image.shape[2:], dtype=np.uint8)
    stats = np.zeros((n_slots, ROW), dtype=np.int64)
    for b in range(image.shape[0]):
        f = deocclude_frame(image[b], mean, std, **params)
        restored[b], mask[b] = f["restored"], f["mask"]
        stats[0] += f["row"]
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            stats[1 + int(cond[b])] += f["row"]
    return restored, mask, stats


def normalise(v, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[..., 3, H, W] values in [0, 1] -> the loader's float32 frames."""
    return ((np.asarray(v, dtype=np.float32) - mean[:, None, None]) / std[:, None, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ fixtures (values in [0, 1])
def background(h: int, w: int, seed: int = 0, texture: float = 0.02):
    """A smooth dim scene [3, H, W]: a gradient per channel in [0.15, 0.45] with a little noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([0.20 + 0.15 * x / max(w - 1, 1), 0.25 + 0.10 * y / max(h - 1, 1), 0.30 + 0.10 * (x + y) / max(h + w - 2, 1)])
    return np.clip(base + texture * rng.standard_normal((3, h, w)), 0.0, 1.0).astype(np.float32)


def blur(v, k: int):
    """k x k box blur with edge replication, as the renderer softens its occluders."""
    if k <= 1:
        return v
    r = k // 2
    p = np.pad(v, [(0, 0), (r, r), (r, r)], mode="edge").astype(np.float32)
    h, w = v.shape[-2:]
    acc = np.zeros_like(v, dtype=np.float32)
    for dy in range(k):
        for dx in range(k):
            acc += p[:, dy:dy + h, dx:dx + w]
    return (acc / np.float32(k * k)).astype(np.float32)


def draw_streaks(v, count: int, length: int, thick: int, seed: int = 1):
    """Rain as the renderer draws it: slanted streaks of RAIN_COLOUR, `thick` (1 or 3) pixels wide, then a 3 x 3 blur."""
    rng = np.random.default_rng(seed)
    out = v.copy()
    _, h, w = v.shape
    for _ in range(count):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        for t in range(length):
            y, x = y0 + t, x0 + t // 3
            for dx in range(thick):
                if 0 <= y < h and 0 <= x + dx < w:
                    out[:, y, x + dx] = RAIN_COLOUR
    return blur(out, 3)


def draw_discs(v, count: int, radius: int, kernel: int, seed: int = 2, lift: float = 0.05):
    """Snow as the renderer draws it: a brightness lift, filled white discs of `radius`, then a kernel x kernel blur."""
    rng = np.random.default_rng(seed)
    out = np.clip(v + np.float32(lift), 0.0, 1.0).astype(np.float32)
    _, h, w = v.shape
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(count):
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        out[:, (yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius] = 1.0
    return blur(out, kernel)


def draw_square(v, side: int, top: int = None, left: int = None):
    """A filled white square of `side` pixels (default: centred): wider than the window, it survives the opening and is not masked."""
    out = v.copy()
    _, h, w = v.shape
    top = (h - side) // 2 if top is None else top
    left = (w - side) // 2 if left is None else left
    out[:, max(top, 0):top + side, max(left, 0):left + side] = 1.0
    return out


def occluder_batch(shape, seed: int = 0):
    """A batch [B, 3, H, W] of normalised frames for the bit comparisons: frame b alternates rain (1- and 3-pixel streaks) and snow
    (discs of radius 2, blurred 3 x 3), dense enough that a few per cent of even a small frame are masked."""
    b, _, h, w = shape
    frames = []
    for k in range(b):
        bg = background(h, w, seed + 10 * k)
        n = max(2, (h * w) // 400)
        if k % 2 == 0:
            v = draw_streaks(draw_streaks(bg, n, max(6, h // 3), 1, seed + k), max(1, n // 2), max(6, h // 3), 3, seed + k + 50)
        else:
            v = draw_discs(bg, n, 2, 3, seed + k)
        frames.append(v)
    return normalise(np.stack(frames))


def unfilled_frame(h: int, w: int, radius: int, dilate: int, seed: int = 0):
    """One normalised frame [1, 3, H, W] whose middle is left unfilled (N == 0).  A FILLED white square of side 2 r + 2 d + 3
    cannot do that: it is wider than the window, the opening keeps it and its top-hat is 0 (test_filled_square_is_kept).  What
    can is a square of that side ruled with white lines one pixel wide and 2 d apart (d >= 1): every line is a seed, the
    dilation closes the gaps, and the pixels in the middle of the square see no unmasked pixel within r."""
    assert dilate >= 1
    v = background(h, w, seed)
    side = 2 * radius + 2 * dilate + 3
    top, left = max((h - side) // 2, 0), max((w - side) // 2, 0)
    step = 2 * dilate + 1
    for y in range(top, min(top + side, h), step):
        v[:, y, left:left + side] = 1.0
    return normalise(v[None])


def nonfinite_frame(h: int, w: int, seed: int = 0):
    """A rain frame [1, 3, H, W] with a NaN, a +inf and a -inf planted: counted, and treated as 0, 1 and 0."""
    x = occluder_batch((1, 3, h, w), seed).copy()
    x[0, 0, h // 2, w // 2] = np.nan
    x[0, 1, 1, 2] = np.inf
    x[0, 2, h - 1, w - 1] = -np.inf
    return x


def specks(h: int, w: int, count: int, seed: int = 3):
    """One normalised frame [1, 3, H, W] with `count` single white pixels, unblurred: what a 3 x 3 window (r = 1) can still take out."""
    rng = np.random.default_rng(seed)
    v = background(h, w, seed)
    idx = rng.choice(h * w, size=count, replace=False)
    v.reshape(3, -1)[:, idx] = 1.0
    return normalise(v[None])


# The shapes of the GPU comparisons (tests/test_gpu_deocclude.py): (id, frames, parameters, float32 elements past a 16-byte boundary).
# tests/test_deocclude_ref.py holds every one of them to a masked share between 2 % and 50 %, and one of them to unfilled pixels.
def gpu_cases():
    r9 = {"radius": 9, "dilate": 1}
    return [("33 x 65: one row and one column past a seam, scalar path", occluder_batch((1, 3, 33, 65), 1), r9, 0),
            ("40 x 72: 16-byte path", occluder_batch((2, 3, 40, 72), 2), r9, 0),
            ("40 x 72, 4 bytes off alignment: scalar path", occluder_batch((2, 3, 40, 72), 2), r9, 1),
            ("5 x 7: every window larger than the frame", specks(5, 7, 1, 4), r9, 0),
            ("37 x 70, r = 15, d = 2: halo 32", occluder_batch((3, 3, 37, 70), 5), {"radius": 15, "dilate": 2}, 0),
            ("64 x 128, r = 1, d = 0: smallest halo, whole tiles", specks(64, 128, 400, 6), {"radius": 1, "dilate": 0}, 0),
            ("48 x 80: a ruled square left unfilled", unfilled_frame(48, 80, 9, 1, 7), r9, 0),
            ("40 x 72 with NaN, +inf and -inf", nonfinite_frame(40, 72, 8), r9, 0)]
