"""numpy float32 model of awseg_relight (include/awseg_restore.h): contrast-limited adaptive histogram equalisation
of the luma with a grey-world white balance, written without the kernels' strips, bands and four-pixel groups: histograms by
np.bincount per tile, tables by np.cumsum, every pixel's four table entries by fancy indexing.  One float32 operation per step in
the header's order (integers and float64 where the header says so), so the kernels have to reproduce every bit.  Importing this
file needs no GPU.

Launch geometry the GPU tests have to cross (csrc/relight.hip): the streaming passes run strips of rows, strips = ceil(256 * R /
(bands * B)) blocks per band, at most one per row of the tallest band (R = 4 and bands = tiles_y for the histogram pass, R = 8 and
bands = tiles_y + 1 for the final pass); a block strides over the rows of its band by that count and over a row by 256 threads (of
four pixels each on the 16-byte path).  STRIDED_ROWS is a shape whose bands are taller than the strip count (a second trip over
the rows), STRIDED_COLUMNS one whose rows are longer than one trip of the block on either path."""
from __future__ import annotations

import numpy as np

ROW = 10
FRAMES, SUM_K0, SUM_K1, SUM_K2, PIXELS, SUM_L, SUM_L_OUT, NONFINITE, CAPPED, SATURATED = range(ROW)
MAX_TILES = 16
Q16 = np.float32(65536.0)
ZERO, ONE = np.float32(0.0), np.float32(1.0)
FLOOR = np.float32(1.0 / 256.0)
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
NIGHT_TINT = np.array([0.8, 0.85, 1.2], dtype=np.float32)         # the renderer's night gains (awseg_night_apply)
# (shape, grid): 8 frames x 16 tile rows of 18 or 19 rows: 1024 / 128 = 8 strips in the histogram pass, 2048 / 136 = 16 in the final
# one, fewer than a band has rows
STRIDED_ROWS = ((8, 3, 300, 12), (16, 4))
# 1028 = 4 * 257 columns (one group more than the block's 256 threads), and 1027 on the scalar path
STRIDED_COLUMNS = (((1, 3, 9, 1028), (2, 8)), ((1, 3, 9, 1027), (2, 8)))


def bounds(size: int, n: int) -> list:
    """Tile k of an axis covers [bounds[k], bounds[k + 1]): floor(k size / n).  No padding, no reflection."""
    return [(k * int(size)) // int(n) for k in range(int(n) + 1)]


def unit(frame, mean, std):
    """v = fmin(fmax(x * std + mean, 0), 1) per channel: [3, H, W] float32; NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = frame.astype(np.float32) * std[:, None, None]
        x = x + mean[:, None, None]
    return np.fmin(np.fmax(x, ZERO), ONE)


def luma(v):
    return (np.float32(0.299) * v[0] + np.float32(0.587) * v[1]) + np.float32(0.114) * v[2]


def table(hist, clip_limit) -> dict:
    """One tile's 256-bin histogram -> {'limit', 'excess', 'h', 'cdf', 'lut' (uint16 [256])}: clip, one redistribution pass, scan."""
    hist = np.asarray(hist, dtype=np.int64)
    n = int(hist.sum())
    limit = max(1, int((np.float32(clip_limit) * np.float32(n)) / np.float32(256.0)))
    excess = int(np.maximum(hist - limit, 0).sum())
    h = np.minimum(hist, limit) + excess // 256
    rest = excess % 256
    if rest:
        step = max(256 // rest, 1)
        h[np.arange(rest) * step] += 1
    cdf = np.cumsum(h)
    lut = ((cdf * 65535 + n // 2) // n).astype(np.uint16)
    return {"limit": limit, "excess": excess, "h": h, "cdf": cdf, "lut": lut, "n": n}


def axis_weights(size: int, n: int):
    """Per position of an axis: (k0, k1, w) = the two tiles whose tables are blended and the weight of the second."""
    b = bounds(size, n)
    twice = [b[k] + b[k + 1] - 1 for k in range(n)]                 # twice the centre: compared as integers
    centre = np.asarray(twice, dtype=np.float32) * np.float32(0.5)
    k0, k1, w = np.zeros(size, np.int64), np.zeros(size, np.int64), np.zeros(size, np.float32)
    for p in range(size):
        before = sum(1 for t in twice if t <= 2 * p)
        if before == 0:
            continue
        if before == n:
            k0[p] = k1[p] = n - 1
            continue
        k0[p], k1[p] = before - 1, before
        w[p] = (np.float32(p) - centre[k0[p]]) / (centre[k1[p]] - centre[k0[p]])
    return k0, k1, w


def relight_frame(frame, mean, std, grid=(8, 8), clip_limit=2.0, max_gain=8.0, white_balance=1) -> dict:
    """One frame [3, H, W] -> {'restored' [3, H, W], 'gains' [3], 'row' int64 [ROW] (frames = 1), and the intermediates 'v', 'l',
    'bins', 'tables' ([ty][tx] of table()), 'lut' uint16 [ty, tx, 256], 'raw', 'J', 'l_out'}."""
    frame = np.asarray(frame, dtype=np.float32)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    ty, tx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    max_gain = np.float32(max_gain)
    _, h, w = frame.shape
    assert 1 <= ty <= min(MAX_TILES, h) and 1 <= tx <= min(MAX_TILES, w)
    v = unit(frame, mean, std)
    l = luma(v)
    bins = np.minimum((l * np.float32(255.0)).astype(np.int32), 255)
    yb, xb = bounds(h, ty), bounds(w, tx)
    tables = [[table(np.bincount(bins[yb[i]:yb[i + 1], xb[j]:xb[j + 1]].ravel(), minlength=256), clip_limit) for j in range(tx)]
              for i in range(ty)]
    lut = np.stack([np.stack([t["lut"] for t in row]) for row in tables])
    gains = np.ones(3, dtype=np.float32)
    if white_balance:
        m = np.empty(3, dtype=np.float32)
        for c in range(3):
            s = int(np.rint(v[c] * Q16).astype(np.int64).sum())
            m[c] = np.float32(np.float64(s) / (np.float64(h * w) * 65536.0))
        grey = ((m[0] + m[1]) + m[2]) / np.float32(3.0)
        gains = np.fmin(np.fmax(grey / np.fmax(m, FLOOR), np.float32(0.25)), np.float32(4.0)).astype(np.float32)
    i0, i1, wy = axis_weights(h, ty)
    j0, j1, wx = axis_weights(w, tx)
    wy, wx = wy[:, None], wx[None, :]
    a, b = lut[i0[:, None], j0[None, :], bins].astype(np.float32), lut[i0[:, None], j1[None, :], bins].astype(np.float32)
    c, d = lut[i1[:, None], j0[None, :], bins].astype(np.float32), lut[i1[:, None], j1[None, :], bins].astype(np.float32)
    top = a + wx * (b - a)
    bot = c + wx * (d - c)
    lp = (top + wy * (bot - top)) / np.float32(65535.0)
    raw = lp / np.fmax(l, FLOOR)
    g = np.fmin(raw, max_gain)
    u = np.stack([(v[ch] * gains[ch]) * g for ch in range(3)])
    J = np.fmin(np.fmax(u, ZERO), ONE)
    restored = np.stack([(J[ch] - mean[ch]) / std[ch] for ch in range(3)]).astype(np.float32)
    l_out = luma(J)
    row = np.zeros(ROW, dtype=np.int64)
    row[FRAMES] = 1
    row[SUM_K0:SUM_K2 + 1] = np.rint(gains * Q16).astype(np.int64)
    row[PIXELS] = h * w
    row[SUM_L] = int(np.rint(l * Q16).astype(np.int64).sum())
    row[SUM_L_OUT] = int(np.rint(np.fmin(l_out, ONE) * Q16).astype(np.int64).sum())
    row[NONFINITE] = int((~np.isfinite(frame)).sum())
    row[CAPPED] = int((raw > max_gain).sum())
    row[SATURATED] = int((u > ONE).sum())
    return {"restored": restored, "gains": gains, "row": row, "v": v, "l": l, "bins": bins, "tables": tables, "lut": lut, "raw": raw,
            "J": J, "l_out": l_out}


def relight(image, mean=None, std=None, cond=None, n_slots=1, **params):
    """image [B, 3, H, W] -> (restored [B, 3, H, W], gains [B, 3], stats int64 [n_slots, ROW]): frame b into slot 0 and slot
    1 + cond[b] when that is a slot."""
    image = np.asarray(image, dtype=np.float32)
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    restored, gains = np.empty_like(image), np.empty((image.shape[0], 3), dtype=np.float32)
    stats = np.zeros((n_slots, ROW), dtype=np.int64)
    for b in range(image.shape[0]):
        f = relight_frame(image[b], mean, std, **params)
        restored[b], gains[b] = f["restored"], f["gains"]
        stats[0] += f["row"]
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            stats[1 + int(cond[b])] += f["row"]
    return restored, gains, stats


def normalise(v, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[..., 3, H, W] values in [0, 1] -> the loader's float32 frames."""
    return ((np.asarray(v, dtype=np.float32) - mean[:, None, None]) / std[:, None, None]).astype(np.float32)


def night_like(frames, brightness=0.4, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """Normalised frames [..., 3, H, W] darkened and tinted as the renderer's night does it (v * brightness * NIGHT_TINT, clipped),
    normalised again."""
    v = np.asarray(frames, dtype=np.float32) * std[:, None, None] + mean[:, None, None]
    v = np.clip(v, 0.0, 1.0) * np.float32(brightness) * NIGHT_TINT[:, None, None]
    return normalise(np.clip(v, 0.0, 1.0), mean, std)
