"""numpy model of awseg_weather_estimate (include/awseg_restore.h): the three frame statistics and the rule that
sends a frame to one of the restoration front-ends, written without the kernel's tiles and halos, and without anything of the
library: every window pass is 2r + 1 shifted views of a padded frame.  One float32 operation per step in the header's order
(integers and float64 where the header says so), so the kernels have to reproduce every bit.  Importing this file needs no GPU.

The dark channel is computed the dehazer's way, the window minimum of min_c v_c; the kernel takes min_c of the window minima e_c it
has anyway.  Minima commute, so both give the same bits (dark_from_channels, held equal in tests/test_estimate_ref.py).

Launch geometry the GPU tests have to cross (csrc/estimate.hip): 32 x 64 tiles with a halo of 2 r (30 at r = 15: LDS above 64 KB);
the 16-byte path needs W % 4 == 0 and an aligned tensor.

The fixtures are the street scenes the thresholds were chosen on, rendered by the CPU renderer of oracle/cpu_oracle.py at the
loader's reference severities."""
from __future__ import annotations

import functools

import numpy as np

ROW = 13
FRAMES, PIXELS, SUM_DARK, SUM_LUMA, SUM_C0, SUM_C1, SUM_C2, SEEDS, NONFINITE, TO_NONE, TO_DARK_CHANNEL, TO_CLAHE, TO_TOPHAT = range(ROW)
NONE, DARK_CHANNEL, CLAHE, TOPHAT = range(4)
ROUTES = ("none", "dark_channel", "clahe", "tophat")
MAX_RADIUS = 15
TILE_H, TILE_W = 32, 64
Q16 = np.float32(65536.0)
ZERO, ONE = np.float32(0.0), np.float32(1.0)
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
DEFAULTS = {"radius": 7, "threshold": 0.06, "bright_min": 0.5, "cast_max": 0.65, "luma_max": 0.5, "dark_min": 0.47, "seed_min": 0.001}
# the loader's reference severities (data.loader.REFERENCE_SEVERITIES; tests/test_estimate_ref.py holds the two equal), in the order
# the scenes are rendered, and the route a blind front-end should take for each kind
SEVERITIES = {"fog": [0.3, 0.6, 0.9], "rain": [0.2, 0.5, 0.8], "snow": [0.2, 0.45, 0.7], "night": [0.4, 0.6, 0.8]}
EXPECTED = {"clean": NONE, "fog": DARK_CHANNEL, "night": CLAHE, "rain": TOPHAT, "snow": TOPHAT}


def unit(frame, mean, std):
    """v = fmin(fmax(x * std + mean, 0), 1) per channel: [3, H, W] float32; NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = frame.astype(np.float32) * std[:, None, None]
        x = x + mean[:, None, None]
    return np.fmin(np.fmax(x, ZERO), ONE)


def window(a, r: int, op, outside):
    """(2r+1)^2 window `op` (np.fmin / np.fmax) of a [..., H, W], clipped to the frame: positions outside hold `outside`."""
    h, w = a.shape[-2:]
    lead = [(0, 0)] * (a.ndim - 2)
    p = np.pad(a, lead + [(0, 0), (r, r)], constant_values=outside)
    rows = p[..., :, 0:w].copy()
    for k in range(1, 2 * r + 1):
        rows = op(rows, p[..., :, k:k + w])
    p = np.pad(rows, lead + [(r, r), (0, 0)], constant_values=outside)
    out = p[..., 0:h, :].copy()
    for k in range(1, 2 * r + 1):
        out = op(out, p[..., k:k + h, :])
    return out


def pixel_maps(v, radius, threshold, bright_min) -> dict:
    """v [3, H, W] -> {'e', 'o', 'm', 'h', 'seed' (bool), 'dark', 'l'}."""
    e = window(v, radius, np.fmin, np.float32(np.inf))
    o = window(e, radius, np.fmax, np.float32(-np.inf))
    m = np.fmin(np.fmin(v[0], v[1]), v[2])
    t = v - o
    h = np.fmin(np.fmin(t[0], t[1]), t[2])
    seed = (h > np.float32(threshold)) & (m >= np.float32(bright_min))
    dark = window(m, radius, np.fmin, np.float32(np.inf))
    l = (np.float32(0.299) * v[0] + np.float32(0.587) * v[1]) + np.float32(0.114) * v[2]
    return {"e": e, "o": o, "m": m, "h": h, "seed": seed, "dark": dark, "l": l.astype(np.float32)}


def dark_from_channels(e):
    """The kernel's form of the dark channel: the minimum over the channels of the window minima."""
    return np.fmin(np.fmin(e[0], e[1]), e[2])


def decide(D, L, M0, M2, O, cast_max, luma_max, dark_min, seed_min) -> int:
    """The first rule that matches, float32 compares."""
    D, L, M0, M2, O = (np.float32(x) for x in (D, L, M0, M2, O))
    if M0 < np.float32(cast_max) * M2 and L < np.float32(luma_max):
        return CLAHE
    if D > np.float32(dark_min):
        return DARK_CHANNEL
    if O > np.float32(seed_min):
        return TOPHAT
    return NONE


def estimate_frame(frame, mean, std, radius=7, threshold=0.06, bright_min=0.5, cast_max=0.65, luma_max=0.5, dark_min=0.47,
                   seed_min=0.001) -> dict:
    """One frame [3, H, W] -> {'route', 'descriptors' float32 [6], 'row' int64 [ROW] (frames = 1) and the pixel maps}."""
    frame = np.asarray(frame, dtype=np.float32)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    assert 1 <= int(radius) <= MAX_RADIUS
    _, h, w = frame.shape
    v = unit(frame, mean, std)
    px = pixel_maps(v, int(radius), threshold, bright_min)
    q_dark = int(np.rint(px["dark"] * Q16).astype(np.int64).sum())
    q_l = int(np.rint(px["l"] * Q16).astype(np.int64).sum())
    q_c = [int(np.rint(v[c] * Q16).astype(np.int64).sum()) for c in range(3)]
    n_seed = int(px["seed"].sum())
    P = np.float64(h * w) * 65536.0
    D, L = np.float32(np.float64(q_dark) / P), np.float32(np.float64(q_l) / P)
    M = [np.float32(np.float64(q) / P) for q in q_c]
    O = np.float32(np.float64(n_seed) / np.float64(h * w))
    route = decide(D, L, M[0], M[2], O, cast_max, luma_max, dark_min, seed_min)
    row = np.zeros(ROW, dtype=np.int64)
    row[FRAMES], row[PIXELS], row[SUM_DARK], row[SUM_LUMA] = 1, h * w, q_dark, q_l
    row[SUM_C0:SUM_C2 + 1] = q_c
    row[SEEDS] = n_seed
    row[NONFINITE] = int((~np.isfinite(frame)).sum())
    row[TO_NONE + route] = 1
    return {"route": route, "descriptors": np.array([D, L, M[0], M[1], M[2], O], dtype=np.float32), "row": row, "v": v, **px}


def estimate(image, mean=None, std=None, cond=None, n_slots=1, **params):
    """image [B, 3, H, W] -> (route int32 [B], descriptors float32 [B, 6], stats int64 [n_slots, ROW]): frame b into slot 0 and
    slot 1 + cond[b] when that is a slot."""
    image = np.asarray(image, dtype=np.float32)
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    route = np.empty(image.shape[0], dtype=np.int32)
    desc = np.empty((image.shape[0], 6), dtype=np.float32)
    stats = np.zeros((n_slots, ROW), dtype=np.int64)
    for b in range(image.shape[0]):
        f = estimate_frame(image[b], mean, std, **params)
        route[b], desc[b] = f["route"], f["descriptors"]
        stats[0] += f["row"]
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            stats[1 + int(cond[b])] += f["row"]
    return route, desc, stats


def normalise(v, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[..., 3, H, W] values in [0, 1] -> the loader's float32 frames."""
    return ((np.asarray(v, dtype=np.float32) - mean[:, None, None]) / std[:, None, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ fixtures
def street_scene(h, w, seed):
    """A synthetic street, uint8 [H, W, 3]: a sky gradient, a road, buildings with dark windows, vegetation, lane markings, noise."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 3), np.float32)
    hor = int(h * (0.35 + 0.1 * rng.random()))
    yy, xx = np.mgrid[0:h, 0:w]
    img[:hor] = np.array([0.55, 0.7, 0.9]) * (0.8 + 0.2 * (yy[:hor, :, None] / max(hor, 1)))
    img[hor:] = np.array([0.32, 0.32, 0.34])
    x = 0
    while x < w:
        bw = int(rng.integers(w // 16, w // 6))
        top = int(rng.integers(hor // 4, hor))
        bot = hor + int(rng.integers(0, h // 8))
        img[top:bot, x:x + bw] = rng.random(3) * 0.6 + 0.1
        for wy in range(top + 4, bot - 4, 10):
            for wx in range(x + 3, min(x + bw - 3, w), 8):
                img[wy:wy + 5, wx:wx + 4] = 0.05
        x += bw
    for _ in range(6):
        cx, cy, r = int(rng.integers(0, w)), int(rng.integers(hor - 10, hor + h // 6)), int(rng.integers(8, 24))
        img[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = np.array([0.1, 0.3 + 0.2 * rng.random(), 0.08])
    img[hor + (h - hor) // 2: hor + (h - hor) // 2 + 3, ::40] = 0.9
    img += rng.normal(0, 0.015, img.shape)
    return np.clip(np.rint(img * 255), 0, 255).astype(np.uint8)


def to_frame(img_u8):
    """uint8 [H, W, 3] -> the loader's normalised float32 [3, H, W] (the oracle's normalize)."""
    from oracle import cpu_oracle
    return cpu_oracle.normalize(np.ascontiguousarray(img_u8, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def rendered_scene(h: int, w: int, seed: int):
    """Scene `seed` clean and at every reference severity -> a tuple of (kind, level or None, normalised frame [3, H, W]), 13 of
    them: np.random.seed(seed), the scene, then the renderer over fog, rain, snow, night in that order.  Computed once and shared:
    do not write into the frames."""
    from oracle import cpu_oracle
    np.random.seed(seed)
    img = street_scene(h, w, seed)
    out = [("clean", None, to_frame(img))]
    for kind, levels in SEVERITIES.items():
        for level in levels:
            out.append((kind, level, to_frame(np.asarray(cpu_oracle.apply_weather_effect(img.copy(), kind, level), dtype=np.uint8))))
    for _, _, f in out:
        f.setflags(write=False)
    return tuple(out)


def scene_batch(h: int, w: int, seed: int, picks):
    """The frames of rendered_scene(h, w, seed) named by `picks` = [(kind, level or None), ...] -> ([B, 3, H, W], kinds)."""
    table = {(k, l): f for k, l, f in rendered_scene(h, w, seed)}
    return np.stack([table[p] for p in picks]), [p[0] for p in picks]


def constant_frame(h: int, w: int, value, b: int = 1):
    """[B, 3, H, W] whose v_c is exactly `value` in every channel: x chosen so that x * std + mean rounds to value (checked), or lies
    beyond the clamp for 0 and 1."""
    value = np.float32(value)
    x = np.empty((3,), np.float32)
    for c in range(3):
        if value in (ZERO, ONE):                                        # the clamp's ends: anything beyond them
            x[c] = np.float32(-3.0) if value == ZERO else np.float32(3.0)
            continue
        guess = np.float32((value - IMAGENET_MEAN[c]) / IMAGENET_STD[c])
        cands = [guess]
        for _ in range(8):
            cands += [np.nextafter(cands[-1], np.float32(np.inf))]
        lo = guess
        for _ in range(8):
            lo = np.nextafter(lo, np.float32(-np.inf))
            cands.append(lo)
        hit = [g for g in cands if np.float32(np.float32(g * IMAGENET_STD[c]) + IMAGENET_MEAN[c]) == value]
        assert hit, (value, c)
        x[c] = hit[0]
    return np.broadcast_to(x[None, :, None, None], (b, 3, h, w)).astype(np.float32).copy()


def seeded_frame(h: int, w: int, count: int, seed: int = 3):
    """One normalised frame [1, 3, H, W]: a constant background of 0.25 with `count` single white pixels, no two within one window
    of r = 1 of each other or of the border's clipping: each is exactly one seed at r = 1 and the defaults."""
    rng = np.random.default_rng(seed)
    v = np.full((3, h, w), 0.25, np.float32)
    cells = [(y, x) for y in range(1, h - 1, 4) for x in range(1, w - 1, 4)]
    for k in rng.choice(len(cells), size=count, replace=False):
        v[:, cells[k][0], cells[k][1]] = 1.0
    return normalise(v[None])


def nonfinite_frame(x):
    """A copy of the batch x with a NaN, a +inf and a -inf planted in frame 0: counted, and treated as 0, 1 and 0."""
    x = np.array(x, dtype=np.float32, copy=True)
    _, _, h, w = x.shape
    x[0, 0, h // 2, w // 2] = np.nan
    x[0, 1, min(1, h - 1), min(2, w - 1)] = np.inf
    x[0, 2, h - 1, w - 1] = -np.inf
    return x


def crop(frames, h: int, w: int, top: int = 0, left: int = 0):
    return np.ascontiguousarray(frames[..., top:top + h, left:left + w])


# The shapes of the GPU comparisons (tests/test_gpu_estimate.py): (id, frames [3, 3, H, W], parameters, float32 elements past a
# 16-byte boundary).  Every batch has three frames: cond holds a valid id, -1 and an id past the slots.
def gpu_cases():
    from tests import quality_ref
    scene, _ = scene_batch(128, 256, 0, [("fog", 0.6), ("snow", 0.45), ("night", 0.6), ("rain", 0.5), ("clean", None)])

    def mixed(h, w, top, left, seed):
        """A crop of a rendered scene, a frame of independent noise, and a crop of another rendered frame."""
        noise = quality_ref.random_frames(seed, 1, 3, h, w)[0][0]
        return np.stack([crop(scene[seed % 2], h, w, top, left), noise, crop(scene[1 + seed % 3], h, w, top + 3, left + 5)]).astype(np.float32)

    big = mixed(64, 128, 40, 100, 4)
    consts = np.concatenate([constant_frame(5, 9, 0.5), constant_frame(5, 9, 0.0), crop(scene[1:2], 5, 9, 60, 100)])
    return [("1 x 1, r = 1: smallest frame", np.concatenate([constant_frame(1, 1, 0.75), crop(scene[0:1], 1, 1, 9, 9), constant_frame(1, 1, 1.0)]),
             {"radius": 1}, 0),
            ("5 x 9, r = 15: window larger than the frame", consts, {"radius": 15}, 0),
            ("37 x 70, r = 7: two tiles each way, scalar path", mixed(37, 70, 50, 90, 1), {"radius": 7, "seed_min": 0.05}, 0),
            ("33 x 68, r = 3: 16-byte path, ragged tiles", nonfinite_frame(mixed(33, 68, 30, 20, 2)), {"radius": 3}, 0),
            ("64 x 128, r = 7: aligned", big, {"radius": 7}, 0),
            ("64 x 128, r = 7: storage shifted by 4 bytes", big, {"radius": 7}, 1),
            ("40 x 72, r = 15: largest halo, LDS above 64 KB", mixed(40, 72, 70, 150, 3), {"radius": 15, "dark_min": 0.3}, 0)]
