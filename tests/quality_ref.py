"""numpy models of the image-quality counters (include/awseg.h, awseg_image_quality), written from the header's text
and independent of the package's code.

counters(): the float32 model, operation for operation as the header gives them (one rounding per operation, the separable window
along the row first, the taps accumulated left to right); the device must reproduce every counter exactly.
ssim_float64(): the second formulation, float64 with a direct two-dimensional 11 x 11 window; it says how accurate the float32
numbers are."""
import numpy as np

IQ_ROW = 10
FRAMES, N_ERR, SUM_ABS, SUM_SQ, BAD_ERR, N_WIN, SUM_L, SUM_CS, SUM_S, BAD_WIN = range(IQ_ROW)
UNIT = 2.0 ** -24
SCALE = np.float32(2.0 ** 24)
TWO = np.float32(2.0)
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
C1, C2 = 1e-4, 9e-4


def taps11() -> np.ndarray:
    """exp(-k^2 / (2 * 1.5^2)) for k = -5 .. 5, normalised in float64, rounded to float32 (Wang et al. 2004)."""
    k = np.arange(-5, 6, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (1.5 * 1.5))
    return (w / w.sum()).astype(np.float32)


def _filter(v: np.ndarray, taps: np.ndarray, axis: int) -> np.ndarray:
    """acc = taps[0] * v0; acc = acc + taps[k] * vk, k = 1 .. 10, over the valid positions along `axis`; float32 throughout."""
    n = v.shape[axis] - 10
    sl = lambda k: tuple(slice(k, k + n) if a == axis else slice(None) for a in range(v.ndim))   # noqa: E731
    acc = taps[0] * v[sl(0)]
    for k in range(1, 11):
        acc = acc + taps[k] * v[sl(k)]
    return acc


def frame_terms(image: np.ndarray, twin: np.ndarray, mean, std, taps, c1, c2) -> np.ndarray:
    """One frame [Ch, H, W] against its twin -> int64 [IQ_ROW] (frames = 1)."""
    image, twin = np.asarray(image, dtype=np.float32), np.asarray(twin, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    c1, c2 = np.float32(c1), np.float32(c2)
    row = np.zeros(IQ_ROW, dtype=np.int64)
    row[FRAMES] = 1
    ch, h, w = image.shape
    with np.errstate(all="ignore"):
        for c in range(ch):
            sd, mu = np.float32(std[c]), np.float32(mean[c])
            d = (image[c] - twin[c]) * sd
            ad = np.abs(d)
            ok = ad <= TWO                                            # NaN fails
            row[N_ERR] += int(ok.sum())
            row[BAD_ERR] += int((~ok).sum())
            row[SUM_ABS] += int(np.rint(ad[ok] * SCALE).astype(np.int64).sum())
            row[SUM_SQ] += int(np.rint((d[ok] * d[ok]) * SCALE).astype(np.int64).sum())
            if h < 11 or w < 11:
                continue
            x, y = image[c] * sd + mu, twin[c] * sd + mu
            m = [_filter(_filter(v, taps, 1), taps, 0) for v in (x, y, x * x, y * y, x * y)]
            mx, my, mxx, myy, mxy = m
            vx, vy, cxy = mxx - mx * mx, myy - my * my, mxy - mx * my
            lum = ((TWO * mx) * my + c1) / ((mx * mx + my * my) + c1)
            cs = (TWO * cxy + c2) / ((vx + vy) + c2)
            s = lum * cs
            assert lum.dtype == cs.dtype == s.dtype == np.float32
            ok = (np.abs(lum) <= TWO) & (np.abs(cs) <= TWO) & (np.abs(s) <= TWO)
            row[N_WIN] += int(ok.sum())
            row[BAD_WIN] += int((~ok).sum())
            for idx, v in ((SUM_L, lum), (SUM_CS, cs), (SUM_S, s)):
                row[idx] += int(np.rint(v[ok] * SCALE).astype(np.int64).sum())
    return row


def counters(image, refs, frame_ref, mean=None, std=None, taps=None, c1=C1, c2=C2, cond=None, n_slots=1):
    """image [B, Ch, H, W], refs [R, Ch, H, W], frame_ref [B] -> (int64 [n_slots, IQ_ROW], oob): frame b into slot 0 and slot
    1 + cond[b] when that is a slot; frame_ref < 0 skips a frame, >= R skips it and adds H * W to oob."""
    image, refs = np.asarray(image, dtype=np.float32), np.asarray(refs, dtype=np.float32)
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    taps = taps11() if taps is None else taps
    stats, oob = np.zeros((n_slots, IQ_ROW), dtype=np.int64), 0
    for b in range(image.shape[0]):
        r = int(frame_ref[b])
        if r < 0:
            continue
        if r >= refs.shape[0]:
            oob += image.shape[2] * image.shape[3]
            continue
        row = frame_terms(image[b], refs[r], mean, std, taps, c1, c2)
        stats[0] += row
        if cond is not None and 0 <= int(cond[b]) < n_slots - 1:
            stats[1 + int(cond[b])] += row
    return stats, oob


def ssim_float64(image, twin, mean, std, taps, c1=C1, c2=C2):
    """The second formulation: float64, the 11 x 11 window applied directly as the outer product of the taps.  One frame
    [Ch, H, W] -> (l, cs, s), each float64 [Ch, H - 10, W - 10]."""
    image, twin = np.asarray(image, dtype=np.float64), np.asarray(twin, dtype=np.float64)
    t = np.asarray(taps, dtype=np.float64)
    w2 = np.outer(t, t)
    sd, mu = np.asarray(std, dtype=np.float64)[:, None, None], np.asarray(mean, dtype=np.float64)[:, None, None]
    x, y = image * sd + mu, twin * sd + mu
    ch, h, w = x.shape

    def win(v):
        out = np.zeros((ch, h - 10, w - 10))
        for i in range(11):
            for j in range(11):
                out += w2[i, j] * v[:, i:i + h - 10, j:j + w - 10]
        return out
    mx, my, mxx, myy, mxy = win(x), win(y), win(x * x), win(y * y), win(x * y)
    vx, vy, cxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    lum = (2 * mx * my + c1) / (mx * mx + my * my + c1)
    cs = (2 * cxy + c2) / (vx + vy + c2)
    return lum, cs, lum * cs


# ----------------------------------------------------------------------------- test inputs (shared by the CPU and the GPU tests)
def rendered_frames(seed, b, ch, h, w, refs=3):
    """float32 frames as the loader normalises 8-bit data: `refs` smooth clean frames, and b variants of rows frame_ref under a
    synthetic corruption each: a fog-like contrast loss, a night-like gain, rain-like streaks, snow-like specks.
    -> (variants, clean, frame_ref, mean, std)."""
    rng = np.random.default_rng(seed)
    mean = IMAGENET_MEAN[:ch] if ch <= 3 else np.full(ch, 0.45, np.float32)
    std = IMAGENET_STD[:ch] if ch <= 3 else np.full(ch, 0.25, np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([[127 + 90 * np.sin(xx / (3.0 + c + 2 * r) + r) * np.cos(yy / (4.0 + r + c)) for c in range(ch)] for r in range(refs)])
    u8 = np.clip(np.rint(base + rng.normal(0, 6, base.shape)), 0, 255)
    norm = lambda v: ((((v / 255.0).astype(np.float32)) - mean[:, None, None]) / std[:, None, None]).astype(np.float32)   # noqa: E731
    fr = rng.integers(0, refs, b).astype(np.int32)
    var = []
    for i in range(b):
        v = u8[fr[i]].copy()
        kind = i % 4
        if kind == 0:
            v = 0.5 * v + 110                                         # fog: contrast
        elif kind == 1:
            v = 0.35 * v                                              # night: luminance
        elif kind == 2:
            v[:, :, ::7] = np.minimum(v[:, :, ::7] + 70, 255)         # rain: structure
        else:
            v = np.where(rng.random(v.shape[1:]) < 0.03, 255.0, v)
        var.append(np.clip(np.rint(v), 0, 255))
    return norm(np.stack(var)), norm(u8), fr, mean, std


def random_frames(seed, b, ch, h, w, refs=2):
    """Independent float32 values whose de-normalised range is [0, 1]: the least smooth input."""
    rng = np.random.default_rng(seed)
    mean = IMAGENET_MEAN[:ch] if ch <= 3 else np.full(ch, 0.45, np.float32)
    std = IMAGENET_STD[:ch] if ch <= 3 else np.full(ch, 0.25, np.float32)
    norm = lambda v: ((v.astype(np.float32) - mean[:, None, None]) / std[:, None, None]).astype(np.float32)   # noqa: E731
    return norm(rng.random((b, ch, h, w))), norm(rng.random((refs, ch, h, w))), rng.integers(0, refs, b).astype(np.int32), mean, std
