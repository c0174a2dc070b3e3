"""numpy model of awseg_tta_view and awseg_tta_accumulate, written from the text of include/awseg_restore.h pixel by whole map (no
groups of four, no grid): align_corners = False bilinear sampling in which every step is one operation of the working dtype.  With
dtype = float32 these are the launchers' bits; `dtype=np.float64` is the twin the float32 model is bounded against
(tests/test_tta_ref.py).  Importing this file needs no GPU."""
import numpy as np

SET, ADD, SCALE_ADD = 0, 1, 2                     # AWSEG_TTA_SET, AWSEG_TTA_ADD, AWSEG_TTA_SCALE_ADD


def axis_taps(src: int, dst: int, dtype=np.float32):
    """The two source positions and their weights of every destination position along one axis: (p0, p1, l0, l1)."""
    t = np.dtype(dtype).type
    scale = t(src) / t(dst)
    p = np.arange(dst).astype(dtype)
    f = np.maximum(scale * (p + t(0.5)) - t(0.5), t(0))
    p0 = np.minimum(f.astype(np.int64), src - 1)
    p1 = p0 + (p0 < src - 1)
    l1 = f - p0.astype(dtype)
    l0 = t(1) - l1
    assert l0.dtype == l1.dtype == np.dtype(dtype)
    return p0, p1, l0, l1


def _term(l, v):
    """l * v, and +0 where the weight is exactly zero (a neighbour that takes no part does not make a NaN)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(l != 0, l * v, np.zeros((), v.dtype))


def sample(src: np.ndarray, size, dtype=np.float32) -> np.ndarray:
    """U: src [..., h, w] sampled at the pixels of a map of `size` = (H, W).  Equal sizes: src itself."""
    src = np.asarray(src, dtype=dtype)
    h, w = src.shape[-2:]
    H, W = int(size[0]), int(size[1])
    if (h, w) == (H, W):
        return src.copy()
    y0, y1, ly0, ly1 = axis_taps(h, H, dtype)
    x0, x1, lx0, lx1 = axis_taps(w, W, dtype)
    r0, r1 = src[..., y0, :], src[..., y1, :]
    with np.errstate(invalid="ignore", over="ignore"):
        top = _term(lx0, r0[..., x0]) + _term(lx1, r0[..., x1])
        bot = _term(lx0, r1[..., x0]) + _term(lx1, r1[..., x1])
        u = _term(ly0[:, None], top) + _term(ly1[:, None], bot)
    assert u.dtype == np.dtype(dtype)
    return u


def view(src: np.ndarray, size, flip: bool, dtype=np.float32) -> np.ndarray:
    """awseg_tta_view: resampled to `size`, then mirrored."""
    u = sample(src, size, dtype)
    return np.ascontiguousarray(u[..., ::-1]) if flip else u


def accumulate(src: np.ndarray, acc: np.ndarray, flip: bool, weight, mode: int, dtype=np.float32) -> np.ndarray:
    """awseg_tta_accumulate -> the new accumulator: the view's logits mirrored back first, resampled then."""
    t = np.dtype(dtype).type
    src, acc = np.asarray(src, dtype=dtype), np.asarray(acc, dtype=dtype)
    u = sample(src[..., ::-1] if flip else src, acc.shape[-2:], dtype)
    wt = t(np.float32(weight))                                        # the launcher takes a float32
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == SET:
            out = wt * u
        elif mode == ADD:
            out = acc + wt * u
        elif mode == SCALE_ADD:
            out = wt * acc + wt * u
        else:
            raise ValueError(f"unknown mode {mode!r}")
    assert out.dtype == np.dtype(dtype)
    return out


def maps(seed: int, shape, lo=-8.0, hi=8.0) -> np.ndarray:
    """Random float32 maps of logit-like magnitude with a few exact zeros and negative zeros."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, size=shape).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 8:
        flat[rng.choice(flat.size, 2, replace=False)] = np.float32(0.0), np.float32(-0.0)
    return x
