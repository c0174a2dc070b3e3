"""Which (input size, output size) pairs break "a tile of T output pixels plus its halo touches at most N source cells"?

Several kernels stage the low-resolution cells a tile of output pixels can reach in a fixed window (LDS or registers): the
window starts at the first source cell of the tile's first halo pixel and has N slots.  Whether a geometry fits is a
question about float32 rounding of torch's source-index rule, tile by tile — at a non-integer factor the fractional phase of
the tile's first pixel drifts from tile to tile and the window is widest where it comes close to 1.  This module restates
the rule and the window in plain numpy (no kernel's code is copied) so that the GPU tests can take their geometries from
it and a reader can see why each pair was chosen.
"""
import numpy as np

F32 = np.float32


def src_index(dst, n_in, n_out, align_corners):
    """torch's F.interpolate(mode="bilinear") source cells of output pixel(s) `dst`, in float32 as the kernels (and torch's
    float32 kernels) compute them: (i0, i1, l0, l1) with out[dst] = l0 * in[i0] + l1 * in[i1].
    align_corners=False: s = max(n_in / n_out * (dst + 0.5) - 0.5, 0);  True: s = (n_in - 1) / (n_out - 1) * dst."""
    d = np.asarray(dst)
    df = d.astype(F32)
    if align_corners:
        scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
        s = (scale * df).astype(F32)
    else:
        scale = F32(n_in) / F32(n_out)
        s = (scale * (df + F32(0.5))).astype(F32) - F32(0.5)
        s = np.maximum(s, F32(0)).astype(F32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def _windows(n_in, n_out, tile, halo, cells, align_corners):
    """Per tile start: (lost weight per window pixel [tiles, tile + 2 halo], pixel index, span in cells, phase of the first pixel)."""
    i0, i1, l0, l1 = src_index(np.arange(n_out), n_in, n_out, align_corners)
    starts = np.arange(0, n_out, tile)
    first = np.maximum(starts - halo, 0)
    px = starts[:, None] - halo + np.arange(tile + 2 * halo)[None, :]
    valid = (px >= 0) & (px < n_out)
    pc = np.clip(px, 0, n_out - 1)
    base = i0[first][:, None]
    out0 = valid & (i0[pc] - base >= cells)
    out1 = valid & (i1[pc] - base >= cells)
    lost = np.maximum(np.where(out0, l0[pc], F32(0)), np.where(out1, l1[pc], F32(0)))
    span = np.where(valid, i1[pc], 0).max(axis=1) - i0[first] + 1
    return lost, pc, span, l1[first]


def window_loss(n_in, n_out, tile, halo, cells, align_corners):
    """Model of a tiled kernel's source window: for every tile start t (0, tile, 2 tile, ...) the window's base is i0 of the
    first halo pixel max(t - halo, 0) and `cells` slots follow; the pixels t - halo .. t + tile - 1 + halo inside the map put
    their two weights into slots i0 - base and i1 - base.  Returns (loss, tile_index, pixel): the largest bilinear weight
    that falls outside its window and where — (0.0, -1, -1) when every weight has a slot."""
    lost, pc, _, _ = _windows(n_in, n_out, tile, halo, cells, align_corners)
    k = int(np.argmax(lost))
    t, j = divmod(k, lost.shape[1])
    loss = float(lost[t, j])
    return (loss, t, int(pc[t, j])) if loss > 0.0 else (0.0, -1, -1)


def window_span(n_in, n_out, tile, halo, align_corners):
    """(span, phase): the largest number of source cells any tile's window pixels reach (by index, weight or not), and among
    the tiles that reach it the largest fractional phase l1 of the window's first pixel (the closer to 1, the closer the
    next rounding step is to pushing the last pixel one cell further)."""
    _, _, span, phase = _windows(n_in, n_out, tile, halo, 1 << 30, align_corners)
    m = int(span.max())
    return m, float(phase[span == m].max())


def worst_geometries(tile, halo, cells, n_in_max, factor_lo, factor_hi, align_corners, k):
    """Search n_in = 1 .. n_in_max, n_out in [factor_lo * n_in, factor_hi * n_in].  Returns (losing, near):
    losing — the k pairs with the largest lost weight, as (n_in, n_out, loss, tile_index, pixel), worst first;
    near   — the k pairs with zero loss closest to losing: largest cell span, then phase nearest 1, as (n_in, n_out, span, phase)."""
    losing, near = [], []
    for n_in in range(1, n_in_max + 1):
        lo, hi = int(np.ceil(factor_lo * n_in)), int(np.floor(factor_hi * n_in))
        for n_out in range(max(lo, 1), hi + 1):
            loss, t, p = window_loss(n_in, n_out, tile, halo, cells, align_corners)
            if loss > 0.0:
                losing.append((n_in, n_out, loss, t, p))
            else:
                near.append((n_in, n_out) + window_span(n_in, n_out, tile, halo, align_corners))
    losing.sort(key=lambda e: (-e[2], e[0], e[1]))
    near.sort(key=lambda e: (-e[2], -e[3], e[0], e[1]))
    return losing[:k], near[:k]


def fits(n_in, n_out, tile, halo, cells, align_corners=False):
    """Index form of the same question (what a launcher can check on the host): no window pixel's i1 lies `cells` or more
    past the window base, whatever its weight."""
    return window_span(n_in, n_out, tile, halo, align_corners)[0] <= cells


def head_tile_rows(h, w, H, W):
    """The row count a 3-row x 4-column-window head kernel with 32-pixel column tiles can use: the largest power of two
    R <= 32 whose row tiles (+1 halo) stay within 3 cell rows, 0 when none does or a 32-column tile (+1 halo) reaches more
    than 4 cell columns."""
    if not fits(w, W, 32, 1, 4):
        return 0
    for r in (32, 16, 8, 4, 2, 1):
        if fits(h, H, r, 1, 3):
            return r
    return 0
