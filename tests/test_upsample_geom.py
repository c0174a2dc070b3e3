"""CPU: the geometry finder the ragged-size GPU tests take their cases from (tests/upsample_geom.py) — its source-index rule
against torch itself, and its window model against the pairs at which a 32-pixel tile with one halo pixel and a three-cell
window is known to lose a bilinear weight."""
import numpy as np
import pytest
import torch

from tests import upsample_geom as G

N_OUTS = (1, 2, 3, 5, 7, 16, 31, 32, 33, 64, 100, 127, 128, 257, 819, 945, 1009, 1024, 1074, 1100)


def _torch_matrix(n_in, n_out, align):
    """The [n_out, n_in] interpolation matrix torch applies along one axis: one-hot float64 rows through F.interpolate."""
    eye = torch.eye(n_in, dtype=torch.float64).view(n_in, 1, 1, n_in)             # image k = one-hot row k, height 1
    out = torch.nn.functional.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=align)
    return out.view(n_in, n_out).t().numpy()


@pytest.mark.parametrize("align", [False, True])
def test_src_index_reproduces_torch(align):
    """Every n_in <= 40 against a spread of n_out up to 1100 (upsampling, identity n_out == n_in, downsampling): the weights
    src_index puts on its two cells are torch's.  torch computes the float64 case in float64 and src_index in float32, so the
    source coordinate differs by its float32 rounding: three roundings (scale, product, difference) of a number <= n_in, i.e.
    <= 3 n_in 2^-24 — compared as dense matrices, so that a coordinate an ulp either side of a cell border (index moves, weight
    ~0) is the small difference it is."""
    worst = 0.0
    for n_in in range(1, 41):
        for n_out in sorted(set(N_OUTS + (n_in, max(n_in - 1, 1), n_in + 1, 2 * n_in, 4 * n_in - 3, 4 * n_in + 1, 32 * n_in, 33 * n_in - 1))):
            if n_out > 1100:
                continue
            i0, i1, l0, l1 = G.src_index(np.arange(n_out), n_in, n_out, align)
            assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
            assert l0.dtype == np.float32 and l1.dtype == np.float32 and (l1 >= 0).all() and (l1 < 1 + 1e-6).all()
            m = np.zeros((n_out, n_in))
            np.add.at(m, (np.arange(n_out), i0), l0.astype(np.float64))
            np.add.at(m, (np.arange(n_out), i1), l1.astype(np.float64))
            err = np.abs(m - _torch_matrix(n_in, n_out, align)).max()
            worst = max(worst, err / n_in)
            assert err <= 3 * n_in * 2.0 ** -24, (n_in, n_out, align, err)
    print(f"src_index vs torch (align_corners={align}): worst weight error {worst:.2e} per input cell, bound {3 * 2.0 ** -24:.2e}")


def test_src_index_scalar_and_float32_rule():
    i0, i1, l0, l1 = G.src_index(704, 25, 819, False)
    s = np.float32(25) / np.float32(819) * np.float32(704.5) - np.float32(0.5)
    assert (int(i0), int(i1)) == (int(s), int(s) + 1) and float(l1) == float(np.float32(s - np.float32(int(s))))
    assert G.src_index(0, 5, 20, False)[0] == 0 and float(G.src_index(0, 5, 20, False)[3]) == 0.0       # clamped at 0
    assert [int(v) for v in G.src_index(19, 5, 20, True)[:2]] == [4, 4]                                      # last cell, no neighbour


@pytest.mark.parametrize("pair", [(25, 819), (29, 945), (31, 1009), (33, 1074)])
def test_three_cell_window_loses_weight_at_factors_between_32_and_33(pair):
    """A 32-pixel tile + 1 halo pixel either side against a 3-cell window: factor >= 32 does not make it fit."""
    loss, tile, pixel = G.window_loss(*pair, tile=32, halo=1, cells=3, align_corners=False)
    print(f"{pair[0]} -> {pair[1]}: weight {loss:.3e} of pixel {pixel} (tile {tile}) falls outside the window")
    assert loss > 1e-3 and pixel == 32 * tile + 32 and not G.fits(*pair, 32, 1, 3)
    # the lost weight is l1 of the tile's last halo pixel: its second cell is the window's fourth
    i0, i1, l0, l1 = G.src_index(pixel, *pair, False)
    base = G.src_index(32 * tile - 1, *pair, False)[0]
    assert int(i1) - int(base) == 3 and int(i0) - int(base) == 2 and loss == float(l1)
    # half the tile always fits at these factors (17 / 32 of a cell crosses one border)
    assert G.window_loss(*pair, tile=16, halo=1, cells=3, align_corners=False)[0] == 0.0 and G.fits(*pair, 16, 1, 3)


@pytest.mark.parametrize("pair", [(32, 1024), (4, 128), (5, 160), (3, 100)])
def test_three_cell_window_is_clean_at_the_sizes_the_suite_used(pair):
    assert G.window_loss(*pair, tile=32, halo=1, cells=3, align_corners=False) == (0.0, -1, -1)
    assert G.fits(*pair, 32, 1, 3)


def test_window_loss_counts_over_the_stride_32_band():
    """h <= 79, H in [32 h, 34 h]: 1094 pairs lose weight (every one of them has H >= 32 h)."""
    n = sum(G.window_loss(h, H, 32, 1, 3, False)[0] > 0 for h in range(1, 80) for H in range(32 * h, 34 * h + 1))
    assert n == 1094


def test_worst_geometries_orders_and_separates():
    losing, near = G.worst_geometries(32, 1, 3, 33, 32, 34, False, 6)
    assert len(losing) == 6 and len(near) == 6
    assert all(e[2] > 0 for e in losing) and [e[2] for e in losing] == sorted((e[2] for e in losing), reverse=True)
    assert (33, 1074) in [e[:2] for e in losing] and (29, 945) in [e[:2] for e in losing]
    for n_in, n_out, span, phase in near:
        assert G.window_loss(n_in, n_out, 32, 1, 3, False)[0] == 0.0 and 0.0 <= phase < 1.0 + 1e-6
    assert [(-e[2], -e[3]) for e in near] == sorted((-e[2], -e[3]) for e in near)
    # identity and downsampling are searched too, with either corner convention
    losing, near = G.worst_geometries(32, 1, 4, 12, 0.5, 1.0, True, 3)
    assert losing and all(e[1] <= e[0] for e in losing)


def test_head_tile_rows_steps_down_with_the_factor():
    """The row counts the 3 x 4-cell head window allows on a 4-row map: every power of two from 32 to 1 and none."""
    got = {r: [H for H in range(4, 160) if G.head_tile_rows(4, 1, H, 32) == r] for r in (32, 16, 8, 4, 2, 1, 0)}
    assert all(got[r] for r in got), got
    assert 128 in got[32] and 125 in got[32] and 100 in got[16] and 4 in got[0]
    assert G.head_tile_rows(32, 2, 1000, 64) == 16                 # 1000 / 32: what a stride-32 encoder gives a 1000-row frame
    assert G.head_tile_rows(1, 5, 32, 32) == 0 and G.head_tile_rows(1, 4, 32, 32) == 32     # five cell columns in one 32-pixel tile
