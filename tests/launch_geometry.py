"""How the launchers split their work, restated in plain Python (no GPU): chunks per plane, blocks per image, trips of a
grid-stride loop, spans per row, lanes per LayerNorm row, and the item counts of the capped 1-D launchers.

The constants are read out of the HIP sources, so a changed constant moves this model with it; the RULES are restated by hand from
the launchers named next to each function.  tests/test_launch_geometry.py holds the case tables of tests/test_gpu_launch_geometry.py
against this model; the GPU file asks the library itself where it exports the count."""
import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "adverse_weather_semantic_segmentation_robustness_benchmark_amd" / "csrc"


def _const(file: str, pattern: str) -> int:
    m = re.search(pattern, (CSRC / file).read_text())
    assert m, f"{file}: no match for {pattern!r} — the source moved, restate the rule here"
    return int(m.group(1))


BN_CHUNK = _const("bntrain.hip", r"constexpr int BN_CHUNK = (\d+);")
BN_T = _const("bntrain.hip", r"constexpr int BN_T = (\d+);")
DW_CHUNK = _const("dwtrain.hip", r"constexpr int DW_CHUNK = (\d+);")
AWSEG_CUS = _const("awseg_common.h", r"#define AWSEG_CUS (\d+)")
MAX_BLOCKS = AWSEG_CUS * _const("awseg_common.h", r"awseg_grid_1d\(int64_t work_items, int per_block, int max_blocks = AWSEG_CUS \* (\d+)\)")
LOSS_THREADS = _const("loss.hip", r"constexpr int kThreads = (\d+);")
LOSS_CAP = AWSEG_CUS * _const("loss.hip", r"int64_t cap = \(AWSEG_CUS \* (\d+) \+ batch - 1\)")
BACKBONE_THREADS = _const("backbone.hip", r"constexpr int kThreads = (\d+);")
HEADS_THREADS = _const("heads.hip", r"constexpr int kThreads = (\d+);")
SMALLOPS_THREADS = _const("smallops.hip", r"constexpr int SO_T = (\d+);")
STEM_SPAN = _const("smallops.hip", r"const int spans = \(W \+ \d+\) / (\d+);")
DEPTH_UP_CAP = _const("backbone.hip", r"awseg_grid_1d\(\(int64_t\)height \* width, kThreads, (\d+)\)")
UP_QUADS = _const("backbone.hip", r"kUpQuads = (\d+)")
ASPP_SLICE = _const("heads.hip", r"constexpr int kAsppSlice = (\d+);")
ASPP_LDS_QUADS = _const("heads.hip", r"constexpr int kAsppLdsQuads = (\d+);")
WAVE = 64


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------------ the rules
def grid_1d(items: int, per_block: int, max_blocks: int = None) -> int:
    """awseg_grid_1d (awseg_common.h)."""
    return max(1, min(ceil_div(items, per_block), MAX_BLOCKS if max_blocks is None else max_blocks))


def stride_loop(items: int, per_block: int, blocks: int) -> dict:
    """A grid of `blocks` x `per_block` lanes walking `items` with `for (v = ...; v < items; v += blocks * per_block)`:
    trips = the most any lane takes; tail = items of the last trip; ragged = the last trip ends inside a wave."""
    per_trip = blocks * per_block
    trips = ceil_div(items, per_trip)
    tail = items - (trips - 1) * per_trip
    return {"blocks": blocks, "trips": trips, "tail": tail, "ragged": tail % WAVE != 0}


def capped_1d(items: int, per_block: int = None, max_blocks: int = None) -> dict:
    """Items of a launcher that sizes its grid with awseg_grid_1d(items, kThreads) and loops beyond the cap."""
    per_block = BACKBONE_THREADS if per_block is None else per_block
    out = stride_loop(items, per_block, grid_1d(items, per_block, max_blocks))
    out["items"] = items
    return out


def bn_chunks(hw: int) -> int:
    """bntrain.hip bn_chunks: blocks per (image, channel) plane."""
    return ceil_div(hw, BN_CHUNK)


def bn_nhwc_blocks(hw: int):
    """bn_relu_drop_bwd_dx_nhwc_kernel: (256-pixel blocks per plane, pixels of the last one)."""
    n = ceil_div(hw, 256)
    return n, hw - (n - 1) * 256


def loss_bpi(hw: int, batch: int) -> int:
    """loss.hip loss_bpi: blocks per image of the loss and density kernels."""
    return max(1, min(ceil_div(hw, LOSS_THREADS), ceil_div(LOSS_CAP, max(batch, 1))))


def loss_vec(hw: int) -> int:
    """Pixels per lane of fog_ce_kernel (16-byte aligned tensors): 4 when the plane is whole float4s, else 1."""
    return 4 if hw % 4 == 0 else 1


def loss_instance(hw: int, classes: int) -> str:
    v = loss_vec(hw)
    return f"vec{v}_ct{classes if v == 4 and classes == 19 else 0}"


def loss_loop(hw: int, batch: int, vec: int = None) -> dict:
    """The per-image grid-stride loop of fog_ce_kernel (vec = loss_vec) / the density kernels (vec = 1)."""
    vec = loss_vec(hw) if vec is None else vec
    return stride_loop(hw // vec, LOSS_THREADS, loss_bpi(hw, batch))


def layernorm_lanes(channels: int) -> int:
    """awseg_layernorm_rows: lanes per row (the kernel instance)."""
    nchunk = channels // 4
    lanes = 8
    while lanes < 64 and lanes * 4 < nchunk:
        lanes <<= 1
    while lanes < 64 and lanes < nchunk and nchunk <= 64:
        lanes <<= 1
    assert nchunk <= 4 * lanes
    return lanes


def layernorm_loop(rows: int, channels: int) -> dict:
    per_block = BACKBONE_THREADS // layernorm_lanes(channels)
    out = stride_loop(rows, per_block, grid_1d(rows, per_block))
    out["ragged"] = out["tail"] % per_block != 0                 # the last block has rows to spare
    return out


def stem_spans(width: int):
    """stem_image_kernel: (spans per row, pixels of the last span)."""
    n = ceil_div(width, STEM_SPAN)
    return n, width - (n - 1) * STEM_SPAN


# ------------------------------------------------------------------ item counts of the launchers that call awseg_grid_1d(items, kThreads)
def conv_out(n: int, k: int, stride: int, pad: int, dil: int = 1) -> int:
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def items_bias_act(n_pixels: int, channels: int) -> int:
    return n_pixels * (channels // 4)


def items_im2col(b, h, w, c, kh, kw, stride, pad, k_padded=None, dil=1) -> int:
    kp = kh * kw * c if k_padded is None else k_padded
    return b * conv_out(h, kh, stride, pad, dil) * conv_out(w, kw, stride, pad, dil) * (kp // 4)


def items_maxpool(b, h, w, c) -> int:
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return b * ho * ceil_div(wo, 2) * (c // 4)


def items_dwconv(b, h, w, c, dil=1):
    """(kernel, items) of awseg_dwconv3x3_nhwc."""
    if dil == 1 and w >= 8 and h >= 2:
        return "strip2", b * ceil_div(h, 2) * ceil_div(w, 8) * (c // 4)
    if dil == 1 and w >= 8:
        return "strip", b * h * ceil_div(w, 8) * (c // 4)
    return "plain", b * h * w * (c // 4)


def items_upcat(b, h, w, ca, ch) -> int:
    """awseg_dwconv3x3_upcat_nhwc on a x4 decoder step: the strip kernel's items.  Where Ca / 4 is a multiple of kUpQuads the
    upsampled channels go to the LDS kernel (its 64 KB budget holds at every width tested) and the strip kernel keeps hi's."""
    H, W = 4 * h, 4 * w
    c4_lo = ca // 4 if (ca // 4) % UP_QUADS == 0 else 0
    return b * H * ceil_div(W, 8) * ((ca + ch) // 4 - c4_lo)


def items_upsample(planes, h, w, H, W, align):
    """(kernel, items) of awseg_upsample_bilinear_strided on a planar map."""
    f32 = np.float32
    if align:
        sy = f32(h - 1) / f32(H - 1) if H > 1 else f32(0)
        sx = f32(w - 1) / f32(W - 1) if W > 1 else f32(0)
    else:
        sy, sx = f32(h) / f32(H), f32(w) / f32(W)
    if W % 4 == 0 and sx * f32(3) < 1 and sy * f32(3) < 1:
        return "4x4", planes * ceil_div(H, 4) * (W // 4)
    return "rows", planes * H * ceil_div(W, 4)


def aspp_kernel(w: int, c: int) -> str:
    """Which kernel awseg_aspp_depthwise3 launches (defaults): only 'flat' sizes its grid with awseg_grid_1d."""
    q = c // 4
    if q % ASPP_LDS_QUADS == 0 and 64 <= w * ASPP_LDS_QUADS <= 1024:
        return "lds"
    return "rows" if q % ASPP_SLICE == 0 else "flat"


def items_aspp(b, h, w, c) -> int:
    return b * h * w * (c // 4)


def depth_up_loop(H: int, W: int) -> dict:
    """depth_up_combine_kernel: per image, capped at DEPTH_UP_CAP blocks."""
    return capped_1d(H * W, BACKBONE_THREADS, DEPTH_UP_CAP)


# ------------------------------------------------------------------ density from depth: the float64 statement of loss.hip's three kernels
def density_depth_input(batch: int, h: int, w: int, seed: int) -> np.ndarray:
    """Depth maps for the density cases: a vertical ramp plus uniform noise, in float32."""
    rs = np.random.RandomState(seed)
    ramp = np.linspace(0.0, 1.0, h, dtype=np.float64)[None, :, None]
    return (0.5 * ramp + rs.rand(batch, h, w) + 0.05 * rs.rand(batch, 1, 1)).astype(np.float32)


def density_from_depth_ref(depth: np.ndarray, margin: float = 1e-5):
    """float64: (density, keep).  min / max / mean gradient magnitude over the WHOLE tensor; forward differences with the last
    row and column replicated; keep = pixels whose gradient magnitude is further than margin * mean from the threshold."""
    d = np.asarray(depth, np.float64)
    mn, mx = d.min(), d.max()
    gx = np.zeros_like(d)
    gy = np.zeros_like(d)
    if d.shape[2] > 1:
        gx[:, :, :-1] = np.abs(d[:, :, 1:] - d[:, :, :-1])
        gx[:, :, -1] = gx[:, :, -2]
    if d.shape[1] > 1:
        gy[:, :-1, :] = np.abs(d[:, 1:, :] - d[:, :-1, :])
        gy[:, -1, :] = gy[:, -2, :]
    mag = np.sqrt(gx * gx + gy * gy + 1e-8)
    mean = mag.mean()
    f = (d - mn) / (mx - mn + 1e-8) * 0.7 - np.where(mag > mean, 0.3, 0.0)
    return np.clip(f, 0.0, 1.0), np.abs(mag - mean) > margin * mean
