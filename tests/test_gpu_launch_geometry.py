"""-m gpu: every kernel's second grid trip and chunk seam against float64.

Most launchers split their work by a rule the small unit shapes never trigger: a fixed chunk per block (bntrain.hip), a block count
capped at AWSEG_CUS * 8 (loss.hip, awseg_grid_1d) or a span per wave (the stem image).  The cases below are the smallest shapes
that cross each rule — tests/launch_geometry.py restates the rules, tests/test_launch_geometry.py holds every table below against
that model on the CPU, and where the library exports the count the test asks the library too.  A wrong seam drops or doubles
elements, an O(1) error; references are float64 expressions written here from the float32 inputs.

A skipped element must not hold the right value by accident: the ops allocate with torch.empty and the caching allocator hands
freed blocks back, so every case whose op allocates its result first runs the op on DIFFERENT inputs into tensors it keeps
(`keep`), and keeps every result alive until its comparison; the in-place ops work on buffers the test filled itself.

Audit of the launchers that size their grid with awseg_grid_1d (cap: 2048 blocks x 256 lanes = 524288 items; items by
tests/launch_geometry.py; "largest" = the largest case of the unit tests in test_gpu_kernels.py / test_gpu_ragged_geometry.py):

  launcher                         largest existing unit case                                   items    crosses  case added here
  bias_act_nhwc_                   test_maxpool3x3s2_nhwc_equals_torch (1, 64, 128, 64)          32768    no       AUDIT_BIAS_ACT
  im2col_nhwc                      test_im2col_patch_gemm_is_the_convolution (2, 12, 16, 128..)  27648    no       AUDIT_IM2COL
  maxpool3x3s2_nhwc (plain)        test_maxpool3x3s2_nhwc_equals_torch (1, 64, 128, 64)          16384    no       AUDIT_MAXPOOL
  maxpool3x3s2_nhwc (shift + ReLU) the same case                                                 16384    no       AUDIT_MAXPOOL
  dwconv3x3_nhwc, strip2           test_depthwise_conv3x3_train_... (1, 64, 96, 304, d=1)        29184    no       AUDIT_DWCONV["strip2"]
  dwconv3x3_nhwc, strip (1 row)    none: no unit case has a one-row map                              0    no       AUDIT_DWCONV["strip"]
  dwconv3x3_nhwc, plain            test_depthwise_conv3x3_train_... (2, 20, 24, 64, d=12)        15360    no       AUDIT_DWCONV["plain"]
  dwconv3x3_upcat (strip kernel)   test_dwconv3x3_upcat_matches_torch (1, 16, 32, 256, 48)       12288    no       AUDIT_UPCAT
  upsample_bilinear, 4x4 kernel    test_upsample_bilinear_matches_torch (1, 19, 256, 512 -> 1024, 2048)  2490368  YES  nothing added
  upsample_bilinear, row kernel    test_upsample_bilinear_matches_torch (1, 2, 5, 9 -> 33, 70)    1188    no       AUDIT_UPSAMPLE_ROWS
  aspp_depthwise3 (flat kernel)    test_aspp_depthwise3 (2, 20, 28, 16)                           4480    no       AUDIT_ASPP
  depth_upsample_combine (cap 1024 blocks = 262144 pixels per image)
                                   test_depth_upsample_combine_matches_torch (1, 64, 128 -> 1024, 2048)  2097152  YES  nothing added
  stem_image_fill (a wave per 256-pixel span; cap = 8192 spans)
                                   test_stem_image_fill_matches_strided_copy (2, 3, 9, 37)          18    no       AUDIT_STEM
  layernorm_rows                   test_layernorm_rows (1000, 32): 32 of 2048 blocks                 -    no       LAYERNORM_CASES
(the other kernels of awseg_aspp_depthwise3 — lds, rows, walk, sliced — size their grids by units, not by awseg_grid_1d;
awseg_change_strata calls awseg_grid_1d with a per-image cap of its own, like loss_bpi's, and is not part of this audit.)

Worst errors measured on an MI355X are written in each test's docstring."""
import copy

import numpy as np
import pytest
import torch

from tests import launch_geometry as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(native):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _report(name, err, gate):
    print(f"{name}: worst {err:.3e} (gate {gate:.3e})")
    return err


# ------------------------------------------------------------------ 1. BatchNorm -> ReLU -> Dropout2d (bntrain.hip)
# (B, C, H, W, p, chunks per plane, pixels of the last 256-pixel block of the channels-last dx kernel or None)
BN_CASES = [
    (2, 3, 128, 128, 0.1, 1, None),          # exactly one full chunk
    (2, 3, 4, 4097, 0.1, 2, None),           # 16388 floats: the second chunk is one float4
    (3, 5, 132, 280, 0.5, 3, None),          # 36960 floats: three chunks, ragged last; c, b and chunk all above 0
    (2, 64, 4, 4097, 0.1, 2, 4),             # + channels-last dx: two 32-channel slices, last block of 4 pixels
    (2, 32, 132, 280, 0.0, 3, 96),           # + channels-last dx: last block of 96 pixels; no dropout
]


@pytest.mark.parametrize("cfg", BN_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_bn_relu_dropout2d_train_across_chunks(ops, native, cfg):
    """ops.bn_relu_dropout2d_train against float64 nn.BatchNorm2d(train) -> ReLU -> the same Dropout2d draw, with planes of one
    full chunk, one chunk + one float4, and three chunks with a ragged last.  x carries a different offset per (image, channel,
    chunk), so a partial sum filed under another channel's index moves that channel's mean.  Gate 3e-5 * max(1, |ref|) as in
    test_bn_relu_dropout2d_train_matches_the_module_graph (the sums are float64: more chunks cost no accuracy).
    Measured worst over the five cases: output 7.6e-7, dx 4.3e-7, dgamma 3.2e-5, dbeta 1.7e-5, running statistics 2.4e-7 — each
    under 0.5 % of its gate (the gates scale with |ref|: dgamma and dbeta are sums over B * H * W elements)."""
    B, C, H, W, p, chunks, last_block = cfg
    hw = H * W
    assert native.lib().awseg_bn_train_workspace(B, C, hw) // (16 * B * C) == chunks == G.bn_chunks(hw)
    g = _gen(sum(int(v * 10) for v in cfg[:5]))
    off = torch.randn(B, C, chunks, device="cuda", generator=g) * 1.5
    chunk_of = torch.arange(hw, device="cuda") // G.BN_CHUNK
    x = (torch.randn(B, C, hw, device="cuda", generator=g) * 2.0 + 0.5 + off[:, :, chunk_of]).view(B, C, H, W).requires_grad_(True)
    gy = torch.randn(B, C, H, W, device="cuda", generator=g)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3); bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0)
    ref_bn = torch.nn.BatchNorm2d(C).cuda().double().train()
    ref_bn.load_state_dict(bn.state_dict())
    relu, drop = torch.nn.ReLU(), (torch.nn.Dropout2d(p).train() if p > 0 else None)
    assert ops.bn_relu_dropout2d_train_ok(x, bn, relu, drop)
    # the same op on different inputs, into tensors that stay alive: what torch.empty hands out next holds none of the values below
    bn_other = copy.deepcopy(bn)
    x_other = (1.0 - x.detach()).requires_grad_(True)
    y_other = ops.bn_relu_dropout2d_train(x_other, bn_other, drop)
    y_other.backward(gy.flip(0))
    keep = [y_other, x_other.grad, bn_other.weight.grad, bn_other.bias.grad]
    torch.manual_seed(1234)
    y = ops.bn_relu_dropout2d_train(x, bn, drop)
    y.backward(gy)
    xd = x.detach().double().requires_grad_(True)
    torch.manual_seed(1234)
    noise = torch.empty(B, C, 1, 1, device="cuda").bernoulli_(1.0 - p).div_(1.0 - p).double() if p > 0 else 1.0
    yr = torch.relu(ref_bn(xd)) * noise
    yr.backward(gy.double())
    for name, a, b in (("output", y.detach(), yr.detach()), ("dx", x.grad, xd.grad), ("dgamma", bn.weight.grad, ref_bn.weight.grad),
                       ("dbeta", bn.bias.grad, ref_bn.bias.grad), ("running_mean", bn.running_mean, ref_bn.running_mean),
                       ("running_var", bn.running_var, ref_bn.running_var)):
        gate = 3e-5 * max(1.0, b.abs().max().item())
        err = _report(f"bn {cfg[:5]} {name}", (a.double() - b).abs().max().item(), gate)
        assert err < gate, (cfg, name, err)
    assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked) == 1
    if last_block is not None:
        # the input gradient handed back over channels-last memory, taken from a non-leaf in front (its incoming gradient keeps
        # the Function's own layout): the planar values, bit for bit
        assert C % 32 == 0 and G.bn_nhwc_blocks(hw)[1] == last_block
        xi = x.detach().clone().requires_grad_(True)
        torch.manual_seed(1234)
        mid = xi * 1.0
        seen = []
        mid.register_hook(lambda gr: seen.append(gr))
        ops.bn_relu_dropout2d_train(mid, bn, drop, dx_channels_last=True).backward(gy)
        assert len(seen) == 1 and seen[0].permute(0, 2, 3, 1).is_contiguous()
        assert torch.equal(seen[0].contiguous(), x.grad)
    del keep


# ------------------------------------------------------------------ 2. loss forward / backward (loss.hip fog_ce_kernel)
# (name, B, C, H, W, label dtype, density given, kernel instance, blocks per image, trips, lanes of the last trip)
LOSS_CASES = [
    ("ct19_vec4", 2048, 19, 4, 385, torch.uint8, True, "vec4_ct19", 1, 2, 129),
    ("runtime_c_vec4", 2048, 7, 4, 385, torch.int64, False, "vec4_ct0", 1, 2, 129),
    ("one_pixel_per_lane", 2048, 19, 9, 37, torch.uint8, True, "vec1_ct0", 1, 2, 77),
    ("mid_batch", 300, 19, 80, 100, torch.uint8, True, "vec4_ct19", 7, 2, 208),       # blocks of one image take 2, 1, ..., 1 trips
]
LOSS_ORACLE_SHAPES = [(2, 19, 16, 24), (1, 19, 7, 9), (2, 5, 8, 8)]                      # test_loss_vs_oracle's
LOSS_GRAD_GATE = 2e-5      # on the gradient normalised by grad_scale = B * hw (coefficient 1, entries O(1)): v_exp_f32 / v_log_f32 at
                           # ~1e-6 relative (loss.hip's header) x weight 1 + 2 density <= 3 x focal factor q^2 + 2 ce pt q <= 2 = 6e-6, x3


def _loss_reference(x, lab, dens, focal, sens, classes):
    """float64: (per-pixel loss, mean, d(sum of the per-pixel losses) / d logits, out-of-range mask)."""
    xd = x.double().requires_grad_(True)
    t = lab.long()
    bad = (t < 0) | (t >= classes)
    ce = -torch.log_softmax(xd, 1).gather(1, torch.where(bad, torch.zeros_like(t), t)[:, None]).squeeze(1)
    if focal:
        ce = (1.0 - torch.exp(-ce)) ** 2 * ce
    if dens is not None:
        ce = ce * (1.0 + sens * dens.double())
    pix = torch.where(bad, torch.zeros_like(ce), ce)
    (grad,) = torch.autograd.grad(pix.sum(), xd)
    return pix.detach(), pix.detach().mean().item(), grad, bad


def _loss_check(ops, name, x, lab, dens, classes, n_bad):
    B, hw = x.shape[0], x[0, 0].numel()
    scale = torch.full((1,), float(B * hw), device="cuda")
    worst = {"mean": 0.0, "pixel": 0.0, "grad": 0.0}
    for focal in (False, True):
        oob_other = torch.zeros(1, dtype=torch.int64, device="cuda")
        keep = [ops.fog_ce_forward(-x, lab, dens, focal, 2.0, oob_other, want_pixel=True), ops.fog_ce_backward(-x, lab, dens, focal, 2.0, scale)]
        oob = torch.zeros(1, dtype=torch.int64, device="cuda")
        mean, pix = ops.fog_ce_forward(x, lab, dens, focal, 2.0, oob, want_pixel=True)
        grad = ops.fog_ce_backward(x, lab, dens, focal, 2.0, scale)
        ref_pix, ref_mean, ref_grad, bad = _loss_reference(x, lab, dens, focal, 2.0, classes)
        assert int(bad.sum()) == n_bad and oob.item() == n_bad
        if n_bad:
            assert (pix[bad] == 0).all() and (grad.permute(0, 2, 3, 1)[bad] == 0).all()
        e_mean = abs(mean.item() - ref_mean)
        e_pix = (pix.double() - ref_pix).abs().max().item()
        e_grad = (grad.double() - ref_grad).abs().max().item()
        print(f"loss {name} {'focal' if focal else 'ce'}: mean {e_mean:.3e} (gate 1e-5), pixel {e_pix:.3e} (gate 1e-4), "
              f"normalised gradient {e_grad:.3e} (gate {LOSS_GRAD_GATE:.0e})")
        assert e_mean < 1e-5 and e_pix < 1e-4
        assert e_grad < LOSS_GRAD_GATE
        worst = {"mean": max(worst["mean"], e_mean), "pixel": max(worst["pixel"], e_pix), "grad": max(worst["grad"], e_grad)}
        del keep
    return worst


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: c[0])
def test_loss_second_trip_vs_float64(ops, native, case):
    """ops.fog_ce_forward / fog_ce_backward, CE and focal, at batches where loss_bpi's cap bites and the grid-stride loop takes a
    second trip with a ragged last wave, in each kernel instance (CT = 19 float4, runtime-C float4, one pixel per lane) and with
    blocks of one image taking different numbers of trips.  Labels >= C (and < 0 for int64) sit at known pixels of the second
    trip: counted, zero loss, zero gradient.  Forward gates are the project's (1e-5 mean, 1e-4 per pixel); the gradient is
    taken with grad_scale = B * hw and gated at LOSS_GRAD_GATE absolute.
    Measured worst (all cases, CE and focal): mean 4.0e-7, per pixel 1.05e-5, normalised gradient 2.0e-6 (a tenth of the gate:
    the derivation of LOSS_GRAD_GATE holds)."""
    name, B, C, H, W, ldt, with_density, instance, blocks, trips, tail = case
    hw = H * W
    vec = G.loss_vec(hw)
    assert native.lib().awseg_loss_partials(B, hw) // B == blocks == G.loss_bpi(hw, B)
    assert hw // vec > blocks * 256 and G.loss_instance(hw, C) == instance
    g = _gen(1000 + B + C + hw)
    x = torch.randn(B, C, H, W, device="cuda", generator=g) * 3
    lab = torch.randint(0, C, (B, H, W), device="cuda", generator=g).to(ldt)
    dens = torch.rand(B, H, W, device="cuda", generator=g) if with_density else None
    # out-of-range labels in the second trip: its first lane's first and last pixel, and the plane's last pixel
    first = blocks * 256 * vec
    bad_values = (255, C, 200) if ldt == torch.uint8 else (-1, C, 1000)
    flat = lab.view(B, hw)
    for img, pixel, value in zip((0, B - 1, B // 2), (first, first + vec - 1, hw - 1), bad_values):
        flat[img, pixel] = value
    _loss_check(ops, name, x, lab, dens, C, 3)


@pytest.mark.parametrize("shape", LOSS_ORACLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_normalised_gradient_at_the_oracle_shapes(ops, shape):
    """test_loss_vs_oracle gates its gradient at 1e-6 absolute whatever 1 / n is; the same shapes here with the normalised gate.
    Measured worst: normalised gradient 8.3e-7 (mean 5.2e-7, per pixel 4.8e-6)."""
    g = _gen(77 + sum(shape))
    x = torch.randn(*shape, device="cuda", generator=g) * 3
    lab = torch.randint(0, shape[1], (shape[0],) + shape[2:], device="cuda", generator=g).to(torch.uint8)
    dens = torch.rand(shape[0], *shape[2:], device="cuda", generator=g)
    _loss_check(ops, f"oracle shape {shape}", x, lab, dens, shape[1], 0)


# ------------------------------------------------------------------ 3. density from depth (loss.hip density_* kernels)
# (B, H, W, seed, blocks per image, trips, pixels of the last trip)
DENSITY_CASES = [
    (2048, 17, 19, 5, 1, 2, 67),             # 2048 partials for the one-wave finish
    (300, 40, 50, 6, 7, 2, 208),
]
DENSITY_MARGIN = 1e-5                        # pixels with |mag - mean| <= margin * mean (float64) are left out: the threshold may fall either way
DENSITY_MAX_LEFT_OUT = 1e-3


@pytest.mark.parametrize("case", DENSITY_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_density_from_depth_second_trip_vs_float64(ops, native, case):
    """ops.fog_density_from_depth against the float64 statement of its three kernels (tests/launch_geometry.py), 1e-6 absolute
    on every pixel further than DENSITY_MARGIN from the `mag > mean` threshold.  min, max and the mean enter every pixel: one lost
    partial moves the threshold for all of them.
    Measured: worst 6.9e-8 and 7.3e-8; left out 10 of 661504 pixels (0.0015 %) and 6 of 600000 (0.0010 %)."""
    B, H, W, seed, blocks, trips, tail = case
    hw = H * W
    assert native.lib().awseg_loss_partials(B, hw) // B == blocks and hw > blocks * 256
    assert native.lib().awseg_density_workspace(B, hw) == blocks * B * 16 + 64
    depth = G.density_depth_input(B, H, W, seed)
    ref, kept = G.density_from_depth_ref(depth, DENSITY_MARGIN)
    d = torch.from_numpy(depth).cuda()
    keep = ops.fog_density_from_depth(d.flip(0) * 0.5 + 0.1)
    got = ops.fog_density_from_depth(d).cpu().numpy().astype(np.float64)
    left_out = 1.0 - kept.mean()
    err = np.abs(got - ref)[kept].max()
    print(f"density {case[:3]}: worst {err:.3e} (gate 1e-6); left out {int((~kept).sum())} of {kept.size} pixels ({100 * left_out:.4f} %, limit 0.1 %)")
    assert left_out <= DENSITY_MAX_LEFT_OUT
    assert err <= 1e-6
    del keep


# ------------------------------------------------------------------ 4. stem image (smallops.hip stem_image_kernel)
STEM_B, STEM_H = 2, 5
STEM_CASES = [(256, 1, 256), (257, 2, 1), (300, 2, 44), (515, 3, 3)]         # (W, 256-pixel spans per row, pixels of the last span)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: f"w{c[0]}")
def test_stem_image_fill_across_spans(ops, case, channels):
    """ops.stem_image_fill == the strided copy (torch.equal) for rows of one full span, one span + 1 pixel, two and three spans with
    a ragged last one; the input is a column slice of a wider tensor (stride_y > W); cells outside the interior keep the 7.0 the
    buffer was made with."""
    W, spans, last = case
    assert G.stem_spans(W) == (spans, last)
    g = _gen(300 + W + channels)
    wide = torch.randn(STEM_B, channels, STEM_H, W + 9, device="cuda", generator=g)
    x = wide[..., 4:4 + W]
    assert x.stride(2) == W + 9 and x.stride(3) == 1
    wp = W + 11
    ref = torch.full((STEM_B, STEM_H, wp, 4), 7.0, device="cuda")
    got = ref.clone()
    ref[:, :, 3:3 + W, :channels] = x.permute(0, 2, 3, 1)
    if channels < 4:
        ref[:, :, 3:3 + W, channels:] = 0.0
    ops.stem_image_fill(x, got)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------ 5. LayerNorm rows (backbone.hip layernorm_rows_kernel)
# (rows, C, lanes per row = kernel instance): rows just past 2048 blocks of 256 / L rows, ragged last block
LAYERNORM_CASES = [
    (65536 + 37, 32, 8),
    (32768 + 21, 64, 16),
    (16384 + 5, 320, 32),                    # 2.5 chunks per lane
    (8192 + 3, 160, 64),                     # 40 of 64 lanes live
    (8192 + 3, 1024, 64),                    # 4 chunks per lane
]


@pytest.mark.parametrize("case", LAYERNORM_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_layernorm_rows_second_trip_vs_float64(ops, case):
    """ops.layernorm_rows against float64 layer_norm with more rows than the capped grid takes in one trip, in each of the four
    instances; inputs and the 2e-5 gate of test_layernorm_rows.
    Measured worst over the five cases: 1.9e-6."""
    rows, C, lanes = case
    loop = G.layernorm_loop(rows, C)
    assert G.layernorm_lanes(C) == lanes and loop["trips"] == 2 and loop["ragged"]
    torch.manual_seed(C + rows)
    x = torch.randn(rows, C, device="cuda") * 3 + 1
    g, b = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    keep = ops.layernorm_rows(x.flip(0), g, b, 1e-5)                 # (a shift or a scale of x would leave the result as it is)
    got = ops.layernorm_rows(x, g, b, 1e-5)
    ref = torch.nn.functional.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    err = _report(f"layernorm {case}", (got.double() - ref).abs().max().item(), 2e-5)
    assert err < 2e-5
    del keep


# ------------------------------------------------------------------ 6. row dot product (smallops.hip rowdot_sigmoid_kernel)
ROWDOT_K = [4, 60, 64, 68, 256]              # one lane; 15 of 16 lanes; one full step; one step + one lane; four steps
ROWDOT_ROWS = [1, 17, 1000]


@pytest.mark.parametrize("k", ROWDOT_K)
def test_rowdot_sigmoid_ragged_steps_vs_float64(ops, k):
    """ops.rowdot_sigmoid with rows shorter than one step of 16 lanes x float4, a ragged last step and several steps; 1, 17 (one
    block + one row) and 1000 rows; with and without bias and sigmoid.  Linear gate 4 k 2^-24 max_r sum_j |x_rj w_j| (the
    forward bound of a length-k float32 dot product, with headroom for the 16-lane tree), computed here in float64; sigmoid
    gate a quarter of it (slope <= 1 / 4) + 2e-7.
    Measured worst error / gate: linear 0.063 (k = 4, 1000 rows, with bias: 4.6e-8 of 7.4e-7), sigmoid 0.18 (k = 4, 17 rows)."""
    g = _gen(40 + k)
    for rows in ROWDOT_ROWS:
        x = torch.randn(rows, k, device="cuda", generator=g)
        w = torch.randn(k, device="cuda", generator=g) * 0.1
        bias = torch.randn(1, device="cuda", generator=g) * 0.1
        lin_gate = 4.0 * k * 2.0 ** -24 * (x.double().abs() @ w.double().abs()).max().item()
        for b in (None, bias):
            v = x.double() @ w.double() + (0.0 if b is None else b.double())
            for sig in (False, True):
                keep = ops.rowdot_sigmoid(-x, w, b, sigmoid=sig)
                got = ops.rowdot_sigmoid(x, w, b, sigmoid=sig)
                gate = lin_gate / 4 + 2e-7 if sig else lin_gate
                err = _report(f"rowdot k={k} rows={rows} bias={b is not None} sigmoid={sig}",
                              (got.double() - (torch.sigmoid(v) if sig else v)).abs().max().item(), gate)
                assert got.shape == (rows,) and err <= gate
                del keep


# ------------------------------------------------------------------ 7. the capped 1-D launchers past 2048 blocks (see the audit above)
AUDIT_BIAS_ACT = (1, 363, 365, 16)                                   # [B, H, W, C]: 529980 items
AUDIT_IM2COL = (2, 69, 69, 96, 3, 3, 2, 1)                           # (b, h, w, c, kh, kw, stride, pad): 529200 items
AUDIT_MAXPOOL = (3, 257, 341, 64)                                    # 532512 items
AUDIT_DWCONV = {"strip2": (7362, 5, 17, 32, 1), "strip": (11043, 1, 17, 64, 1), "plain": (2, 131, 253, 32, 2)}   # (B, H, W, C, dilation)
AUDIT_UPCAT = (3, 81, 37, 96, 20)                                    # (B, h, w, Ca, Ch): 535572 items
AUDIT_UPSAMPLE_ROWS = (2, 3, 150, 170, 301, 1174)                    # (B, C, h, w, H, W): 530964 items
AUDIT_ASPP = (1, 363, 365, 16)                                       # 529980 items, the flat kernel
AUDIT_STEM = (2, 3, 1401, 515)                                       # 8406 spans for 8192 waves


def _dw3x3_ref(x_nhwc, w9, bias, dilation):
    """float64 depthwise 3x3 (zero pad = dilation) on an NHWC tensor as nine shifted products; w9 [9, C] tap-major."""
    x, w = x_nhwc.double(), w9.double()
    d = dilation
    H, W = x.shape[1], x.shape[2]
    xp = torch.nn.functional.pad(x, (0, 0, d, d, d, d))
    out = torch.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky * d:ky * d + H, kx * d:kx * d + W, :] * w[ky * 3 + kx]
    return out if bias is None else out + bias.double()


def test_bias_act_nhwc_past_the_grid_cap(ops):
    B, H, W, C = AUDIT_BIAS_ACT
    g = _gen(1)
    y = torch.randn(B, H, W, C, device="cuda", generator=g); r = torch.randn(B, H, W, C, device="cuda", generator=g)
    b = torch.randn(C, device="cuda", generator=g)
    assert torch.equal(ops.bias_act_nhwc_(y.clone(), b, r, 1), torch.relu(y + b + r))
    assert torch.equal(ops.bias_act_nhwc_(y.clone(), b, None, 0), y + b)


def test_im2col_nhwc_past_the_grid_cap(ops):
    b, h, w, c, kh, kw, s, p = AUDIT_IM2COL
    x = torch.randn(b, h, w, c, device="cuda", generator=_gen(2))
    keep = ops.im2col_nhwc(-x, kh, kw, s, p, 1, kh * kw * c)
    cols, ho, wo = ops.im2col_nhwc(x, kh, kw, s, p, 1, kh * kw * c)
    un = torch.nn.functional.unfold(x.permute(0, 3, 1, 2), (kh, kw), dilation=1, padding=p, stride=s)
    un = un.view(b, c, kh * kw, ho * wo).permute(0, 3, 2, 1).reshape(b * ho * wo, kh * kw * c)
    assert torch.equal(cols, un)
    del keep


def test_maxpool3x3s2_nhwc_past_the_grid_cap(ops):
    g = _gen(3)
    x = torch.randn(*AUDIT_MAXPOOL, device="cuda", generator=g)
    shift = torch.randn(AUDIT_MAXPOOL[3], device="cuda", generator=g)
    keep = [ops.maxpool3x3s2_nhwc(-x), ops.maxpool3x3s2_nhwc(-x, shift=shift)]
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(ops.maxpool3x3s2_nhwc(x), ref)
    assert torch.equal(ops.maxpool3x3s2_nhwc(x, shift=shift), torch.relu(ref + shift))
    del keep


@pytest.mark.parametrize("kernel", sorted(AUDIT_DWCONV))
def test_dwconv3x3_nhwc_past_the_grid_cap(ops, kernel):
    """Gate 1e-5 as in test_dwconv3x3_nhwc_and_bias_act.  Measured worst: 8.7e-7 (strip2), 1.5e-7 (strip), 4.3e-7 (plain)."""
    B, H, W, C, dil = AUDIT_DWCONV[kernel]
    g = _gen(4 + H)
    x = torch.randn(B, H, W, C, device="cuda", generator=g)
    w9 = (torch.rand(9, C, device="cuda", generator=g) - 0.5) * (2.0 / 3.0)
    bias = torch.randn(C, device="cuda", generator=g) if kernel == "strip2" else None
    act = 0 if kernel == "strip2" else 1
    keep = ops.dwconv3x3_nhwc(-x, w9, bias, act, dilation=dil)
    got = ops.dwconv3x3_nhwc(x, w9, bias, act, dilation=dil)
    ref = _dw3x3_ref(x, w9, bias, dil)
    err = _report(f"dwconv3x3 {kernel}", (got.double() - (torch.relu(ref) if act else ref)).abs().max().item(), 1e-5)
    assert err < 1e-5
    del keep


def test_dwconv3x3_upcat_past_the_grid_cap(ops):
    """Gate 1e-5 as in test_dwconv3x3_upcat_matches_torch.  Measured worst: 4.7e-6."""
    B, h, w, Ca, Ch = AUDIT_UPCAT
    g = _gen(5)
    a = torch.randn(B, Ca, h, w, device="cuda", generator=g)
    hi = torch.randn(B, Ch, 4 * h, 4 * w, device="cuda", generator=g)
    w9 = torch.randn(9, Ca + Ch, device="cuda", generator=g)
    cat = torch.cat([torch.nn.UpsamplingBilinear2d(scale_factor=4)(a), hi], dim=1).permute(0, 2, 3, 1)
    ref = _dw3x3_ref(cat, w9, None, 1)
    al, hl = a.permute(0, 2, 3, 1).contiguous(), hi.permute(0, 2, 3, 1).contiguous()
    keep = ops.dwconv3x3_upcat(-al, hl, w9)
    got = ops.dwconv3x3_upcat(al, hl, w9)
    err = _report("dwconv3x3_upcat", (got.double() - ref).abs().max().item(), 1e-5)
    assert err < 1e-5
    del keep


@pytest.mark.parametrize("align", [False, True])
def test_upsample_bilinear_row_kernel_past_the_grid_cap(ops, align):
    """Gate 1e-6 * max(1, |ref|) as in test_upsample_bilinear_matches_torch.  Measured worst: 0 (bit-identical)."""
    B, C, h, w, H, W = AUDIT_UPSAMPLE_ROWS
    x = torch.randn(B, C, h, w, device="cuda", generator=_gen(6))
    keep = ops.upsample_bilinear(-x, (H, W), align)
    got = ops.upsample_bilinear(x, (H, W), align)
    ref = torch.nn.functional.interpolate(x, size=(H, W), mode="bilinear", align_corners=align)
    gate = 1e-6 * max(1.0, ref.abs().max().item())
    err = _report(f"upsample_bilinear rows align={align}", (got - ref).abs().max().item(), gate)
    assert err < gate
    del keep


def test_aspp_depthwise3_flat_kernel_past_the_grid_cap(ops):
    """Gate 1e-4 as in test_aspp_depthwise3.  Measured worst: 2.7e-6."""
    B, h, w, C = AUDIT_ASPP
    g = _gen(7)
    x = torch.randn(B, h, w, C, device="cuda", generator=g)
    wdw = torch.randn(3, 9, C, device="cuda", generator=g)
    rates = (3, 6, 9)
    keep = ops.aspp_depthwise3(-x, wdw, rates)
    out = ops.aspp_depthwise3(x, wdw, rates)
    for r in range(3):
        err = _report(f"aspp_depthwise3 rate {rates[r]}", (out[r].double() - _dw3x3_ref(x, wdw[r], None, rates[r])).abs().max().item(), 1e-4)
        assert err < 1e-4
    del keep


def test_stem_image_fill_past_the_grid_cap(ops):
    B, C, H, W = AUDIT_STEM
    x = torch.randn(B, C, H, W, device="cuda", generator=_gen(8))
    ref = torch.full((B, H, W + 11, 4), 7.0, device="cuda")
    got = ref.clone()
    ref[:, :, 3:3 + W, :C] = x.permute(0, 2, 3, 1)
    ref[:, :, 3:3 + W, C:] = 0.0
    ops.stem_image_fill(x, got)
    assert torch.equal(got, ref)
