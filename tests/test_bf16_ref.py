"""CPU checks of tests/bf16_ref.py: the rounding, the Winograd image decoder, the models against exact float64, and that the
arithmetic gate accepts the models recomputed in float32 (another summation order, the kernels' own precision) and rejects
the degraded forms a subtly wrong bf16 kernel would compute.  e_twin is stood in for by torch's float32 result of the
unrounded operands against float64 (the float32-grade twin's role)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bf16_ref as R
from tests.split_ref import gate_bound


def bits(x):
    return torch.tensor([x], dtype=torch.float32)


# ------------------------------------------------------------------ rounding
@pytest.mark.parametrize("x,want", [
    (1.0 + 2.0 ** -8, 1.0),                           # tie, even neighbour below
    (1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -6),           # tie, even neighbour above
    (1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -7),  # just past the tie
    (-(1.0 + 2.0 ** -8), -1.0),
    (2.0 - 2.0 ** -9, 2.0),                           # next to a power of two: rounds up into the next binade
    (2.0 - 2.0 ** -8, 2.0),                           # tie between 2 - 2^-7 (odd) and 2 (even)
    (2.0 - 2.0 ** -7, 2.0 - 2.0 ** -7),               # representable
    (2.0 + 2.0 ** -7, 2.0),                           # tie above a power of two, even = 2
    (2.0 ** -126 * (1 + 2.0 ** -8), 2.0 ** -126),
])
def test_bf16_rne_ties_and_binades(x, want):
    assert R.bf16_rne(bits(x)).item() == want
    assert R.bf16_rne(bits(x)).item() == bits(x).to(torch.bfloat16).float().item()


def test_bf16_rne_specials_and_rtz():
    t = torch.tensor([0.0, -0.0, math.inf, -math.inf, math.nan], dtype=torch.float32)
    r = R.bf16_rne(t)
    assert r[0].item() == 0 and math.copysign(1, r[1].item()) == -1 and r[2].item() == math.inf and r[3].item() == -math.inf
    assert math.isnan(r[4].item())
    assert R.bf16_rtz(bits(1.0 + 2.0 ** -7 - 2.0 ** -20)).item() == 1.0
    assert R.bf16_rtz(bits(-(2.0 - 2.0 ** -20))).item() == -(2.0 - 2.0 ** -7)


def test_tie_delta():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 2.0 + 2.0 ** -30, 0.0], dtype=torch.float64)
    d = R.tie_delta(x, torch.full_like(x, 2.0 ** -20))
    assert d[0] > 0 and d[1] == 0 and d[3] > 0
    assert d[2] == 0                                       # 2 + 2^-30: 2^-9 from the boundary below 2, 2^-7 from the one above
    assert R.tie_delta(x[2:3], torch.tensor([2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)).item() > 0


# ------------------------------------------------------------------ the Winograd image
@pytest.mark.parametrize("cin,cout", [(16, 64), (32, 128), (256, 256)])
def test_winograd_image_decoder_round_trip(cin, cout):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    scale = torch.exp2(-8 * torch.rand(cout, generator=g))
    u = R.winograd_u_exact(wt, scale)
    eu = math.floor(math.log2(u.abs().max().item())) - 13
    U, us = R.decode_winograd_image(ops.winograd_bf16_weights(wt, scale), cin, cout)
    assert us == 2.0 ** eu
    assert torch.equal(U, (u * 2.0 ** -eu).to(torch.bfloat16).double())
    # the split image decodes to the same U within the f16 pair's precision
    Us, us2 = R.decode_winograd_image(ops.winograd_split_weights(wt, scale), cin, cout, bf16=False)
    assert us2 == us and ((Us - u * 2.0 ** -eu).abs() <= 2.0 ** -20 * u.abs() * 2.0 ** -eu + 2.0 ** -24).all()


# ------------------------------------------------------------------ cases
def gemm_case(m=300, n=128, k=136, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g) * 2.0
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g)
    r = torch.randn(m, n, generator=g)
    return x, w, b, r


def gemm_twin(x, w, b, r):
    y, D = R.gemm_exact(x, w, b, r, 1)
    f = torch.relu(x @ w.t() + b + r)
    return R.arith_error(f, y, 0, D)


WINO = [((1, 19, 23, 32, 64, 2), False), ((2, 10, 14, 48, 64, 1), True)]


def wino_case(shape, mode1, seed=1):
    B, H, W, cin, cout, d = shape
    g = torch.Generator().manual_seed(seed + H)
    x = torch.randn(B, H, W, cin, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.3
    res = None if mode1 else torch.randn(B, H, W, cout, generator=g)
    w2 = torch.randn(cout, generator=g) * 0.2 if mode1 else None
    b2 = torch.randn(1, generator=g) if mode1 else None
    return x, wt, scale, shift, d, res, w2, b2


def wino_twin(x, wt, scale, shift, d, res, w2, b2):
    ref, D = R.winograd_exact(x, wt, scale, shift, d, res, 1, w2, b2)
    y = F.conv2d(x.permute(0, 3, 1, 2), wt * scale.view(-1, 1, 1, 1), None, 1, d, d).permute(0, 2, 3, 1) + shift
    if res is not None:
        y = y + res
    y = torch.relu(y)
    if w2 is not None:
        y = torch.sigmoid(y @ w2 + b2)
    return R.arith_error(y, ref, 0, D)


def attn_case(B=1, nh=2, nq=100, nkv=256, logit=1.0, offset=0.0, seed=2):
    """logits with spread ~logit around a common offset (a shared component of every query and key)"""
    g = torch.Generator().manual_seed(seed + nkv)
    q, k, v = (torch.randn(B, n, nh * 32, generator=g) for n in (nq, nkv, nkv))
    f = (logit / 32 ** -0.5 / 32 ** 0.5) ** 0.5
    q, k = q * f, k * f
    a = (offset / 32 ** -0.5) ** 0.5
    q[..., 0::32] += a
    k[..., 0::32] = a
    return q, k, v


def attn_twin(q, k, v, nh):
    ref, D = R.attention_exact(q, k, v, nh, 32 ** -0.5)
    B, nq, C = q.shape
    qh, kh, vh = (t.view(B, -1, nh, 32).transpose(1, 2) for t in (q, k, v))
    f = (torch.softmax(qh @ kh.transpose(-1, -2) * 32 ** -0.5, -1) @ vh).transpose(1, 2).reshape(B, nq, C)
    return R.arith_error(f, ref, 0, D)


# ------------------------------------------------------------------ models against exact float64 (precision bound)
def test_models_within_precision_bound():
    x, w, b, r = gemm_case()
    y, _, _ = R.gemm_model(x, w, b, r, 1)
    ref, D = R.gemm_exact(x, w, b, r, 1)
    e = R.arith_error(y, ref, 0, D)
    assert 2.0 ** -12 < e <= R.PREC_BOUND, e
    for shape, mode1 in WINO:
        from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
        x, wt, sc, sh, d, res, w2, b2 = wino_case(shape, mode1)
        y, _, _ = R.winograd_model(x, ops.winograd_bf16_weights(wt, sc), wt.shape[0], sh, d, res, 1, w2, b2)
        ref, D = R.winograd_exact(x, wt, sc, sh, d, res, 1, w2, b2)
        e = R.arith_error(y, ref, 0, D)
        assert 2.0 ** -18 < e <= R.PREC_BOUND, (shape, e)


# ------------------------------------------------------------------ the gate: healthy forms pass, degraded forms fail
def test_gemm_gate():
    x, w, b, r = gemm_case()
    et = gemm_twin(x, w, b, r)
    y, T, D = R.gemm_model(x, w, b, r, 1)
    f32 = torch.relu(R.bf16_rne(x).flip(1) @ R.bf16_rne(w).flip(1).t() + b + r)      # float32 accumulation, reversed K order
    assert R.arith_ok(R.arith_error(f32, y, T, D), et)
    for name, bad in (("rtz", R.gemm_model(x, w, b, r, 1, rnd=R.bf16_rtz)[0]),
                      ("residual twice", R.gemm_model(x, w, b, r, 1, twice="residual")[0]),
                      ("bias twice", R.gemm_model(x, w, b, r, 1, twice="bias")[0])):
        assert not R.arith_ok(R.arith_error(bad, y, T, D), et), name


@pytest.mark.parametrize("shape,mode1", WINO)
def test_winograd_gate(shape, mode1):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    x, wt, sc, sh, d, res, w2, b2 = wino_case(shape, mode1)
    ub = ops.winograd_bf16_weights(wt, sc)
    cout = wt.shape[0]
    et = wino_twin(x, wt, sc, sh, d, res, w2, b2)
    y, T, D = R.winograd_model(x, ub, cout, sh, d, res, 1, w2, b2)
    assert T.abs().max() == 0
    ok = R.winograd_model(x, ub, cout, sh, d, res, 1, w2, b2, f32_sum=True)[0]
    e = R.arith_error(ok, y, T, D)
    assert R.arith_ok(e, et), (e, et)
    bad = {"V rounded toward zero": dict(v_round="rtz"), "V rounded between the transforms": dict(v_round="mid"),
           "one Cin chunk dropped": dict(drop_chunk=1), "shift twice": dict(twice="shift")}
    if res is not None:
        bad["residual twice"] = dict(twice="residual")
    for name, kw in bad.items():
        e = R.arith_error(R.winograd_model(x, ub, cout, sh, d, res, 1, w2, b2, **kw)[0], y, T, D)
        assert not R.arith_ok(e, et), (name, e, gate_bound(et))


# the last case: logits near 10^3, where float32 logits carry ~2^-13 of error and the tie window covers most probabilities —
# the gate must accept the kernel's own arithmetic there, and cannot be asked to see 2^-9 rounding differences
ATTN = [(1, 2, 100, 256, 1.0, 0.0), (1, 1, 64, 2048, 4.0, 0.0), (1, 1, 70, 64, 2.0, 1000.0)]


@pytest.mark.parametrize("B,nh,nq,nkv,logit,offset", ATTN)
def test_attention_gate(B, nh, nq, nkv, logit, offset):
    q, k, v = attn_case(B, nh, nq, nkv, logit, offset)
    et = attn_twin(q, k, v, nh)
    y, T, D = R.attention_model(q, k, v, nh, 32 ** -0.5)
    for name, kw in (("float32 steps", dict(f32_steps=True)), ("jitter +w_p", dict(jitter=0.99)), ("jitter -w_p", dict(jitter=-0.99))):
        e = R.arith_error(R.attention_model(q, k, v, nh, 32 ** -0.5, gen=torch.Generator().manual_seed(3), **kw)[0], y, T, D)
        assert R.arith_ok(e, et), (name, e, gate_bound(et))
    if offset:
        return
    bad = {"p rounded toward zero": dict(p_round="rtz"), "one key tile dropped": dict(drop_tile=1), "alpha rescale missing": dict(no_alpha=True),
           "q rounded before the scale product": dict(q_round_first=True)}
    for name, kw in bad.items():
        e = R.arith_error(R.attention_model(q, k, v, nh, 32 ** -0.5, **kw)[0], y, T, D)
        assert not R.arith_ok(e, et), (name, e, gate_bound(et))


def test_attention_l_from_rounded_probabilities():
    """l summed from bf16(p) (with O using bf16(p) too) is a normalisation by a slightly different sum: out scales by
    l / l_rounded, a relative error of about 2^-9 / sqrt(32 nkv) — the gate sees it."""
    q, k, v = attn_case(1, 2, 100, 256, 1.0)
    et = attn_twin(q, k, v, 2)
    y, T, D = R.attention_model(q, k, v, 2, 32 ** -0.5)
    e = R.arith_error(R.attention_model(q, k, v, 2, 32 ** -0.5, l_rounded=True)[0], y, T, D)
    assert not R.arith_ok(e, et), (e, gate_bound(et))


def _depth_head(hidden=128, seed=4):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.models.model import DepthEstimationHead
    torch.manual_seed(seed)
    head = DepthEstimationHead(in_channels=256, hidden_channels=hidden).eval()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.normal_(0, 0.3)
            if isinstance(m, torch.nn.Conv2d) and m.bias is not None:
                m.bias.normal_(0, 0.2)
        head.depth_head[7].weight.mul_(0.02)          # O(1) depth logits: the sigmoid is not saturated
    return head


def test_depth_model_gate():
    """The depth model on the image and shift the module itself builds (_fold_conv_bn in float32), with the float64 hidden map
    rounded to float32 standing in for the upconv kernel's.  Two launches (fetched map, T = 0): the listed faults are rejected.
    Fused (MODE 2, tie window on V): a hidden map moved by the window's full width passes, gross faults are rejected."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.models.model import _fold_conv_bn
    head = _depth_head()
    feats = torch.randn(1, 1, 2, 256)
    h = head.depth_head
    sc2, sh2 = _fold_conv_bn(h[4], h[5])
    ub = ops.winograd_bf16_weights(h[4].weight, sc2)
    hid, den = R.depth_hidden(head, feats)
    ref, Dx = R.depth_exact(head, feats)
    with torch.no_grad():
        up = F.interpolate(feats.permute(0, 3, 1, 2), size=(32, 64), mode="bilinear", align_corners=False)
        et = R.arith_error(head(up)[:, 0], ref, 0, Dx)
    w2, b2 = h[7].weight.double().view(-1), h[7].bias.double()
    run = lambda x, **kw: R.winograd_model(x, ub, 64, sh2, w2=w2, b2=b2, **kw)[0]       # noqa: E731
    y, T, D = R.depth_model(head, feats, hid.float(), ub, sh2, fused=False)
    assert T.abs().max() == 0 and R.precision_ok(R.arith_error(y, ref, 0, Dx), et)
    assert R.arith_ok(R.arith_error(run(hid.float(), f32_sum=True), y, T, D), et)
    for name, kw in (("V rounded toward zero", dict(v_round="rtz")), ("V rounded between the transforms", dict(v_round="mid")),
                     ("one Cmid chunk dropped", dict(drop_chunk=3)), ("shift twice", dict(twice="shift"))):
        assert not R.arith_ok(R.arith_error(run(hid.float(), **kw), y, T, D), et), name
    y, T, D = R.depth_model(head, feats, hid.float(), ub, sh2, fused=True)
    g = torch.Generator().manual_seed(0)
    for j in (0.99, -0.99):                                  # each pixel moved by j w D_h moves V by at most j w |B^T| D_h |B|
        sign = torch.randint(0, 2, hid.shape, generator=g) * 2.0 - 1.0
        assert R.arith_ok(R.arith_error(run((hid.float().double() + j * R.DEPTH_V_WINDOW * den * sign).float()), y, T, D), et)
    for name, kw in (("one Cmid chunk dropped", dict(drop_chunk=3)), ("shift twice", dict(twice="shift"))):
        assert not R.arith_ok(R.arith_error(run(hid.float(), **kw), y, T, D), et), name
