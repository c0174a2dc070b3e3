"""-m gpu: every split-operand entry point against float64 across operand MAGNITUDES, under the floor-free componentwise gate of
tests/split_ref.py: e = |got - ref64| / D with D = sum |x||w| + |bias| + |residual| (no absolute floor), and
max e_split <= max(4 max e_f32, 2^-20), e_f32 being the same metric for the kernel's float32 twin on the same inputs.

Activations are scaled by 2^s, s in {0, -4, -8, -12, -16, -20} (whole tensors: the last two make the f16 high parts subnormal);
weights take std 1/sqrt(K), 0.02 and 2^-10, and 0.02 with per-output-channel scales log-uniform in [2^-8, 1] (BatchNorm folding).
The kernels keep 22-bit operands at small magnitudes through the same two devices at every entry point: weights normalised by a
power of two when they are split, and a small-side range guard that redoes an operand block whose maximum is small with
power-of-two scaled activations.  The guard is per TILE (per block of rows), not per row: the mixed-magnitude cases put half the
rows of every tile at 2^-12 next to O(1) rows and hold the kernel to the documented per-tile contract, a per-column normaliser
max_m D(m, n)."""
import math
import pytest
import torch
import torch.nn.functional as F

from tests.split_ref import gate_bound

pytestmark = pytest.mark.gpu

SCALES = (0, -4, -8, -12, -16, -20)
WEIGHTS = ("inv_sqrt_k", "0.02", "2^-10", "0.02_per_channel")


@pytest.fixture(scope="module")
def ops(native):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    return ops


def err(got, ref, den) -> float:
    """max |got - ref| / D on the device (float64); D == 0 demands an exact result."""
    got = got.double()
    if not torch.isfinite(got).all():
        return math.inf
    e = (got - ref).abs()
    zero = den == 0
    if (e[zero] != 0).any():
        return math.inf
    return (e[~zero] / den[~zero]).max().item()


def col_err(got, ref, den) -> float:
    """per-tile contract: |got - ref| / max_m D(m, n), columns of a [..., N] result"""
    d = den.reshape(-1, den.shape[-1]).amax(dim=0)
    e = (got.double() - ref).abs().reshape(-1, den.shape[-1])
    return (e / d).max().item()


def check(failures, what, e_s, e_f):
    bound = gate_bound(e_f)
    ok = e_s <= bound
    print(f"{'ok  ' if ok else 'FAIL'} {what}: e_split {e_s / 2 ** -22:8.2f}  e_f32 {e_f / 2 ** -22:6.2f}  (units of 2^-22; gate {bound / 2 ** -22:.2f})")
    if not ok:
        failures.append(f"{what}: e_split {e_s:.3e} > {bound:.3e}")


def weights(kind, n, k, g):
    w = torch.randn(n, k, device="cuda", generator=g)
    if kind == "inv_sqrt_k":
        return w / k ** 0.5
    if kind == "2^-10":
        return w * 2.0 ** -10
    w = w * 0.02
    if kind == "0.02_per_channel":
        w = w * torch.exp2(-8 * torch.rand(n, 1, device="cuda", generator=g))
    return w


def gemm_ref(x, w, b, r, act):
    ref = x.double() @ w.double().t()
    den = x.double().abs() @ w.double().abs().t()
    if b is not None:
        ref, den = ref + b.double(), den + b.double().abs()
    if r is not None:
        ref, den = ref + r.double(), den + r.double().abs()
    return (ref.clamp_min(0) if act else ref), den


# ------------------------------------------------------------------ awseg_gemm_split_bias_act, one shape per kernel configuration
# The dispatcher (gemm_launch, gemm_split.hip) sends a shape to the LDS-DMA kernel of gemm_split3.hip whenever it is eligible
# (K >= 32 among other things) and has at least CUs / 2 tiles (256 CUs: 128); the rest reach the register-staged two-accumulator
# kernels of gemm_split.hip: 128 x 256 when N % 256 == 0 and ceil(M/128) N/256 >= 256, else 128 x 128.
GEMM_CONFIGS = [
    ((300, 256, 128), "128x128 two-accumulator kernel (gemm_split.hip): 6 tiles, too few for gemm_split3"),
    ((300, 256, 136), "128x128 two-accumulator kernel, K tail (gemm_split.hip)"),
    ((32768, 256, 16), "128x256 two-accumulator kernel, K tail (gemm_split.hip): K < 32, 256 tiles"),
    ((32768, 256, 24), "128x256 two-accumulator kernel, K tail (gemm_split.hip): K < 32, 256 tiles"),
    ((38400, 256, 128), "gemm_split3.hip, 256-row tiles (150 tiles)"),
    ((70000, 384, 136), "gemm_split3.hip, K tail (K % 32 = 8)"),
    ((262300, 32, 32), "gemm_split3.hip, masked 64-column tile"),
    ((65536, 256, 256), "gemm_split3.hip, 256x256 tiles"),
]


@pytest.mark.parametrize("shape,kernel", GEMM_CONFIGS, ids=[f"{m}x{n}x{k}" for (m, n, k), _ in GEMM_CONFIGS])
def test_gemm_split_magnitude_sweep(ops, shape, kernel):
    failures = _gemm_sweep(ops, shape, kernel)
    assert not failures, "\n".join(failures)


def _gemm_sweep(ops, shape, kernel):
    M, Nn, K = shape
    g = torch.Generator(device="cuda").manual_seed(M + Nn + K + 1)
    x0 = torch.randn(M, K, device="cuda", generator=g)
    bias = torch.randn(Nn, device="cuda", generator=g)
    failures = []
    for wk in WEIGHTS:
        w = weights(wk, Nn, K, g)
        ws = ops.gemm_split_weights(w)
        for s in SCALES:
            x = x0 * 2.0 ** s
            # epilogue-free product; at s = -8 also bias + residual + ReLU at the product's own scale (they must not dominate D)
            epi = s == -8
            b = bias * 2.0 ** s * 0.1 if epi else None
            r = torch.randn(M, Nn, device="cuda", generator=g) * 2.0 ** s * 0.1 if epi else None
            act = 1 if epi else 0
            ref, den = gemm_ref(x, w, b, r, act)
            got = ops.gemm_split_bias_act(x, ws, b, act, residual=r)
            lib = ops.gemm_bias_act(x, w, b if b is not None else torch.zeros(Nn, device="cuda"), act, residual=r, split=False)
            check(failures, f"gemm {shape} [{kernel}] w {wk} x*2^{s}{' +bias+res+relu' if epi else ''}", err(got, ref, den), err(lib, ref, den))
    # mixed-magnitude tiles: half the rows at 2^-12 beside O(1) rows; per-column normaliser (per-tile contract)
    w = weights("0.02", Nn, K, g)
    x = x0.clone(); x[1::2] *= 2.0 ** -12
    ref, den = gemm_ref(x, w, None, None, 0)
    got = ops.gemm_split_bias_act(x, ops.gemm_split_weights(w), None, 0)
    lib = ops.gemm_bias_act(x, w, torch.zeros(Nn, device="cuda"), 0, split=False)
    check(failures, f"gemm {shape} [{kernel}] mixed rows 1 | 2^-12 (per-column D)", col_err(got, ref, den), col_err(lib, ref, den))
    return failures


# ------------------------------------------------------------------ gathered convolutions, two-source and piecewise A operands
def test_conv_gemm_split_dilated_magnitudes(ops):
    """awseg_conv_gemm_split_bias_act: atrous 3x3, dilation 2, the A operand gathered from the NHWC image"""
    B, H, W, C, Nn = 2, 33, 47, 64, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.randn(B, H, W, C, device="cuda", generator=g)
    failures = []
    for wk in WEIGHTS:
        wt = weights(wk, Nn, C * 9, g).view(Nn, C, 3, 3)
        w2 = wt.permute(0, 2, 3, 1).reshape(Nn, 9 * C).contiguous()
        ws = ops.gemm_split_weights(w2)
        for s in SCALES:
            x = x0 * 2.0 ** s
            got = ops.conv_gemm_split(x, ws, None, 0, 3, 3, 1, 2, 2)
            xd = x.permute(0, 3, 1, 2).double()
            ref = F.conv2d(xd, wt.double(), None, 1, 2, 2).permute(0, 2, 3, 1)
            den = F.conv2d(xd.abs(), wt.double().abs(), None, 1, 2, 2).permute(0, 2, 3, 1)
            cols, ho, wo = ops.im2col_nhwc(x, 3, 3, 1, 2, 2, 9 * C)
            lib = ops.gemm_bias_act(cols, w2, torch.zeros(Nn, device="cuda"), 0, split=False).view(B, ho, wo, Nn)
            check(failures, f"conv gather 3x3 d2 w {wk} x*2^{s}", err(got, ref, den), err(lib, ref, den))
    # mixed-magnitude tiles: every other image row at 2^-12 (per-column D: the per-tile contract)
    x = x0.clone(); x[:, 1::2] *= 2.0 ** -12
    got = ops.conv_gemm_split(x, ws, None, 0, 3, 3, 1, 2, 2)
    xd = x.permute(0, 3, 1, 2).double()
    ref = F.conv2d(xd, wt.double(), None, 1, 2, 2).permute(0, 2, 3, 1)
    den = F.conv2d(xd.abs(), wt.double().abs(), None, 1, 2, 2).permute(0, 2, 3, 1)
    cols, ho, wo = ops.im2col_nhwc(x, 3, 3, 1, 2, 2, 9 * C)
    lib = ops.gemm_bias_act(cols, w2, torch.zeros(Nn, device="cuda"), 0, split=False).view(B, ho, wo, Nn)
    check(failures, "conv gather 3x3 d2 mixed rows 1 | 2^-12 (per-column D)", col_err(got, ref, den), col_err(lib, ref, den))
    assert not failures, "\n".join(failures)


def test_conv_rows_gemm_split_stem_magnitudes(ops):
    """awseg_conv_rows_gemm_split_bias_act: the 7x7 / stride-2 stem on 3 channels"""
    B, H, W, Nn = 2, 200, 328, 64
    g = torch.Generator(device="cuda").manual_seed(6)
    x0 = torch.randn(B, 3, H, W, device="cuda", generator=g)
    wo = (W + 6 - 7) // 2 + 1
    wp = max(W + 3, (wo - 1) * 2 + 8)
    failures = []
    mixed = x0.clone(); mixed[:, :, 1::2] *= 2.0 ** -12                 # every other image row at 2^-12: the per-tile contract
    for wk in WEIGHTS + ("mixed",):
        wt = weights("0.02" if wk == "mixed" else wk, Nn, 147, g).view(Nn, 3, 7, 7)
        ws = ops.gemm_split_weights(ops.stem_rows_weights(wt))
        for s in ((0,) if wk == "mixed" else SCALES):
            x = mixed if wk == "mixed" else x0 * 2.0 ** s
            xp = torch.zeros(B, H, wp, 4, device="cuda")
            xp[:, :, 3:3 + W, :3] = x.permute(0, 2, 3, 1)
            got = ops.conv_rows_gemm_split(xp, ws, None, 0, 7, 2, 3, wo)
            assert got is not None
            ref = F.conv2d(x.double(), wt.double(), None, 2, 3).permute(0, 2, 3, 1)
            den = F.conv2d(x.double().abs(), wt.double().abs(), None, 2, 3).permute(0, 2, 3, 1)
            cols = F.unfold(x, 7, padding=3, stride=2).transpose(1, 2).reshape(-1, 147)
            lib = ops.gemm_bias_act(F.pad(cols, (0, 5)), F.pad(wt.reshape(Nn, 147), (0, 5)), torch.zeros(Nn, device="cuda"), 0,
                                    split=False).view(B, ref.shape[1], ref.shape[2], Nn)
            if wk == "mixed":
                check(failures, "stem rows 7x7 mixed rows 1 | 2^-12 (per-column D)", col_err(got, ref, den), col_err(lib, ref, den))
            else:
                check(failures, f"stem rows 7x7 w {wk} x*2^{s}", err(got, ref, den), err(lib, ref, den))
    assert not failures, "\n".join(failures)


def _pieces_case(ops, failures, what, pieces, w, run, metric=err):
    x = torch.cat(pieces, dim=1)
    ref, den = gemm_ref(x, w, None, None, 0)
    got = run()
    assert got is not None, what
    lib = ops.gemm_bias_act(x, w, torch.zeros(w.shape[0], device="cuda"), 0, split=False)
    check(failures, what, metric(got, ref, den), metric(lib, ref, den))


def _mixed_rows(t):
    t = t.clone(); t[1::2] *= 2.0 ** -12
    return t


def test_gemm_split_dual_magnitudes(ops):
    """awseg_gemm_split_dual_bias_act: [x | x2] with each source scaled on its own; only the FIRST source large (>= 2^11) and
    only one source tiny — the range guard must see every source"""
    m, k1, k2, n = 70000, 256, 256, 256
    g = torch.Generator(device="cuda").manual_seed(7)
    a0, b0 = torch.randn(m, k1, device="cuda", generator=g), torch.randn(m, k2, device="cuda", generator=g)
    failures = []
    for wk in WEIGHTS:
        w = weights(wk, n, k1 + k2, g)
        ws = ops.gemm_split_weights(w)
        for s in SCALES:
            a, b = a0 * 2.0 ** s, b0 * 2.0 ** s
            _pieces_case(ops, failures, f"dual w {wk} x*2^{s}", [a, b], w, lambda: ops.gemm_split_dual(a, b, ws, None, 0))
    w = weights("0.02", n, k1 + k2, g)
    ws = ops.gemm_split_weights(w)
    for what, a, b in (("first source x 3e4", a0 * 3e4, b0), ("first source x 2^-14", a0 * 2.0 ** -14, b0),
                       ("second source x 2^-14", a0, b0 * 2.0 ** -14)):
        _pieces_case(ops, failures, f"dual {what}", [a, b], w, lambda: ops.gemm_split_dual(a, b, ws, None, 0))
    a, b = _mixed_rows(a0), _mixed_rows(b0)
    _pieces_case(ops, failures, "dual mixed rows 1 | 2^-12 (per-column D)", [a, b], w, lambda: ops.gemm_split_dual(a, b, ws, None, 0), col_err)
    assert not failures, "\n".join(failures)


def test_gemm_split_pieces_magnitudes(ops):
    """awseg_gemm_split_pieces_bias_act: four pieces; only the first piece large, only one piece tiny"""
    m, n, kp, npc = 70000, 256, 256, 4
    g = torch.Generator(device="cuda").manual_seed(8)
    p0 = [torch.randn(m, kp, device="cuda", generator=g) for _ in range(npc)]
    failures = []
    for wk in WEIGHTS:
        w = weights(wk, n, kp * npc, g)
        ws = ops.gemm_split_weights(w)
        for s in SCALES:
            ps = [p * 2.0 ** s for p in p0]
            _pieces_case(ops, failures, f"pieces w {wk} x*2^{s}", ps, w, lambda: ops.gemm_split_pieces(ps, ws, None, 0))
    w = weights("0.02", n, kp * npc, g)
    ws = ops.gemm_split_weights(w)
    for what, mult in (("first piece x 3e4", (3e4, 1, 1, 1)), ("first piece x 2^-14", (2.0 ** -14, 1, 1, 1)),
                       ("third piece x 2^-14", (1, 1, 2.0 ** -14, 1))):
        ps = [p * f for p, f in zip(p0, mult)]
        _pieces_case(ops, failures, f"pieces {what}", ps, w, lambda: ops.gemm_split_pieces(ps, ws, None, 0))
    ps = [_mixed_rows(p) for p in p0]
    _pieces_case(ops, failures, "pieces mixed rows 1 | 2^-12 (per-column D)", ps, w, lambda: ops.gemm_split_pieces(ps, ws, None, 0), col_err)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ Winograd 3x3
def test_conv3x3_winograd_split_magnitudes(ops):
    """awseg_conv3x3_winograd_split against a float64 direct convolution; D = conv2d(|x|, |w scale|) + |shift|; scales straddling
    the kernel's 2^-4 small-side guard (2^-3.9, 2^-4.1)"""
    B, H, W, Cin, Cout = 2, 37, 29, 64, 128
    g = torch.Generator(device="cuda").manual_seed(9)
    x0 = torch.randn(B, H, W, Cin, device="cuda", generator=g)
    failures = []
    for wk in WEIGHTS:
        wt = weights(wk, Cout, Cin * 9, g).view(Cout, Cin, 3, 3)
        scale = torch.exp2(-2 * torch.rand(Cout, device="cuda", generator=g))
        for s in SCALES + (-3.9, -4.1):
            x = x0 * 2.0 ** s
            shift = torch.randn(Cout, device="cuda", generator=g) * 2.0 ** s * 0.1
            wsc = (wt * scale.view(-1, 1, 1, 1)).double()
            xd = x.permute(0, 3, 1, 2).double()
            ref = (F.conv2d(xd, wsc, None, 1, 1) + shift.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
            den = (F.conv2d(xd.abs(), wsc.abs(), None, 1, 1) + shift.double().abs().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
            got = ops.conv3x3_winograd_split(x, ops.winograd_split_weights(wt, scale), Cout, shift)
            lib = ops.conv3x3_winograd(x, ops.winograd_weights(wt, scale), shift)
            check(failures, f"winograd w {wk} x*2^{s}", err(got, ref, den), err(lib, ref, den))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ SegFormer head
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="open: heads.hip splits W2, T and the hidden activations unscaled with no small-side guard "
                   "(up to ~800 x 2^-22 at small features / weights); the fix is the normalisation + guard the GEMMs have")
@pytest.mark.parametrize("cmid", [128, 256])
def test_segformer_head_split_magnitudes(ops, cmid):
    """awseg_segformer_head_fused_split: features at {1, 2^-6, 2^-10}, conv1 / conv2 at default init, std 0.01, std 2^-10.
    Per logit D = sum_c |mid_c| |w2_oc| + |b2_o|, mid the float64 hidden map after ReLU."""
    B, h, w, H, W, cout, cin = 2, 5, 7, 160, 224, 19, 32
    torch.manual_seed(cmid + 1)
    f0 = torch.randn(B, cin, h, w, device="cuda")
    failures = []
    for wk in ("default", "0.01", "2^-10"):
        conv1 = torch.nn.Conv2d(cin, cmid, 3, padding=1).cuda()
        conv2 = torch.nn.Conv2d(cmid, cout, 1).cuda()
        with torch.no_grad():
            if wk != "default":
                sd = 0.01 if wk == "0.01" else 2.0 ** -10
                for c in (conv1, conv2):
                    c.weight.normal_(0, sd); c.bias.normal_(0, sd)
        for fs in (0, -6, -10):
            feat = f0 * 2.0 ** fs
            shift = torch.randn(cmid, device="cuda") * 0.3 * conv1.weight.abs().mean() * 2.0 ** fs
            w2 = conv2.weight.view(cout, cmid).contiguous()
            with torch.no_grad():
                g9 = torch.einsum("bchw,ockl->bhwklo", feat, conv1.weight).reshape(B, h, w, 9, cmid).contiguous()
                up = F.interpolate(feat.double(), size=(H, W), mode="bilinear", align_corners=False)
                mid = torch.relu(F.conv2d(up, conv1.weight.double(), None, padding=1) + shift.double().view(1, -1, 1, 1))
                ref = F.conv2d(mid, conv2.weight.double(), conv2.bias.double())
                den = F.conv2d(mid, conv2.weight.double().abs(), conv2.bias.double().abs())
                f32 = ops.segformer_head_fused(g9, None, shift, w2, conv2.bias, H, W, split=False)
                spl = ops.segformer_head_fused(g9, None, shift, w2, conv2.bias, H, W, split=True)
            check(failures, f"head Cmid {cmid} w {wk} features*2^{fs}", err(spl, ref, den), err(f32, ref, den))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ Mix-FFN
@pytest.mark.parametrize("C", [32, 64])
def test_mixffn_fused_magnitudes(ops, C):
    """awseg_mixffn_fused against the five torch operations in float64, next to the unfused float32 launches (LayerNorm,
    hipBLASLt fc1, depthwise 3x3, GELU, hipBLASLt fc2): w1 / w2 std in {1/sqrt(C), 0.02, 2^-9}, LayerNorm gamma ~1 and ~0.05.
    D = sum_j |gelu_j| |w2_cj| + |b2_c| + |tok|, tok at 2^-12 so the residual does not dominate D (LayerNorm makes the
    fc2 input independent of tok's scale)."""
    B, H, W = 2, 20, 70
    g = torch.Generator(device="cuda").manual_seed(C)
    tok = (torch.randn(B, H, W, C, device="cuda", generator=g) * 2.0 + 0.3) * 2.0 ** -12
    beta0 = torch.randn(C, device="cuda", generator=g)
    wd, bd = torch.randn(4 * C, 1, 3, 3, device="cuda", generator=g) * 0.3, torch.randn(4 * C, device="cuda", generator=g) * 0.1
    taps = wd.view(4 * C, 9).t().contiguous()
    td = tok.double()
    failures = []
    for wk, sd in (("1/sqrt(C)", None), ("0.02", 0.02), ("2^-9", 2.0 ** -9)):
        w1 = torch.randn(4 * C, C, device="cuda", generator=g) * (C ** -0.5 if sd is None else sd)
        w2 = torch.randn(C, 4 * C, device="cuda", generator=g) * ((4 * C) ** -0.5 if sd is None else sd)
        b1 = torch.randn(4 * C, device="cuda", generator=g) * 0.1
        b2 = torch.randn(C, device="cuda", generator=g) * w2.abs().mean()
        for gk, gs in (("~1", 1.0), ("~0.05", 0.05)):
            gamma = (torch.rand(C, device="cuda", generator=g) * 0.5 + 0.75) * gs
            beta = beta0 * 0.2 * gs
            got = ops.mixffn_fused(tok, gamma, beta, 1e-6, w1, b1, taps, bd, w2, b2)
            assert got is not None
            h1 = F.linear(F.layer_norm(td, (C,), gamma.double(), beta.double(), 1e-6), w1.double(), b1.double())
            h1 = F.conv2d(h1.permute(0, 3, 1, 2), wd.double(), bd.double(), 1, 1, 1, 4 * C).permute(0, 2, 3, 1)
            ge = F.gelu(h1)
            ref = td + F.linear(ge, w2.double(), b2.double())
            den = td.abs() + F.linear(ge.abs(), w2.double().abs(), b2.double().abs())
            # the unfused float32 launches
            ln = F.layer_norm(tok, (C,), gamma, beta, 1e-6).reshape(-1, C)
            f1 = ops.gemm_bias_act(ln, w1, b1, 0, split=False).view(B, H, W, 4 * C)
            f1 = F.conv2d(f1.permute(0, 3, 1, 2), wd, bd, 1, 1, 1, 4 * C).permute(0, 2, 3, 1)
            f32 = ops.gemm_bias_act(F.gelu(f1).reshape(-1, 4 * C), w2, b2, 0, residual=tok.reshape(-1, C), split=False).view(B, H, W, C)
            check(failures, f"mixffn C {C} w {wk} gamma {gk}", err(got, ref, den), err(f32, ref, den))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ attention
def _attn_ref(q, k, v, nh, scale):
    B, nq, C = q.shape
    qh, kh, vh = (t.double().view(B, -1, nh, 32).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    ref = (p @ vh).transpose(1, 2).reshape(B, nq, C)
    # D = sum_k P_k |v_k| + 2 max_k |v_k| scale max_k sum_d |q_d| |k_kd|
    pv = (p @ vh.abs()).transpose(1, 2).reshape(B, nq, C)
    sm = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(dim=-1, keepdim=True) * scale             # [B, nh, nq, 1]
    vm = vh.abs().amax(dim=2, keepdim=True)                                                      # [B, nh, 1, 32]
    den = pv + (2 * sm * vm).transpose(1, 2).reshape(B, nq, C)
    return ref, den


@pytest.mark.parametrize("form", ["in_block", "prepared_image", "packed_kv"])
def test_attention_d32_split_magnitudes(ops, form):
    """awseg_attention_d32_split (keys staged in the query blocks), the prepared key / value image (_ws) and packed key | value
    rows: q, k, v each at whole-tensor scales {2^-4, 2^-8, 2^-12}, and a dominant key with the others e^-2 .. e^-8 below it
    (P.V low parts of probabilities below 2^-3)"""
    B, nh = 2, 2
    nq, nkv = (2100, 256) if form == "prepared_image" else (300, 256)
    C = nh * 32
    g = torch.Generator(device="cuda").manual_seed(nq + len(form))
    q0, k0, v0 = (torch.randn(B, n, C, device="cuda", generator=g) for n in (nq, nkv, nkv))
    scale = 32 ** -0.5

    def run(q, k, v, split):
        if form == "packed_kv":
            return ops.attention_d32_packed_kv(q, torch.cat([k, v], dim=-1), nh, scale, split=split)
        prev = ops.ATTN_KV_IMAGE
        try:
            ops.ATTN_KV_IMAGE = form == "prepared_image"
            return ops.attention_d32(q, k, v, nh, scale, split=split)
        finally:
            ops.ATTN_KV_IMAGE = prev

    cases = []
    for which in ("q", "k", "v"):
        for s in (-4, -8, -12):
            f = {"q": 1.0, "k": 1.0, "v": 1.0}; f[which] = 2.0 ** s
            cases.append((f"{which}*2^{s}", q0 * f["q"], k0 * f["k"], v0 * f["v"]))
    # dominant key: one key per head far ahead, the others' scores spread over e^-2 .. e^-8 below it
    qd = torch.zeros_like(q0); qd[..., 0::32] = 1.0
    kd = torch.zeros_like(k0)
    kd[..., 0::32] = (-(2.0 + 6.0 * torch.rand(B, nkv, nh, device="cuda", generator=g)) / scale)
    kd[:, 0, 0::32] = 0.0
    cases.append(("dominant key", qd, kd, v0))
    failures = []
    for what, q, k, v in cases:
        ref, den = _attn_ref(q, k, v, nh, scale)
        check(failures, f"attention {form} {what}", err(run(q, k, v, True), ref, den), err(run(q, k, v, False), ref, den))
    assert not failures, "\n".join(failures)
