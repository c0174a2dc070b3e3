"""-m gpu: the bf16 MFMA kernels (BASELINE config 5) against the float64 models of tests/bf16_ref.py, instance by instance.

Two gates per case (tests/bf16_ref.py): ARITHMETIC, max(|got - model| - T)_+ / D <= gate_bound(e_twin), the model rounding
exactly where the kernel rounds; and PRECISION (GEMM, Winograd, depth head), |got - exact64| / D_unrounded <= 2^-7 + 2^-16 +
gate_bound(e_twin).  e_twin is the float32-grade twin kernel's error on the same inputs against exact float64.  Every shape
is labelled with the kernel instance the dispatcher really picks (a restatement of the launchers' rules, below); the
AWSEG_WINO8_TPB variants, which the launcher reads once per process, run in child processes.  Errors print in units of 2^-22."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import bf16_ref as R
from tests.split_ref import gate_bound

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CUS = 256
SCALES = (-40, -20, 0, 20, 40)
WEIGHTS = ("inv_sqrt_k", "0.02", "0.02_per_channel")


@pytest.fixture(scope="module")
def ops(native):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    return ops


# ------------------------------------------------------------------ which instance the dispatcher picks
def _env(name, default):
    v = os.environ.get(name)
    return int(v) if v else default


def wino_instance(B, H, W, cin, cout, d, mode):
    """launch_ws / launch_gen of csrc/wino_split.hip: 8x8-tile blocks, nblocks = ceil(tiles / 8) (Cout / 64) 8; the persistent
    kernel when tpb = AWSEG_WINO8_TPB or ceil(nblocks / 512), clamped to [1, 64], exceeds 1, else wino8s_kernel"""
    tpb_env = _env("AWSEG_WINO8_TPB", 0)
    hs, ws = -(-H // d), -(-W // d)
    tiles = -(-ws // 16) * d * -(-hs // 16) * d * B
    nblocks = -(-tiles // 8) * (cout // 64) * 8
    tpb = min(64, max(1, tpb_env if tpb_env > 0 else -(-nblocks // 512)))
    if mode == 2:
        return f"wino8p_kernel<2, bf16> tpb {tpb}"
    if tpb > 1:
        return f"wino8p_kernel<{mode}, bf16> tpb {tpb}"
    return f"wino8s_kernel<{mode}, bf16>"


def gemm_instance(m, n, k):
    """gemm_launch of csrc/gemm_split.hip (bf16, 256 CUs): gemm_split3 when K >= 32, N % 256 == 0 and ceil(M / 256) N / 256 >=
    CUs / 2; else 128x256 when N % 256 == 0 and ceil(M / 128) N / 256 >= CUs; else 128x128.  K % 32 != 0: the K-tail instance."""
    tail = " K tail" if k % 32 else ""
    if k >= 32 and n % 256 == 0 and -(-m // 256) * (n // 256) >= CUS // 2:
        return "gemm_split3 bf16" + tail
    if n % 256 == 0 and -(-m // 128) * (n // 256) >= CUS:
        return "gemm_split 128x256 bf16" + tail
    return "gemm_split 128x128 bf16" + tail + (" N<64" if n < 64 else "")


def check(failures, what, inst, e_a, e_p, e_t, same):
    bound = gate_bound(e_t)
    ok = e_a <= bound and (e_p is None or e_p <= R.PREC_BOUND + bound) and not same
    u = 2.0 ** -22
    prec = f"  prec {e_p / 2.0 ** -8:6.3f} x 2^-8" if e_p is not None else ""
    print(f"{'ok  ' if ok else 'FAIL'} [{inst}] {what}: e_arith {e_a / u:8.2f}  e_twin {e_t / u:6.2f}  (gate {bound / u:.2f}){prec}"
          f"{'  SAME AS TWIN' if same else ''}")
    if not ok:
        failures.append(f"[{inst}] {what}: e_arith {e_a:.3e} (gate {bound:.3e}), e_prec {e_p}, same as twin {same}")


def weights(kind, n, k, g):
    w = torch.randn(n, k, device="cuda", generator=g)
    if kind == "inv_sqrt_k":
        return w / k ** 0.5
    w = w * 0.02
    if kind == "0.02_per_channel":
        w = w * torch.exp2(-8 * torch.rand(n, 1, device="cuda", generator=g))
    return w


# ------------------------------------------------------------------ GEMM
GEMM_TABLE = [                       # (M, N, K); instance from gemm_instance at run time
    (38400, 256, 128), (70000, 256, 136), (300, 256, 128), (300, 256, 136), (129, 64, 64), (4100, 40, 72), (32768, 256, 16),
    (66000, 320, 320),
]


def gemm_case(ops, failures, shape, wk="inv_sqrt_k", s=0, bias=True, res=True, act=1, seed=0):
    M, Nn, K = shape
    g = torch.Generator(device="cuda").manual_seed(M + Nn + K + seed)
    x = torch.randn(M, K, device="cuda", generator=g) * 2.0 ** s
    w = weights(wk, Nn, K, g)
    b = torch.randn(Nn, device="cuda", generator=g) * 2.0 ** s * 0.1 if bias else None
    r = torch.randn(M, Nn, device="cuda", generator=g) * 2.0 ** s * 0.1 if res else None
    got = ops.gemm_bf16_bias_act(x, ops.gemm_bf16_weights(w), b, act, residual=r)
    twin = ops.gemm_split_bias_act(x, ops.gemm_split_weights(w), b, act, residual=r)
    y, T, D = R.gemm_model(x, w, b, r, act)
    ref, Dx = R.gemm_exact(x, w, b, r, act)
    e_t = R.arith_error(twin, ref, 0, Dx)
    what = f"gemm {shape} w {wk} x*2^{s}{'' if bias else ' bias=None'}{' +res' if res else ''}{' relu' if act else ''}"
    check(failures, what, gemm_instance(M, Nn, K), R.arith_error(got, y, T, D), R.arith_error(got, ref, 0, Dx), e_t, torch.equal(got, twin))


@pytest.mark.parametrize("shape", GEMM_TABLE, ids=[f"{m}x{n}x{k}" for m, n, k in GEMM_TABLE])
def test_gemm_bf16_instances(ops, shape):
    failures = []
    gemm_case(ops, failures, shape)
    gemm_case(ops, failures, shape, bias=False, res=False, act=0)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("shape", [(300, 256, 136), (38400, 256, 128)])
def test_gemm_bf16_magnitude_sweep(ops, shape):
    failures = []
    for wk in WEIGHTS:
        for s in SCALES:
            gemm_case(ops, failures, shape, wk, s)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ Winograd
# (B, H, W, Cin, Cout, dilation, mode, residual, relu)
WINO_TABLE = [
    (2, 20, 36, 32, 64, 1, 0, True, True),
    (1, 33, 47, 32, 128, 2, 0, True, True),            # ragged, dilation 2
    (1, 37, 29, 16, 64, 4, 0, False, False),           # one Cin chunk, dilation 4, no residual, no ReLU
    (2, 16, 32, 2048, 64, 1, 0, False, True),          # Cin 2048
    (2, 160, 256, 64, 128, 1, 0, True, True),          # persistent, tpb 2
    (1, 192, 192, 256, 256, 2, 0, False, True),        # persistent, tpb 2, dilation 2
    (2, 20, 36, 32, 64, 1, 1, False, True),            # fused 1x1 + sigmoid
    (1, 33, 47, 16, 64, 2, 1, False, True),
    (4, 160, 256, 32, 64, 1, 1, False, True),          # fused head, persistent, tpb 2
]


def wino_case(ops, failures, case, wk="inv_sqrt_k", s=0, seed=0):
    B, H, W, cin, cout, d, mode, res, relu = case
    g = torch.Generator(device="cuda").manual_seed(B + H + W + cin + cout + d + seed)
    x = torch.randn(B, H, W, cin, device="cuda", generator=g) * 2.0 ** s
    wt = weights(wk, cout, cin * 9, g).view(cout, cin, 3, 3)
    scale = torch.rand(cout, device="cuda", generator=g) + 0.5
    shift = torch.randn(cout, device="cuda", generator=g) * 2.0 ** s * 0.1
    r = torch.randn(B, H, W, cout, device="cuda", generator=g) * 2.0 ** s * 0.1 if res else None
    w2 = torch.randn(cout, device="cuda", generator=g) * 0.2 if mode == 1 else None
    b2 = torch.randn(1, device="cuda", generator=g) if mode == 1 else None
    act = 1 if relu else 0
    ub = ops.winograd_bf16_weights(wt, scale)
    got = ops.conv3x3_winograd_bf16(x, ub, cout, shift, act=act, dilation=d, residual=r, w2=w2, b2=b2)
    twin = ops.conv3x3_winograd_split(x, ops.winograd_split_weights(wt, scale), cout, shift, act=act, dilation=d, residual=r, w2=w2, b2=b2)
    y, T, D = R.winograd_model(x, ub, cout, shift, d, r, act, w2, b2)
    ref, Dx = R.winograd_exact(x, wt, scale, shift, d, r, act, w2, b2)
    e_t = R.arith_error(twin, ref, 0, Dx)
    what = f"winograd {case[:6]}{' +res' if res else ''}{' relu' if relu else ''} w {wk} x*2^{s}"
    check(failures, what, wino_instance(B, H, W, cin, cout, d, mode), R.arith_error(got, y, T, D), R.arith_error(got, ref, 0, Dx), e_t,
          torch.equal(got, twin))


@pytest.mark.parametrize("case", WINO_TABLE, ids=[f"{c[:6]}m{c[6]}" for c in WINO_TABLE])
def test_winograd_bf16_instances(ops, case):
    failures = []
    wino_case(ops, failures, case)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", [WINO_TABLE[1], WINO_TABLE[4]], ids=["wino8s", "wino8p"])
def test_winograd_bf16_magnitude_sweep(ops, case):
    failures = []
    for wk in WEIGHTS:
        for s in SCALES:
            wino_case(ops, failures, case, wk, s)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ switch variants, one child process each
VARIANTS = [("AWSEG_WINO8_TPB", "3"), ("AWSEG_WINO8_TPB", "64")]
VARIANT_WINO = [WINO_TABLE[1], WINO_TABLE[2], WINO_TABLE[6]]


@pytest.mark.parametrize("name,value", VARIANTS, ids=[f"{n}={v}" for n, v in VARIANTS])
def test_bf16_switch_variants(name, value):
    env = dict(os.environ, **{name: value})
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_bf16_arith import _variant_main; _variant_main()"],
                       cwd=str(ROOT), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0, out[-3000:]
    rows = out.count("ok   [") + out.count("FAIL [")
    assert rows == len(VARIANT_WINO)
    assert out.count("wino8p_kernel") == len(VARIANT_WINO)


def _variant_main():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native, ops
    _native.lib()
    failures = []
    for case in VARIANT_WINO:
        wino_case(ops, failures, case)
    if failures:
        print("\n".join(failures))
        sys.exit(1)


# ------------------------------------------------------------------ attention
ATTN_TABLE = [(2, 1, 300, 32), (1, 8, 200, 64), (2, 5, 300, 2048), (1, 2, 1000, 64)]


def attn_case(ops, failures, shape, packed, vs=0, spread=1.0, offset=0.0, seed=0):
    B, nh, nq, nkv = shape
    g = torch.Generator(device="cuda").manual_seed(B + nh + nq + nkv + seed)
    C = nh * 32
    q, k = (torch.randn(B, n, C, device="cuda", generator=g) * (spread ** 0.5) for n in (nq, nkv))
    v = torch.randn(B, nkv, C, device="cuda", generator=g) * 2.0 ** vs
    if offset:                                           # logits ~ offset: a component every query and key share
        a = (offset / 32 ** -0.5) ** 0.5
        q[..., 0::32] += a
        k[..., 0::32] = a
    scale = 32 ** -0.5
    with ops.precision("bf16"):
        got = ops.attention_d32_packed_kv(q, torch.cat([k, v], -1), nh, scale) if packed else ops.attention_d32(q, k, v, nh, scale)
    twin = ops.attention_d32(q, k, v, nh, scale, split=True)
    y, T, D = R.attention_model(q, k, v, nh, scale)
    ref, Dx = R.attention_exact(q, k, v, nh, scale)
    e_t = R.arith_error(twin, ref, 0, Dx)
    tie = (T / D).median().item() / 2.0 ** -22                         # how wide the window is: median T / D, units of 2^-22
    what = (f"attention {shape} {'packed k|v' if packed else 'plain'} v*2^{vs} logit spread {spread:g}{f' offset {offset:g}' if offset else ''}"
            f" (median T/D {tie:.0f})")
    check(failures, what, "attention_d32_bf16_kernel" + (" (packed_kv mode 2)" if packed else ""), R.arith_error(got, y, T, D), None, e_t,
          torch.equal(got, twin))


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed_kv"])
@pytest.mark.parametrize("shape", ATTN_TABLE, ids=[f"{b}x{h}x{q}x{k}" for b, h, q, k in ATTN_TABLE])
def test_attention_bf16_instances(ops, shape, packed):
    failures = []
    attn_case(ops, failures, shape, packed)
    assert not failures, "\n".join(failures)


def test_attention_bf16_magnitude_sweep(ops):
    failures = []
    for vs in SCALES:
        attn_case(ops, failures, (2, 2, 300, 256), False, vs=vs)
    for spread, offset in ((16.0, 0.0), (2.0, 1000.0)):
        attn_case(ops, failures, (2, 2, 300, 256), False, spread=spread, offset=offset)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ depth head in bf16 (MODE 2 and the two-launch path)
DEPTH = [(1, 1, 1, 128), (2, 1, 2, 128), (2, 2, 3, 128), (1, 3, 2, 128), (2, 4, 5, 128), (2, 8, 10, 128)]


@pytest.mark.parametrize("cfg", DEPTH, ids=[f"{b}x{h}x{w}" for b, h, w, _ in DEPTH])
def test_depth_head_bf16(ops, cfg):
    """DepthEstimationHead.forward_from_lowres under ops.precision("bf16"): ops.DEPTH_FUSED = False (the upconv kernel writes the
    hidden map, the MODE 1 Winograd fetches it: modelled on that map with T = 0) and the fused launch (wino8p_kernel<2, bf16>,
    hidden map generated in the kernel: the same model with the tie window of tests/bf16_ref.py), on the weight image and shift
    the module caches.  Precision against the as-written module in float64.  The 1x1's weights are scaled so the depth logits
    are O(1) (a saturated sigmoid would hide any error).  Each row prints the largest absolute error the arithmetic gate allows."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.models.model import DepthEstimationHead, upconv3x3_bn_relu
    B, h, w, hidden = cfg
    torch.manual_seed(B * 1000 + h * 100 + w * 10)
    head = DepthEstimationHead(in_channels=256, hidden_channels=hidden).eval()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.normal_(0, 0.3)
            if isinstance(m, torch.nn.Conv2d) and m.bias is not None:
                m.bias.normal_(0, 0.2)
        head.depth_head[7].weight.mul_(0.02)
    head = head.cuda()
    feats = torch.randn(B, h, w, 256, device="cuda")
    hd = head.depth_head
    failures = []
    saved = ops.DEPTH_FUSED
    try:
        with torch.no_grad():
            ops.DEPTH_FUSED = True
            twin = head.forward_from_lowres(feats, 32 * h, 32 * w)[:, 0]
            got = {}
            with ops.precision("bf16"):
                for fused in (True, False):
                    ops.DEPTH_FUSED = fused
                    got[fused] = head.forward_from_lowres(feats, 32 * h, 32 * w)[:, 0]
                mid = upconv3x3_bn_relu(feats, hd[0], hd[1], 32 * h, 32 * w).permute(0, 2, 3, 1)    # the map the two-launch path fetches
            ub, sh2 = hd[4]._awseg_wino_bf16[1]                                                 # the image the module built and cached
            ref, Dx = R.depth_exact(head, feats)
            e_t = R.arith_error(twin, ref, 0, Dx)
            for fused in (True, False):
                y, T, D = R.depth_model(head, feats, mid, ub, sh2, fused=fused)
                allow = (T + gate_bound(e_t) * D).max().item()
                inst = wino_instance(B, 32 * h, 32 * w, hidden, 64, 1, 2 if fused else 1)
                check(failures, f"depth head {cfg} {'fused' if fused else 'two launches'} (allows {allow:.1e} abs)", inst,
                      R.arith_error(got[fused], y, T, D), R.arith_error(got[fused], ref, 0, Dx), e_t, torch.equal(got[fused], twin))
    finally:
        ops.DEPTH_FUSED = saved
    assert not failures, "\n".join(failures)
