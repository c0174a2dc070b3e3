"""-m gpu: the stale-integer-maximum loop of the split-operand attention kernels (csrc/attn.hip) on inputs built around its branch.

The in-range passes of attention_d32_split_kernel (awseg_attention_d32_split, awseg_attention_d32_packed_kv mode 1) and of
attention_d32_split_img_kernel (awseg_attention_d32_split_ws) subtract a stale integer maximum m per query and rescale, a whole wave
at a time, only when a tile's maximum lies more than TAU = kTau bits above it.  Every case prescribes the scores in log2 units,

    s[i, j] = base[j] + shift[i] + sel[i] * boost[j] (+ noise[i, j]),

through four operand dimensions (q = (1, shift, sel, ...), k = (base, 1, boost, ...) / (scale log2 e)), so that a known set of
(query, tile) pairs takes the rescale path; `stale_path` below restates the loop's control flow on the float64 scores and the test
asserts that the inputs do what the case says before it looks at the kernels.  Each split entry point is then held to float64 softmax
attention under the gate of tests/test_gpu_split_magnitudes.py (e = |got - ref64| / D, D = sum_k P_k |v_k| + 2 max|v| scale max_k
sum_d |q_d||k_kd|, e_split <= max(4 e_f32, 2^-20) with e_f32 the float32-MFMA kernel awseg_attention_d32 on the same inputs) and
to the absolute form of tests/test_gpu_kernels.py (|err| < 4 |err_f32| + 1e-6); the three float32-grade forms must agree bit for
bit.  The bf16 instance (awseg_attention_d32_bf16, packed_kv mode 2) keeps the exact running maximum — tests/bf16_ref.py pins the
constant its probabilities are rounded against — and is held to that model on cases (a)-(c).

Shapes: head_dim 32, 1 / 2 / 3 key tiles, 33 / 128 / 160 queries (a ragged wave, one full block, a ragged second block), 1 and 2
heads, 2 images."""
import math

import pytest
import torch

from tests import bf16_ref as R
from tests.split_ref import gate_bound

pytestmark = pytest.mark.gpu

TAU = 4                                     # kTau of csrc/attn.hip: the cases are built around it
LIMIT = 2048                                # kStaleLimit: |m| beyond it sends the block to the exact-maximum loop
LOG2E = 1.4426950408889634
SCALE = 32 ** -0.5
KAPPA = 1.0 / (SCALE * LOG2E)               # operand value worth one bit of score
EPS = 2.0 ** -9                             # margin that the float32 rounding of KAPPA-scaled operands (~1e-6 relative) cannot cross
B = 2
SHAPES = [(nq, nkv, nh) for nq in (33, 128, 160) for nkv in (32, 64, 96) for nh in (1, 2)]
SPLIT_FORMS = ("in_block", "prepared_image", "packed_kv_mode1")


@pytest.fixture(scope="module")
def N(native):
    return native


def run(N, form, q, k, v, nh):
    """one entry point through _native.call: q [B,nq,C], k / v [B,nkv,C] -> [B,nq,C]"""
    b, nq, _ = q.shape
    nkv = k.shape[1]
    out = torch.empty_like(q)
    plain = {"float32": "awseg_attention_d32", "in_block": "awseg_attention_d32_split", "bf16": "awseg_attention_d32_bf16"}
    if form in plain:
        N.call(plain[form], N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(out), b, nh, nq, nkv, SCALE, N.stream())
    elif form == "prepared_image":
        ws = torch.empty(int(N.lib().awseg_attention_d32_split_workspace(b, nh, nkv)), dtype=torch.uint8, device=q.device)
        N.call("awseg_attention_d32_split_ws", N.ptr(q), N.ptr(k), N.ptr(v), 0, N.ptr(out), b, nh, nq, nkv, SCALE, N.ptr(ws), N.stream())
    else:
        kv = torch.cat([k, v], dim=-1).contiguous()
        N.call("awseg_attention_d32_packed_kv", N.ptr(q), N.ptr(kv), N.ptr(out), b, nh, nq, nkv, SCALE, {"packed_kv_mode1": 1, "packed_kv_mode2": 2}[form], N.stream())
    return out


def build(nq, nkv, nh, base, shift=None, sel=None, boost=None, noise=0.0, seed=0):
    """q, k, v [B, n, nh*32] (every image and head alike but for noise and v) with the docstring's scores; base / boost [nkv],
    shift / sel [nq] in bits."""
    g = torch.Generator(device="cuda").manual_seed(1000 * nq + 10 * nkv + nh + seed)
    C = nh * 32
    q = torch.randn(B, nq, C, device="cuda", generator=g) * noise
    k = torch.randn(B, nkv, C, device="cuda", generator=g) * noise * KAPPA
    v = torch.randn(B, nkv, C, device="cuda", generator=g)
    dev = lambda t, n: (torch.zeros(n, device="cuda") if t is None else torch.as_tensor(t, dtype=torch.float32, device="cuda"))   # noqa: E731
    for h in range(nh):
        q[..., 32 * h + 0] = 1.0
        k[..., 32 * h + 0] = (dev(base, nkv).double() * KAPPA).float()
        q[..., 32 * h + 1] = dev(shift, nq)
        k[..., 32 * h + 1] = KAPPA
        q[..., 32 * h + 2] = dev(sel, nq)
        k[..., 32 * h + 2] = (dev(boost, nkv).double() * KAPPA).float()
    return q, k, v


def scores_bits(q, k, nh):
    qh, kh = (t.double().view(B, -1, nh, 32).transpose(1, 2) for t in (q, k))
    return qh @ kh.transpose(-1, -2) * (SCALE * LOG2E)                     # [B, nh, nq, nkv]


def stale_path(q, k, nh):
    """The loop's control flow on float64 scores: rescales[b, h, i, t] (tile t >= 1: query i's tile maximum is more than TAU above its
    stale m), waves[b, h, w, t] (the branch is taken: some query of the 32 does), and m_first = ceil(first tile's maximum)."""
    s = scores_bits(q, k, nh)
    nq, T = s.shape[2], s.shape[3] // 32
    tm = s.view(B, nh, nq, T, 32).amax(-1)
    pad = (-nq) % 32
    if pad:
        tm = torch.cat([tm, tm[:, :, -1:].expand(-1, -1, pad, -1)], 2)    # a ragged wave's idle lanes repeat the last query
    m = tm[..., 0].ceil()
    m_first = m[:, :, :nq].clone()
    resc = torch.zeros(B, nh, nq + pad, T, dtype=torch.bool, device=s.device)
    waves = torch.zeros(B, nh, (nq + pad) // 32, T, dtype=torch.bool, device=s.device)
    for t in range(1, T):
        trig = tm[..., t] - m > TAU
        wv = trig.view(B, nh, -1, 32).any(-1)
        resc[..., t], waves[..., t] = trig, wv
        m = torch.where(wv.repeat_interleave(32, -1), torch.maximum(m, tm[..., t].ceil()), m)
    return resc[:, :, :nq], waves, m_first


def reference(q, k, v, nh):
    """float64 softmax attention and the denominator D of tests/test_gpu_split_magnitudes.py"""
    _, nq, C = q.shape
    qh, kh, vh = (t.double().view(B, -1, nh, 32).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * SCALE, dim=-1)
    back = lambda t: t.transpose(1, 2).reshape(B, nq, C)                   # noqa: E731
    sm = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(dim=-1, keepdim=True) * SCALE
    vm = vh.abs().amax(dim=2, keepdim=True)
    return back(p @ vh), back(p @ vh.abs()) + back(2 * sm * vm)


def err(got, ref, den):
    got = got.double()
    if not torch.isfinite(got).all():
        return math.inf
    return ((got - ref).abs() / den).max().item()


def check_split(N, failures, what, q, k, v, nh):
    """every float32-grade split form against float64 under both gate forms, and the forms against each other bit for bit"""
    ref, den = reference(q, k, v, nh)
    f32 = run(N, "float32", q, k, v, nh)
    e_f, a_f = err(f32, ref, den), (f32.double() - ref).abs().max().item()
    outs = {}
    for form in SPLIT_FORMS:
        outs[form] = got = run(N, form, q, k, v, nh)
        e_s, a_s = err(got, ref, den), (got.double() - ref).abs().max().item() if torch.isfinite(got).all() else math.inf
        ok = e_s <= gate_bound(e_f) and a_s < 4 * a_f + 1e-6
        u = 2.0 ** -22
        print(f"{'ok  ' if ok else 'FAIL'} {what} [{form}]: e_split {e_s / u:8.2f}  e_f32 {e_f / u:6.2f} (x 2^-22; gate {gate_bound(e_f) / u:.2f})"
              f"  |err| {a_s:.2e} (float32 kernel {a_f:.2e})")
        if not ok:
            failures.append(f"{what} [{form}]: e_split {e_s:.3e} > {gate_bound(e_f):.3e} or |err| {a_s:.3e} >= 4 x {a_f:.3e} + 1e-6")
    for form in SPLIT_FORMS[1:]:
        if not torch.equal(outs[form], outs["in_block"]):
            failures.append(f"{what}: {form} differs from in_block by {(outs[form] - outs['in_block']).abs().max().item():.3e}")
    return outs["in_block"]


def tiles_of(nkv):
    return torch.arange(nkv) // 32


def case_inputs(case, nq, nkv, nh):
    """(q, k, v) of a float32-grade case and a predicate on stale_path's output that says the inputs do what the case is about"""
    T = nkv // 32
    t_of = tiles_of(nkv).float()
    within = (torch.arange(nkv) % 32).float()
    wobble = torch.linspace(-3.0, 3.0, nq).round() + 0.25 * (torch.arange(nq) % 4)      # per-query shift: m sits 0 .. 0.75 above the maximum
    if case == "a_every_tile_rescales":
        base = 6.0 * t_of - 2.0 * within / 31.0 - EPS                      # tile maxima 0, 6, 12 (- EPS), the rest up to 2 bits lower
        q, k, v = build(nq, nkv, nh, base, shift=wobble, noise=0.15)
        return q, k, v, lambda r, w, m: bool(r[..., 1:].all())
    if case == "b_drift_below_trigger":
        # integer-shift queries: maximum -EPS, then TAU - 2 EPS above m in tile 1 and again in tile 2: the largest rise that stays under
        # the trigger, probabilities up to 2^(15 - 2 EPS); no tile rescales for any query
        top = torch.tensor([-EPS, TAU - 2 * EPS, TAU - 2 * EPS])[:T]
        base = top[tiles_of(nkv)] - 3.0 * (within > 0)
        q, k, v = build(nq, nkv, nh, base, shift=wobble)
        return q, k, v, lambda r, w, m: not bool(r.any())
    if case == "b_drift_then_trigger":
        # TAU - 2 EPS per tile, twice: the second rise is 2 TAU - 4 EPS against the stale value and rescales (integer-shift queries;
        # the others, whose m sits a fraction above their maximum, have more headroom and follow their wave)
        top = torch.tensor([-EPS, TAU - 3 * EPS, 2 * TAU - 5 * EPS])[:T]
        base = top[tiles_of(nkv)] - 3.0 * (within > 0)
        q, k, v = build(nq, nkv, nh, base, shift=wobble)
        return q, k, v, lambda r, w, m: (not bool(r[..., :2].any())) and (T < 3 or bool(w[..., 2].all()))
    if case == "c_maximum_first_then_floor":
        base = torch.where(t_of == 0, -3.0 * within / 31.0 - EPS, -20.0 - 10.0 * within / 31.0)     # later keys 20 .. 30 bits down
        q, k, v = build(nq, nkv, nh, base, shift=wobble, noise=0.15)
        return q, k, v, lambda r, w, m: not bool(r.any())
    if case == "d_maximum_in_upper_half_wave":
        # every tile's leading key is key 5 of the tile (accumulator row 5: wave half 1); the others sit 12 bits lower
        base = torch.where(within == 5, 7.0 * t_of - EPS, 7.0 * t_of - 12.0)
        q, k, v = build(nq, nkv, nh, base, shift=wobble, noise=0.15)
        return q, k, v, lambda r, w, m: bool(r[..., 1:].all())
    if case == "e_one_query_of_a_wave":
        # query 5 of every wave alone sees key 9 of the later tiles 10 bits up
        sel = (torch.arange(nq) % 32 == 5).float()
        base = -EPS - 2.0 * within / 31.0
        boost = torch.where((within == 9) & (t_of > 0), 10.0 + 2.0, 0.0)
        q, k, v = build(nq, nkv, nh, base, shift=wobble, sel=sel, boost=boost)
        one = lambda r: bool((r[..., 1].view(B, nh, -1).sum(-1) == ((nq + 31 - 5) // 32)).all())   # noqa: E731
        return q, k, v, lambda r, w, m: T == 1 or one(r)
    if case == "f_maximum_out_of_integer_range":
        # queries 1 and 2 of the first block: every score near +2500 / -2500 bits (operands in range: no range-guard rerun)
        shift = wobble.clone(); shift[1] = 2500.0; shift[2] = -2500.0
        base = -EPS - 6.0 * within / 31.0 + 5.0 * t_of
        q, k, v = build(nq, nkv, nh, base, shift=shift, noise=0.15)
        out = lambda m: (m.abs() > LIMIT)                                   # noqa: E731
        return q, k, v, lambda r, w, m: bool(out(m)[:, :, 1:3].all()) and int(out(m).sum()) == 2 * B * nh and float(q.abs().max() * SCALE * LOG2E) < 32768
    if case == "g_query_beyond_f16_range":
        base = 6.0 * t_of - 2.0 * within / 31.0 - EPS
        q, k, v = build(nq, nkv, nh, base, shift=wobble, noise=0.15)
        q[:, 1, 3::32] = 2.0 ** 18                                          # |q scale log2 e| = 2^18 x 0.255 >= 2^15 in the first block
        k[:, :, 3::32] *= 2.0 ** -17
        return q, k, v, lambda r, w, m: float(q.abs().max() * SCALE * LOG2E) >= 32768
    raise ValueError(case)


CASES = ["a_every_tile_rescales", "b_drift_below_trigger", "b_drift_then_trigger", "c_maximum_first_then_floor", "d_maximum_in_upper_half_wave",
         "e_one_query_of_a_wave", "f_maximum_out_of_integer_range", "g_query_beyond_f16_range"]


@pytest.mark.parametrize("case", CASES)
def test_split_attention_stale_maximum(N, case):
    failures = []
    for nq, nkv, nh in SHAPES:
        q, k, v, built = case_inputs(case, nq, nkv, nh)
        assert built(*stale_path(q, k, nh)), f"{case} {nq} q x {nkv} k x {nh} heads: the inputs do not take the path the case is about"
        check_split(N, failures, f"{case} {nq} q x {nkv} k x {nh} h", q, k, v, nh)
    assert not failures, "\n".join(failures)


def test_escape_is_block_uniform(N):
    """Case (f) again at 160 queries: the first block (queries 0..127) holds the two out-of-range queries and runs the exact-maximum
    loop whole; the second block does not.  Rows of the second block must equal, bit for bit, what the kernel gives for them when no
    query of the launch is out of range; rows of the first block must equal the in-range launch's only up to the gate (another loop)."""
    nq, nkv, nh = 160, 96, 2
    q, k, v, built = case_inputs("f_maximum_out_of_integer_range", nq, nkv, nh)
    assert built(*stale_path(q, k, nh))
    q_in = q.clone()
    q_in[:, 1:3, 1::32] = 0.0                                               # the same launch with queries 1, 2 in range
    assert not bool((stale_path(q_in, k, nh)[2].abs() > LIMIT).any())
    for form in SPLIT_FORMS:
        esc, plain = run(N, form, q, k, v, nh), run(N, form, q_in, k, v, nh)
        assert torch.equal(esc[:, 128:], plain[:, 128:]), form
        ref, den = reference(q_in, k, v, nh)
        keep = [i for i in range(128) if i not in (1, 2)]
        e = ((esc[:, keep].double() - ref[:, keep]).abs() / den[:, keep]).max().item()
        e_f = ((run(N, "float32", q_in, k, v, nh)[:, keep].double() - ref[:, keep]).abs() / den[:, keep]).max().item()
        assert e <= gate_bound(e_f), (form, e, e_f)


def test_prepared_image_and_in_block_agree_bit_for_bit_mid_size(N):
    """2 images x 2 heads x 1000 queries x 256 keys, standard normal q, k at x 1 (rescales in well under 1 % of the wave-tiles) and
    x 2 (in most): the three float32-grade forms give identical bits, within the float64 gate."""
    nh, nq, nkv = 2, 1000, 256
    g = torch.Generator(device="cuda").manual_seed(77)
    q0, k0, v = (torch.randn(B, n, nh * 32, device="cuda", generator=g) for n in (nq, nkv, nkv))
    failures = []
    for mult in (1.0, 2.0):
        q, k = q0 * mult, k0 * mult
        w = stale_path(q, k, nh)[1][..., 1:].float().mean().item()
        print(f"x{mult:g}: {100 * w:.1f} % of the wave-tiles behind the first rescale")
        check_split(N, failures, f"mid-size x{mult:g}", q, k, v, nh)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", CASES[:4])
def test_bf16_instance_keeps_the_exact_maximum_model(N, case):
    """(h) the bf16 instance (plain and packed_kv mode 2) on cases (a)-(c) against tests/bf16_ref.attention_model, gated by the
    float32-grade twin's error as in tests/test_gpu_bf16_arith.py"""
    failures = []
    for nq, nkv, nh in [(33, 96, 1), (160, 64, 2), (128, 96, 2)]:
        q, k, v, _ = case_inputs(case, nq, nkv, nh)
        twin = run(N, "in_block", q, k, v, nh)
        y, T, D = R.attention_model(q, k, v, nh, SCALE)
        ref, Dx = R.attention_exact(q, k, v, nh, SCALE)
        e_t = R.arith_error(twin, ref, 0, Dx)
        for form in ("bf16", "packed_kv_mode2"):
            got = run(N, form, q, k, v, nh)
            e_a = R.arith_error(got, y, T, D)
            ok = e_a <= gate_bound(e_t) and not torch.equal(got, twin)
            print(f"{'ok  ' if ok else 'FAIL'} {case} {nq} q x {nkv} k x {nh} h [{form}]: e_arith {e_a / 2 ** -22:8.2f}  e_twin {e_t / 2 ** -22:6.2f} (x 2^-22)")
            if not ok:
                failures.append(f"{case} {nq} x {nkv} x {nh} [{form}]: e_arith {e_a:.3e} > {gate_bound(e_t):.3e}")
    assert not failures, "\n".join(failures)
