"""Reference side of the bf16 accuracy tests (nothing in the package imports this module).

The bf16 MFMA path (BASELINE config 5, `ops.precision("bf16")`) rounds operands to bf16 (round to nearest even, as
v_cvt_pk_bf16_f32 and torch's `.to(torch.bfloat16)` do) and accumulates their exact products in float32.  This module
holds float64 MODELS of what each bf16 kernel is asked to compute — every rounding the kernel makes, at the place it makes
it — and the two gates the kernels are held to.  The models are device-agnostic torch (float64 plus explicit float32
steps), so tests/test_bf16_ref.py checks them and the gates on the CPU with the same code the GPU tests run.

(a) ARITHMETIC gate.  A model returns (y, T, D) per output element: y in float64, a tie window T and the denominator D of
the componentwise metric

        e = max(|got - y| - T, 0) / D,      e <= split_ref.gate_bound(e_twin),

where e_twin is the same metric for the float32-grade twin kernel on the same inputs against the exact float64 result
(gemm_split_bias_act, conv3x3_winograd_split, attention_d32_split, the fused depth head on the split image).  No constant of
its own: the float32 accumulation noise a bf16 kernel may add is the noise its twin adds.  T = 0 where the model's bf16
operands are bit-exact (GEMM; Winograd on fetched inputs).  Where the kernel computes an operand in float32 that the model
computes in float64 (attention's probabilities, the depth head's generated hidden map), the two may round to different bf16
neighbours when the value lies within the float32 error w of a rounding boundary; T sums ulp_bf16 x |partner| over those
elements only.

(b) PRECISION gate (GEMM, Winograd).  |got - exact64| / D_unrounded <= 2^-7 + 2^-16 + gate_bound(e_twin), with exact64 and D
from the UNROUNDED operands: a product of two RNE-rounded operands is off by at most (2u + u^2)|a||b|, u = 2^-8 the unit
roundoff of bf16's 8-bit significand (|bf16(a) - a| <= 2^-8 |a|): 2^-7 + 2^-16.  (K = 16 products already reach 2^-7.8.)

Window derivations.
  * Attention: the kernel's logit s32 = sum_d q~_d k~_d is a float32 MFMA accumulation of 32 exact products, so
    |s32 - s64| <= gamma_32 S, gamma_32 = 32 * 2^-24, S = max_j sum_d |q~_d k~_jd| (per query).  The probability's exponent
    s - m_sh carries that error twice (s and the running maximum) plus the float32 roundings of m_new - 15 and s - m_sh
    (<= 3 ulp_f32(max|s| + 16)), and v_exp_f32 adds <= 2^-22 relative:  w_p = ln2 (2 gamma_32 S + 3 ulp_f32(max|s| + 16))
    + 2^-22, relative to p.  The same w_p bounds the relative difference of l (which sums the unrounded p) and the float32
    sum of l adds (ntiles + 20) 2^-24 (16 adds per lane, one exchange, one rescale per tile, 1/l and the final product);
    both shift out / D by at most that much, so T_attn = sum_tie ulp_bf16(p_j)|v~_j| / l + (w_p + gamma_l) D.
  * Depth head.  The two-launch path fetches the hidden map the upconv kernel wrote: its model is the Winograd model on that
    very map (T = 0).  The fused path (MODE 2) generates the same map inside the kernel from bilinear forms of the SAME g9
    (tok @ W1, computed once): the forms are float64 sums rounded once (<= 36 terms), evaluated in a few float32 operations,
    while the upconv kernel sums <= 36 float32 terms.  The two maps therefore differ by at most (36 + 36 + 8) 2^-24 of the
    hidden layer's own denominator D_h = conv(|up|, |w1 scale|) + |shift1| (not of |hidden|: a value near ReLU's kink is a
    difference of large terms), and MODE 2 is modelled on the fetched map with the tie window w_v = 80 2^-24 |B^T| D_h |B|
    on V.  D is built from |hidden| in both.  That window still covers a bf16 rounding boundary for a few per cent of the V
    elements, so the MODE 2 arithmetic gate holds the fused kernel to the level of its T (printed by the GPU test), not to
    bf16 rounding: it does not see a rounding-mode error, which the two-launch and Winograd MODE 0 / 1 cases (the same
    transform code) do.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests.split_ref import gate_bound

LOG2E = 1.4426950408889634
PREC_BOUND = 2.0 ** -7 + 2.0 ** -16          # (2u + u^2), u = 2^-8: product of two RNE-rounded operands
GAMMA32 = 32 * 2.0 ** -24                    # float32 accumulation of 32 exact products (attention logits)
EXP_REL = 2.0 ** -22                         # v_exp_f32, relative

BT = ((1.0, 0.0, -1.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, -1.0, 1.0, 0.0), (0.0, 1.0, 0.0, -1.0))
AT = ((1.0, 1.0, 1.0, 0.0), (0.0, 1.0, -1.0, -1.0))
G3 = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


# ------------------------------------------------------------------ rounding
def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """float32 -> bf16 (round to nearest even) -> float32."""
    return t.float().to(torch.bfloat16).float()


def bf16_rtz(t: torch.Tensor) -> torch.Tensor:
    """float32 -> bf16 rounded toward zero (the top 16 bits kept) -> float32: the rounding a sabotaged kernel would make."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()


def ulp_bf16(a: torch.Tensor) -> torch.Tensor:
    """spacing of bf16 numbers at |a| (float64; the smallest normal's spacing below 2^-126)"""
    _, e = torch.frexp(a.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a, dtype=torch.float64), e - 8)


def ulp_f32(a: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(a.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a, dtype=torch.float64), e - 24)


def tie_delta(x: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    """Largest |bf16(a) - bf16(x)| over |a - x| <= win: 0 where no bf16 rounding boundary lies within win of x, else
    ulp_bf16(|x| + win) + win (one boundary crossed; within a few ulp of zero, several)."""
    x = x.double()
    win = torch.as_tensor(win, dtype=torch.float64, device=x.device).expand_as(x)
    u = ulp_bf16(x)
    q = x.abs() / u
    frac = q - q.floor()
    dist = (frac - 0.5).abs() * u                                         # to the midpoint inside this binade
    lower = torch.where(q.floor() == 128, (frac + 0.25) * u, torch.full_like(u, math.inf))   # just above a power of two
    tie = (torch.minimum(dist, lower) <= win) | (u < 4 * win)
    return torch.where(tie, ulp_bf16(x.abs() + win) + win, torch.zeros_like(x))


# ------------------------------------------------------------------ metrics
def arith_error(got, y, T, D) -> float:
    """max (|got - y| - T)_+ / D; D == 0 demands |got - y| <= T.  Non-finite output: inf."""
    got = got.double()
    if not torch.isfinite(got).all():
        return math.inf
    e = ((got - y).abs() - T).clamp_min(0)
    zero = D == 0
    if (e[zero] != 0).any():
        return math.inf
    return (e[~zero] / D[~zero]).max().item() if (~zero).any() else 0.0


def arith_ok(e: float, e_twin: float) -> bool:
    return e <= gate_bound(e_twin)


def precision_ok(e: float, e_twin: float) -> bool:
    return e <= PREC_BOUND + gate_bound(e_twin)


# ------------------------------------------------------------------ GEMM
def gemm_model(x, w, bias=None, residual=None, act=0, rnd=bf16_rne, twice=None):
    """act(bf16(x) @ bf16(w)^T + bias + residual) in float64, T = 0, D = |x~| @ |w~|^T + |bias| + |residual|.
    twice = 'bias' | 'residual': a degraded model that adds that term twice."""
    xt, wt = rnd(x).double(), rnd(w).double()
    y, D = xt @ wt.t(), xt.abs() @ wt.abs().t()
    for name, t in (("bias", bias), ("residual", residual)):
        if t is not None:
            y, D = y + t.double() * (2 if twice == name else 1), D + t.double().abs()
    return (y.clamp_min(0) if act else y), torch.zeros_like(y), D


def gemm_exact(x, w, bias=None, residual=None, act=0):
    """exact float64 result and D of the unrounded operands"""
    return gemm_model(x, w, bias, residual, act, rnd=lambda t: t.double())[::2]


# ------------------------------------------------------------------ Winograd F(2x2, 3x3)
def _mat(rows, like):
    return torch.tensor(rows, dtype=torch.float64, device=like.device)


def decode_winograd_image(buf: torch.Tensor, cin: int, cout: int, bf16: bool = True):
    """ops.winograd_bf16_weights / winograd_split_weights image -> (U~ [16, Cin, Cout] float64 as stored, i.e. of U 2^-eu,
    2^eu).  Layout (include/awseg.h): [Cin/16][16 positions][Cout/32][hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15][32][8]
    + the float32 2^eu.  bf16: the high slots hold bf16 bits; else f16 high + low parts."""
    nch, ncb = cin // 16, cout // 32
    n = 16 * cin * cout * 2
    img = buf[:n].view(nch, 16, ncb, 2, 2, 32, 8)

    def back(t):                                    # [nch][p][ncb][h][32][8] -> [p][ci][co]
        return t.permute(1, 0, 3, 5, 2, 4).reshape(16, cin, cout).contiguous()
    hi = back(img[:, :, :, 0])
    if bf16:
        u = hi.view(torch.bfloat16).double()
    else:
        u = hi.view(torch.float16).double() + back(img[:, :, :, 1]).view(torch.float16).double()
    scale = buf[n:n + 2].contiguous().view(torch.float32).double().item()
    return u, scale


def winograd_u_exact(weight, scale=None):
    """U = G g G^T (times the per-Cout scale) in float64, [16, Cin, Cout]"""
    g = weight.double()
    if scale is not None:
        g = g * scale.double().view(-1, 1, 1, 1)
    G = _mat(G3, g)
    return torch.einsum("ik,ockl,jl->ijco", G, g, G).reshape(16, weight.shape[1], weight.shape[0])


def _patches(x, dil):
    """x [B,H,W,C] -> per residue (ry, rx): (d [B, nty, ntx, C, 4, 4] of the zero-padded sub-lattice, (ry, rx, Hs, Ws))"""
    B, H, W, C = x.shape
    out = []
    for ry in range(dil):
        for rx in range(dil):
            sub = x[:, ry::dil, rx::dil, :]
            Hs, Ws = sub.shape[1], sub.shape[2]
            nty, ntx = (Hs + 1) // 2, (Ws + 1) // 2
            p = F.pad(sub, (0, 0, 1, 2 * ntx + 1 - Ws, 1, 2 * nty + 1 - Hs))
            out.append((p.unfold(1, 4, 2).unfold(2, 4, 2), (ry, rx, Hs, Ws)))
    return out


def _input_transform_f32(d, v_round):
    """B^T d B in float32 in the kernel's order (rows: d0-d2, d1+d2, d2-d1, d1-d3, then the same on columns), rounded to bf16.
    v_round: 'rne' | 'rtz' | 'mid' (rounded between the row and the column transform too) | 'none' (float32 V)"""
    d = d.float()
    rnd = bf16_rtz if v_round == "rtz" else (lambda t: t) if v_round == "none" else bf16_rne

    def tr(t, dim):
        a, b, c, e = t.unbind(dim)
        return torch.stack([a - c, b + c, c - b, b - e], dim)
    t = tr(d, -2)
    if v_round == "mid":
        t = bf16_rne(t)
    return rnd(tr(t, -1)).double()


def winograd_model(x, u_img, cout, shift, dilation=1, residual=None, act=0, w2=None, b2=None, *, v_round="rne",
                   drop_chunk=None, twice=None, f32_sum=False, v_window=None, x_den=None, u=None):
    """Model of awseg_conv3x3_winograd_bf16_nhwc on x [B,H,W,Cin] float32: returns (y, T, D), y [B,H,W,Cout] (MODE 0) or the
    sigmoid [B,H,W] (MODE 1: w2 . relu(conv + shift) + b2; D and T of the logit divided by 4, the sigmoid's Lipschitz constant).
    U~ and 2^eu are decoded from the weight image (`u`: (U, 2^eu) given instead, e.g. unrounded for the precision gate).
    Degraded variants: v_round 'rtz' / 'mid', drop_chunk (a 16-channel chunk of Cin left out), twice 'shift' / 'residual'.
    f32_sum: the channel sum and output transform in float32, channels summed in reverse order (a different summation order).
    v_window / x_den: the depth head's generated input — V computed in float64 from x (float64) and a tie window
    v_window |B^T| x_den |B| around it (D still from |x|)."""
    B, H, W, cin = x.shape
    U, us = u if u is not None else decode_winograd_image(u_img, cin, cout)
    if drop_chunk is not None:
        U = U.clone(); U[:, 16 * drop_chunk:16 * drop_chunk + 16] = 0
    BTm, ATm = _mat(BT, U), _mat(AT, U)
    act = 1 if w2 is not None else act
    y = torch.zeros(B, H, W, cout, dtype=torch.float64, device=x.device)
    Dy, Ty = torch.zeros_like(y), torch.zeros_like(y)
    dens = _patches(x_den.double(), dilation) if x_den is not None else None
    for i, (d, (ry, rx, Hs, Ws)) in enumerate(_patches(x, dilation)):
        nb, nty, ntx = d.shape[:3]
        if v_window is not None:
            v = torch.einsum("ik,btsckl,jl->btscij", BTm, d.double(), BTm)
            win = v_window * torch.einsum("ik,btsckl,jl->btscij", BTm.abs(), dens[i][0], BTm.abs())
            dv = tie_delta(v, win)
            v = bf16_rne(v).double()
            vbar = torch.einsum("ik,btsckl,jl->btscij", BTm.abs(), d.double().abs(), BTm.abs())   # D from |hidden|, as for fetched inputs
        else:
            if v_round == "exact":                                       # float64 transform of float64 input (precision gate)
                v = torch.einsum("ik,btsckl,jl->btscij", BTm, d.double(), BTm)
            else:
                v = _input_transform_f32(d, v_round)
            vbar = torch.einsum("ik,btsckl,jl->btscij", BTm.abs(), d.double().abs(), BTm.abs())
            dv = None
        v, vbar = v.reshape(nb, nty, ntx, cin, 16), vbar.reshape(nb, nty, ntx, cin, 16)
        if f32_sum:
            m = torch.einsum("btscp,pco->btspo", v.float().flip(3), U.float().flip(1)).double()
        else:
            m = torch.einsum("btscp,pco->btspo", v, U)
        dm = torch.einsum("btscp,pco->btspo", vbar, U.abs())
        tm = torch.einsum("btscp,pco->btspo", dv.reshape(nb, nty, ntx, cin, 16), U.abs()) if dv is not None else None

        def out_tr(t, a):
            t = t.reshape(nb, nty, ntx, 4, 4, cout)
            if f32_sum and a is ATm:
                return torch.einsum("ai,btsijo,cj->btsaco", a.float(), t.float(), a.float()).double()
            return torch.einsum("ai,btsijo,cj->btsaco", a, t, a)

        def place(dst, t):
            t = t.permute(0, 1, 3, 2, 4, 5).reshape(nb, 2 * nty, 2 * ntx, cout)[:, :Hs, :Ws]
            dst[:, ry::dilation, rx::dilation] = t * us
        place(y, out_tr(m, ATm))
        place(Dy, out_tr(dm, ATm.abs()))
        if tm is not None:
            place(Ty, out_tr(tm, ATm.abs()))
    sh = shift.double()
    y, Dy = y + sh * (2 if twice == "shift" else 1), Dy + sh.abs()
    if residual is not None:
        r = residual.double()
        y, Dy = y + r * (2 if twice == "residual" else 1), Dy + r.abs()
    if act:
        y = y.clamp_min(0)
    if w2 is None:
        return y, Ty, Dy
    w2d = w2.double()
    z = y @ w2d + b2.double()
    return torch.sigmoid(z), (Ty @ w2d.abs()) / 4, (Dy @ w2d.abs() + b2.double().abs()) / 4


def winograd_exact(x, weight, scale, shift, dilation=1, residual=None, act=0, w2=None, b2=None):
    """exact float64 result (direct convolution of the unrounded operands) and D of the unrounded Winograd operands
    (D = |A^T| (sum_c |U| |B^T||d||B|) |A| + |shift| + |residual|; MODE 1 as in winograd_model)"""
    wsc = (weight * scale.view(-1, 1, 1, 1)).double() if scale is not None else weight.double()
    xd = x.double().permute(0, 3, 1, 2)
    y = F.conv2d(xd, wsc, None, 1, dilation, dilation).permute(0, 2, 3, 1) + shift.double()
    if residual is not None:
        y = y + residual.double()
    if act or w2 is not None:
        y = y.clamp_min(0)
    uex = winograd_u_exact(weight, scale)
    _, _, D = winograd_model(x.double(), None, weight.shape[0], shift, dilation, residual, act, v_round="exact", u=(uex, 1.0))
    if w2 is None:
        return y, D
    z = y @ w2.double() + b2.double()
    return torch.sigmoid(z), (D @ w2.double().abs() + b2.double().abs()) / 4


# ------------------------------------------------------------------ attention, head_dim 32
def attention_model(q, k, v, nh, scale, *, p_round="rne", drop_tile=None, no_alpha=False, q_round_first=False,
                    l_rounded=False, f32_steps=False, jitter=0.0, gen=None):
    """Model of attention_d32_bf16_kernel: q [B,nq,nh*32], k / v [B,nkv,nh*32] float32 -> (out, T, D) [B,nq,nh*32].
    q~ = bf16(fl32(q fl32(scale log2e))), k~ = bf16(k), v~ = bf16(v); 32-key tiles in order: m_new = max(m_run, tile max),
    m_sh = fl32(m_new - 15), p = 2^(s - m_sh), l = l alpha + sum p (unrounded), O = O alpha + V~^T bf16(p); out = O / l.
    T and D as in the module docstring.  Degraded variants: p_round 'rtz', drop_tile, no_alpha, q_round_first (q rounded
    before the scale product), l_rounded (l sums bf16(p)).  f32_steps: logits, probabilities, l and O in float32 (the kernel's
    own precision, a different summation order); jitter in [-1, 1]: every p moved by jitter * w_p * (random sign)."""
    B, nq, C = q.shape
    nkv = k.shape[1]
    qs = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).item()
    qq = bf16_rne(q) if q_round_first else q.float()
    qt = bf16_rne(qq * qs).double()
    kt, vt = bf16_rne(k).double(), bf16_rne(v).double()
    heads = lambda t: t.view(B, -1, nh, 32).transpose(1, 2)            # noqa: E731
    qh, kh, vh = heads(qt), heads(kt), heads(vt)
    s = qh @ kh.transpose(-1, -2)                                        # [B, nh, nq, nkv]
    if f32_steps:
        s = (qh.float() @ kh.float().transpose(-1, -2)).double()
    S = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    smax = s.abs().amax(-1, keepdim=True)
    w_p = math.log(2) * (2 * GAMMA32 * S + 3 * ulp_f32(smax + 16)) + EXP_REL          # [B, nh, nq, 1]
    ntiles = nkv // 32
    gamma_l = (ntiles + 20) * 2.0 ** -24
    rnd = bf16_rtz if p_round == "rtz" else bf16_rne
    m_run = torch.full_like(s[..., :1], -math.inf)
    l = torch.zeros_like(m_run)
    O = torch.zeros(B, nh, nq, 32, dtype=torch.float64, device=q.device)
    Tn, Dn = torch.zeros_like(O), torch.zeros_like(O)
    for t in range(ntiles):
        st, vtile = s[..., 32 * t:32 * t + 32], vh[:, :, 32 * t:32 * t + 32]
        if t == drop_tile:
            continue
        m_new = torch.maximum(m_run, st.amax(-1, keepdim=True))
        alpha = torch.exp2(m_run - m_new)
        m_sh = f32(m_new.float() - 15.0)
        if f32_steps:
            p = torch.exp2((st.float() - m_sh.float())).double()
        else:
            p = torch.exp2(st - m_sh)
        if jitter:
            sign = torch.randint(0, 2, p.shape, generator=gen, device="cpu").to(p.device) * 2.0 - 1.0
            p = p * (1 + jitter * w_p * sign)
        pr = rnd(p.float()).double()
        if no_alpha:
            alpha = torch.ones_like(alpha)
        if f32_steps:
            l = f32(l.float() * alpha.float() + p.float().sum(-1, keepdim=True))
            O = f32(O.float() * alpha.float() + pr.float() @ vtile.float())
        else:
            l = l * alpha + (pr if l_rounded else p).sum(-1, keepdim=True)
            O = O * alpha + pr @ vtile
        Tn = Tn * alpha + tie_delta(p, w_p * p) @ vtile.abs()
        Dn = Dn * alpha + pr @ vtile.abs()
        m_run = m_new
    back = lambda t: t.transpose(1, 2).reshape(B, nq, C)                # noqa: E731
    D = Dn / l
    return back(O / l), back(Tn / l + (w_p + gamma_l) * D), back(D)


def attention_exact(q, k, v, nh, scale):
    """exact float64 softmax attention of the unrounded operands and D = sum_j P_j |v_j|"""
    B, nq, C = q.shape
    qh, kh, vh = (t.double().view(B, -1, nh, 32).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    back = lambda t: t.transpose(1, 2).reshape(B, nq, C)                # noqa: E731
    return back(p @ vh), back(p @ vh.abs())


# ------------------------------------------------------------------ depth head (MODE 2)
def depth_hidden(head, feats):
    """The as-written module's hidden map in float64 and its denominator: up = F.interpolate(feats) (x32, bilinear),
    hidden = relu(bn(conv3x3(up))) [B,H,W,Cmid] NHWC, D_h = conv3x3(|up|, |w1 bn_scale|) + |shift1| (before the ReLU)."""
    h = head.depth_head
    B, hq, wq, _ = feats.shape
    up = F.interpolate(feats.double().permute(0, 3, 1, 2), size=(32 * hq, 32 * wq), mode="bilinear", align_corners=False)
    bn = h[1]
    sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    sh = (h[0].bias.double() - bn.running_mean.double()) * sc + bn.bias.double()
    w1 = h[0].weight.double() * sc.view(-1, 1, 1, 1)
    hid = torch.relu(F.conv2d(up, w1, None, 1, 1) + sh.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    den = (F.conv2d(up.abs(), w1.abs(), None, 1, 1) + sh.abs().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    return hid, den


def depth_bn2(head):
    """(scale, shift) of the second 3x3's BatchNorm fold, float64"""
    h = head.depth_head
    bn = h[5]
    sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return sc, (h[4].bias.double() - bn.running_mean.double()) * sc + bn.bias.double()


DEPTH_V_WINDOW = 80 * 2.0 ** -24             # generated against fetched hidden map, relative to |B^T| D_h |B|


def depth_model(head, feats, hidden, u_img, shift2, fused=True, window=DEPTH_V_WINDOW):
    """Model of the bf16 depth head on `hidden`, the float32 map the upconv kernel writes ([B,H,W,Cmid]), with the weight image
    and folded shift the module hands the kernel: (depth [B,H,W], T, D).  fused=False (two launches): the kernel fetches that
    map, T = 0.  fused=True (MODE 2): the kernel generates its own map, tie window `window` |B^T| D_h |B| on V."""
    h = head.depth_head
    kw = dict(w2=h[7].weight.double().view(-1), b2=h[7].bias.double())
    if not fused:
        return winograd_model(hidden.float(), u_img, 64, shift2.double(), **kw)
    _, den = depth_hidden(head, feats)
    return winograd_model(hidden.double(), u_img, 64, shift2.double(), v_window=window, x_den=den, **kw)


def depth_exact(head, feats):
    """exact float64 depth of the as-written module and D of the unrounded second-3x3 operands (|hidden| for the inputs)"""
    hid, _ = depth_hidden(head, feats)
    sc2, sh2 = depth_bn2(head)
    h = head.depth_head
    return winograd_exact(hid, h[4].weight.double(), sc2, sh2, w2=h[7].weight.double().view(-1), b2=h[7].bias.double())
