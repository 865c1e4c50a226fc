"""Yardsticks of the chained encoder kernels' stage tests (test_chain_kernel_util_cpu.py, test_encoder_tail_stages_gpu.py,
test_fine_layer_stages_gpu.py): float64 references of the encoder tail (csrc/encoder_tail.hip, encoder_tail_bwd.hip) and of the fine window
layer (csrc/fine_layer.hip), a model of their split-bf16 arithmetic, the designed inputs and the parameter holders.

Plain torch on the CPU (or on whatever device the inputs live on); nothing here launches a kernel, and nothing touches a GPU at import.

    tail forward:   a = xh + att . Wo^T;   u = W1 . LN2(a) + b1;   y = xh + W2 . gelu(u) + b2
    tail backward:  g1 = dy . W2;  du = g1 o gelu'(u);  g2 = du . W1;  d_a = LN2'(a; g2);  d_xh = dy + d_a;  d_att = d_a . Wo

THE BAR of every comparison that is not exact by construction:  |code - fp64| <= 4 E_model + 2^-20 max|fp64|  (model_bar), with
E_model = max|model - fp64| on the test's own inputs.  The model splits every operand as the kernels do (x~ = hi + lo, hi = bf16(x),
lo = bf16(x - hi); a product is w_hi x_hi + w_hi x_lo + w_lo x_hi), rounds every stage output the kernels hold in fp32 to fp32, but
accumulates in float64 and evaluates exp, 1/x and sqrt exactly.  The kernels accumulate up to 256 fp32 terms per product and use the
hardware's approximations: hence the margin of 4 and the floor of 2^-20 of the largest entry."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

# the probe column of test_linear_family_gpu.test_gelu_routes_at_probe_values: zeros of both signs, the linear range, the tails where
# 1 + erf cancels, arguments far outside any erf table
PROBES = (0.0, -0.0, 1e-8, -1e-8, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0, 1e4)
EPS_VALUES = (1e-5, 1e-3, 1e-6)
FLOOR = 2.0**-20
CARRY = 2.0**-16  # what x = hi + lo in bf16 leaves of an operand (the split-carry bar of test_gelu_routes_at_probe_values: 1e-6 + 2^-16 |value|)


def probe_row(dim, shift=0):
    """The probes tiled to `dim` columns, rotated by `shift` (so that rows of one test put different probes into one column)."""
    n = len(PROBES)
    return torch.tensor([PROBES[(i + shift) % n] for i in range(dim)], dtype=torch.float32)


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ----------------------------------------------------------------------------------------------- GELU
def gelu64(u):
    u = u.double()
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad64(u):
    u = u.double()
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


AS_7_1_26 = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)  # a1 .. a5 of Abramowitz & Stegun 7.1.26 (p = 0.3275911)


def _as_tail(v, coef):
    """(p t, exp(-v^2 / 2)) of gelu_erf / gelu_grad in plain fp32: erf(x) = 1 - (a1 t + ... + a5 t^5) exp(-x^2), t = 1 / (1 + p x)."""
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    x = v.abs() * f(0.70710678118654752440)
    t = 1.0 / (f(0.3275911) * x + 1.0)
    p = f(coef[4]) * t + f(coef[3])
    p = p * t + f(coef[2])
    p = p * t + f(coef[1])
    p = p * t + f(coef[0])
    return p * t, torch.exp2(-(x * x) * f(1.44269504088896340736))


def gelu_erf_f32(v, coef=AS_7_1_26):
    """gelu_erf of csrc/bf16x3.h, statement by statement, in torch float32 (the tail forwards and the fine layer use it)."""
    assert v.dtype == torch.float32
    pt, ex = _as_tail(v, coef)
    e = 1.0 - pt * ex
    return 0.5 * v * (1.0 + torch.copysign(e, v))


def gelu_grad_f32(v, coef=AS_7_1_26):
    """gelu_grad of csrc/encoder_tail_bwd.hip in torch float32: Phi(v) + v phi(v), the same polynomial plus the Gaussian term."""
    assert v.dtype == torch.float32
    pt, ex = _as_tail(v, coef)
    e = 1.0 - pt * ex
    return v * torch.tensor(0.39894228040143267794, dtype=torch.float32) * ex + 0.5 * (1.0 + torch.copysign(e, v))


# ----------------------------------------------------------------------------------------------- LayerNorm
def ln64(x, g, b, eps):
    x = x.double()
    xc = x - x.mean(-1, keepdim=True)
    return xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps) * g.double() + b.double()


def ln_bwd64(a, g2, gamma, eps):
    """d_a = rstd (g - mean(g) - xhat mean(g xhat)),  g = g2 gamma,  xhat = (a - mean) rstd  (the closed form in encoder_tail_bwd.hip)."""
    a, g = a.double(), g2.double() * gamma.double()
    xc = a - a.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xh = xc * rstd
    return rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))


def ln_two_pass_f32(x, eps):
    """Normalised rows by the kernels' form in SEQUENTIAL fp32: mean, then the centred sum of squares."""
    x = x.float()
    s = torch.zeros(x.shape[0], dtype=torch.float32)
    for j in range(x.shape[1]):
        s = s + x[:, j]
    mean = s * torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
    d = x - mean[:, None]
    vs = torch.zeros_like(s)
    for j in range(x.shape[1]):
        vs = vs + d[:, j] * d[:, j]
    return d * (1.0 / torch.sqrt(vs * torch.tensor(1.0 / x.shape[1], dtype=torch.float32) + torch.tensor(eps, dtype=torch.float32)))[:, None]


def ln_one_pass_f32(x, eps):
    """The form the kernels must NOT use: variance as E[x^2] - mean^2 in sequential fp32."""
    x = x.float()
    s, ss = torch.zeros(x.shape[0], dtype=torch.float32), torch.zeros(x.shape[0], dtype=torch.float32)
    for j in range(x.shape[1]):
        s = s + x[:, j]
        ss = ss + x[:, j] * x[:, j]
    inv = torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
    mean = s * inv
    var = ss * inv - mean * mean
    return (x - mean[:, None]) * (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32)))[:, None]


# ----------------------------------------------------------------------------------------------- designed inputs
def exact_offset_rows(n, dim, offset=1024, seed=0):
    """Rows offset + s_i with every s_i a multiple of 1/4 in [-4, 4] and sum s_i = 0: all partial sums of the row (< 2^19, two fraction
    bits) and of the centred squares (multiples of 1/16, < 2^12) are fp32 numbers, so mean and centred sum of squares are exact in fp32 in
    ANY summation order -- while E[x^2] - mean^2 cancels 2^20 against a variance of a few units."""
    assert dim % 2 == 0
    g = torch.Generator().manual_seed(seed)
    half = torch.randint(-16, 17, (n, dim // 2), generator=g)
    s = torch.cat([half, -half], 1)
    perm = torch.stack([torch.randperm(dim, generator=g) for _ in range(n)])
    return (offset + torch.gather(s, 1, perm).double() / 4.0).float()


def constant_rows(n, dim, value=2.5):
    return torch.full((n, dim), value, dtype=torch.float32)


def negligible_variance_rows(n, dim, seed=0):
    """1e-3 N(0, 1): variance 1e-6, below every eps the tests use -- rstd is eps's."""
    return rnd(n, dim, seed=seed, scale=1e-3)


def large_rows(n, dim, seed=0):
    return rnd(n, dim, seed=seed, scale=50.0)


KINDS = ("offset", "constant", "negligible", "large", "benign")


def designed_rows(dim, per_kind=4, seed=0):
    """(rows, {kind: slice}): per_kind rows of every kind in KINDS, stacked in that order."""
    parts = [exact_offset_rows(per_kind, dim, seed=seed), constant_rows(per_kind, dim), negligible_variance_rows(per_kind, dim, seed=seed + 1),
             large_rows(per_kind, dim, seed=seed + 2), rnd(per_kind, dim, seed=seed + 3)]
    return torch.cat(parts), {k: slice(i * per_kind, (i + 1) * per_kind) for i, k in enumerate(KINDS)}


# ----------------------------------------------------------------------------------------------- the split arithmetic
def split2(x):
    """(hi, lo) of x~ = hi + lo, hi = bf16(x), lo = bf16(x - hi), as float64 (for an fp32 x: the kernels' bits; x - hi is exact in fp32)."""
    x = x.double()
    hi = x.float().bfloat16().double()
    return hi, (x - hi).float().bfloat16().double()


def split3(x):
    """(h, m, l) of the fine layer's score operands: three bf16 terms."""
    x = x.double()
    h = x.float().bfloat16().double()
    r1 = x - h
    m = r1.float().bfloat16().double()
    return h, m, (r1 - m).float().bfloat16().double()


def carry(x):
    """hi + lo of an fp32 tensor, in fp32: what an identity weight hands on of an operand."""
    hi, lo = split2(x)
    return (hi + lo).float()


def sprod(x, w):
    """x . w^T in the split arithmetic (w stored (N, K) like nn.Linear), accumulated in float64."""
    xh, xl = split2(x)
    wh, wl = split2(w)
    return xh @ wh.T + xl @ wh.T + xh @ wl.T


def r32(t, on=True):
    return t.float().double() if on else t


def model_bar(e_model, ref):
    return 4.0 * e_model + FLOOR * ref.abs().max().item()


def maxerr(a, ref):
    return (a.detach().cpu().double() - ref.detach().cpu().double()).abs().max().item()


# ----------------------------------------------------------------------------------------------- encoder tail: parameters
def _holder(wo, gamma, beta, eps, w1, b1, w2, b2):
    f = lambda t: t.float().contiguous()
    return SimpleNamespace(wo=f(wo), norm2=SimpleNamespace(weight=f(gamma), bias=f(beta), eps=eps), ffn0=SimpleNamespace(weight=f(w1), bias=f(b1)),
                           ffn2=SimpleNamespace(weight=f(w2), bias=f(b2)))


def tail_params(kind="synth", eps=1e-5, seed=3, dim=256, **over):
    """The objects ops.encoder_tail* take: .wo, .norm2 (weight, bias, eps), .ffn0 / .ffn2 (weight, bias).  kind "synth": the weights of
    synth._encoder_layer; "identity": Wo = W1 = W2 = I, zero biases, random gamma / beta.  Keyword overrides: wo, gamma, beta, w1, b1, w2, b2."""
    from nerfmatch_amd import synth

    sd = {}
    synth._encoder_layer(sd, np.random.default_rng(seed), "L", dim)
    p = dict(wo=sd["L.attention.proj_out.0.weight"], gamma=sd["L.norm2.weight"], beta=sd["L.norm2.bias"], w1=sd["L.feedforward.layers.0.weight"],
             b1=sd["L.feedforward.layers.0.bias"], w2=sd["L.feedforward.layers.2.weight"], b2=sd["L.feedforward.layers.2.bias"])
    if kind == "identity":
        p.update(wo=torch.eye(dim), w1=torch.eye(dim), w2=torch.eye(dim), b1=torch.zeros(dim), b2=torch.zeros(dim))
    elif kind != "synth":
        raise ValueError(kind)
    p.update(over)
    return _holder(p["wo"], p["gamma"], p["beta"], eps, p["w1"], p["b1"], p["w2"], p["b2"])


def tail_to(p, device, eps=None):
    """The holder on `device` (the same tensors when eps is all that changes: the packed-weight cache finds them again)."""
    m = lambda t: t.to(device)
    return SimpleNamespace(wo=m(p.wo), norm2=SimpleNamespace(weight=m(p.norm2.weight), bias=m(p.norm2.bias), eps=p.norm2.eps if eps is None else eps),
                           ffn0=SimpleNamespace(weight=m(p.ffn0.weight), bias=m(p.ffn0.bias)), ffn2=SimpleNamespace(weight=m(p.ffn2.weight), bias=m(p.ffn2.bias)))


def with_eps(p, eps):
    return SimpleNamespace(wo=p.wo, norm2=SimpleNamespace(weight=p.norm2.weight, bias=p.norm2.bias, eps=eps), ffn0=p.ffn0, ffn2=p.ffn2)


def tail_args(p):
    return p.wo, p.norm2, p.ffn0, p.ffn2


# ----------------------------------------------------------------------------------------------- encoder tail: fp64 and model
def tail_fp64(att, xh, params, eps):
    """(a, u, y) in float64 from the fp32 inputs."""
    d = lambda t: t.detach().cpu().double() if not t.requires_grad else t
    a = d(xh) + d(att) @ d(params.wo).T
    u = ln64(a, d(params.norm2.weight), d(params.norm2.bias), eps) @ d(params.ffn0.weight).T + d(params.ffn0.bias)
    y = d(xh) + gelu64(u) @ d(params.ffn2.weight).T + d(params.ffn2.bias)
    return a, u, y


def tail_bwd_fp64(dy, a_pre, u_pre, params, eps):
    """(d_att, d_xh) in float64, closed form (the header of csrc/encoder_tail_bwd.hip), from a_pre / u_pre as given."""
    d = lambda t: t.detach().cpu().double()
    g1 = d(dy) @ d(params.ffn2.weight)
    g2 = (g1 * gelu_grad64(d(u_pre))) @ d(params.ffn0.weight)
    d_a = ln_bwd64(d(a_pre), g2, d(params.norm2.weight), eps)
    return d_a @ d(params.wo), d(dy) + d_a


def tail_bwd_autograd(dy, att, xh, params, eps):
    """(d_att, d_xh) by torch autograd through tail_fp64."""
    att, xh = att.double().requires_grad_(True), xh.double().requires_grad_(True)
    with torch.enable_grad():
        _, _, y = tail_fp64(att, xh, params, eps)
        (y * dy.double()).sum().backward()
    return att.grad, xh.grad


def tail_model(att, xh, params, eps, round_stages=True):
    """(a, u, y) of the split-arithmetic model; round_stages=False leaves the stage outputs in float64 (what the fp32 registers cost)."""
    r = lambda t: r32(t, round_stages)
    x64 = xh.double()
    a = r(x64 + sprod(att, params.wo))
    n = r(ln64(a, params.norm2.weight, params.norm2.bias, eps))
    u = r(sprod(n, params.ffn0.weight) + params.ffn0.bias.double())
    h = r(gelu64(u))
    y = r(x64 + sprod(h, params.ffn2.weight) + params.ffn2.bias.double())
    return a, u, y


def tail_bwd_model(dy, a_pre, u_pre, params, eps, round_stages=True):
    """(d_att, d_xh) of the split-arithmetic model: d_xh adds the fp32 d_a, d_att multiplies its split."""
    r = lambda t: r32(t, round_stages)
    g1 = r(sprod(dy, params.ffn2.weight.T))
    du = r(g1 * r(gelu_grad64(u_pre)))
    g2 = r(sprod(du, params.ffn0.weight.T))
    d_a = r(ln_bwd64(a_pre, g2, params.norm2.weight, eps))
    return r(sprod(d_a, params.wo.T)), r(dy.double() + d_a)


# ----------------------------------------------------------------------------------------------- fine window layer
FINE_KEYS = ("ln1_g", "ln1_b", "wq", "wk", "wv", "wo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2")


def fine_block(kind="synth", seed=5, eps1=1e-5, eps2=1e-5, **over):
    """A SelfAttentionBlock of the fine stage's shape (one pre-norm layer, width 128, 8 heads of 16) with the weights of
    synth._encoder_layer ("synth"), or Wq .. W2 = I and zero biases ("identity").  Overrides by FINE_KEYS.  A fresh module every call: the
    one-launch path keeps its packed weights on the module."""
    from nerfmatch_amd import synth
    from nerfmatch_amd.modules.attention import SelfAttentionBlock

    sd = {}
    synth._encoder_layer(sd, np.random.default_rng(seed), "layers.0", 128)
    names = dict(ln1_g="norm1.0.weight", ln1_b="norm1.0.bias", wq="attention.proj_q.weight", wk="attention.proj_k.weight", wv="attention.proj_v.weight",
                 wo="attention.proj_out.0.weight", ln2_g="norm2.weight", ln2_b="norm2.bias", w1="feedforward.layers.0.weight",
                 b1="feedforward.layers.0.bias", w2="feedforward.layers.2.weight", b2="feedforward.layers.2.bias")
    if kind == "identity":
        for k in ("wq", "wk", "wv", "wo", "w1", "w2"):
            sd[f"layers.0.{names[k]}"] = torch.eye(128)
        for k in ("b1", "b2"):
            sd[f"layers.0.{names[k]}"] = torch.zeros(128)
    elif kind != "synth":
        raise ValueError(kind)
    for k, v in over.items():
        sd[f"layers.0.{names[k]}"] = v.float().clone()
    block = SelfAttentionBlock(1, 128, att_type="full", head_dim=16)
    block.load_state_dict(sd, strict=True)
    block.layers[0].norm1[0].eps, block.layers[0].norm2.eps = eps1, eps2
    for p in block.parameters():
        p.requires_grad_(False)
    return block.eval()


def offset_score_block(level=32.0, seed=5):
    """A fine block whose scores all sit near 0.25 level^2 (256) without being decided: input channel 0 leaves LN1 as the constant
    `level` (gamma 0, beta level), reaches no other q / k dim (column 0 of Wq, Wk zeroed) and is added to dim 0 of every head's q and k.
    s_ij = 0.25 (level + q0_i)(level + k0_j) + ...: the keys differ by 0.25 level k0_j, a few units, and a two-term split of
    k0 ~ level (2^-17 level) times q0 ~ level puts ~1e-3 into the exponent, differently for every key.  Wo = W1 = W2 = I and zero
    biases hand the attention's output on at unit gain."""
    base = fine_block("synth", seed=seed)
    l = base.layers[0]
    g1, b1 = l.norm1[0].weight.clone(), l.norm1[0].bias.clone()
    g1[0], b1[0] = 0.0, level
    wq, wk = l.attention.proj_q.weight.clone(), l.attention.proj_k.weight.clone()
    for w in (wq, wk):
        w[:, 0] = 0.0
        w[0::16, 0] = 1.0
    z, eye = torch.zeros(128), torch.eye(128)
    return fine_block("synth", seed=seed, ln1_g=g1, ln1_b=b1, wq=wq, wk=wk, wo=eye, w1=eye, w2=eye, b1=z, b2=z)


def gather_windows(ffeat, map_ids, i_ids, stride=4):
    """(K, 25, C): the 5 x 5 window (zero padded by 2) around cell i of map b, tokens in row-major order (FinePreprocess's unfold)."""
    B, C, Hf, Wf = ffeat.shape
    cells_w = (Wf + 4 - 5) // stride + 1
    pad = torch.nn.functional.pad(ffeat, (2, 2, 2, 2))
    out = []
    for b, i in zip(map_ids.tolist(), i_ids.tolist()):
        y0, x0 = (i // cells_w) * stride, (i % cells_w) * stride  # (padded coordinates of the window's first pixel)
        out.append(pad[b, :, y0:y0 + 5, x0:x0 + 5].reshape(C, 25).T)
    return torch.stack(out)


def _fine_parts(block):
    l = block.layers[0]
    at, ff = l.attention, l.feedforward
    return l, at, ff, float(at.attend.scale())


def fine_layer_fp64(win, block):
    """y of the fine self-attention layer on windows (n, 25, 128), in float64 with torch ops, on the device of `win`."""
    n = win.shape[0]
    l, at, ff, scale = _fine_parts(block)
    W = lambda t: t.detach().to(win.device).double()
    x = win.double()
    ln = lambda t, m: torch.nn.functional.layer_norm(t, (128,), W(m.weight), W(m.bias), m.eps)
    xh = ln(x, l.norm1[0])
    q, k_, v = (xh @ W(w.weight).T for w in (at.proj_q, at.proj_k, at.proj_v))
    sp = lambda t: t.reshape(n, 25, 8, 16).transpose(1, 2)
    att = torch.softmax(sp(q) @ sp(k_).transpose(-1, -2) * scale, -1) @ sp(v)
    a_ = xh + att.transpose(1, 2).reshape(n, 25, 128) @ W(at.proj_out[0].weight).T
    h1 = torch.nn.functional.gelu(ln(a_, l.norm2) @ W(ff.layers[0].weight).T + W(ff.layers[0].bias))
    return xh + h1 @ W(ff.layers[2].weight).T + W(ff.layers[2].bias)


def fine_scores_fp64(win, block):
    """The scaled scores (n, 8, 25 queries, 25 keys) of the float64 reference."""
    n = win.shape[0]
    l, at, _, scale = _fine_parts(block)
    W = lambda t: t.detach().cpu().double()
    xh = ln64(win.cpu(), W(l.norm1[0].weight), W(l.norm1[0].bias), l.norm1[0].eps)
    sp = lambda t: t.reshape(n, 25, 8, 16).transpose(1, 2)
    return sp(xh @ W(at.proj_q.weight).T) @ sp(xh @ W(at.proj_k.weight).T).transpose(-1, -2) * scale


def fine_layer_model(win, block, score_terms=3):
    """y of the fine layer in the split-arithmetic model (CPU).  Scores: q and k in THREE bf16 terms, the six products the kernel issues
    (k_l q_h, k_h q_l, k_m q_m, k_m q_h, k_h q_m, k_h q_h; the three smallest are dropped); probabilities and values in two terms.
    score_terms=2: the split of every other product for the scores too -- what the kernel must NOT do (test_chain_kernel_util_cpu.py)."""
    n = win.shape[0]
    l, at, ff, scale = _fine_parts(block)
    W = lambda t: t.detach().cpu()
    xh = r32(ln64(win.cpu(), W(l.norm1[0].weight), W(l.norm1[0].bias), l.norm1[0].eps))
    q, k_, v = (r32(sprod(xh, W(w.weight))) for w in (at.proj_q, at.proj_k, at.proj_v))
    sp = lambda t: t.reshape(n, 25, 8, 16).transpose(1, 2)
    (qh, qm, ql), (kh, km, kl) = split3(sp(q)), split3(sp(k_))
    T = lambda t: t.transpose(-1, -2)
    if score_terms == 3:
        s = r32(qh @ T(kl) + ql @ T(kh) + qm @ T(km) + qh @ T(km) + qm @ T(kh) + qh @ T(kh))
    else:
        s = r32(qh @ T(km) + qm @ T(kh) + qh @ T(kh))
    s = r32(s * float(np.float32(scale)))
    p = r32(torch.exp(r32(s - s.max(-1, keepdim=True).values)))
    (ph, pl), (vh, vl) = split2(p), split2(sp(v))
    o = r32(r32(pl @ vh + ph @ vl + ph @ vh) / r32(p.sum(-1, keepdim=True)))
    a_ = r32(xh + sprod(o.transpose(1, 2).reshape(n, 25, 128), W(at.proj_out[0].weight)))
    a_n = r32(ln64(a_, W(l.norm2.weight), W(l.norm2.bias), l.norm2.eps))
    h1 = r32(gelu64(r32(sprod(a_n, W(ff.layers[0].weight)) + W(ff.layers[0].bias).double())))
    return r32(r32(sprod(h1, W(ff.layers[2].weight)) + W(ff.layers[2].bias).double()) + xh)


def fine_expectation_fp64(pt_f, y):
    """(E[x], E[y], std) of FineMatching in float64: soft-max of <pt_f, y[j]> / sqrt(C) over the 25 window positions, expectation over the
    normalised 5 x 5 grid, std = sum over the axes of sqrt(max(var, 1e-10)) -- the reference's clamp."""
    pt_f, y = pt_f.double(), y.double()
    p = torch.softmax((pt_f[:, None] * y).sum(-1) / math.sqrt(y.shape[-1]), -1)
    grid = torch.linspace(-1, 1, 5, dtype=torch.float64, device=y.device)
    gx, gy = grid.repeat(5), grid.repeat_interleave(5)
    ex, ey = (p * gx).sum(-1), (p * gy).sum(-1)
    vx, vy = (p * gx * gx).sum(-1) - ex * ex, (p * gy * gy).sum(-1) - ey * ey
    return ex, ey, torch.sqrt(vx.clamp_min(1e-10)) + torch.sqrt(vy.clamp_min(1e-10))


@functools.lru_cache(maxsize=None)
def benign_tail_case(rows=257, seed=1):
    """(att, xh, dy) N(0, 1) rows shared by the row-count and placement tests; a launch of R rows takes the first R."""
    return rnd(rows, 256, seed=seed), rnd(rows, 256, seed=seed + 1, scale=1.3), rnd(rows, 256, seed=seed + 2)
