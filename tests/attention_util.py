"""Reference, input builders and bounds shared by the attention route tests (test_attention_util_cpu.py, test_attention_routes_gpu.py).
Plain torch on the CPU, float64 where it computes; nothing here touches the GPU or the package."""

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rel(a, b, floor=1e-3):
    """max |a - b| relative to the largest reference entry (at least `floor`): the measure of test_train_gpu.py."""
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(floor)).item()


def _heads(t, heads):
    B, n, C = t.shape
    return t.double().view(B, n, heads, C // heads).transpose(1, 2)  # (B, H, n, D)


def _tokens(t):
    B, H, n, D = t.shape
    return t.transpose(1, 2).reshape(B, n, H * D)


def scores_log2(q, k, heads, scale):
    """(B, H, L, S) float64: scale log2(e) q.k, the scores as the kernels hold them."""
    return (_heads(q, heads) @ _heads(k, heads).transpose(-1, -2)) * (scale * LOG2E)


def reference(q, k, v, d_o, heads, scale):
    """q, d_o (B,L,C); k, v (B,S,C) -> o (B,L,C), nlse (B,heads,L), dq, dk, dv, all float64.
    nlse = -log2 sum_s exp2(scale log2e q.k).  Gradients by the formulas in the header of csrc/attention_bwd.hip, not by autograd:
        D_l = sum_c dO[l,c] O[l,c]   dP = dO V^T   dS = P o (dP - D)   dQ = scale dS K   dK = scale dS^T Q   dV = P^T dO"""
    qh, kh, vh, doh = (_heads(t, heads) for t in (q, k, v, d_o))
    s2 = scores_log2(q, k, heads, scale)
    nlse = -torch.logsumexp(s2 * LN2, -1) / LN2
    p = torch.exp2(s2 + nlse[..., None])
    oh = p @ vh
    dsum = (doh * oh).sum(-1, keepdim=True)
    ds = p * (doh @ vh.transpose(-1, -2) - dsum)
    dq, dk, dv = scale * (ds @ kh), scale * (ds.transpose(-1, -2) @ qh), p.transpose(-1, -2) @ doh
    return _tokens(oh), nlse, _tokens(dq), _tokens(dk), _tokens(dv)


def autograd_grads(q, k, v, d_o, heads, scale, dtype):
    """o, dq, dk, dv of the textbook einsum attention by torch.autograd in `dtype` (float64: the check of reference();
    float32: what plain fp32 arithmetic makes of the same inputs)."""
    B, L, C = q.shape
    S, D = k.shape[1], C // heads
    with torch.enable_grad():
        qq, kk, vv = (t.detach().to(dtype).clone().requires_grad_() for t in (q, k, v))
        sc = torch.einsum("blhd,bshd->blsh", qq.view(B, L, heads, D) * scale, kk.view(B, S, heads, D))
        o = torch.einsum("blsh,bshd->blhd", torch.softmax(sc, 2), vv.view(B, S, heads, D)).reshape(B, L, C)
        o.backward(d_o.to(dtype))
    return o.detach(), qq.grad, kk.grad, vv.grad


def _pack(rows, parts, pad_cols, poison):
    assert pad_cols % 4 == 0, "the kernels move 16-byte row pieces: every column offset is a multiple of 4 floats"
    width = sum(p.shape[-1] for p in parts) + (len(parts) + 1) * pad_cols
    buf = torch.full((rows, width), poison, dtype=torch.float32)
    cols, c = [], pad_cols
    for p in parts:
        w = p.shape[-1]
        buf[:, c:c + w] = p.reshape(rows, w)
        cols.append(c)
        c += w + pad_cols
    return buf, cols


def pack_self(q, k, v, pad_cols=0, poison=float("nan")):
    """[pad | q | pad | k | pad | v | pad] as ONE (B*L, 3 dim + 4 pad_cols) float32 buffer -> buffer, (q_col, k_col, v_col)."""
    assert q.shape == k.shape == v.shape
    buf, cols = _pack(q.shape[0] * q.shape[1], (q, k, v), pad_cols, poison)
    return buf, tuple(cols)


def pack_cross(q, k, v, pad_cols=0, poison=float("nan")):
    """[pad | q | pad] (B*L, dim + 2 pad_cols) beside [pad | k | pad | v | pad] (B*S, 2 dim + 3 pad_cols) -> q buffer, kv buffer,
    (q_col, k_col, v_col)."""
    qb, (qc,) = _pack(q.shape[0] * q.shape[1], (q,), pad_cols, poison)
    kvb, (kc, vc) = _pack(k.shape[0] * k.shape[1], (k, v), pad_cols, poison)
    return qb, kvb, (qc, kc, vc)


def peaked_l0(i, L):
    """The query that the i-th dominating key belongs to."""
    return (5 + 11 * i) % L


def peaked_inputs(B, L, S, H, D, where, gain, seed):
    """q, k, v, d_o ~ N(0,1) with k[b, where[i]] = gain * q[b, l0_i], l0_i = peaked_l0(i, L): that key dominates query l0_i in every
    head, wherever it sits among the key tiles.
    One step beyond the plain construction: in every head the l0 queries are made orthogonal to one another and every other query
    orthogonal to all of them.  Without it the planted key scores gain * q_l.q_l0 * scale ~ N(0, gain^2) against the OTHER queries
    (natural-log units; N(0,1) for an ordinary key), which over L * H draws makes some of them as peaked as l0 itself: the 'flat'
    queries would not be flat, and which rows exercise the raise of the running maximum would be an accident of the seed."""
    q, k, v, d_o = rnd(B, L, H * D, seed=seed), rnd(B, S, H * D, seed=seed + 1), rnd(B, S, H * D, seed=seed + 2), rnd(B, L, H * D, seed=seed + 3)
    l0 = [peaked_l0(i, L) for i in range(len(where))]
    assert len(set(l0)) == len(l0) and len(set(where)) == len(where) and max(where) < S
    qh = q.double().view(B, L, H, D)
    basis = []  # orthonormal, per (batch, head)
    for l in l0:
        u = qh[:, l].clone()
        for e in basis:
            u -= (u * e).sum(-1, keepdim=True) * e
        qh[:, l] = u
        basis.append(u / u.norm(dim=-1, keepdim=True))
    others = [l for l in range(L) if l not in l0]
    for e in basis:
        qo = qh[:, others]
        qh[:, others] = qo - (qo * e[:, None]).sum(-1, keepdim=True) * e[:, None]
    q = qh.reshape(B, L, H * D).float()
    for w, l in zip(where, l0):
        k[:, w] = gain * q[:, l]
    return q, k, v, d_o


def very_negative_inputs(B, L, S, H, D, l0, factor, seed):
    """q, k, v, d_o ~ N(0,1) with every key made non-negative (k = |k|) and q[b, l0] = -factor |q[b, l0]|: every score of query l0 is
    far below zero, so is its log-sum-exp, and 2^(-lse) -- the 'probability' of a key of score 0, which is what a zero-padded key
    past the end of a ragged tile has when nobody masks it -- lies beyond the fp32 range.  The other queries see ordinary scores."""
    q, k, v, d_o = rnd(B, L, H * D, seed=seed), rnd(B, S, H * D, seed=seed + 1).abs(), rnd(B, S, H * D, seed=seed + 2), rnd(B, L, H * D, seed=seed + 3)
    q[:, l0] = -factor * q[:, l0].abs()
    return q, k, v, d_o


def nlse_bound(q, k, scale, heads):
    """(B, heads, L) bound on |nlse - nlse_ref| of the split-bf16 forward kernel:
        4 ( 2^-16 max_s sum_d |q_ld k_sd| scale log2e  +  2^-22 (1 + |nlse_ref,l|) )
    first term: x = hi + lo in bf16 keeps 16 significand bits, and of the four hi / lo products the lo.lo one is dropped: <= 2^-16
    relative per product, and a log-sum-exp moves by at most the largest score error; second term: v_exp_f32, v_log_f32 and the
    fp32 row sum; the factor 4 covers the accumulation order."""
    mag = (_heads(q, heads).abs() @ _heads(k, heads).abs().transpose(-1, -2)).amax(-1) * (scale * LOG2E)
    s2 = scores_log2(q, k, heads, scale)
    nlse = -torch.logsumexp(s2 * LN2, -1) / LN2
    return 4.0 * (2.0 ** -16 * mag + 2.0 ** -22 * (1.0 + nlse.abs()))


def bwd_tol(precision, L, S, D):
    """The bound of test_attention_backward (test_train_gpu.py) on rel(., ref, 0.1), copied: 2e-5; 5e-5 for the window-sized head-dim-32
    shapes on the split-bf16 kernels; 5e-4 for a single key on them (dq is exactly 0 there)."""
    tol = 5e-4 if (S == 1 and precision == "bf16x3") else 2e-5
    if precision == "bf16x3" and D == 32 and 1 < S <= 65 and L <= 65:
        tol = 5e-5
    return tol


def peaked_tols(e32, max_score_log2):
    """Item by item from the float32-autograd error e32 = rel(., ref, 0.1) of the same gradients: fp32 kernels max(2e-5, 4 e32) (4: the
    tile-wise summation order); split-bf16 kernels max(5e-5, 4 e32 + 4 ln2 2^-16 max|score_log2|) (the dropped lo.lo terms of the score
    reaching P = exp2(score - lse))."""
    return {"fp32": max(2e-5, 4 * e32), "bf16x3": max(5e-5, 4 * e32 + 4 * LN2 * 2.0 ** -16 * max_score_log2)}


# ------------------------------------------------------------------------------------------------------------ the cases
# (B, L, S, H) at head dim 32: 1 / 2 / 3 / 4+ key tiles, ragged last tiles on both axes, more than one 128-query workgroup,
# B H mod 8 in {0, 1, 2, 4, 5}
TILED = [(1, 65, 32, 8),    # one key tile, first non-small L
         (1, 1, 65, 5),     # single query, ragged S, B H = 5
         (3, 70, 33, 3),    # B H = 9, ragged second key tile
         (2, 129, 96, 8),   # two workgroups, exactly three tiles
         (1, 127, 97, 1),   # B H = 1, ragged fourth tile
         (2, 100, 160, 5),  # five tiles, B H = 10
         (1, 385, 127, 4),  # four query blocks, B H = 4
         (2, 70, 70, 5)]    # L == S: the only tiled shape that can go through pack_self ([q | k | v] in one buffer)
SMALL = [(7, 25, 25, 8, 16), (2, 64, 49, 8, 16), (3, 49, 64, 3, 32), (1, 9, 9, 5, 16)]
SHAPES = [s + (32,) for s in TILED] + SMALL
PADS = (0, 4, 36)

# (B, L, S, H, D, where, gain): dominating keys in the first, a middle and the last (ragged) key tile
PEAKED = [(1, 70, 160, 8, 32, (3, 70, 159), 6.0),
          (2, 129, 97, 5, 32, (96,), 6.0),
          (2, 49, 64, 5, 16, (40,), 8.0)]


# (B, L, S, H, D, l0, factor): ragged last key tile, B H = 10
VERY_NEGATIVE = (2, 70, 97, 5, 32, 5, 60.0)


def shape_id(s):
    return "x".join(str(x) for x in s[:5])
