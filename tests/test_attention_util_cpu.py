"""The reference, the packers and the peaked inputs of the attention route tests (attention_util.py) hold what
test_attention_routes_gpu.py relies on.  No GPU."""
import pytest
import torch

import attention_util as au


@pytest.mark.parametrize("B,L,S,H,D", [(2, 37, 70, 5, 32), (3, 25, 25, 8, 16)])
def test_reference_equals_float64_autograd(B, L, S, H, D):
    q, k, v, d_o = (au.rnd(B, n, H * D, seed=s).double() for n, s in ((L, 1), (S, 2), (S, 3), (L, 4)))
    scale = D**-0.5
    o, nlse, dq, dk, dv = au.reference(q, k, v, d_o, H, scale)
    o_a, dq_a, dk_a, dv_a = au.autograd_grads(q, k, v, d_o, H, scale, torch.float64)
    for name, got, want in (("o", o, o_a), ("dq", dq, dq_a), ("dk", dk, dk_a), ("dv", dv, dv_a)):
        err = ((got - want).abs().max() / want.abs().max()).item()
        print(f"{name}: {err:.2e}")
        assert err < 1e-12, name
    # nlse against the definition, term by term
    s2 = torch.einsum("blhd,bshd->bhls", q.view(B, L, H, D), k.view(B, S, H, D)) * scale * au.LOG2E
    want = -torch.log2(torch.exp2(s2).sum(-1))
    assert nlse.shape == (B, H, L) and ((nlse - want).abs().max() / want.abs().max()).item() < 1e-12


@pytest.mark.parametrize("pad", au.PADS)
def test_packers_round_trip(pad):
    B, L, S, dim = 2, 5, 7, 24
    q, k, v = au.rnd(B, L, dim, seed=1), au.rnd(B, S, dim, seed=2), au.rnd(B, S, dim, seed=3)
    qb, kvb, (qc, kc, vc) = au.pack_cross(q, k, v, pad)
    assert qb.shape == (B * L, dim + 2 * pad) and kvb.shape == (B * S, 2 * dim + 3 * pad) and qb.dtype == kvb.dtype == torch.float32
    assert (qc, kc, vc) == (pad, pad, 2 * pad + dim) and all(c % 4 == 0 for c in (qc, kc, vc))
    assert torch.equal(qb[:, qc:qc + dim], q.reshape(-1, dim)) and torch.equal(kvb[:, kc:kc + dim], k.reshape(-1, dim))
    assert torch.equal(kvb[:, vc:vc + dim], v.reshape(-1, dim))
    assert torch.isnan(qb).sum() == B * L * 2 * pad and torch.isnan(kvb).sum() == B * S * 3 * pad
    k2, v2 = au.rnd(B, L, dim, seed=4), au.rnd(B, L, dim, seed=5)
    sb, cols = au.pack_self(q, k2, v2, pad)
    assert sb.shape == (B * L, 3 * dim + 4 * pad) and cols == (pad, 2 * pad + dim, 3 * pad + 2 * dim) and all(c % 4 == 0 for c in cols)
    for t, c in zip((q, k2, v2), cols):
        assert torch.equal(sb[:, c:c + dim], t.reshape(-1, dim))
    assert torch.isnan(sb).sum() == B * L * 4 * pad
    sb7, _ = au.pack_self(q, k2, v2, pad, poison=7.0)
    assert not torch.isnan(sb7).any() and (sb7 == 7.0).sum() >= B * L * 4 * pad


@pytest.mark.parametrize("case", au.PEAKED, ids=au.shape_id)
def test_peaked_inputs_are_peaked(case):
    B, L, S, H, D, where, gain = case
    q, k, v, d_o = au.peaked_inputs(B, L, S, H, D, where, gain, seed=11)
    for w, i in zip(where, range(len(where))):
        assert torch.equal(k[:, w], gain * q[:, au.peaked_l0(i, L)])
    s2 = au.scores_log2(q, k, H, D**-0.5)  # (B, H, L, S)
    p = torch.softmax(s2 * au.LN2, -1)
    flat = torch.ones(L, dtype=torch.bool)
    for i, w in enumerate(where):
        l0 = au.peaked_l0(i, L)
        flat[l0] = False
        p0 = p[:, :, l0, w].min().item()
        first = 32 * (w // 32)  # first key of the tile that holds the dominating key
        jump = (s2[:, :, l0, w] - s2[:, :, l0, :first].amax(-1)).min().item() if first else float("inf")
        print(f"key {w} -> query {l0}: probability >= {p0:.6f}, score {s2[:, :, l0, w].min():.1f} .. {s2[:, :, l0, w].max():.1f} (log2), "
              f"{jump:.1f} above every earlier tile")
        assert p0 >= 0.99
        # above the TRUE maximum of all earlier tiles by more than RAISE = 8, hence above the lazy running maximum (which is never
        # higher than the true one): pass 1 of the backward has to raise at this tile.  (A key in tile 0 sets the first maximum.)
        assert jump > 8.0
    pmax = p[:, :, flat].max().item()
    print(f"flat queries: largest probability {pmax:.3f}; largest |score| {s2.abs().max():.1f} (log2)")
    assert pmax < 0.5
    assert any(w >= 32 for w in where)


def test_very_negative_inputs_overflow_an_unmasked_key():
    B, L, S, H, D, l0, factor = au.VERY_NEGATIVE
    q, k, v, d_o = au.very_negative_inputs(B, L, S, H, D, l0, factor, seed=21)
    assert S % 32 != 0
    _, nlse, *_ = au.reference(q, k, v, d_o, H, D**-0.5)
    others = torch.arange(L) != l0
    print(f"-lse of query {l0}: {nlse[:, :, l0].min():.1f} .. {nlse[:, :, l0].max():.1f} (log2); of the others: |.| <= {nlse[:, :, others].abs().max():.1f}")
    assert nlse[:, :, l0].min() > 128.0  # 2^(-lse) is not an fp32 number
    assert nlse[:, :, others].abs().max() < 30.0
