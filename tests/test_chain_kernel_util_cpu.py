"""The yardsticks of the chained encoder kernels' stage tests, tested themselves (no GPU): the designed LayerNorm rows discriminate, the
fp32 statement of the kernels' GELU polynomial is inside the probe bar while one moved coefficient is outside it, the split-arithmetic
model behaves as tests/chain_kernel_util.py says, and the closed-form backward is autograd's."""
import pytest
import torch

import chain_kernel_util as ck


def _grid():
    return torch.cat([ck.probe_row(len(ck.PROBES)), torch.linspace(-12.0, 12.0, 48001)])


def test_exact_offset_rows_are_what_they_claim():
    x = ck.exact_offset_rows(16, 256)
    s = (x.double() - 1024.0) * 4.0
    assert torch.equal(s, s.round()) and s.abs().max().item() <= 16 and bool((s.sum(-1) == 0).all())
    assert bool((x.double().mean(-1).abs() / x.double().std(-1, unbiased=False) > 100).all())
    # exact in fp32 in any order: forwards, backwards and pairwise give the float64 sums
    for order in (torch.arange(256), torch.arange(255, -1, -1), torch.randperm(256, generator=torch.Generator().manual_seed(0))):
        acc = torch.zeros(16)
        for j in order.tolist():
            acc = acc + x[:, j]
        assert torch.equal(acc.double(), x.double().sum(-1))
    assert torch.equal(x.sum(-1).double(), x.double().sum(-1))


@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("eps", ck.EPS_VALUES)
def test_exact_offset_rows_discriminate_the_variance_formula(dim, eps):
    x = ck.exact_offset_rows(32, dim, seed=dim)
    want = ck.ln64(x, torch.ones(dim), torch.zeros(dim), eps)
    two, one = ck.ln_two_pass_f32(x, eps), ck.ln_one_pass_f32(x, eps)
    e2 = (two.double() - want).abs().max().item()
    e1 = (one.double() - want).abs().max().item()  # (NaN when the cancelled variance comes out negative: also "more than 1e-3 off")
    print(f"dim {dim} eps {eps:g}: two-pass fp32 {e2:.2e}, one-pass fp32 {e1:.2e} from float64")
    assert e2 <= 2e-7 * want.abs().max().item()
    assert not e1 <= 1e-3


def test_fp32_statement_of_the_chained_gelu_is_inside_the_probe_bar():
    u = _grid()
    e_f, e_g = (ck.gelu_erf_f32(u).double() - ck.gelu64(u)).abs(), (ck.gelu_grad_f32(u).double() - ck.gelu_grad64(u)).abs()
    i, j = int(e_f.argmax()), int(e_g.argmax())
    print(f"gelu_erf fp32 statement: max err {e_f.max().item():.2e} at u = {u[i].item():g}; gelu_grad: {e_g.max().item():.2e} at u = {u[j].item():g}")
    assert e_f.max().item() <= 1e-6 and e_g.max().item() <= 1e-6


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_moved_coefficient_is_outside_the_probe_bar(which, sign):
    coef = list(ck.AS_7_1_26)
    coef[which] += sign * 1e-4
    u = ck.probe_row(len(ck.PROBES))
    e_f, e_g = (ck.gelu_erf_f32(u, coef).double() - ck.gelu64(u)).abs(), (ck.gelu_grad_f32(u, coef).double() - ck.gelu_grad64(u)).abs()
    assert bool((e_f > 1e-6 + ck.CARRY * ck.gelu64(u).abs()).any()), e_f.max().item()
    assert bool((e_g > 1e-6 + ck.CARRY * ck.gelu_grad64(u).abs()).any()), e_g.max().item()


def test_split_helpers():
    x = torch.cat([ck.rnd(4096, seed=1), ck.probe_row(15), ck.rnd(64, seed=2, scale=1e4)])
    hi, lo = ck.split2(x)
    assert bool(((hi + lo - x.double()).abs() <= ck.CARRY * x.double().abs()).all())
    h, m, l = ck.split3(x)
    assert bool(((h + m + l - x.double()).abs() <= 2.0**-23 * x.double().abs()).all())
    assert torch.equal(ck.carry(x).double(), hi + lo)
    w = ck.rnd(8, 32, seed=3)
    assert (ck.sprod(x[:64].reshape(2, 32), w) - x[:64].reshape(2, 32).double() @ w.double().T).abs().max().item() < 1e-3


def test_tail_model_on_benign_rows():
    att, xh, dy = (t[:128] for t in ck.benign_tail_case())
    p = ck.tail_params("synth")
    ref, mod = ck.tail_fp64(att, xh, p, 1e-5), ck.tail_model(att, xh, p, 1e-5)
    e = [ck.maxerr(m, r) for m, r in zip(mod, ref)]
    print("tail E_model benign 128 x 256 (a, u, y): " + ", ".join(f"{v:.2e}" for v in e))
    assert all(0.0 < v < 2e-5 for v in e)
    a, u, _ = ref
    rb, mb = ck.tail_bwd_fp64(dy, a.float(), u.float(), p, 1e-5), ck.tail_bwd_model(dy, a.float(), u.float(), p, 1e-5)
    eb = [ck.maxerr(m, r) / r.abs().max().item() for m, r in zip(mb, rb)]
    print("tail backward E_model / scale (d_att, d_xh): " + ", ".join(f"{v:.2e}" for v in eb))
    assert all(0.0 < v < 2e-5 for v in eb)


def test_stage_rounding_shows_on_offset_rows():
    """On rows of 1024 + s_i with a non-zero att . Wo^T the fp32 register that holds `a` keeps 2^-14 of it: the model with the stage
    rounding differs from the one without, and the rounding of `a` alone carries the difference (the inherent part)."""
    xh, att = ck.exact_offset_rows(32, 256), ck.rnd(32, 256, seed=7)
    p = ck.tail_params("synth")
    with_r, without = ck.tail_model(att, xh, p, 1e-5), ck.tail_model(att, xh, p, 1e-5, round_stages=False)
    d_u = ck.maxerr(with_r[1], without[1])
    # only a rounded: the model without rounding, started from the fp32 a
    a32 = with_r[0].float()
    only_a = ck.tail_model(torch.zeros_like(att), a32, p, 1e-5, round_stages=False)[1]
    d_a_only = ck.maxerr(only_a, without[1])
    e_round = ck.maxerr(with_r[1], ck.tail_fp64(att, xh, p, 1e-5)[1])
    print(f"offset rows: u with / without stage rounding differ by {d_u:.2e}; rounding a alone {d_a_only:.2e}; E_model(u) {e_round:.2e}")
    assert d_u > 1e-5 and d_a_only > 0.5 * d_u


@pytest.mark.parametrize("kind", ["synth", "identity"])
@pytest.mark.parametrize("eps", ck.EPS_VALUES)
def test_closed_form_backward_is_autograd(kind, eps):
    att, xh, dy = (t[:24] for t in ck.benign_tail_case())
    rows, _ = ck.designed_rows(256, per_kind=4)
    xh = torch.cat([xh, rows])
    att = torch.cat([att, ck.rnd(rows.shape[0], 256, seed=9)])
    dy = torch.cat([dy, ck.rnd(rows.shape[0], 256, seed=10)])
    p = ck.tail_params(kind, eps=eps)
    a, u, _ = ck.tail_fp64(att, xh, p, eps)
    d_att, d_xh = ck.tail_bwd_autograd(dy, att, xh, p, eps)
    # (a and u in float64: the closed form is handed what autograd sees)
    g1 = dy.double() @ p.ffn2.weight.double()
    g2 = (g1 * ck.gelu_grad64(u)) @ p.ffn0.weight.double()
    d_a = ck.ln_bwd64(a, g2, p.norm2.weight, eps)
    for got, want in ((d_a @ p.wo.double(), d_att), (dy.double() + d_a, d_xh)):
        for r in range(want.shape[0]):  # (row by row: the constant and negligible-variance rows are 1 / sqrt(eps) larger)
            assert (got[r] - want[r]).abs().max().item() <= 1e-11 * max(1.0, want[r].abs().max().item())
    # and through the helper, from fp32 copies of a and u: within what their rounding moves
    f_att, f_xh = ck.tail_bwd_fp64(dy, a.float(), u.float(), p, eps)
    assert ck.maxerr(f_att, d_att) <= 1e-4 * d_att.abs().max().item() and ck.maxerr(f_xh, d_xh) <= 1e-4 * d_xh.abs().max().item()


def test_fine_references_agree_with_each_other():
    g = torch.Generator().manual_seed(4)
    ffeat = torch.randn(2, 128, 24, 32, generator=g)
    map_ids, i_ids = torch.tensor([0, 1, 1, 0, 0, 1, 0, 1]), torch.tensor([0, 7, 47, 19, 9, 10, 27, 38])
    win = ck.gather_windows(ffeat, map_ids, i_ids)
    assert win.shape == (8, 25, 128)
    assert torch.equal(win[3, 12], ffeat[0, :, 8, 12]) and torch.equal(win[0, 12], ffeat[0, :, 0, 0]) and float(win[0, :2].abs().max()) == 0.0
    assert torch.equal(win[2, 0], ffeat[1, :, 18, 26]) and torch.equal(win[2, 24], ffeat[1, :, 22, 30]) and float(win[1, 4].abs().max()) == 0.0
    block = ck.fine_block("synth")
    y, ym = ck.fine_layer_fp64(win, block), ck.fine_layer_model(win, block)
    e = ck.maxerr(ym, y) / y.abs().max().item()
    print(f"fine layer E_model / largest entry, benign: {e:.2e}")
    assert 0.0 < e < 1e-5
    # the expectation: a one-hot correlation gives the grid position and the clamp's spread (windows 4 .. 7 lie inside the map: no two
    # tokens of them are the same zero padding)
    j = torch.tensor([0, 2, 12, 24])
    pt = 1e3 * y[torch.arange(4, 8), j]
    ex, ey, sd = ck.fine_expectation_fp64(pt, y[4:])
    grid = torch.linspace(-1, 1, 5, dtype=torch.float64)
    assert torch.allclose(ex, grid[j % 5], atol=1e-12) and torch.allclose(ey, grid[j // 5], atol=1e-12)
    assert torch.allclose(sd, torch.full((4,), 2e-5, dtype=torch.float64), rtol=1e-6)


def test_offset_scores_discriminate_the_score_split():
    """offset_score_block: every score is large (|s| >= 50), most soft-maxes are undecided, and the model with a TWO-term split of the
    score operands is outside the bar that the three-term model sets -- the case tells the two apart."""
    ffeat = ck.rnd(1, 128, 24, 32, seed=36)
    win = ck.gather_windows(ffeat, torch.zeros(8, dtype=torch.int64), torch.tensor([9, 19, 27, 38, 10, 12, 29, 36]))
    block = ck.offset_score_block()
    s = ck.fine_scores_fp64(win, block)
    top = torch.softmax(s, -1).max(-1).values
    assert s.abs().min().item() >= 50 and (top < 0.9).double().mean().item() >= 0.5
    y = ck.fine_layer_fp64(win, block)
    e3, e2 = ck.maxerr(ck.fine_layer_model(win, block), y), ck.maxerr(ck.fine_layer_model(win, block, score_terms=2), y)
    print(f"offset scores {s.abs().min().item():.0f} .. {s.abs().max().item():.0f}: E_model three-term {e3:.2e} (bar {ck.model_bar(e3, y):.2e}), two-term {e2:.2e}")
    assert e2 > 2.0 * ck.model_bar(e3, y)
