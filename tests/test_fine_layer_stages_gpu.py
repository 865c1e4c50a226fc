"""The one-launch fine stage (nm_fine_window_layer / nm_fine_stage, csrc/fine_layer.hip) stage by stage at edge inputs, through
ops.fine_window_layer on a 24 x 32 fine map, with 1, 5 (a ragged group of four) and 8 matches in 11 slots.

The kernel keeps a whole encoder layer in accumulator registers and re-implements two LayerNorms, a soft-max over 25 keys, the polynomial
GELU of bf16x3.h and FineMatching's expectation inline; its other tests feed it N(0, 1) maps and 0.08 N(0, 1) weights only.  Here:
  * LN1 alone (W2 = 0, b2 = 0: `out` is the parked LN1(window), fp32, no split in the way) on pixels of 1024 + s_i, a constant pixel, a
    pixel whose variance eps dominates and the zero padding of border windows, two values of eps;
  * LN2 and the GELU at the probe values (both LayerNorms with gamma = beta = 0, b1 = the probes, W2 = I);
  * the inner soft-max peaked: Wq, Wk scaled until the scores reach 50 and beyond, against float64 at the bar of the split-arithmetic
    model with three-term scores (tests/chain_kernel_util.py), beside the benign case; and large scores that stay UNDECIDED (all
    near 256, keys a few units apart), where a score error in proportion to its size shows in the output;
  * a near-one-hot correlation in the FineMatching tail: the max(var, 1e-10) clamp and the exx - ex^2 cancellation.
Only valid slots are compared; slots behind the count follow the existing contract (expec_f zeros, out unwritten).

Measured on the MI355X:
  LN1 alone: 1.0e-7 .. 1.1e-7 of the largest entry at both eps (bar 2^-20 = 9.5e-7); padding tokens and the constant pixel give beta exactly.
  GELU probes: worst error / bar 0.196 (at u = 3: the carry of the value).
  inner soft-max, error / E_model / model bar: benign (|s| <= 2.0) 4.9e-6 .. 5.8e-6 / 5.4e-6 / 2.5e-5 (1.4e-6 of the largest entry);
    peaked (|s| up to 126, 58 .. 61 % of the soft-maxes above 0.99) 8.9e-6 .. 1.19e-5 / 1.07e-5 / 4.6e-5 (3.0e-6 of the largest entry).
    undecided at s = 230 .. 282 (75 .. 90 % of the soft-maxes below 0.9): 5.5e-5 .. 6.3e-5 / 5.5e-5 .. 6.2e-5 / 2.6e-4 .. 2.9e-4; the same kernel
    with the scores' operands split in two terms instead of three: 3.8e-4 .. 7.2e-4 (fails), while it passes the peaked case at 1.9e-5.
  near-one-hot expectation: lambda 1 (top p >= 0.9995) E[x], E[y] off by <= 1.8e-7, std by <= 1.4e-5; lambda 30 and 1e3: E[x], E[y] exact,
    std = 2e-5 (the clamp) to 5e-13.
Every test takes 0.01 s.
"""
import math

import pytest
import torch

import chain_kernel_util as ck
from nerfmatch_amd import ops

pytestmark = pytest.mark.gpu
HF, WF, K = 24, 32, 11
COUNTS = (1, 5, 8)
# cells of the 6 x 8 coarse grid: the first five are the map's corners (windows hanging over its top / left border) and an inner cell
BORDER_IDS = (0, 19, 7, 47, 40, 19, 10, 0, 27, 38, 9)
INNER_IDS = (9, 19, 27, 38, 10, 12, 29, 36, 20, 21, 30)  # every window inside the map: no two tokens are the same zero padding


@pytest.fixture(autouse=True)
def _split_precision(monkeypatch):
    monkeypatch.setattr(ops, "LINEAR_PRECISION", "bf16x3")
    yield


def run(ffeat, ids, count, block, gpu, pt_f=None):
    i_ids = torch.tensor(ids, dtype=torch.int64, device=gpu)
    cnt = torch.tensor([count], dtype=torch.int32, device=gpu)
    block = block.to(gpu)
    assert ops.fine_window_layer_supported(block, 5, 128)
    return ops.fine_window_layer(ffeat.to(gpu), torch.zeros(K, dtype=torch.int64, device=gpu), i_ids, cnt, block, 4, pt_f=None if pt_f is None else pt_f.to(gpu)).cpu()


def windows(ffeat, ids, count):
    return ck.gather_windows(ffeat, torch.zeros(count, dtype=torch.int64), torch.tensor(ids[:count]))


# ----------------------------------------------------------------------------------------------- LN1 alone
def _ln1_map():
    px = ck.exact_offset_rows(HF * WF, 128, seed=31)
    ffeat = px.T.reshape(1, 128, HF, WF).clone()
    for (y, x) in ((0, 1), (8, 12)):
        ffeat[0, :, y, x] = 2.5  # a constant pixel in the windows of cells 0 and 19
    for j, (y, x) in enumerate(((1, 0), (9, 13))):
        ffeat[0, :, y, x] = ck.negligible_variance_rows(1, 128, seed=32 + j)[0]
    return ffeat


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("eps1", [1e-5, 1e-3])
def test_ln1_in_isolation(gpu, built_lib, count, eps1):
    """W2 = 0 and b2 = 0: the output is xh = LN1(window) as the kernel parks it.  Against float64 at 2^-20 of the largest entry."""
    ffeat = _ln1_map()
    g1, b1 = 1.0 + ck.rnd(128, seed=33, scale=0.3), ck.rnd(128, seed=34, scale=0.3)
    block = ck.fine_block("synth", eps1=eps1, ln1_g=g1, ln1_b=b1, w2=torch.zeros(128, 128), b2=torch.zeros(128))
    out = run(ffeat, BORDER_IDS, count, block, gpu)
    assert out.shape == (K, 25, 128)
    win = windows(ffeat, BORDER_IDS, count)
    w64 = win.double()
    # the case is what it claims to be: slot 0 is a border window with padding, a constant and a negligible-variance pixel and offset pixels
    std, mean = w64[0].std(-1, unbiased=False), w64[0].mean(-1)
    assert bool((w64[0].abs().max(-1).values == 0).any()) and bool(((std == 0) & (mean == 2.5)).any()) and bool(((std > 0) & (std**2 < 2e-6)).any())
    assert bool((mean.abs() / std.clamp_min(1e-30) > 100)[std > 1].any())
    want = ck.ln64(win, g1, b1, eps1)
    err, scale = ck.maxerr(out[:count], want), want.abs().max().item()
    print(f"fine LN1 alone count {count} eps {eps1:g}: err {err:.2e} = {err / scale:.2e} of the largest entry (bar 2^-20 = {ck.FLOOR:.2e})")
    assert bool(torch.isfinite(out[:count]).all())
    assert err <= ck.FLOOR * scale
    zero_tok = w64.abs().max(-1).values == 0
    const_tok = zero_tok | ((w64.std(-1, unbiased=False) == 0) & (w64.mean(-1) == 2.5))
    assert torch.equal(out[:count][const_tok], b1.expand(int(const_tok.sum()), 128)), "padding tokens and constant pixels normalise to beta"


def test_ln1_follows_its_eps(gpu, built_lib):
    """The negligible-variance pixel under the two eps values: outputs differ as float64 says (a hard-coded eps fails)."""
    ffeat = _ln1_map()
    g1, b1 = 1.0 + ck.rnd(128, seed=33, scale=0.3), ck.rnd(128, seed=34, scale=0.3)
    tok = 5 * 3 + 2  # pixel (1, 0) in the window of cell 0
    assert torch.equal(windows(ffeat, BORDER_IDS, 1)[0, tok], ffeat[0, :, 1, 0])
    got, want = {}, {}
    for eps1 in (1e-5, 1e-3):
        block = ck.fine_block("synth", eps1=eps1, ln1_g=g1, ln1_b=b1, w2=torch.zeros(128, 128), b2=torch.zeros(128))
        got[eps1] = run(ffeat, BORDER_IDS, 1, block, gpu)[0, tok].double()
        want[eps1] = ck.ln64(ffeat[0, :, 1, 0][None], g1, b1, eps1)[0]
    d_want, d_got = want[1e-5] - want[1e-3], got[1e-5] - got[1e-3]
    assert d_want.abs().max().item() > 0.1
    assert (d_got - d_want).abs().max().item() <= 2 * ck.FLOOR * max(want[1e-5].abs().max().item(), want[1e-3].abs().max().item())


# ----------------------------------------------------------------------------------------------- LN2 and the GELU at the probes
@pytest.mark.parametrize("count", COUNTS)
def test_ln2_and_gelu_probes(gpu, built_lib, count):
    """ln1 gamma = beta = 0: xh = 0, attention of zeros.  ln2 gamma = beta = 0: the first FFN product sees zeros, u = b1 = the probes.
    W2 = I, b2 = 0: out = hi + lo of gelu(b1) in every token of every valid match, within 1e-6 + 2^-16 |gelu| of float64."""
    probes = ck.probe_row(128)
    assert probes.abs().max().item() >= 12 and bool((probes > 0).any()) and bool((probes < 0).any())
    assert set(probes.tolist()) == set(torch.tensor(ck.PROBES).tolist())  # every probe is in the row
    z = torch.zeros(128)
    block = ck.fine_block("synth", ln1_g=z, ln1_b=z, ln2_g=z, ln2_b=z, b1=probes, w2=torch.eye(128), b2=z)
    ffeat = ck.rnd(1, 128, HF, WF, seed=35)
    out = run(ffeat, BORDER_IDS, count, block, gpu)[:count]
    want = ck.gelu64(probes).expand(count, 25, 128)
    err, bar = (out.double() - want).abs(), 1e-6 + ck.CARRY * want.abs()
    i = int((err / bar).argmax())
    print(f"fine layer GELU probes count {count}: max err {err.max().item():.2e}; worst err / bar {(err / bar).max().item():.3f} at u = {probes[i % 128].item():g}")
    assert bool(torch.isfinite(out).all())
    assert bool((err <= bar).all()), [(probes[j % 128].item(), err.flatten()[j].item()) for j in torch.nonzero(err.flatten() > bar.flatten()).flatten().tolist()[:8]]


# ----------------------------------------------------------------------------------------------- the inner soft-max, peaked
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("gain", [1.0, 8.0], ids=["benign", "peaked"])
def test_inner_softmax_peaked(gpu, built_lib, gain, count):
    """Wq and Wk times `gain`.  gain 8: the float64 scores reach |s| >= 50 (83 .. 126 here) and at least half of the (match, head, query)
    soft-maxes put more than 0.99 on one key -- the regime the three-term split of the score operands exists for.  `out` against float64
    at the model bar; the benign case (gain 1) also at the project's 1e-5 of the largest entry.  Windows inside the map: the identical
    padding tokens of a border window tie as keys and keep a soft-max from peaking."""
    base = ck.fine_block("synth")
    at = base.layers[0].attention
    block = ck.fine_block("synth", wq=at.proj_q.weight * gain, wk=at.proj_k.weight * gain)
    ffeat = ck.rnd(1, 128, HF, WF, seed=36)
    win = windows(ffeat, INNER_IDS, count)
    s = ck.fine_scores_fp64(win, block)
    top = torch.softmax(s, -1).max(-1).values
    frac = (top > 0.99).double().mean().item()
    if gain > 1:
        assert s.abs().max().item() >= 50 and frac >= 0.5, (s.abs().max().item(), frac)
    else:
        assert s.abs().max().item() < 5 and frac == 0.0
    out = run(ffeat, INNER_IDS, count, block, gpu)[:count]
    y, ym = ck.fine_layer_fp64(win, block), ck.fine_layer_model(win, block)
    err, e_model, scale = ck.maxerr(out, y), ck.maxerr(ym, y), y.abs().max().item()
    print(f"fine layer gain {gain:g} count {count}: max |s| {s.abs().max().item():.1f}, {frac:.2f} of the soft-maxes above 0.99; err {err:.2e}, "
          f"E_model {e_model:.2e}, model bar {ck.model_bar(e_model, y):.2e}, largest entry {scale:.2f} (err / scale {err / scale:.2e})")
    assert bool(torch.isfinite(out).all()) and e_model > 0.0
    assert err <= ck.model_bar(e_model, y), (err, e_model)
    if gain == 1:
        assert err <= 1e-5 * scale


@pytest.mark.parametrize("count", COUNTS)
def test_inner_softmax_undecided_at_large_scores(gpu, built_lib, count):
    """chain_kernel_util.offset_score_block: every score near 256, the keys a few units apart, most soft-maxes undecided -- where an error
    of the score in proportion to its size reaches the output (a saturated soft-max forgives it).  At the model bar; the model with a
    two-term score split is 2.5 bars off on these inputs (test_chain_kernel_util_cpu.py)."""
    block = ck.offset_score_block()
    ffeat = ck.rnd(1, 128, HF, WF, seed=36)
    win = windows(ffeat, INNER_IDS, count)
    s = ck.fine_scores_fp64(win, block)
    top = torch.softmax(s, -1).max(-1).values
    assert s.abs().min().item() >= 50 and (top < 0.9).double().mean().item() >= 0.5
    out = run(ffeat, INNER_IDS, count, block, gpu)[:count]
    y, ym = ck.fine_layer_fp64(win, block), ck.fine_layer_model(win, block)
    err, e_model = ck.maxerr(out, y), ck.maxerr(ym, y)
    print(f"fine layer offset scores count {count}: s {s.abs().min().item():.0f} .. {s.abs().max().item():.0f}, {(top < 0.9).double().mean().item():.2f} of the soft-maxes "
          f"below 0.9; err {err:.2e}, E_model {e_model:.2e}, model bar {ck.model_bar(e_model, y):.2e}, largest entry {y.abs().max().item():.1f}")
    assert bool(torch.isfinite(out).all()) and e_model > 0.0
    assert err <= ck.model_bar(e_model, y), (err, e_model)


# ----------------------------------------------------------------------------------------------- FineMatching's tail, near one-hot
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("lam", [1.0, 30.0, 1e3])
def test_near_one_hot_expectation(gpu, built_lib, lam, count):
    """pt_f = lambda y[k, j*] with j* a corner, an edge or the centre of the window: the correlation's soft-max is (nearly) one-hot at
    j*.  All outputs finite; E[x], E[y] within the project's 2e-4 of float64; std within 2 sqrt(2^-22) ~ 1e-3 (the fp32 exx - ex^2 carries
    a few ulp of 1, and |sqrt(v + d) - sqrt(v)| <= sqrt|d| per axis) and at least the clamp's 2e-5; zeros behind the count."""
    block = ck.fine_block("synth")
    ffeat = ck.rnd(1, 128, HF, WF, seed=37)
    win = windows(ffeat, INNER_IDS, count)
    assert bool((win.abs().max(-1).values > 0).all())
    y = ck.fine_layer_fp64(win, block)
    jstar = torch.tensor([(0, 2, 12, 24, 10, 14, 22, 4)[k % 8] for k in range(count)])  # corners, edges, the centre
    pt = torch.zeros(K, 128)
    pt[:count] = (lam * y[torch.arange(count), jstar]).float()
    ex64, ey64, sd64 = ck.fine_expectation_fp64(pt[:count], y)
    p64 = torch.softmax((pt[:count].double()[:, None] * y).sum(-1) / math.sqrt(128.0), -1)
    assert torch.equal(p64.argmax(-1), jstar) and bool((p64.max(-1).values > 0.99).all()), p64.max(-1).values
    ex = run(ffeat, INNER_IDS, count, block, gpu, pt_f=pt)
    assert ex.shape == (K, 3) and bool(torch.isfinite(ex).all())
    assert bool((ex[count:] == 0).all())
    e_x, e_y = (ex[:count, 0].double() - ex64).abs().max().item(), (ex[:count, 1].double() - ey64).abs().max().item()
    e_sd = (ex[:count, 2].double() - sd64).abs().max().item()
    print(f"near one-hot lambda {lam:g} count {count}: top p >= {p64.max(-1).values.min().item():.6f}; |E[x]| err {e_x:.2e}, |E[y]| err {e_y:.2e}, "
          f"std err {e_sd:.2e} (std fp64 {sd64.min().item():.2e} .. {sd64.max().item():.2e}, kernel min {ex[:count, 2].min().item():.2e})")
    assert e_x <= 2e-4 and e_y <= 2e-4
    assert e_sd <= 2.0 * math.sqrt(2.0**-22)
    assert ex[:count, 2].min().item() >= 2e-5 * (1 - 1e-3)
