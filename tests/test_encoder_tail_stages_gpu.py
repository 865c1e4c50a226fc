"""The three chained encoder-tail kernels stage by stage at edge inputs: nm_encoder_tail_bf16x3, nm_encoder_tail_save_bf16x3 and
nm_encoder_tail_bwd_bf16x3 (csrc/encoder_tail.hip, encoder_tail_bwd.hip, encoder_tail_chain.h) through ops.encoder_tail,
ops.encoder_tail_save and ops.encoder_tail_bwd.

The other tests of these kernels are end to end on N(0, 1) rows with eps = 1e-5.  Here every stage the kernels re-implement inline is
isolated by the choice of the weights (a zero or identity matrix takes a product out of the way), fed the inputs at which such code goes
wrong, and compared with float64 (tests/chain_kernel_util.py):
  * row counts 1 .. 257 (below one wavefront's 32 rows every lane clamps to row R - 1), all five outputs, and placement invariance;
  * LayerNorm 2 alone: rows of 1024 + s_i (a one-pass variance is 4e-2 off there), constant rows, rows whose variance eps dominates,
    large rows, three values of eps;
  * the chained GELU (gelu_erf, bf16x3.h: a polynomial, not erff) and its derivative (gelu_grad) at the probe values;
  * the backward on a_pre / u_pre chosen by the test.
Bars: exact where the construction makes it exact; the split carry 1e-6 + 2^-16 |value| behind an identity weight; otherwise
4 E_model + 2^-20 max|fp64| with E_model the split-arithmetic model's error on the same inputs, beside the project's 2e-5 of scale.

Measured on the MI355X: the kernels sit ON the model (the fp32 accumulation and the hardware rcp / exp add nothing one can see).
  rows 1 .. 257, error / E_model / model bar: y 3.6e-6 .. 6.5e-6 / 3.5e-6 .. 6.6e-6 / 1.8e-5 .. 3.2e-5; a_out 1.10e-5 / 1.13e-5 / 5.1e-5;
    u_out 1.09e-5 / 1.06e-5 / 4.5e-5; d_att 2.6e-6 / 2.6e-6 / 1.1e-5 (2e-5 of scale: 8.2e-6); d_xh 4.4e-6 / 4.3e-6 / 2.2e-5; placement: bit-equal.
  LayerNorm 2 alone, every eps: worst error / bar 0.39 .. 0.48 in u_out (the split carry itself), 0.19 .. 0.39 in y; a_out = xh and the
    constant rows' carry of beta exact.  eps 1e-5 / 1e-3 / 1e-6 move the variance-1e-6 rows by 1.1 .. 3.0; the kernels follow to 2e-5.
  GELU probes: worst error / bar 0.196 (at u = 3: the carry of the value; the polynomial's own 4.6e-7 is below it), u_out = b1 exact.
  backward on chosen intermediates, error / E_model / bar: offset rows d_xh 7.1e-6 / 7.1e-6 / 3.2e-5 (identity), 2.3e-6 / 2.3e-6 / 1.2e-5 (synth);
    constant rows (scale 1.3e3 at eps 1e-5) 6.8e-3 / 6.8e-3 / 2.9e-2; large rows d_att 5.8e-8 / 6.0e-8 / 2.5e-7; benign 3.1e-6 / 3.2e-6 / 1.3e-5.
Every test takes 0.2 s or less.
"""
import pytest
import torch

import chain_kernel_util as ck
from nerfmatch_amd import ops

pytestmark = pytest.mark.gpu
ROW_COUNTS = (1, 2, 31, 32, 33, 127, 128, 129, 257)
POSITIONS = (0, 31, 32, 63, 64, 127, 128)  # and R - 1
NAMES = ("y", "a_out", "u_out", "d_att", "d_xh")


@pytest.fixture(autouse=True)
def _split_precision(monkeypatch):
    monkeypatch.setattr(ops, "LINEAR_PRECISION", "bf16x3")
    yield


_ON_GPU = {}


def on_gpu(p, gpu, eps=None):
    """The holder's tensors on the device, once per holder (the packed-weight cache is keyed on the tensor), with `eps` of the caller's choice."""
    key = id(p)
    if key not in _ON_GPU:
        _ON_GPU[key] = (p, ck.tail_to(p, gpu))  # (p kept: its id stays its own)
    q = _ON_GPU[key][1]
    return q if eps is None else ck.with_eps(q, eps)


def run_all(att, xh, dy, p, gpu, eps=None):
    """(y, y_save, a_out, u_out, d_att, d_xh) on the CPU: the two forwards, and the backward fed the saving forward's own intermediates."""
    q = on_gpu(p, gpu, eps)
    ag, xg = att.to(gpu), xh.to(gpu)
    y = ops.encoder_tail(ag, xg, *ck.tail_args(q))
    y_s, a, u = ops.encoder_tail_save(ag, xg, *ck.tail_args(q))
    d_att, d_xh = ops.encoder_tail_bwd(dy.to(gpu), a, u, *ck.tail_args(q))
    return tuple(t.cpu() for t in (y, y_s, a, u, d_att, d_xh))


SYNTH = ck.tail_params("synth")


@pytest.fixture(scope="module")
def benign_refs():
    """float64 and model values of the 257 benign rows, computed once; a launch of R rows is their first R rows."""
    att, xh, dy = ck.benign_tail_case()
    a, u, y = ck.tail_fp64(att, xh, SYNTH, 1e-5)
    ma, mu, my = ck.tail_model(att, xh, SYNTH, 1e-5)
    d_att, d_xh = ck.tail_bwd_fp64(dy, a, u, SYNTH, 1e-5)  # (float64 all the way: nothing of the kernels' enters the reference)
    m_att, m_xh = ck.tail_bwd_model(dy, ma.float(), mu.float(), SYNTH, 1e-5)
    return dict(ref=dict(a_out=a, u_out=u, y=y, d_att=d_att, d_xh=d_xh), model=dict(a_out=ma, u_out=mu, y=my, d_att=m_att, d_xh=m_xh))


# ----------------------------------------------------------------------------------------------- 1. row counts and placement
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_all_five_outputs(gpu, built_lib, benign_refs, rows):
    """Benign rows, non-trivial gamma, beta, b1, b2 (synth._encoder_layer), R from 1 to 257: y, a_out, u_out against float64 at the model
    bar and at 2e-5 of scale, y of the plain forward = y of the saving forward bit for bit, d_att and d_xh (the backward kernel fed the
    saving forward's a_out / u_out, as the iNeRF matching term runs them) against the float64 chain, each against its own scale."""
    att, xh, dy = (t[:rows] for t in ck.benign_tail_case())
    y, y_s, a, u, d_att, d_xh = run_all(att, xh, dy, SYNTH, gpu)
    assert torch.equal(y, y_s), "the plain forward and the saving forward differ in y"
    for name, got in (("y", y), ("a_out", a), ("u_out", u), ("d_att", d_att), ("d_xh", d_xh)):
        ref, mod = benign_refs["ref"][name][:rows], benign_refs["model"][name][:rows]
        assert got.shape == ref.shape and bool(torch.isfinite(got).all())
        err, e_model, scale = ck.maxerr(got, ref), ck.maxerr(mod, ref), ref.abs().max().item()
        print(f"rows {rows} {name}: err {err:.2e}, E_model {e_model:.2e}, model bar {ck.model_bar(e_model, ref):.2e}, 2e-5 of scale {2e-5 * scale:.2e}")
        assert e_model > 0.0
        assert err <= ck.model_bar(e_model, ref), (name, err, e_model)
        assert err <= 2e-5 * scale, (name, err, scale)


@pytest.mark.parametrize("rows", [129, 257])
def test_placement_invariance(gpu, built_lib, rows):
    """Every lane pair owns its row from end to end: a row's five outputs in an R-row launch are the bits of that row launched alone
    (where every lane of the one wavefront clamps to it), at the first and last lanes of the wavefronts and workgroups and at R - 1."""
    att, xh, dy = (t[:rows] for t in ck.benign_tail_case())
    q = on_gpu(SYNTH, gpu)
    whole = run_all(att, xh, dy, SYNTH, gpu)
    a_g, u_g = whole[2].to(gpu), whole[3].to(gpu)
    for pos in sorted({p for p in POSITIONS if p < rows} | {rows - 1}):
        s = slice(pos, pos + 1)
        alone = run_all(att[s], xh[s], dy[s], SYNTH, gpu)
        for name, w, o in zip(("y", "y_save") + NAMES[1:], whole, alone):
            assert torch.equal(w[s], o), (name, pos, (w[s] - o).abs().max().item())
        # ... and the backward alone on the SAME intermediates (run_all's came from the one-row forward, equal by the lines above)
        d_att, d_xh = ops.encoder_tail_bwd(dy[s].to(gpu), a_g[s], u_g[s], *ck.tail_args(q))
        assert torch.equal(d_att.cpu(), whole[4][s]) and torch.equal(d_xh.cpu(), whole[5][s]), pos


# ----------------------------------------------------------------------------------------------- 2. LayerNorm 2 alone
LN_ROWS, LN_KIND = ck.designed_rows(256, per_kind=9, seed=11)  # 45 rows: two wavefronts, the second ragged
LN_PARAMS = ck.tail_params("synth", seed=7, wo=torch.zeros(256, 256), w1=torch.eye(256), b1=torch.zeros(256), w2=torch.eye(256), b2=torch.zeros(256),
                           gamma=1.0 + ck.rnd(256, seed=12, scale=0.3), beta=ck.rnd(256, seed=13, scale=0.3))


def _ln_run(gpu, eps):
    """(a_out, u_out, y of the plain forward) -- after checking that the saving forward's y is the same bits."""
    att = ck.rnd(LN_ROWS.shape[0], 256, seed=14).to(gpu)
    q = on_gpu(LN_PARAMS, gpu, eps)
    y = ops.encoder_tail(att, LN_ROWS.to(gpu), *ck.tail_args(q))
    y_s, a, u = ops.encoder_tail_save(att, LN_ROWS.to(gpu), *ck.tail_args(q))
    assert torch.equal(y, y_s), f"eps {eps:g}: the plain forward and the saving forward differ in y"
    return a.cpu(), u.cpu(), y.cpu()


def _ln_want(rows, eps):
    """float64 (u, y, bar of u, bar of y) of the isolated LayerNorm: u = LN2(xh), y = xh + gelu(u) behind two identity weights.
    bar(u) = the split carry 1e-6 + 2^-16 |u|.  bar(y): gelu is 1.13-Lipschitz, so bar(u) arrives as 1.13 bar(u); the polynomial GELU's
    1e-6; the carry 2^-16 |gelu(u)| of the second identity; the final fp32 sum's 2^-23 |y| (on the offset rows that term is all one sees)."""
    u = ck.ln64(rows, LN_PARAMS.norm2.weight, LN_PARAMS.norm2.bias, eps)
    y = rows.double() + ck.gelu64(u)
    bar_u = 1e-6 + ck.CARRY * u.abs()
    return u, y, bar_u, 1.13 * bar_u + 1e-6 + ck.CARRY * ck.gelu64(u).abs() + 2.0**-23 * y.abs()


@pytest.mark.parametrize("eps", ck.EPS_VALUES)
def test_layernorm2_in_isolation(gpu, built_lib, eps):
    """Wo = 0: a_out is xh bit for bit.  W1 = I, b1 = 0: u_out is hi + lo of LN2(a).  Against the float64 LayerNorm within the split
    carry 1e-6 + 2^-16 |value|; the constant rows give exactly the carry of beta.  W2 = I, b2 = 0: y = xh + hi + lo of gelu(u), through
    both forwards (the same bits), within the bar of _ln_want."""
    a, u, y = _ln_run(gpu, eps)
    assert torch.equal(a, LN_ROWS), "Wo = 0: a_out must be xh"
    want, want_y, bar_u, bar_y = _ln_want(LN_ROWS, eps)
    # the cases are what they claim to be
    x64 = LN_ROWS.double()
    mean, std = x64.mean(-1), x64.std(-1, unbiased=False)
    assert bool((mean[LN_KIND["offset"]].abs() / std[LN_KIND["offset"]] > 100).all())
    assert bool((std[LN_KIND["constant"]] == 0).all()) and bool((std[LN_KIND["negligible"]] ** 2 < 2e-6).all())
    assert bool((std[LN_KIND["large"]] > 40).all()) and float(x64[LN_KIND["large"]].abs().max()) > 100
    for kind, s in LN_KIND.items():
        err, err_y = (u[s].double() - want[s]).abs(), (y[s].double() - want_y[s]).abs()
        print(f"LN2 eps {eps:g} {kind}: u max err {err.max().item():.2e}, worst err / bar {(err / bar_u[s]).max().item():.2f}; "
              f"y max err {err_y.max().item():.2e}, worst err / bar {(err_y / bar_y[s]).max().item():.2f}")
        assert bool((err <= bar_u[s]).all()), (kind, eps, (err / bar_u[s]).max().item())
        assert bool((err_y <= bar_y[s]).all()), (kind, eps, (err_y / bar_y[s]).max().item())
    b = LN_PARAMS.norm2.bias
    assert torch.equal(u[LN_KIND["constant"]], ck.carry(b).expand(9, 256)), "constant rows: u_out must be the carry of beta"


def test_layernorm2_follows_its_eps(gpu, built_lib):
    """On the rows of variance 1e-6 the three eps values give outputs that differ as float64 says they do (by far more than the bars), in
    u_out of the saving forward and in y of both forwards: a kernel that ignored its eps argument, or used a constant, fails here."""
    s = LN_KIND["negligible"]
    got = {eps: tuple(t[s].double() for t in _ln_run(gpu, eps)[1:]) for eps in ck.EPS_VALUES}
    want = {eps: _ln_want(LN_ROWS[s], eps) for eps in ck.EPS_VALUES}
    for e0, e1 in ((1e-5, 1e-3), (1e-5, 1e-6), (1e-3, 1e-6)):
        for i, name in enumerate(("u_out", "y")):
            d_want, d_got = want[e0][i] - want[e1][i], got[e0][i] - got[e1][i]
            bar = want[e0][2 + i] + want[e1][2 + i]
            assert d_want.abs().max().item() > 0.1, "the eps values must move these rows"
            print(f"eps {e0:g} vs {e1:g} {name}: differ by up to {d_want.abs().max().item():.3f} in float64; kernel off by {(d_got - d_want).abs().max().item():.2e}")
            assert bool(((d_got - d_want).abs() <= bar).all()), (name, e0, e1)


# ----------------------------------------------------------------------------------------------- 3. the chained GELU at the probes
PROBE_PARAMS = ck.tail_params("synth", seed=9, gamma=torch.zeros(256), beta=torch.zeros(256), b1=ck.probe_row(256), w2=torch.eye(256), b2=torch.zeros(256))


@pytest.mark.parametrize("rows", [1, 33])
def test_gelu_probes_through_both_forwards(gpu, built_lib, rows):
    """gamma = beta = 0: the first FFN product sees zeros and u = b1, the probes, bit for bit (up to the sign of zero: 0 + -0 = +0).
    W2 = I, b2 = 0, xh = 0: y = hi + lo of gelu(b1).  Against float64 0.5 u (1 + erf(u / sqrt 2)) within 1e-6 + 2^-16 |gelu|."""
    probes = ck.probe_row(256)
    assert probes.abs().max().item() >= 12 and bool((probes > 0).any()) and bool((probes < 0).any())
    assert set(probes.tolist()) == set(torch.tensor(ck.PROBES).tolist())  # every probe is in the row
    q = on_gpu(PROBE_PARAMS, gpu)
    att, xh = ck.rnd(rows, 256, seed=15).to(gpu), torch.zeros(rows, 256, device=gpu)
    y = ops.encoder_tail(att, xh, *ck.tail_args(q)).cpu()
    y_s, a, u = (t.cpu() for t in ops.encoder_tail_save(att, xh, *ck.tail_args(q)))
    assert torch.equal(y, y_s)
    assert torch.equal(u, probes.expand(rows, 256)), "u_out must be b1"  # (torch.equal compares values: -0.0 == +0.0)
    assert bool(torch.isfinite(a).all())
    want = ck.gelu64(probes).expand(rows, 256)
    err, bar = (y.double() - want).abs(), 1e-6 + ck.CARRY * want.abs()
    i = int((err / bar).argmax())
    print(f"chained GELU rows {rows}: max err {err.max().item():.2e}; worst err / bar {(err / bar).max().item():.3f} at u = {probes[i % 256].item():g}")
    assert bool((err <= bar).all()), [(probes[j % 256].item(), err.flatten()[j].item()) for j in torch.nonzero(err.flatten() > bar.flatten()).flatten().tolist()[:8]]


# ----------------------------------------------------------------------------------------------- 4. the backward on chosen intermediates
BWD_A, BWD_KIND = ck.designed_rows(256, per_kind=9, seed=21)
BWD_U = torch.stack([ck.probe_row(256, shift=r) for r in range(BWD_A.shape[0])])
BWD_DY = ck.rnd(BWD_A.shape[0], 256, seed=22)
BWD_PARAMS = {"identity": ck.tail_params("identity", seed=23, gamma=1.0 + ck.rnd(256, seed=24, scale=0.3)), "synth": ck.tail_params("synth", seed=23)}


@pytest.mark.parametrize("eps", ck.EPS_VALUES)
@pytest.mark.parametrize("weights", ["identity", "synth"])
def test_backward_on_chosen_intermediates(gpu, built_lib, weights, eps):
    """u_pre = the probes (every column sees every probe over the rows), a_pre = the designed rows and benign ones, dy random: d_att and
    d_xh against the closed-form float64 backward at the model bar, every kind of row against its own scale (rstd is 1 / sqrt(eps) on the
    constant rows, 1 / 50 on the large ones).  With Wo = I, d_att is the split of the d_a that d_xh - dy holds in fp32."""
    p = BWD_PARAMS[weights]
    q = on_gpu(p, gpu, eps)
    assert BWD_U.abs().max().item() >= 12 and bool((BWD_U > 0).any()) and bool((BWD_U < 0).any())
    a64 = BWD_A.double()
    assert bool((a64[BWD_KIND["offset"]].mean(-1).abs() / a64[BWD_KIND["offset"]].std(-1, unbiased=False) > 100).all())
    d_att, d_xh = (t.cpu() for t in ops.encoder_tail_bwd(BWD_DY.to(gpu), BWD_A.to(gpu), BWD_U.to(gpu), *ck.tail_args(q)))
    assert bool(torch.isfinite(d_att).all()) and bool(torch.isfinite(d_xh).all())
    refs, mods = ck.tail_bwd_fp64(BWD_DY, BWD_A, BWD_U, p, eps), ck.tail_bwd_model(BWD_DY, BWD_A, BWD_U, p, eps)
    for name, got, ref, mod in zip(("d_att", "d_xh"), (d_att, d_xh), refs, mods):
        for kind, s in BWD_KIND.items():
            err, e_model = ck.maxerr(got[s], ref[s]), ck.maxerr(mod[s], ref[s])
            bar = ck.model_bar(e_model, ref[s])
            print(f"backward {weights} eps {eps:g} {name} {kind}: scale {ref[s].abs().max().item():.3g}, err {err:.2e}, E_model {e_model:.2e}, bar {bar:.2e}")
            assert err <= bar, (name, kind, err, e_model, bar)
    if weights == "identity":
        d_a = d_xh.double() - BWD_DY.double()
        assert bool(((d_att.double() - d_a).abs() <= ck.CARRY * d_a.abs() + 1e-6).all()), (d_att.double() - d_a).abs().max().item()
