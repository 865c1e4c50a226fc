"""GPU: the generic (unfused) fine stage beyond the shipped configuration -- window sides 2..8, 256-d fine features, 0 / 2 fine layers,
locality self-attention -- at kernel level against float64 references, end to end against the reference's own numbers
(tests/golden/matcher_fine_envelope.npz, synth.FINE_VARIANTS), and the > 65,535-window launches of the small-window attention.

Bars of the end-to-end comparisons.  The reference's own fp32 evaluation of the fixture lies within 2.1e-7 of its float64 one on
expec_f (every variant, both the batch and the single pair; 2.3e-6 on mpt2d_f, whose pixel coordinates up to 48 carry ulps of 4e-6).
The kernels see the same inputs but run the 5 encoder layers in front of the fine stage in another summation order (MFMA tiles; in
bf16x3 with 16-bit operand halves), each layer adding ~1e-6 relative: the fine stage's inputs differ by ~1e-5 relative, which the
window soft-max passes on to expec_f with a gain below 1.  EXPEC_BAR = 2e-5 = 100 x the reference's own fp32-vs-fp64 distance holds that
with room and is 5 x tighter than the 1e-4 of the shipped configuration's tests; mpt2d_f = mpt2d_c + expec_f * win / 2 * 2 takes
EXPEC_BAR * win plus the coordinates' own rounding (5e-6)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from nerfmatch_amd import _lib, ops, synth
from nerfmatch_amd.matcher import NeRFMatcherMS
from nerfmatch_amd.modules import PrecomputedBackbone
from oracle import matcher_oracle as mo

pytestmark = pytest.mark.gpu

EXPEC_BAR = 2e-5
MPT_ROUND = 5e-6


@pytest.fixture(params=["fp32", "bf16x3"])
def precision(request):
    import nerfmatch_amd

    nerfmatch_amd.set_precision(request.param)
    yield request.param
    nerfmatch_amd.set_precision("fp32")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rel(a, b, floor=1e-3):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(floor)).item()


def build(fx, name, gpu, sl=slice(0, 2), grad=False):
    cfg, sd = synth.fine_variant(name, int(fx["weights_seed"]))
    model = NeRFMatcherMS(cfg)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    model = model.to(gpu)
    cfeat, ffeat = fx["cfeat"][sl].to(gpu), fx["ffeat"][sl].to(gpu)
    if grad:
        cfeat.requires_grad_()
        ffeat.requires_grad_()
    model.backbone = PrecomputedBackbone((cfeat, ffeat), [256, 128])
    return model, cfeat, ffeat


def batch(fx, gpu, sl=slice(0, 2), train=False):
    t = lambda k: fx[k][sl].to(gpu)
    B = sl.stop - sl.start
    d = dict(image=torch.zeros(B, 3, 8, 8, device=gpu), im_mask=t("im_mask"), pt_mask=t("pt_mask"), pt3d=t("pt3d"), pt2d=t("pt2d"),
             pt_feat=t("pt_feat"))
    if train:
        d.update(conf_gt=t("conf_gt"), pt2d_proj=t("pt2d_proj"))
        d["pt_feat"].requires_grad_()
    return d


# ----------------------------------------------------------------------------- end to end against the reference
@pytest.mark.parametrize("name", synth.FINE_VARIANTS)
def test_fine_variant_forward_vs_reference(gpu, built_lib, precision, name):
    """Pair 0 alone (B = 1: the speculative single-pair path) and the batch of 2 (nm_fine_windows_batch with map ids): match lists equal
    to the reference's, expec_f / mpt2d_f within the bars above of the reference's float64 evaluation."""
    fx = load_golden("matcher_fine_envelope")
    win = synth.fine_variant(name)[0].win_sz
    for pre, sl in (("p0_", slice(0, 1)), ("", slice(0, 2))):
        model, _, _ = build(fx, name, gpu, sl)
        model.eval()
        data = batch(fx, gpu, sl)
        model.forward(data, mutual=True)
        b, i, j = (t.cpu() for t in data["match_ids"])
        t, t64 = f"{name}_fwd_{pre}", f"{name}_f64_{pre}"
        assert torch.equal(b, fx[t + "b_ids"]) and torch.equal(i, fx[t + "i_ids"]) and torch.equal(j, fx[t + "j_ids"])
        assert (data["mconf"].cpu() - fx[t + "mconf"]).abs().max() < 1e-4
        e = (data["expec_f"].cpu().double() - fx[t64 + "expec_f"]).abs().max().item()
        m = (data["mpt2d_f"].cpu().double() - fx[t64 + "mpt2d_f"]).abs().max().item()
        print(f"{name} {precision} {pre or 'batch'}: {len(i)} matches  |expec_f - f64| {e:.2e}  |mpt2d_f - f64| {m:.2e}")
        assert e < EXPEC_BAR, e
        assert m < EXPEC_BAR * win + MPT_ROUND, m
        assert torch.equal(data["mpt3d"].cpu(), fx[t + "mpt3d"])


@pytest.mark.parametrize("name", synth.FINE_VARIANTS)
def test_fine_variant_training_step_vs_reference(gpu, built_lib, precision, name):
    """One training step of every variant with the reference's GT padding: losses, padded ids, expec_f and the gradients of every
    fine_sa.* / pt_ffeat_proj.* / ffeat_proj.* parameter and of ffeat / pt_feat -- tolerances of test_training_step_vs_reference."""
    fx = load_golden("matcher_fine_envelope")
    t = f"{name}_trn_"
    with torch.enable_grad():
        model, cfeat, ffeat = build(fx, name, gpu, grad=True)
        data = batch(fx, gpu, train=True)
        np.random.seed(int(fx["np_seed"]))
        metrics = model.forward_with_metrics(data, training=True)
        assert abs(metrics["coarse_loss"].item() - float(fx[t + "coarse_loss"])) < 2e-6 * float(fx[t + "coarse_loss"]) + 1e-6
        b, i, j = (x.cpu() for x in data["match_ids"])
        assert torch.equal(b, fx[t + "b_ids"]) and torch.equal(i, fx[t + "i_ids"]) and torch.equal(j, fx[t + "j_ids"])
        assert data["pred_num"] == int(fx[t + "pred_num"])
        assert (data["expec_f"].detach().cpu() - fx[t + "expec_f"]).abs().max() < 1e-4
        assert abs(metrics["fine_loss"].item() - float(fx[t + "fine_loss"])) < 1e-4 * float(fx[t + "fine_loss"])
        assert abs(metrics["loss"].item() - float(fx[t + "loss"])) < 1e-4 * float(fx[t + "loss"])
        metrics["loss"].backward()
    assert rel(ffeat.grad.flatten()[::211], fx[t + "g_ffeat_sub"]) < 1e-3
    assert abs(ffeat.grad.norm().item() - float(fx[t + "g_ffeat_norm"])) < 1e-3 * float(fx[t + "g_ffeat_norm"])
    assert rel(data["pt_feat"].grad.flatten()[::37], fx[t + "g_pt_feat_sub"]) < 1e-3
    assert abs(data["pt_feat"].grad.norm().item() - float(fx[t + "g_pt_feat_norm"])) < 1e-3 * float(fx[t + "g_pt_feat_norm"])
    names = dict(model.named_parameters())
    checked = 0
    for key in fx:
        if not key.startswith(t + "gn__"):
            continue
        pname = key[len(t) + 4:].replace("__", ".")
        g = names[pname].grad
        assert g is not None, pname
        gf = g.flatten()
        mine = gf if gf.numel() <= 512 else gf[::97]
        assert rel(mine, fx[t + "gs__" + key[len(t) + 4:]]) < 2e-3, pname
        assert abs(gf.norm().item() - float(fx[key])) < 1e-3 * float(fx[key]) + 1e-6, pname
        checked += 1
    n_sa = {"fsa0": 0, "fsa2": 2}.get(name, 1)
    assert checked == 4 + 12 * n_sa + (1 if name == "fsa_lsa" else 0) + (2 if name == "ffeat256" else 0), checked


# ----------------------------------------------------------------------------- kernel level against float64
def _cells(n, win, stride=4):
    return (n + 2 * (win // 2) - win) // stride + 1


def _window_case(win, B=2, C=24, Hf=12, Wf=20, seed=0):
    """Every cell of the (reference's unfold) grid -- border and corner cells included -- plus repeats of the four corners and of one
    inner cell (overlapping scatter-adds in the backward)."""
    ch, cw = _cells(Hf, win), _cells(Wf, win)
    n = ch * cw
    corners = [0, cw - 1, (ch - 1) * cw, n - 1]
    i_ids = torch.tensor(list(range(n)) + corners * 3 + [cw + 1] * 5, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    map_ids = torch.randint(0, B, (len(i_ids),), generator=g)
    return rnd(B, C, Hf, Wf, seed=seed + 1).double(), map_ids, i_ids


@pytest.mark.parametrize("win", range(2, 9))
def test_fine_windows_vs_unfold(gpu, built_lib, win):
    """nm_fine_windows / _batch: the window gather equals F.unfold(padding=win // 2, stride 4) at every cell, bit for bit (a copy)."""
    ff, map_ids, i_ids = _window_case(win)
    K = len(i_ids)
    cnt = torch.tensor([K], dtype=torch.int32, device=gpu)
    ffg = ff.float().to(gpu)
    ref = mo.fine_windows(ff.float(), map_ids, i_ids, win=win)
    out = ops.fine_windows_batch(ffg, map_ids.to(gpu), i_ids.to(gpu), cnt, win, 4)
    assert torch.equal(out.cpu(), ref)
    out0 = ops.fine_windows(ffg[1].contiguous(), i_ids.to(gpu), cnt, win, 4)
    assert torch.equal(out0.cpu(), mo.fine_windows(ff.float(), torch.ones_like(i_ids), i_ids, win=win))


@pytest.mark.parametrize("win", range(2, 9))
def test_fine_windows_bwd_vs_fold(gpu, built_lib, win):
    """nm_fine_windows_bwd: the scatter-add of window gradients equals the float64 gradient of the unfold gather (corners repeated: the
    atomics overlap)."""
    ff, _, i_ids = _window_case(win, B=1)
    K = len(i_ids)
    dwin = rnd(K, win * win, ff.shape[1], seed=7).double()
    x = ff.clone().requires_grad_()
    with torch.enable_grad():
        mo.fine_windows(x, torch.zeros_like(i_ids), i_ids, win=win).backward(dwin)
    cnt = torch.tensor([K], dtype=torch.int32, device=gpu)
    d = ops.fine_windows_bwd(dwin.float().to(gpu), tuple(ff.shape[1:]), i_ids.to(gpu), cnt, win, 4)
    assert (d.cpu().double() - x.grad[0]).abs().max().item() < 1e-5


def _expectation64(pt, win_f, win):
    C = pt.shape[-1]
    sim = torch.einsum("kc,krc->kr", pt, win_f) / C**0.5
    p = torch.softmax(sim, 1)
    lin = torch.linspace(-1, 1, win, dtype=torch.float64)
    gx, gy = lin.repeat(win), lin.repeat_interleave(win)
    ex, ey = (p * gx).sum(1), (p * gy).sum(1)
    vx, vy = (p * gx * gx).sum(1) - ex * ex, (p * gy * gy).sum(1) - ey * ey
    return torch.stack([ex, ey, vx.clamp_min(1e-10).sqrt() + vy.clamp_min(1e-10).sqrt()], 1)


def _expectation_raw(pt, win_f, count, max_k, win, out):
    """nm_fine_expectation on a caller-filled output: the slots the kernel must not write stay visible."""
    _lib.check(_lib.lib().nm_fine_expectation(_lib.dptr(pt), _lib.dptr(win_f), _lib.dptr(count, torch.int32), max_k, win, pt.shape[1],
                                              _lib.dptr(out), _lib.stream()), "nm_fine_expectation")


def _expectation_bwd_raw(pt, win_f, d_e, count, max_k, win, d_pt, d_win):
    _lib.check(_lib.lib().nm_fine_expectation_bwd(_lib.dptr(pt), _lib.dptr(win_f), _lib.dptr(d_e), _lib.dptr(count, torch.int32), max_k, win,
                                                  pt.shape[1], _lib.dptr(d_pt), _lib.dptr(d_win), _lib.stream()), "nm_fine_expectation_bwd")


@pytest.mark.parametrize("C", [16, 128, 256])
@pytest.mark.parametrize("win", range(2, 9))
def test_fine_expectation_vs_float64(gpu, built_lib, win, C):
    """nm_fine_expectation / _bwd against float64 (scores / sqrt(C), soft-max, linspace(-1, 1, win) grid, std): K = 39 matches (not a
    multiple of the 4 per block), *count = 30 < max_k -- the slots past *count keep the caller's sentinel."""
    K, cnt_v, ww = 39, 30, win * win
    pt, wf = rnd(K, C, seed=1).double(), rnd(K, ww, C, seed=2).double()
    pt[3] *= 4.0  # (a peaked window: one position dominates)
    ref = _expectation64(pt, wf, win)
    ptg, wfg = pt.float().to(gpu), wf.float().to(gpu)
    cnt = torch.tensor([cnt_v], dtype=torch.int32, device=gpu)
    out = torch.full((K, 3), 7.5, device=gpu)
    _expectation_raw(ptg, wfg, cnt, K, win, out)
    out = out.cpu()
    # (the peaked row's scores, |pt| x 4, are C-term fp32 dot products of magnitude up to ~50: their rounding, ~1e-6 relative in the
    # kernel's summation order, moves that window's expectation by ~1e-6; a 1 / sqrt(128) scale at C = 16 / 256 moves it by > 1e-2)
    assert (out[:cnt_v].double() - ref[:cnt_v]).abs().max().item() < 4e-6
    assert bool((out[cnt_v:] == 7.5).all())
    # backward: gradients of sum(expec * d_e) through the float64 expression
    d_e = rnd(K, 3, seed=3).double()
    x, y = pt.clone().requires_grad_(), wf.clone().requires_grad_()
    with torch.enable_grad():
        (_expectation64(x, y, win) * d_e).sum().backward()
    d_pt, d_win = torch.full((K, C), 7.5, device=gpu), torch.full((K, ww, C), 7.5, device=gpu)
    _expectation_bwd_raw(ptg, wfg, d_e.float().to(gpu), cnt, K, win, d_pt, d_win)
    d_pt, d_win = d_pt.cpu(), d_win.cpu()
    assert rel(d_pt[:cnt_v], x.grad[:cnt_v], 1e-2) < 1e-5 and rel(d_win[:cnt_v], y.grad[:cnt_v], 1e-2) < 1e-5
    assert bool((d_pt[cnt_v:] == 7.5).all()) and bool((d_win[cnt_v:] == 7.5).all())
    # ops wrappers (count = K): the same numbers
    full = torch.tensor([K], dtype=torch.int32, device=gpu)
    assert (ops.fine_expectation(ptg, wfg, full, win).cpu().double() - ref).abs().max().item() < 4e-6


@pytest.mark.parametrize("win", range(2, 9))
def test_fine_expectation_grid(gpu, built_lib, win):
    """A window whose soft-max is one-hot returns that position's grid value: linspace(-1, 1, win) to the rounding of its fp32 step (an
    ulp of the value for win <= 6; the inexact 1/3 and 2/7 steps of win 7 / 8 leave up to ~7e-8)."""
    C, ww = 16, win * win
    tol = 3e-8 if win <= 6 else 1e-7
    lin = torch.linspace(-1, 1, win, dtype=torch.float64)
    pt = torch.full((ww, C), 6.0)
    wf = torch.zeros(ww, ww, C)
    wf[torch.arange(ww), torch.arange(ww)] = 6.0  # match r: score 144 at position r, 0 elsewhere (exp(-144) is 0 in fp32)
    cnt = torch.tensor([ww], dtype=torch.int32, device=gpu)
    out = ops.fine_expectation(pt.to(gpu), wf.to(gpu), cnt, win).cpu().double()
    r = torch.arange(ww)
    assert (out[:, 0] - lin[r % win]).abs().max().item() <= tol
    assert (out[:, 1] - lin[r // win]).abs().max().item() <= tol


# ----------------------------------------------------------------------------- more than 65,535 windows in one launch
def _attn64(q, k, v, H, scale):
    B, L, C = q.shape
    D = C // H
    sc = torch.einsum("blhd,bshd->blsh", q.view(B, L, H, D) * scale, k.view(B, -1, H, D))
    return torch.einsum("blsh,bshd->blhd", torch.softmax(sc, 2), v.view(B, -1, H, D)).reshape(B, L, C)


def test_small_attention_beyond_65535_windows(gpu, built_lib):
    """The small-window attention (forward and backward) is launched with the window count on a grid axis: 70,001 windows of 25 tokens,
    8 heads of 16 -- windows 0, 65,534, 65,535, 65,536 and the last one against float64."""
    B, L, H, D = 70_001, 25, 8, 16
    g = torch.Generator(device=gpu).manual_seed(3)
    q, k, v, d_o = (torch.randn(B, L, H * D, device=gpu, generator=g) for _ in range(4))
    scale = D**-0.5
    o = ops.attention(q, k, v, H, scale)
    dq, dk, dv = ops.attention_bwd(q, k, v, o, d_o, H, scale)
    torch.cuda.synchronize()
    idx = torch.tensor([0, 65_534, 65_535, 65_536, B - 1], device=gpu)
    qs, ks, vs, ds = (t[idx].cpu().double().requires_grad_() for t in (q, k, v, d_o))
    with torch.enable_grad():
        ref = _attn64(qs, ks, vs, H, scale)
        ref.backward(ds)
    assert (o[idx].cpu().double() - ref).abs().max().item() < 2e-5
    assert rel(dq[idx], qs.grad, 0.1) < 2e-5 and rel(dk[idx], ks.grad, 0.1) < 2e-5 and rel(dv[idx], vs.grad, 0.1) < 2e-5


def test_generic_fine_stage_beyond_65535_matches(gpu, built_lib, monkeypatch):
    """The whole generic fine stage (fp32, FINE_LAYER_FUSED off) on 70,001 matches of one pair: sampled matches against the oracle."""
    monkeypatch.setattr(ops, "FINE_LAYER_FUSED", False)
    cfg = synth.matcher_config("c2f")
    sd = synth.matcher_state_dict("c2f", seed=4)
    model = NeRFMatcherMS(cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(gpu).eval()
    h, w, N, K = 12, 16, 300, 70_001
    g = torch.Generator().manual_seed(9)
    pt_c = torch.randn(1, N, 256, generator=g)
    ffeat = torch.randn(1, 128, 4 * h, 4 * w, generator=g)
    i_ids = torch.randint(0, h * w, (K,), generator=g)
    j_ids = torch.randint(0, N, (K,), generator=g)
    b_ids = torch.zeros(K, dtype=torch.int64)
    cnt = torch.tensor([K], dtype=torch.int32, device=gpu)
    expec = model._fine_stage(pt_c.to(gpu), ffeat.to(gpu), b_ids.to(gpu), i_ids.to(gpu), j_ids.to(gpu), cnt).cpu()
    assert expec.shape == (K, 3)
    sel = torch.tensor([0, 1, 65_534, 65_535, 65_536, 65_537, K - 1])
    pf = torch.nn.functional.linear(pt_c[0], sd["pt_ffeat_proj.0.weight"], sd["pt_ffeat_proj.0.bias"])
    pf = torch.nn.functional.linear(pf, sd["pt_ffeat_proj.1.weight"], sd["pt_ffeat_proj.1.bias"])
    win = mo.self_attention_block(sd, "fine_sa", mo.fine_windows(ffeat, b_ids[sel], i_ids[sel]), 1, heads=8)
    ref = mo.fine_matching(pf[j_ids[sel]], win)
    assert (expec[sel] - ref).abs().max().item() < 1e-5
