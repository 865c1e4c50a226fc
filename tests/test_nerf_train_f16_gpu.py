"""GPU: the fp16 mixed-precision NeRF training mode (NerfRenderer.train_precision = "f16") -- its chain GEMM and
weight-gradient kernels pointwise against float64 of the fp16-rounded operands with derived bounds, loud overflow, the fp16 encode, the whole
step against the float64 emulation of its own arithmetic (tests/nerf_train_f16_util.py), chunking, and the trainer's loss scaling.

Tens of rays and at most 300 rows everywhere: the kernels' tiles are 128 rows (chain GEMM) and 64-row stages (weight gradient), so 257 rows
and 3 slices + 5 rows cross every boundary they have."""
from argparse import Namespace

import pytest
import torch

import nerf_train_f16_util as f16u
import nerf_train_util as ntu
from nerfmatch_amd import ops, synth
from test_nerf_train_gpu import R, draws_for, gpu_step, make_rays, rel, renderer_for, scene, sorted_t

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
MS_ROWS = (1, 127, 128, 129, 257)


def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------- chain GEMM
# (name, K, K2, N, transposed, relu, bias, residual, gate, alpha, out): every shape the walk launches, every epilogue form
CHAIN = [
    ("layer0", 96, 0, 256, False, True, True, False, False, 1.0, F16),
    ("hidden", 256, 0, 256, False, True, True, False, False, 1.0, F16),
    ("skip", 256, 96, 256, False, True, True, False, False, 1.0, F16),
    ("density", 256, 0, 8, False, False, True, False, False, 1.0, F32),
    ("feature", 256, 0, 256, False, False, True, False, False, 1.0, F16),
    ("views", 256, 48, 128, False, True, True, False, False, 1.0, F16),
    ("rgb", 128, 0, 8, False, False, True, False, False, 1.0, F32),
    ("d_rgb", 8, 0, 128, True, False, False, False, True, 1.0, F16),
    ("d_density", 8, 0, 256, True, False, False, False, False, 1.0, F16),
    ("d_views_feat", 128, 0, 256, True, False, False, False, False, 1.0, F16),
    ("d_feature", 256, 0, 256, True, False, False, True, True, 1.0, F16),
    ("d_hidden", 256, 0, 256, True, False, False, False, True, 1.0, F16),
    ("d_views_xd", 128, 0, 48, True, False, False, False, False, 2.0 ** -16, F32),
]


def chain_case(K, K2, N, transposed, relu, bias, residual, gate, alpha, out, seed=0):
    """257 rows and the float64 result of the fp16-rounded operands with its pointwise bound (test_convformer_f16_gpu.linear_case's):
      accumulator (bias its start value)   |v^ - v| <= (K + K2 + 8) 2^-24 (sum |a||w| + |bias| + |res|)   (relu is 1-Lipschitz; the residual
                                                                                                         add is one more rounding)
      gate and alpha (a power of two)      exact: both sides are multiplied
      fp16 output                          + 2^-11 |ref| + 2^-25                                          (one rounding; half a subnormal step)"""
    M = 257
    x = randn((M, K), 10 + seed).to(F16)
    w = randn((K, N) if transposed else (N, K), 20 + seed) / (K + K2) ** 0.5
    x2 = randn((M, K2), 50 + seed).to(F16) if K2 else None
    w2 = randn((N, K2), 60 + seed) / (K + K2) ** 0.5 if K2 else None
    b = randn((N,), 30 + seed) if bias else None
    res = randn((M, N), 40 + seed).to(F16) if residual else None
    gt = torch.relu(randn((M, N), 70 + seed)).to(F16) if gate else None
    wd = w.to(F16).double()
    wd = wd if transposed else wd.t()
    v, mag = x.double() @ wd, x.double().abs() @ wd.abs()
    if K2:
        v, mag = v + x2.double() @ w2.to(F16).double().t(), mag + x2.double().abs() @ w2.to(F16).double().abs().t()
    if bias:
        v, mag = v + b.double(), mag + b.double().abs()
    if relu:
        v = v.clamp_min(0)
    if residual:
        v, mag = v + res.double(), mag + res.double().abs()
    bound = (K + K2 + 8) * 2.0 ** -24 * mag
    if gate:
        open_ = gt.double() > 0
        v, bound = v * open_, bound * open_
    v, bound = alpha * v, alpha * bound
    if out == F16:
        bound = bound + 2.0 ** -11 * v.abs() + 2.0 ** -25
    return dict(x=x, w=w, x2=x2, w2=w2, b=b, res=res, gate=gt), v, bound


@pytest.mark.parametrize("name,K,K2,N,transposed,relu,bias,residual,gate,alpha,out", CHAIN, ids=[c[0] for c in CHAIN])
def test_chain_gemm_against_float64(gpu, built_lib, name, K, K2, N, transposed, relu, bias, residual, gate, alpha, out):
    """Pointwise inside the derived bound at 257 rows; a row's result is the same bits for every M and at another place in its tile (rows
    129.. handed over as rows 0..); the gate closes exactly; no overflow event."""
    c, ref, bound = chain_case(K, K2, N, transposed, relu, bias, residual, gate, alpha, out)
    d = {k: None if v is None else v.to(gpu) for k, v in c.items()}
    events = ops.f16_events(gpu)

    def run(lo, hi):
        cut = lambda t: None if t is None else t[lo:hi]
        return ops.linear_chain_f16(cut(d["x"]), d["w"], d["b"], x2=cut(d["x2"]), weight2=d["w2"], relu=relu, residual=cut(d["res"]),
                                    gate=cut(d["gate"]), alpha=alpha, transposed=transposed, out_dtype=out, events=events)

    full = run(0, 257)
    assert full.dtype == out and full.shape == (257, N)
    err = (full.double().cpu() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0 else 0.0
    print(f"chain {name}: worst error / bound {worst:.3f}, max |ref| {float(ref.abs().max()):.3g}")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float(ref.abs().max()) > 0
    if gate:
        closed = (c["gate"] <= 0)
        assert closed.any() and not full.cpu()[closed].any()
    for M in MS_ROWS:
        assert torch.equal(run(0, M), full[:M]), M
    assert torch.equal(run(129, 257), full[129:257])
    assert int(events.item()) == 0


def test_chain_gemm_overflow_is_loud(gpu, built_lib):
    """A dX product beyond 65504 is stored as +-inf and counted, once per stored value; the same product with fp32 output is finite and is
    not counted."""
    dy = torch.ones(5, 8, dtype=F16)
    dy[0], dy[1] = 100.0, -100.0
    w = torch.full((8, 128), 100.0)  # stored (N_out = 8, K_in = 128): row 0 of dy . w = 8 x 100 x 100 = 80000
    events = ops.f16_events(gpu)
    y = ops.linear_chain_f16(dy.to(gpu), w.to(gpu), transposed=True, events=events).cpu()
    assert torch.isposinf(y[0]).all() and torch.isneginf(y[1]).all() and torch.equal(y[2:], torch.full((3, 128), 800.0, dtype=F16))
    assert int(events.item()) == 2 * 128
    y32 = ops.linear_chain_f16(dy.to(gpu), w.to(gpu), transposed=True, out_dtype=F32, events=events).cpu()
    assert torch.equal(y32[:2], torch.tensor([[80000.0], [-80000.0]]).expand(2, 128)) and int(events.item()) == 2 * 128
    # a residual that already is infinite is not a new event: the value that is rounded is not finite itself
    res = torch.zeros(5, 128, dtype=F16)
    res[3, 7] = float("inf")
    ev2 = ops.f16_events(gpu)
    y = ops.linear_chain_f16(torch.ones(5, 8, dtype=F16, device=gpu), w.to(gpu), transposed=True, residual=res.to(gpu), events=ev2).cpu()
    assert torch.isposinf(y[3, 7]) and int(ev2.item()) == 0


# ------------------------------------------------------------------------------------------------------------------- weight gradient
WGRAD_PAIRS = [(8, 128), (8, 256), (128, 256), (128, 48), (256, 256), (256, 96)]  # every (N, K) of the chain's dW launches


@pytest.mark.parametrize("N,K", WGRAD_PAIRS)
def test_wgrad_against_float64(gpu, built_lib, N, K):
    """dw = alpha dy^T x and db = alpha column sums of dy against float64 of the fp16 operands:
      |dw^ - dw| <= (M + 8) 2^-24 |alpha| sum |dy||x|   (fp32 accumulation of exact products, in the MFMA and over the slices' partials; db: x = 1)
      accumulate: + 2^-24 |out|                          (the add onto the fp32 output is one more rounding)
    dy and x are the leading M rows of tensors whose following rows hold 1e4: a row read past M shows in every sum.  M crosses the 8-row
    operand columns, the 16-row K-steps, the 64-row stage and the slice (one workgroup's rows)."""
    slice_rows = ops.linear_wgrad_f16_slice_rows(1)
    MS = (1, 7, 8, 9, 31, 32, 33, slice_rows - 1, slice_rows, slice_rows + 1, 3 * slice_rows + 5)
    assert slice_rows % 64 == 0 and MS[-1] <= 300 and all(ops.linear_wgrad_f16_slice_rows(M) == slice_rows for M in MS)
    top = MS[-1]
    dy_all, x_all = randn((top, N), N + K).to(F16), randn((top, K), N + K + 1).to(F16)
    poison = lambda t, M: torch.cat([t[:M], torch.full((64, t.shape[1]), 1e4, dtype=F16)]).to(gpu)
    w0, b0 = randn((N, K), 5).to(gpu), randn((N,), 6).to(gpu)
    worst = 0.0
    for M in MS:
        dy_big, x_big = poison(dy_all, M), poison(x_all, M)
        dy, x = dy_big[:M], x_big[:M]
        dyd, xd = dy_all[:M].double(), x_all[:M].double()
        for alpha in (1.0, 2.0 ** -16):
            ref_w, ref_b = alpha * dyd.t() @ xd, alpha * dyd.sum(0)
            bw = (M + 8) * 2.0 ** -24 * alpha * (dyd.abs().t() @ xd.abs())
            bb = (M + 8) * 2.0 ** -24 * alpha * dyd.abs().sum(0)
            dw, db = ops.linear_wgrad_f16(dy, x, alpha=alpha)
            again = ops.linear_wgrad_f16(dy, x, alpha=alpha)
            assert torch.equal(dw, again[0]) and torch.equal(db, again[1]), (M, alpha)
            ew, eb = (dw.double().cpu() - ref_w).abs(), (db.double().cpu() - ref_b).abs()
            assert bool((ew <= bw).all()) and bool((eb <= bb).all()), (M, alpha, float((ew - bw).max()), float((eb - bb).max()))
            worst = max(worst, float((ew / bw.clamp_min(1e-300)).max()), float((eb / bb.clamp_min(1e-300)).max()))
            out = (w0.clone(), b0.clone())
            got = ops.linear_wgrad_f16(dy, x, out=out, alpha=alpha)
            assert got[0] is out[0] and got[1] is out[1]
            tw, tb = w0.double().cpu() + ref_w, b0.double().cpu() + ref_b
            ew, eb = (out[0].double().cpu() - tw).abs(), (out[1].double().cpu() - tb).abs()
            assert bool((ew <= bw + 2.0 ** -24 * tw.abs()).all()) and bool((eb <= bb + 2.0 ** -24 * tb.abs()).all()), (M, alpha, "accumulate")
            only_w = ops.linear_wgrad_f16(dy, x, alpha=alpha, bias=False)
            assert only_w[1] is None and torch.equal(only_w[0], dw)
    print(f"wgrad N={N} K={K}: worst error / bound {worst:.3f} over M in {MS}")


# ------------------------------------------------------------------------------------------------------------------- encode
@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("app", [False, True])
def test_encode_f16_is_the_fp32_kernel_rounded(gpu, built_lib, S, app):
    from nerfmatch_amd.nerf import train_render as tr

    g = torch.Generator().manual_seed(S + app)
    rays, t = make_rays(R, 9).to(gpu), sorted_t(R, S, g, 0.01, 0.9).to(gpu)
    ids = torch.randint(0, 5, (R,), generator=g).to(gpu) if app else None
    table = torch.randn(5, 16, generator=g).to(gpu) if app else None
    xi, xd = tr.encode(rays, t, ids, table)
    xi16, xd16 = tr.encode(rays, t, ids, table, dtype=F16)
    assert xi16.dtype == xd16.dtype == F16 and xi16.shape == (R * S, 96) and xd16.shape == (R * S, 48)
    assert torch.equal(xi16, xi.to(F16)) and torch.equal(xd16, xd.to(F16))
    assert bool(xd16[:, 27:43].any()) == app


# ------------------------------------------------------------------------------------------------------------------- the whole step
def f16_step(gpu, app, S, seed=17):
    cfg, sd = scene(app)
    ren = renderer_for(cfg, sd, gpu, app, S)
    ren.train_precision = "f16"
    g = torch.Generator().manual_seed(seed + S)
    n = 48
    rays, gt = make_rays(n, 11), torch.rand(n, 3, generator=g)
    ids = mask = None
    if app:
        ids = torch.randint(0, 4, (n,), generator=g)
        ids[ids == 2] = 4
        mask = torch.rand(n, 1, generator=g)
    return cfg, sd, ren, rays, gt, ids, mask, draws_for(n, S, 23)


@pytest.mark.parametrize("app,S", [(False, 32), (True, 32), (True, 64)])
def test_f16_training_step_vs_emulation(gpu, built_lib, app, S):
    """The whole "f16" step (48 rays; render with draws given, losses, backward at loss scale 65536) against the fp64 helper, measured with
    the float64 EMULATION of the walk's arithmetic as the yardstick: d_e = the emulation's whole-network relative L2 gradient distance to
    the unrounded fp64 helper, computed here for the same inputs and the kernels' own fence posts.  The kernels' distance to the fp64 helper
    must be <= 1.5 d_e per network and for the appearance table (the margin: fp32 accumulation and the rare stored value that rounds the
    other way; a wrong layer costs O(1)); the same rule for the preds (max error of scale).  No number is fixed beforehand.
    Measured on an MI355X, 2026-10-21 (d_e / kernels to fp64 / kernels to the emulation; the table of DESIGN.md 3.8l):
      app=False S=32   coarse 2.644e-3 / 2.644e-3 / 5.3e-5   fine 3.446e-3 / 3.445e-3 / 1.3e-4
      app=True  S=32   coarse 1.680e-3 / 1.680e-3 / 3.0e-5   fine 2.473e-3 / 2.473e-3 / 4.2e-5   table 1.898e-3 / 1.898e-3 / 1.4e-6
      app=True  S=64   coarse 4.624e-4 / 4.702e-4 / 1.0e-4   fine 2.829e-3 / 2.841e-3 / 2.7e-4   table 2.801e-3 / 2.725e-3 / 3.5e-4
    preds: colours 2.0e-5 ... 3.4e-5 of scale, depths and weights 1e-6 ... 6e-6, 0.89 ... 1.21 x the emulation's; loss within 2.1e-6 of fp64."""
    cfg, sd, ren, rays, gt, ids, mask, draws = f16_step(gpu, app, S)
    preds, metrics, grads = gpu_step(ren, rays, gt, draws, ids, mask, cfg.loss, gpu)
    assert ren.train_overflow_events() == (0, 0)
    assert all(g.dtype == F32 for g in grads.values())
    kw = dict(noise_coarse=draws["noise_coarse"], noise_fine=draws["noise_fine"], noise_std=1.0, white_bg=app, ray_id=ids, mask=mask,
              ray_reg_weight=cfg.loss.ray_reg_weight, t_coarse=preds["t_coarse"].cpu(), t_fine=preds["t_fine"].cpu())
    ref = ntu.train_step(sd, rays, gt, **kw)
    emu = f16u.train_step(sd, rays, gt, scale=ren.train_loss_scale, **kw)
    for k in ("rgb_coarse", "rgb_fine", "depth_coarse", "depth_fine", "weights_fine"):
        e, e_emu = rel(preds[k], ref["preds"][k]), rel(emu["preds"][k], ref["preds"][k])
        print(f"  {k}: kernels {e:.2e}  emulation {e_emu:.2e}  kernels to emulation {rel(preds[k], emu['preds'][k]):.2e}")
        assert e <= 1.5 * e_emu, (k, e, e_emu)
    assert rel(preds["s_fine"], ref["preds"]["s_fine"]) < 1e-4  # (no MLP in it: test_training_step_vs_fp64_helper's bar)
    e_loss = abs(float(metrics["loss"]) - float(ref["loss"])) / float(ref["loss"])
    print(f"  loss {float(metrics['loss']):.6f} vs fp64 {float(ref['loss']):.6f} ({e_loss:.2e}), emulation {float(emu['loss']):.6f}")
    nets = list(ntu.NETS) + (["embedding_a"] if app else [])
    for n in nets:
        d_e, d_k, d_ke = ntu.net_l2(emu["grads"], ref["grads"], n), ntu.net_l2(grads, ref["grads"], n), ntu.net_l2(grads, emu["grads"], n)
        print(f"f16 step app={app} S={S} {n}: d_e {d_e:.3e}  kernels to fp64 {d_k:.3e}  kernels to emulation {d_ke:.3e}")
        assert d_e > 0 and d_k <= 1.5 * d_e, (n, d_k, d_e)
    for k, gr in ref["grads"].items():
        assert float(gr.abs().max()) > 0 and grads[k].shape == gr.shape, k
    if app:
        assert not grads["embedding_a.weight"][2].any()
        assert all(grads["embedding_a.weight"][i].abs().max() > 0 for i in (0, 1, 3, 4))


def test_f16_chunked_step_matches_one_chunk(gpu, built_lib):
    """Three chunks of 16 rays (the last ragged: 37 rays) against one chunk: the forward rows do not depend on the chunking, the weight
    gradients are summed in another order: preds at 1e-5 of scale, gradients within 1e-5 whole-network L2 (test_chunked_step_matches_one_chunk's bars)."""
    cfg, sd = scene(True)
    g = torch.Generator().manual_seed(5)
    rays, gt, ids, mask = make_rays(R, 13), torch.rand(R, 3, generator=g), torch.randint(0, 5, (R,), generator=g), torch.rand(R, 1, generator=g)
    draws = draws_for(R, 32, 29)
    out = []
    for chunk in (None, 16):
        ren = renderer_for(cfg, sd, gpu, True, 32)
        ren.train_precision, ren.train_chunk_rays = "f16", chunk
        out.append(gpu_step(ren, rays, gt, draws, ids, mask, cfg.loss, gpu))
        assert ren.train_overflow_events() == (0, 0)
    (p1, m1, g1), (p2, m2, g2) = out
    assert all(rel(p2[k], p1[k]) < 1e-5 for k in p1), {k: rel(p2[k], p1[k]) for k in p1}
    dist = {n: ntu.net_l2(g2, g1, n) for n in list(ntu.NETS) + ["embedding_a"]}
    print("f16, chunk of 16 rays against one chunk: " + "  ".join(f"{k} {v:.2e}" for k, v in dist.items()))
    assert all(v < 1e-5 for v in dist.values()), dist


# ------------------------------------------------------------------------------------------------------------------- trainer
NEW_ENTRY_POINTS = ("nm_linear_pack_t_f16", "nm_linear_chain_f16", "nm_linear_wgrad_f16", "nm_linear_wgrad_f16_workspace_bytes",
                    "nm_nerf_g4_split_f16", "nm_nerf_train_encode_f16")


def trainer_and_batch(gpu, precision):
    from nerfmatch_amd.nerf_trainer import NerfTrainer

    cfg, sd = scene(True)
    cfg.optim = Namespace(optimizer="adam", lr=5e-4, weight_decay=0.0, lr_scheduler=None)
    cfg.train_precision = precision
    tr = NerfTrainer(cfg, num_frames=5, device=gpu)
    tr.model.load_state_dict(sd)
    n = 64
    g = torch.Generator().manual_seed(41)
    batch = dict(rays=make_rays(n, 15, scale=1.0)[None].to(gpu), rgbs=torch.rand(1, n, 3, generator=g).to(gpu), ts=torch.randint(0, 5, (1, n), generator=g),
                 mask=torch.rand(n, 1, generator=g).to(gpu), seq_ind=[1], img_idx=[0], img_wh=torch.tensor([[8, 8]]))
    return tr, batch, {k: v.to(gpu) for k, v in draws_for(n, 32, 47).items()}


def test_f16_trainer_steps_and_skipped_step(gpu, built_lib, tmp_path):
    """Three "f16" steps: finite loss, the parameters move, fp32 .grad, the checkpoint loads back.  Then the loss scale forced to 2^40: the
    gradient rows overflow, the step is skipped -- parameters and optimiser state bit-identical --, counted, and the scale halved."""
    from nerfmatch_amd.nerf_evaluator import load_nerf_render_from_ckpt

    tr, batch, draws = trainer_and_batch(gpu, "f16")
    assert tr.model.train_precision == "f16" and tr.loss_scale == 65536.0 and tr.skipped_steps == 0 and tr.overflow_events == (0, 0)
    trained = lambda: [(k, p) for k, p in tr.model.named_parameters() if p.requires_grad]  # (the encoders' frequency tables are int64 constants)
    before = {k: v.detach().clone() for k, v in trained()}
    assert len(before) == 2 * 24 + 1
    losses = [float(tr.training_step(batch, i, **draws)["loss"]) for i in range(3)]
    print("f16 losses of three steps:", losses, " skipped", tr.skipped_steps, " scale", tr.loss_scale, " events", tr.overflow_events)
    assert all(torch.isfinite(torch.tensor(losses))) and tr.skipped_steps == 0 and tr.overflow_events == (0, 0) and tr.loss_scale == 65536.0
    assert losses[-1] < losses[0]
    for k, p in trained():
        assert p.dtype == F32 and p.grad is not None and p.grad.dtype == F32 and torch.isfinite(p.grad).all(), k
        assert not torch.equal(p.detach(), before[k]), k
    tr.save_checkpoint(tmp_path / "scene.ckpt")
    fresh = load_nerf_render_from_ckpt(tmp_path / "scene.ckpt", gpu)
    have = tr.model.state_dict()
    for k, v in fresh.state_dict().items():
        assert v.dtype == have[k].dtype and torch.equal(v, have[k]), k

    tr.loss_scale = 2.0 ** 40
    params = {k: v.detach().clone() for k, v in tr.model.named_parameters()}
    state = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in tr.optimizer.state_dict()["state"].items()}
    assert len(state) > 0
    out = tr.training_step(batch, 3, **draws)
    assert torch.isfinite(out["loss"])  # (the forward pass does not see the scale)
    assert tr.skipped_steps == 1 and tr.loss_scale == 2.0 ** 39 and tr.overflow_events[0] == 0 and tr.overflow_events[1] > 0
    for k, p in tr.model.named_parameters():
        assert torch.equal(p.detach(), params[k]), k
    after = tr.optimizer.state_dict()["state"]
    assert set(after) == set(state)
    for i, st in after.items():
        for k, v in st.items():
            assert torch.equal(v, state[i][k]) if torch.is_tensor(v) else v == state[i][k], (i, k)


def test_same_precision_never_touches_the_f16_entry_points(gpu, built_lib, monkeypatch):
    from nerfmatch_amd import _lib

    def boom(*a, **kw):
        raise AssertionError("an fp16 training entry point was called under train_precision='same'")

    for name in NEW_ENTRY_POINTS:
        monkeypatch.setattr(_lib.lib(), name, boom)
    for name in ("linear_chain_f16", "linear_wgrad_f16"):
        monkeypatch.setattr(ops, name, boom)
    tr, batch, draws = trainer_and_batch(gpu, "same")
    before = {k: v.detach().clone() for k, v in tr.model.named_parameters()}
    loss = float(tr.training_step(batch, 0, **draws)["loss"])
    assert loss == loss and tr.skipped_steps == 0 and tr.loss_scale == 65536.0 and tr.overflow_events == (0, 0)
    assert any(not torch.equal(p.detach(), before[k]) for k, p in tr.model.named_parameters())
    tr.model.train_precision = "f16"  # the patch is live: the same trainer under "f16" does call them
    with pytest.raises(AssertionError, match="fp16 training entry point"):
        tr.training_step(batch, 1, **draws)
