#!/usr/bin/env python3
"""Golden vectors of one NeRF TRAINING step (tests/golden/nerf_train_7s.npz, nerf_train_cam.npz), from the REFERENCE's own NerfRenderer in
training mode, compute_nerf_metrics and backward().

    python tests/golden/make_golden_nerf_train.py        # rewrites the two files (NM_GOLDEN_OUT=<dir>: elsewhere)

Needs the reference tree (make_golden.py's REF and stub modules).  Only arrays are written.

  nerf_train_7s   no appearance embedding, black background, no mask
  nerf_train_cam  appearance embedding (V = 5, per-ray ids), white background, loss mask
R = 37 rays with rays[:, 3:6] = 1.3 x rays[:, 8:11] (direction and view direction cannot be confused), S = 32, noise_std = 1,
ray_reg_weight = 0.01 (synth.nerf_config: the values of the shipped yamls).

The four random draws of the step are captured by replaying the seeded global generator in the reference's order -- coarse torch.rand
(render_utils.py:444), coarse randn_like (:190), the resampler's uniform_ (:483), fine randn_like -- and the replay is checked: the helper
(tests/nerf_train_util.py) fed with the captured draws must reproduce the reference's preds.

Seed choice: a training step's gradient is discontinuous where a ReLU or the density gate raw + noise sits at a rounding boundary, and a
fixture recorded there could not be compared per tensor.  The script scans seeds (weights and draws) from 0 and keeps the first one for
which the fp32-vs-fp64 per-tensor distance of the helper's own gradients is <= 1e-5, i.e. no gate flips under rounding; that distance is
recorded (`ref_fp32_vs_fp64`).

Stored: inputs, draws, every pred, the loss and metrics; gradients in full for the biases, the heads and the table (g_<name>), and for the
256-wide matrices the fixed strided subsample gsub_<name> = flat[::sub_stride] plus the norm gnorm_<name>."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import make_golden as mg  # noqa: E402
import nerf_train_util as ntu  # noqa: E402
from nerfmatch_amd import synth  # noqa: E402

R, S, STRIDE = 37, 32, 29
FULL = ("bias", "alpha_linear.weight", "rgb_linear.weight", "embedding_a.weight")


def inputs(seed, app):
    g = np.random.default_rng(4000 + seed)
    o = (g.random((R, 3)) - 0.5) * 0.4
    v = g.standard_normal((R, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    od = (o * v).sum(1, keepdims=True)
    far = np.sqrt(od * od + 1.0 - (o * o).sum(1, keepdims=True)) - od
    rays = np.concatenate([o, 1.3 * v, np.full((R, 1), 0.01), far / 1.3, v, np.full((R, 1), 2.0 / np.sqrt(12.0) / 525.0)], 1).astype(np.float32)
    fx = dict(rays=torch.from_numpy(rays), rgbs=torch.from_numpy(g.random((R, 3)).astype(np.float32)))
    if app:
        fx["ray_id"] = torch.from_numpy(g.integers(0, 5, R))
        fx["mask"] = torch.from_numpy(g.random((R, 1)).astype(np.float32))
    return fx


def draws(rng_seed):
    torch.manual_seed(rng_seed)
    t_rand = torch.rand(R, S + 1)
    noise_c = torch.randn(R, S)
    jitter = torch.empty(R, S + 1).uniform_(to=(1 / (S + 1) - torch.finfo(torch.float32).eps))
    noise_f = torch.randn(R, S)
    return dict(t_rand=t_rand, noise_coarse=noise_c, jitter=jitter, noise_fine=noise_f)


def helper_step(sd, fx, dr, cfg, app, dtype):
    return ntu.train_step(sd, fx["rays"], fx["rgbs"], noise_std=1.0, white_bg=app, ray_id=fx.get("ray_id"), mask=fx.get("mask"),
                          ray_reg_weight=cfg.loss.ray_reg_weight, dtype=dtype, **dr)


def fixture(tag, app):
    from nerfmatch.nerf.renderer import NerfRenderer
    from nerfmatch.utils.metrics import compute_nerf_metrics

    cfg = synth.nerf_config("cambridge" if app else "7scenes", num_pts=S, img_wh=(8, 8))
    for seed in range(64):
        sd = synth.nerf_state_dict(seed=seed, app_vocab=5 if app else 0, density_bias=3.0)
        fx, dr = inputs(seed, app), draws(2000 + seed)
        h32, h64 = helper_step(sd, fx, dr, cfg, app, torch.float32), helper_step(sd, fx, dr, cfg, app, torch.float64)
        dist = max(float((h32["grads"][k].double() - g).abs().max() / g.abs().max()) for k, g in h64["grads"].items())
        print(f"{tag}: seed {seed}: helper fp32 vs fp64, worst per-tensor distance {dist:.2e}")
        if dist <= 1e-5:
            break
    else:
        raise SystemExit("no flip-free seed found")
    assert all(float(g.abs().max()) > 0 for g in h64["grads"].values())
    torch.set_grad_enabled(True)
    ren = NerfRenderer(cfg, num_frames=5 if app else None, training=True)
    ren.load_state_dict(sd, strict=True)
    ren.ret_pfeat = False
    ren.set_training_mode(True)
    torch.manual_seed(2000 + seed)
    preds = ren.forward(fx["rays"].clone(), ray_id=fx.get("ray_id"))
    metrics = compute_nerf_metrics(preds, fx["rgbs"], mask_loss=fx.get("mask"), cnfg_loss=cfg.loss)
    metrics["loss"].backward()
    torch.set_grad_enabled(False)
    assert sorted(preds) == ["depth_coarse", "depth_fine", "rgb_coarse", "rgb_fine", "s_fine", "weights_fine"], sorted(preds)
    for k, v in preds.items():  # the replayed draws are the reference's: the helper reproduces its preds from them
        e = float((v.detach().double() - h64["preds"][k]).abs().max() / h64["preds"][k].abs().max())
        assert e < 1e-5, (k, e)
    out = dict(fx, **dr)
    out.update(S=S, app=int(app), white_bg=int(ren.white_bg), weights_seed=seed, draw_seed=2000 + seed, ref_fp32_vs_fp64=dist, sub_stride=STRIDE,
               noise_std=cfg.render.noise_std, ray_reg_weight=cfg.loss.ray_reg_weight, loss=metrics["loss"])
    for k, v in preds.items():
        out[f"pred_{k}"] = v
    for k, v in metrics.items():
        out[f"metric_{k}"] = v
    for k, p in ren.named_parameters():
        if not k.startswith(ntu.NETS + ("embedding_a",)):
            continue  # (the encoders' frequency tables)
        assert p.grad is not None and float(p.grad.abs().max()) > 0, k
        if k.endswith(FULL):
            out[f"g_{k}"] = p.grad
        else:
            out[f"gsub_{k}"] = p.grad.reshape(-1)[::STRIDE].clone()
            out[f"gnorm_{k}"] = p.grad.double().norm()
    np.savez_compressed(mg.OUT / f"nerf_train_{tag}.npz", **mg.to_np(out))
    print(f"nerf_train_{tag}: seed {seed}, loss {float(metrics['loss']):.6f}, {len(out)} arrays")


if __name__ == "__main__":
    assert mg.REF.exists(), "the reference is only present in the build container"
    torch.set_num_threads(1)  # (summation order of the host GEMMs: the same bits on any core count)
    mg.install_stubs()
    fixture("7s", False)
    fixture("cam", True)
