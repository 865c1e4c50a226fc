#!/usr/bin/env python3
"""Step time of a NeRF training step (render + losses + backward, no optimiser) at the reference's batch -- 9216 rays x (128 + 128) samples,
configs/nerf/*.yaml -- in HIP events, for both ops.LINEAR_PRECISION values and for the opt-in fp16 mixed-precision walk
(NerfRenderer.train_precision = "f16") IN THIS PROCESS, side by side, each with its peak device memory and split into encode /
chain forward / per-ray kernels / chain dX / dW, and beside it the same step with the two MLPs and the compositing done by torch autograd (fp32, rocBLAS GEMMs) on the same device from
the same encoded inputs: what the reference's stack would run for that part.  No pass / fail: prints one JSON line per configuration.

    python scripts/perf_nerf_train.py [--rays 9216] [--samples 128] [--steps 5] [--warmup 2] [--app] [--converge STEPS] [--out FILE]

--converge STEPS adds a short convergence leg: a student scene model trained by NerfTrainer for STEPS steps on the colours a fixed teacher
model renders for a pool of rays -- same pool, same initial weights, same seeds and therefore the same draws -- once under bf16x3 and once
under "f16"; it reports the mean rgb_fine_psnr of the last ten steps of both, the skipped steps and the final loss scale.

The split comes from a separate run with an event pair around every call (which serialises host and device: its parts add up to more than
the un-instrumented step time, which is the figure to quote)."""
import argparse
import json
import sys
from collections import defaultdict
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import nerfmatch_amd  # noqa: E402
from nerfmatch_amd import ops, synth  # noqa: E402
from nerfmatch_amd.nerf import train_render as tr  # noqa: E402
from nerfmatch_amd.nerf.renderer import NerfRenderer  # noqa: E402


def bundle(n, S, dev, app):
    g = torch.Generator().manual_seed(0)
    o = (torch.rand(n, 3, generator=g) - 0.5) * 0.4
    v = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    od = (o * v).sum(1, keepdim=True)
    far = torch.sqrt(od * od + 1.0 - (o * o).sum(1, keepdim=True)) - od
    rays = torch.cat([o, v, torch.full((n, 1), 0.01), far, v, torch.full((n, 1), 2.0 / 12**0.5 / 525.0)], 1)
    b = dict(rays=rays, gt=torch.rand(n, 3, generator=g), ids=torch.randint(0, 300, (n,), generator=g) if app else None,
             mask=torch.rand(n, 1, generator=g) if app else None)
    return {k: None if x is None else x.to(dev).contiguous() for k, x in b.items()}


def hip_step(ren, b, loss_cfg, debug=False):
    ren.zero_grad(set_to_none=True)
    with torch.enable_grad():
        preds = ren.render_rays(b["rays"], ray_id=b["ids"], validation=False, debug=debug)
        m = tr.training_metrics(preds, b["gt"], b["mask"], loss_cfg)
        m["loss"].backward()
    return preds, m


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


class Split:
    """event pairs around the calls of one step, summed per category"""

    def __init__(self):
        self.pairs, self.phase, self.saved, self.depth = defaultdict(list), "forward", [], 0

    def wrap(self, mod, name, cat):
        fn = getattr(mod, name)
        self.saved.append((mod, name, fn))

        def inner(*a, **kw):
            if self.depth:  # (a wrapped call inside a wrapped call -- linear_wgrad under linear_wgrad_bias -- belongs to the outer one)
                return fn(*a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.depth += 1
            e0.record()
            try:
                out = fn(*a, **kw)
            finally:
                self.depth -= 1
            e1.record()
            self.pairs[cat(self) if callable(cat) else cat].append((e0, e1))
            return out
        setattr(mod, name, inner)

    def __enter__(self):
        self.wrap(tr, "encode", "encode")
        self.wrap(ops, "linear", lambda s: "chain_forward" if s.phase == "forward" else "chain_dX")
        self.wrap(ops, "linear_wgrad_bias", "dW")
        self.wrap(ops, "linear_wgrad", "dW")
        self.wrap(ops, "linear_chain_f16", lambda s: "chain_forward" if s.phase == "forward" else "chain_dX")
        self.wrap(ops, "linear_wgrad_f16", "dW")
        self.wrap(tr, "g4_split_f16", "per_ray")
        for name in ("composite", "composite_bwd", "_distortion", "distortion_bwd", "app_grad"):
            self.wrap(tr, name, "per_ray")
        for cls in (tr.Chain, tr.Chain16):
            self.wrap_backward(cls)
        return self

    def wrap_backward(self, cls):
        back = cls.backward
        self.saved.append((cls, "backward", back))

        def backward(chain, *a, **kw):
            self.phase = "backward"
            try:
                return back(chain, *a, **kw)
            finally:
                self.phase = "forward"
        cls.backward = backward

    def __exit__(self, *exc):
        for mod, name, fn in reversed(self.saved):
            setattr(mod, name, fn)

    def totals(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.pairs.items()}


def torch_step(P, enc, b, t, noise, loss_cfg, white_bg):
    """both MLPs, the compositing, the losses and backward in torch autograd from the encoded inputs (xi, xd) of the HIP step"""
    F = torch.nn.functional
    for p in P.values():
        p.grad = None
    with torch.enable_grad():
        preds = {}
        for key in ("coarse", "fine"):
            xi, xd = enc[key]
            pre = f"nerf_{key}"
            h = xi
            for l in range(8):
                h = F.relu(F.linear(h, P[f"{pre}.pts_linears.{l}.weight"], P[f"{pre}.pts_linears.{l}.bias"]))
                if l == 4:
                    h = torch.cat([xi, h], -1)
            sigma = F.linear(h, P[f"{pre}.alpha_linear.weight"], P[f"{pre}.alpha_linear.bias"])
            feat = F.linear(h, P[f"{pre}.feature_linear.weight"], P[f"{pre}.feature_linear.bias"])
            hv = F.relu(F.linear(torch.cat([feat, xd], -1), P[f"{pre}.views_linears.0.weight"], P[f"{pre}.views_linears.0.bias"]))
            rgb = torch.sigmoid(F.linear(hv, P[f"{pre}.rgb_linear.weight"], P[f"{pre}.rgb_linear.bias"]))
            R, S = t[key].shape[0], t[key].shape[1] - 1
            dens = F.relu(sigma.reshape(R, S) + noise[key])
            delta = (t[key][:, 1:] - t[key][:, :-1]) * b["rays"][:, 3:6].norm(dim=-1, keepdim=True)
            alpha = 1.0 - torch.exp(-dens * delta)
            w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
            rgb_map = (w[..., None] * rgb.reshape(R, S, 3)).sum(-2)
            if white_bg:
                rgb_map = rgb_map + (1.0 - w.sum(-1, keepdim=True))
            preds[f"rgb_{key}"], preds[f"weights_{key}"] = rgb_map, w
        m = 1 if b["mask"] is None else b["mask"]
        loss = 0.5 * (m * (preds["rgb_coarse"] - b["gt"]) ** 2).mean() + 0.5 * (m * (preds["rgb_fine"] - b["gt"]) ** 2).mean()
        from nerfmatch_amd.utils.metrics import distortion_loss
        loss = loss + loss_cfg.ray_reg_weight * distortion_loss(tr.t_to_s(t["fine"]), preds["weights_fine"])
        loss.backward()
    return loss


def converge(a, dev):
    """bf16x3 against "f16": the same student trained on a teacher's colours with the same draws -> one JSON line per mode"""
    from argparse import Namespace

    from nerfmatch_amd.nerf_trainer import NerfTrainer

    S, n, batches = a.samples, a.converge_rays, 8
    cfg = synth.nerf_config("7scenes", num_pts=S)
    cfg.optim = Namespace(optimizer="adam", lr=5e-4, weight_decay=0.0, lr_scheduler=None)
    pool = bundle(n * batches, S, dev, False)["rays"]
    teacher = NerfRenderer(cfg, training=False)
    teacher.load_state_dict(synth.nerf_state_dict(seed=1, density_bias=3.0))
    teacher.to(dev).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        gt = torch.cat([teacher.render_rays(pool[i * n:(i + 1) * n], validation=True, t_rand=torch.rand(n, S + 1, generator=g).to(dev),
                                            jitter=synth.resample_jitter((n, S + 1), 11 + i).to(dev))["rgb_fine"] for i in range(batches)])
    out = []
    for mode in ("bf16x3", "f16"):
        nerfmatch_amd.set_precision("bf16x3")
        cfg.train_precision = "f16" if mode == "f16" else "same"
        trainer = NerfTrainer(cfg, device=dev)
        trainer.model.load_state_dict(synth.nerf_state_dict(seed=0, density_bias=3.0))
        torch.manual_seed(0)  # the renders draw t_rand / jitter / noise on the device: the same sequence in both modes
        psnr = []
        for i in range(a.converge):
            k = i % batches
            m = trainer.training_step(dict(rays=pool[None, k * n:(k + 1) * n], rgbs=gt[None, k * n:(k + 1) * n]), i)
            psnr.append(float(m["rgb_fine_psnr"]))
        out.append(dict(path="converge", mode=mode, steps=a.converge, rays=n, samples=S, first_rgb_fine_psnr=round(psnr[0], 3),
                        final_rgb_fine_psnr=round(sum(psnr[-10:]) / len(psnr[-10:]), 3), skipped_steps=trainer.skipped_steps,
                        final_loss_scale=trainer.loss_scale, overflow_events=list(trainer.overflow_events)))
        print(json.dumps(out[-1]), flush=True)
    nerfmatch_amd.set_precision("fp32")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=9216)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--app", action="store_true", help="appearance embedding, white background, loss mask (the cambridge yaml)")
    ap.add_argument("--converge", type=int, default=0, help="steps of the convergence leg (0: none)")
    ap.add_argument("--converge-rays", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_nerf_train.py needs a GPU: there is no CPU timing to report")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = synth.nerf_config("cambridge" if a.app else "7scenes", num_pts=a.samples)
    sd = synth.nerf_state_dict(seed=0, app_vocab=300 if a.app else 0, density_bias=3.0)
    ren = NerfRenderer(cfg, num_frames=300 if a.app else None, training=True)
    ren.load_state_dict(sd)
    ren.to(dev)
    b = bundle(a.rays, a.samples, dev, a.app)
    lines = []
    for precision in ("fp32", "bf16x3", "f16"):
        f16 = precision == "f16"
        nerfmatch_amd.set_precision("bf16x3" if f16 else precision)  # (the "f16" walk does not read ops.LINEAR_PRECISION)
        ren.train_precision = "f16" if f16 else "same"
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        whole = timed(lambda: hip_step(ren, b, cfg.loss), a.steps, a.warmup)
        peak = torch.cuda.max_memory_allocated()
        with Split() as sp:
            hip_step(ren, b, cfg.loss)
            parts = sp.totals()
        lines.append(dict(path="hip", precision=precision, rays=a.rays, samples=a.samples, app=a.app, step=whole, peak_memory_mib=round(peak / 2**20, 1),
                          split_ms={k: round(v, 3) for k, v in sorted(parts.items())}, split_sum_ms=round(sum(parts.values()), 3),
                          chunk_rays=ren.train_chunk_rays or tr.chunk_rays_for(a.samples, ren.train_chunk_bytes, 2 if f16 else 4)))
        if f16:
            lines[-1]["overflow_events"] = list(ren.train_overflow_events())
        print(json.dumps(lines[-1]), flush=True)
    ren.train_precision = "same"
    nerfmatch_amd.set_precision("fp32")
    # the torch-autograd step on the HIP step's own fence posts and encodings
    with torch.no_grad():
        preds, _ = hip_step(ren, b, cfg.loss, debug=True)
        t = dict(coarse=preds["t_coarse"], fine=preds["t_fine"])
        table = ren.embedding_a.weight.detach() if a.app else None
        enc = {}
        for key in t:
            xi, xd = tr.encode(b["rays"], t[key], b["ids"], table, ren.mip_var_scale)
            enc[key] = (xi[:, :90].contiguous(), xd[:, : 43 if a.app else 27].contiguous())
        noise = {key: torch.randn(a.rays, a.samples, device=dev) for key in t}
    P = {k: v.detach().clone().requires_grad_(True) for k, v in ren.state_dict().items() if k.startswith(("nerf_coarse", "nerf_fine"))}
    whole = timed(lambda: torch_step(P, enc, b, t, noise, cfg.loss, ren.white_bg), a.steps, a.warmup)
    lines.append(dict(path="torch_autograd_from_encoded_inputs", precision="fp32", rays=a.rays, samples=a.samples, app=a.app, step=whole,
                      note="MLPs, compositing, losses and backward in torch; sampling and encoding not included"))
    print(json.dumps(lines[-1]), flush=True)
    if a.converge:
        lines += converge(a, dev)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
