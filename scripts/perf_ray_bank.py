#!/usr/bin/env python3
"""What producing a training batch costs with nerf.ray_bank.RayBank, beside the two forms of the reference's pre-expanded ray table
(NerfBaseDataset.process_train_data, nerfmatch/datasets/nerfbase.py:351-385: 12 ray floats + 3 rgb floats + an id per pixel), for a bank of
--frames frames of 640 x 480 and batches of --rays rays:

  bank        one nm_raybank_gather launch per batch from uint8 frames + one camera row per frame (positions of the epoch permutation)
  table_gpu   (i)  the same rows indexed out of the pre-expanded [N,16] fp32 table held on the same GPU (a shuffled index per batch)
  table_host  (ii) the reference's own form: index the table in host memory, then copy the rows to the device

and the device memory each form holds, and the bank's batch time as a share of a measured training step (render + losses + backward at
the same ray count, --samples samples, as scripts/perf_nerf_train.py times it).  Times are HIP events over windows of --calls batches
(host clock ending in a synchronise for table_host), --reps windows each, median / min / max over the windows.  No pass / fail: prints
one JSON line.

    python scripts/perf_ray_bank.py [--frames 200] [--rays 9216] [--calls 100] [--reps 7] [--samples 128] [--no-step] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nerfmatch_amd import synth  # noqa: E402
from nerfmatch_amd.nerf.ray_bank import RayBank  # noqa: E402

H, W = 480, 640


def spread(vals):
    v = sorted(vals)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def event_windows(fn, calls, reps, warmup=20):
    """microseconds per call of fn(i): `reps` windows of `calls` calls between two events"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for r in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(r * calls + i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return spread(out)


def host_windows(fn, calls, reps, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for r in range(reps):
        t0 = time.perf_counter()
        for i in range(calls):
            fn(r * calls + i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / calls)
    return spread(out)


def train_step_ms(bank, samples, steps=5, warmup=2):
    """render + losses + backward of one batch of the bank (no optimiser), HIP events"""
    from nerfmatch_amd.nerf import train_render as tr
    from nerfmatch_amd.nerf.renderer import NerfRenderer

    cfg = synth.nerf_config("7scenes", num_pts=samples)
    ren = NerfRenderer(cfg, num_frames=None, training=True)
    ren.load_state_dict(synth.nerf_state_dict(seed=0, density_bias=3.0))
    ren.to(bank.device)
    b = bank.train_batch(0)

    def step():
        ren.zero_grad(set_to_none=True)
        with torch.enable_grad():
            preds = ren.render_rays(b["rays"][0], ray_id=None, validation=False)
            tr.training_metrics(preds, b["rgbs"][0], None, cfg.loss)["loss"].backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return spread([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rays", type=int, default=9216)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step measurement")
    ap.add_argument("--no-host-table", action="store_true", help="skip form (ii) (it needs the whole table in host memory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_ray_bank.py needs a GPU: there is no CPU timing to report")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    F, R = a.frames, a.rays
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    poses = torch.stack([synth.camera_pose(100 + f) for f in range(F)])
    bank = RayBank(images, poses, synth.intrinsics(H, W, 525.0), batch_rays=R, device=dev)
    del images
    N = bank.num_train
    bank_bytes = sum(t.numel() * t.element_size() for t in (bank.images, bank.cams, bank.flags, bank.ts_table))
    res = dict(frames=F, height=H, width=W, rays=R, pixels=N, calls_per_window=a.calls, windows=a.reps, bank_bytes=bank_bytes)
    res["bank_us_per_batch"] = event_windows(lambda i: bank.train_batch(i % len(bank)), a.calls, a.reps)

    # the pre-expanded table, built frame by frame with the bank's own rows: [N,16] = rays | rgbs | id
    table = torch.empty(N, 16, device=dev)
    for f in range(F):
        fb = bank.frame_batch(f)
        table[f * H * W : (f + 1) * H * W] = torch.cat([fb["rays"][0], fb["rgbs"][0], fb["ts"][0][:, None].float()], 1)
    res["table_bytes"] = table.numel() * table.element_size()
    res["memory_ratio_table_over_bank"] = res["table_bytes"] / bank_bytes
    shuffled = torch.randperm(N, device=dev)
    n_batches = N // R
    res["table_gpu_us_per_batch"] = event_windows(lambda i: table[shuffled[(i % n_batches) * R : (i % n_batches + 1) * R]], a.calls, a.reps)
    same = table[shuffled[:R]]
    rows = bank.batch(shuffled[:R])
    res["table_rows_equal_bank_rows"] = bool(torch.equal(same[:, :12], rows[0]) and torch.equal(same[:, 12:15], rows[1]))

    if not a.no_host_table:
        table_host, shuffled_host = table.cpu(), shuffled.cpu()
        calls = max(a.calls // 10, 5)
        res["table_host_us_per_batch"] = host_windows(
            lambda i: table_host[shuffled_host[(i % n_batches) * R : (i % n_batches + 1) * R]].to(dev), calls, a.reps)
        res["table_host_calls_per_window"] = calls
        del table_host
    del table

    if not a.no_step:
        res["train_step_ms"] = step = train_step_ms(bank, a.samples)
        res["samples"] = a.samples
        res["bank_batch_share_of_step"] = res["bank_us_per_batch"]["median"] * 1e-3 / step["median"]
    res["bad_ids"] = bank.bad_ids
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
