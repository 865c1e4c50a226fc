#!/usr/bin/env python3
"""What producing a batch's reference point sets costs with ref_bank.ReferencePointBank, beside two other forms of the same rule
(NeRFMatchMultiPair.load_ref_pts, nerfmatch/datasets/nerfmatch_dataset.py:441-518), for a bank of --frames cached frames of --points points
with --dim features and batches of --batch queries with --topk frames each, sampled to --sample-pts rows at 640 x 480:

  bank        nm_refbank_visibility + nm_refbank_select + nm_refbank_gather on the device-resident cache through reference_sets (new
              round keys every batch), and `bank_launches`: the three launches alone
  torch_gpu   (a) the same rule in torch ops on the same GPU (the bank's own plain-torch statement, on device tensors; it reads Nv back)
  host        (b) the reference's form: numpy on the host from in-memory arrays -- stack the k frames, project into the k cameras, the
              co-visibility loop, a permutation draw -- then the copy of the sampled rows to the device (the .npy reads are NOT counted)

and the stacked layout (sample_mode=None) of bank and torch_gpu.  Times are HIP events over windows of --calls batches (host clock ending
in a synchronise for `host`), --reps windows each, median / min / max over the windows.  No pass / fail: prints one JSON line.

    python scripts/perf_ref_bank.py [--frames 200] [--points 4800] [--dim 256] [--batch 16] [--topk 10] [--sample-pts 3600] [--calls 50]
                                    [--reps 7] [--no-host] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nerfmatch_amd import synth  # noqa: E402
from nerfmatch_amd.ref_bank import ReferencePointBank  # noqa: E402

H, W = 480, 640


def spread(vals):
    v = sorted(vals)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def event_windows(fn, calls, reps, warmup=5):
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


def host_windows(fn, calls, reps, warmup=1):
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


def host_sets(pt3d, feat, mask, K, w2c, ref_ids, P, rng, dev):
    """form (b) for one batch: numpy per query, then one copy per tensor"""
    o3, of, om = [], [], []
    for row in ref_ids:
        p = np.concatenate([pt3d[f] for f in row])
        x = np.concatenate([feat[f] for f in row])
        m = np.concatenate([mask[f] for f in row])
        visible = np.ones(len(p), np.bool_)
        for f in row:
            cam = p @ w2c[f][:, :3].T + w2c[f][:, 3]
            pix = ((cam / cam[:, 2:3]) @ K[f].T)[:, :2]
            inside = (pix >= 0).all(-1) & (pix[:, 0] < W) & (pix[:, 1] < H)
            both = visible & inside
            visible = (visible | inside) if 3 * both.sum() < visible.sum() else both
        idx = np.nonzero(visible)[0]
        idx = np.tile(idx[rng.permutation(len(idx))], P // len(idx) + 1)[:P]
        o3.append(p[idx]); of.append(x[idx]); om.append(m[idx])
    return torch.from_numpy(np.stack(o3)).to(dev), torch.from_numpy(np.stack(of)).to(dev), torch.from_numpy(np.stack(om)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--points", type=int, default=4800)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--sample-pts", type=int, default=3600)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip form (b)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_ref_bank.py needs a GPU: there is no CPU timing to report")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    F, n, D, B, k, P = a.frames, a.points, a.dim, a.batch, a.topk, a.sample_pts
    g = np.random.default_rng(0)
    pt3d = np.stack([g.uniform(-2.5, 2.5, (F, n)), g.uniform(-1.9, 1.9, (F, n)), g.uniform(1.0, 5.0, (F, n))], -1).astype(np.float32)
    feat = g.standard_normal((F, n, D), dtype=np.float32)
    c2w = torch.stack([synth.camera_pose(100 + f, max_t=0.5, max_angle=0.3) for f in range(F)])
    bank = ReferencePointBank(pt3d, feat, c2w, synth.intrinsics(H, W, 525.0), (W, H), (W, H), device=dev)
    batches = [torch.from_numpy(g.integers(0, F, (B, k))) for _ in range(8)]
    dev_batches = [b.to(dev) for b in batches]
    bank_bytes = sum(t.numel() * t.element_size() for t in (bank.pt3d, bank.pt_feat, bank.pt_mask, bank.cams, bank.c2w))
    res = dict(frames=F, points=n, dim=D, batch=B, topk=k, sample_pts=P, calls_per_window=a.calls, windows=a.reps, bank_bytes=bank_bytes)
    kw = dict(sample_mode="rand", sample_pts=P)
    res["bank_us_per_batch"] = event_windows(lambda i: bank.reference_sets(dev_batches[i % 8], draw=i, **kw), a.calls, a.reps)
    # the three launches alone, with the round keys already on the device: what the GPU spends (the line above includes ~10 us of Python
    # integer arithmetic per query for the keys of a (query, draw) that has not been asked for before, and their upload)
    from nerfmatch_amd import ops

    rk = torch.zeros(B, 4, dtype=torch.int32, device=dev)

    def launches(i):
        sel = ops.refbank_select(bank.pt3d, bank.cams, dev_batches[i % 8], bank.img_wh)
        ops.refbank_gather(bank.pt3d, bank.pt_feat, bank.pt_mask, dev_batches[i % 8], bank._bad, P, select=sel, perm_keys=rk)

    res["bank_launches_us_per_batch"] = event_windows(launches, a.calls, a.reps)
    res["bank_stacked_us_per_batch"] = event_windows(lambda i: bank.reference_sets(dev_batches[i % 8]), a.calls, a.reps)
    keys = list(range(B))
    calls = max(a.calls // 10, 3)
    res["torch_gpu_us_per_batch"] = event_windows(lambda i: bank._sets_torch(dev_batches[i % 8], "rand", P, keys, i), calls, a.reps, warmup=2)
    res["torch_gpu_stacked_us_per_batch"] = event_windows(lambda i: bank._sets_torch(dev_batches[i % 8], None, k * n, keys, 0), calls, a.reps, warmup=2)
    res["torch_gpu_calls_per_window"] = calls
    got = bank.reference_sets(dev_batches[0], draw=3, **kw)
    (t3, tf, tm), tsel = bank._sets_torch(dev_batches[0], "rand", P, keys, 3)
    res["bank_equals_torch_gpu"] = bool(torch.equal(got["pt3d"], t3) and torch.equal(got["pt_feat"], tf) and torch.equal(got["pt_mask"], tm)
                                        and torch.equal(got["n_visible"], tsel["n_visible"]) and torch.equal(got["decisions"], tsel["decisions"]))
    res["n_visible_first_batch"] = got["n_visible"].tolist()
    if not a.no_host:
        mask = np.ones((F, n), np.bool_)
        K64, w2c64 = bank.cams[:, :9].reshape(F, 3, 3).cpu().numpy(), bank.cams[:, 9:].reshape(F, 3, 4).cpu().numpy()
        rng = np.random.default_rng(1)
        hcalls = 2
        res["host_us_per_batch"] = host_windows(lambda i: host_sets(pt3d, feat, mask, K64, w2c64, batches[i % 8].tolist(), P, rng, dev), hcalls,
                                                min(a.reps, 3))
        res["host_calls_per_window"] = hcalls
    res["bad_ids"] = bank.bad_ids
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
