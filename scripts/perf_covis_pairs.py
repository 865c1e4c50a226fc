#!/usr/bin/env python3
"""What a scene's covisibility pair list costs with nerfmatch_amd.covis_pairs, beside two other forms of the same rule, on synthetic
banks of --frames frames (default 1200 and 4000) of --points points (4800: the 80 x 60 cells of a 640 x 480 frame), each with and
without the depth test:

  kernels     nm_covis_self_depth, nm_covis_scores and nm_covis_topk, each timed on its own with HIP events (--reps windows of --calls
              calls after a warm-up; median / min / max over the windows), and the projections per second of nm_covis_scores
  torch_gpu   the module's plain-torch statement of the rule on the same device tensors, on the first --torch-rows query rows (the full
              matrix is F / rows times that; the row chunks are independent)
  numpy_host  the rule in numpy on the host, smallest bank only, on the first --numpy-rows query rows

The bound nm_covis_scores is judged against is arithmetic, not memory: a projection is ~25 fp32 operations (18 for R X + t, 2 divisions,
4 + 2 for the two pixel rows, comparisons apart), and the chip issues 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12 non-fused fp32
operations per second, so 3.1e12 projections per second; frame j's points are read once per 32 cameras (12 bytes per 32 projections).
No pass / fail beyond checking that the three forms agree: prints one JSON line.

    python scripts/perf_covis_pairs.py [--frames 1200 4000] [--points 4800] [--calls 3] [--reps 5] [--torch-rows 64] [--numpy-rows 2] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nerfmatch_amd import covis_pairs as cp  # noqa: E402
from nerfmatch_amd import ops, synth  # noqa: E402

H, W, GW, GH = 480, 640, 80, 60
TOL = 0.05
PEAK_FP32_OPS = 256 * 4 * 32 * 2.4e9  # non-fused fp32 operations per second (MI355X: 256 CUs, 4 SIMD-32 each, 2.4 GHz)
OPS_PER_PROJECTION = 25


def spread(vals):
    v = sorted(vals)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def event_windows(fn, calls, reps, warmup=1):
    """microseconds per call of fn(): `reps` windows of `calls` calls between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return spread(out)


def make_bank(F, n, seed=0):
    """cameras around the origin looking down +z at a slab of random points, 640 x 480 px"""
    g = np.random.default_rng(seed)
    pt3d = np.stack([g.uniform(-2.5, 2.5, (F, n)), g.uniform(-1.9, 1.9, (F, n)), g.uniform(1.0, 5.0, (F, n))], -1).astype(np.float32)
    c2w = torch.stack([synth.camera_pose(100 + f, max_t=0.5, max_angle=0.3) for f in range(F)])
    mask = torch.from_numpy(g.uniform(size=(F, n)) > 0.05)
    return torch.from_numpy(pt3d), mask, cp.camera_rows(c2w, synth.intrinsics(H, W, 525.0), (W, H), (W, H))


def numpy_scores(pt3d, mask, cams, rows, depth):
    """the rule in numpy, one query row at a time (fp32 throughout)"""
    F, n, _ = pt3d.shape
    K, w2c = cams[:, :9].reshape(F, 3, 3), cams[:, 9:].reshape(F, 3, 4)
    X = pt3d.reshape(-1, 3)
    zself = np.stack([pt3d[f] @ w2c[f, 2, :3] + w2c[f, 2, 3] for f in range(F)]) if depth else None
    out = np.zeros((len(rows), F), np.int32)
    with np.errstate(all="ignore"):
        for q, i in enumerate(rows):
            p = X @ w2c[i, :, :3].T + w2c[i, :, 3]
            pix = ((p / p[:, 2:3]) @ K[i].T)[:, :2]
            seen = np.isfinite(pix).all(-1) & (p[:, 2] > 0) & (pix >= 0).all(-1) & (pix[:, 0] < W) & (pix[:, 1] < H)
            if depth:
                xi, yi = np.where(seen, pix[:, 0], 0).astype(np.int64), np.where(seen, pix[:, 1], 0).astype(np.int64)
                c = (yi * GH // H) * GW + xi * GW // W
                zq = zself[i][c]
                seen &= mask[i][c] & (zq > 0) & (np.abs(p[:, 2] - zq) <= np.float32(TOL) * zq)
            out[q] = (seen & mask.reshape(-1)).reshape(F, n).sum(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1200, 4000])
    ap.add_argument("--points", type=int, default=GW * GH)
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-rows", type=int, default=64)
    ap.add_argument("--numpy-rows", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_covis_pairs.py needs a GPU: there is no CPU timing to report")
    if a.points != GW * GH:
        raise SystemExit(f"--points must be {GW * GH}: the depth test runs on the {GW} x {GH} grid")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, k = a.points, a.topk
    res = dict(points=n, topk=k, calls_per_window=a.calls, windows=a.reps, ops_per_projection=OPS_PER_PROJECTION,
               bound_projections_per_s=PEAK_FP32_OPS / OPS_PER_PROJECTION, banks=[])
    for F in a.frames:
        pt3d, mask, cams = make_bank(F, n)
        d3, dm, dc = pt3d.to(dev), mask.to(dev), cams.to(dev)
        proj = F * F * n
        bank = dict(frames=F, projections=proj)
        bank["self_depth_us"] = event_windows(lambda: ops.covis_self_depth(d3, dc, dm), max(a.calls, 20), a.reps)
        zself = ops.covis_self_depth(d3, dc, dm)
        for tag, kw in (("plain", dict()), ("depth", dict(zself=zself, grid_wh=(GW, GH), depth_tol=TOL))):
            t = event_windows(lambda: ops.covis_scores(d3, dm, dc, None, (W, H), **kw), a.calls, a.reps)
            scores = ops.covis_scores(d3, dm, dc, None, (W, H), **kw)
            bank[f"scores_{tag}_us"] = t
            bank[f"scores_{tag}_projections_per_s"] = proj / (t["median"] * 1e-6)
            bank[f"scores_{tag}_share_of_bound"] = bank[f"scores_{tag}_projections_per_s"] / res["bound_projections_per_s"]
            bank[f"topk_{tag}_us"] = event_windows(lambda: ops.covis_topk(scores, None, k), max(a.calls, 20), a.reps)
            bank[f"pairs_{tag}_mean"] = float(ops.covis_topk(scores, None, k)[1].float().mean())
            # the same rule in torch on the same GPU, on the first rows
            rk = dict() if tag == "plain" else dict(depth_tol=TOL, grid_wh=(GW, GH))
            rows = torch.arange(min(a.torch_rows, F), device=dev)
            fn = lambda: cp._scores_torch(d3, dm, dc, rows, (W, H), rk.get("depth_tol"), rk.get("grid_wh"))
            tt = event_windows(fn, 1, min(a.reps, 3))
            bank[f"torch_gpu_{tag}_us_per_row"] = {key: v / len(rows) for key, v in tt.items()}
            bank[f"torch_gpu_{tag}_projections_per_s"] = len(rows) * F * n / (tt["median"] * 1e-6)
            bank[f"torch_gpu_{tag}_full_matrix_s_extrapolated"] = tt["median"] * 1e-6 * F / len(rows)
            bank[f"kernel_equals_torch_gpu_{tag}"] = bool(torch.equal(fn(), scores[: len(rows)]))
            if F == min(a.frames) and a.numpy_rows > 0:
                nrows = list(range(min(a.numpy_rows, F)))
                t0 = time.perf_counter()
                got = numpy_scores(pt3d.numpy(), mask.numpy(), cams.numpy(), nrows, tag == "depth")
                dt = time.perf_counter() - t0
                bank[f"numpy_host_{tag}_s_per_row"] = dt / len(nrows)
                bank[f"numpy_host_{tag}_projections_per_s"] = len(nrows) * F * n / dt
                bank[f"numpy_host_{tag}_full_matrix_s_extrapolated"] = dt * F / len(nrows)
                # numpy's matrix products may round differently from the rule's fixed order: report how many scores differ, assert nothing
                bank[f"numpy_host_{tag}_scores_differing"] = int((torch.from_numpy(got) != scores[: len(nrows)].cpu()).sum())
        res["banks"].append(bank)
        del d3, dm, dc, zself, scores
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
