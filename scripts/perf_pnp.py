"""Timing of nm_pnp_ransac (csrc/pnp.hip) at 16 queries x ~4k matches x 1024 hypotheses and at one query.

Two measurements, both of the native entry point called through ops.pnp_ransac on PREALLOCATED inputs (no wrapper tensor work inside
a timed window beyond the output allocations of that one call):

  * per kernel: the script starts a child of itself under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, nothing
    else traced) which warms up and then issues `--repeats` calls; the three kernels' rows of the kernel-stats table -- calls, mean,
    min and max duration in microseconds -- are what is reported as hypotheses / scoring / refinement.  The warm-up launches are in
    the rows too (same shapes; `calls` says how many).
  * per call: HIP events on the launch stream around one call (three kernels, two memsets and the launch gaps between them), median,
    minimum and 90th percentile of `--repeats` calls after `--warmup` calls, profiler off.

    python scripts/perf_pnp.py [--queries 16 1] [--matches 4096] [--hyps 1024] [--repeats 50] [--no-kernels]

Prints one JSON line per configuration.  The scenes are synthetic (points at depth 2-10 in front of a 640 x 480 camera, 0.5 px noise,
half of the matches replaced by uniform outliers); the line also carries the worst pose error over the queries, so a run that timed a
solver that does not solve is visible."""
import argparse
import csv
import json
import math
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

KERNELS = {"hypotheses": "pnp_hypotheses_kernel", "scoring": "pnp_score_kernel", "refinement": "pnp_refine_kernel"}


def make_batch(Q, matches, dev):
    """-> pt2d (n,2), pt3d (n,3), offsets (Q+1,) int32, K (Q,3,3) on the device; host copies of the true poses and the counts."""
    import torch

    rng = np.random.default_rng(Q)
    counts = [int(matches * rng.uniform(0.9, 1.1)) for _ in range(Q)]
    p2, p3, Ks, poses = [], [], [], []
    for n in counts:
        f = 500.0 + rng.uniform(-20, 20)
        K = np.array([[f, 0, 320 + rng.uniform(-5, 5)], [0, f, 240 + rng.uniform(-5, 5)], [0, 0, 1]])
        A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        R, t = A * np.sign(np.linalg.det(A)), rng.uniform(-1, 1, 3)
        pix = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)
        z = rng.uniform(2, 10, n)
        Xc = np.stack([(pix[:, 0] - K[0, 2]) / f * z, (pix[:, 1] - K[1, 2]) / f * z, z], 1)
        obs = pix + 0.5 * rng.normal(size=(n, 2))
        out = rng.permutation(n)[: n // 2]
        obs[out] = np.stack([rng.uniform(0, 640, len(out)), rng.uniform(0, 480, len(out))], 1)
        p2.append(obs), p3.append((Xc - t) @ R), Ks.append(K), poses.append((R, t))
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    offsets = to(np.concatenate([[0], np.cumsum(counts)]), torch.int32)
    return to(np.concatenate(p2), torch.float32), to(np.concatenate(p3), torch.float32), offsets, to(np.stack(Ks), torch.float32), poses, counts


def pose_error(R_true, t_true, w):
    R, t = w[:, :3].astype(np.float64), w[:, 3].astype(np.float64)
    ang = math.degrees(2 * math.asin(min(1.0, np.linalg.norm(R - R_true) / (2 * math.sqrt(2)))))
    return ang, float(np.linalg.norm(R_true.T @ t_true - R.T @ t))


def kernel_times(args, Q):
    """Child run under rocprofv3 -> {stage: dict(calls, mean_us, min_us, max_us)}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, str(Path(__file__).resolve()),
               "--child", "--queries", str(Q), "--matches", str(args.matches), "--hyps", str(args.hyps), "--repeats", str(args.repeats),
               "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        tables = sorted(Path(d).rglob("*kernel_stats.csv"))
        if r.returncode or not tables:
            raise SystemExit(f"the traced run failed (rc {r.returncode}, {len(tables)} kernel-stats tables):\n{r.stdout[-2000:]}")
        out = {}
        with open(tables[0]) as fh:
            for row in csv.DictReader(fh):
                for stage, name in KERNELS.items():
                    if name in row["Name"]:
                        out[stage] = dict(calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                          max_us=float(row["MaxNs"]) / 1e3)
        if set(out) != set(KERNELS):
            raise SystemExit(f"kernel rows missing from {tables[0]}: found {sorted(out)}")
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[16, 1])
    ap.add_argument("--matches", type=int, default=4096)
    ap.add_argument("--hyps", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true", help="skip the traced child run")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    # the traced children run BEFORE this process touches the GPU
    kernels = {} if (args.child or args.no_kernels) else {Q: kernel_times(args, Q) for Q in args.queries}

    import torch

    from nerfmatch_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("perf_pnp.py needs the GPU: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    for Q in args.queries:
        pt2d, pt3d, offsets, K, poses, counts = make_batch(Q, args.matches, dev)
        call = lambda: ops.pnp_ransac(pt2d, pt3d, offsets, K, thr_px=1.0, n_hyps=args.hyps, refine_iters=10, seed=0)
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        if args.child:
            for _ in range(args.repeats):
                call()
            torch.cuda.synchronize()
            continue
        ts = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts = np.sort(np.array(ts))
        pose, n_inl, _, _ = call()
        errs = [pose_error(R, t, pose[q].cpu().numpy().reshape(3, 4)) for q, (R, t) in enumerate(poses)]
        print(json.dumps(dict(queries=Q, matches=int(sum(counts)), hyps=args.hyps, reprojections=int(sum(counts)) * args.hyps,
                              call_us=dict(median=float(np.median(ts)), min=float(ts[0]), p90=float(ts[int(0.9 * (len(ts) - 1))])),
                              call_us_per_query=float(np.median(ts)) / Q, kernels_us=kernels.get(Q), min_inliers=int(n_inl.min()),
                              worst_R_err_deg=max(e[0] for e in errs), worst_center_err=max(e[1] for e in errs))), flush=True)


if __name__ == "__main__":
    main()
