"""Time of cosine mutual-NN feature matching (ops.feature_mutual_nn, csrc/match_fused.hip) at the sizes of a NeRF validation pair:
4800 x 4800 x 256 (480 x 640 px at ds = 8) and 6360 x 6360 x 256.  Three forms of the same formula, interleaved, HIP events around
every call (each call ends in its own read-back of the match count / of the lists, so the events see the whole call):

  (i)   the native op
  (ii)  torch on the same GPU: normalise, matmul, two max calls, the index test
  (iii) the reference's form: both feature sets copied to the host, the same statements in torch on the CPU (host clock)

and, for scale, the fused dual-softmax matcher on one pair of the same size (two tile passes where the op runs one).

    python scripts/perf_feature_nn.py [--reps 20] [--cpu-reps 3]      # prints one JSON line per size"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nerfmatch_amd import ops  # noqa: E402
from nerfmatch_amd.utils.geometry import _mutual_nn_torch  # noqa: E402


def planted(n, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    d1 = torch.randn(n, C, generator=g)
    d2 = d1[torch.randperm(n, generator=g)] + 0.7 * torch.randn(n, C, generator=g)
    return d1.to(dev), d2.to(dev)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_feature_nn.py measures on the GPU: no device found")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ops.MATCH_PRECISION = "bf16x3"
    for n in (4800, 6360):
        d1, d2 = planted(n, 256, n, dev)
        forms = {
            "native": lambda: ops.feature_mutual_nn(d1, d2),
            "torch_gpu": lambda: _mutual_nn_torch(d1, d2, None, 1e-9),
            "matcher_fused_1pair": lambda: ops.dual_softmax_match_batch(d1[None], d2[None], 10.0, threshold=0.2, mutual=True, want_conf=False)["count"].item(),
        }
        for f in forms.values():  # warm-up: code objects, workspaces, the BLAS library's choice of algorithm
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(args.reps):  # interleaved: drifts of clocks and neighbours hit every form alike
            for k, f in forms.items():
                times[k].append(event_ms(f)[0])
        cpu = []
        for _ in range(args.cpu_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m_cpu, _ = _mutual_nn_torch(d1.cpu(), d2.cpu(), None, 1e-9)
            cpu.append((time.perf_counter() - t0) * 1e3)
        m_nat, m_gpu = forms["native"]()[0], forms["torch_gpu"]()[0]
        res = dict(n1=n, n2=n, C=256, reps=args.reps)
        for k, v in times.items():
            res[f"{k}_ms_median"], res[f"{k}_ms_min"] = round(statistics.median(v), 4), round(min(v), 4)
        res["host_copy_cpu_ms_median"], res["host_copy_cpu_ms_min"] = round(statistics.median(cpu), 2), round(min(cpu), 2)
        res["matches_native"], res["matches_torch_gpu"], res["matches_cpu"] = len(m_nat), len(m_gpu), len(m_cpu)
        res["same_as_cpu"] = bool(torch.equal(m_nat.cpu(), m_cpu))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
