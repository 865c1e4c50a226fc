"""The epilogue truth table of ops.linear, shared by tests/test_linear_family_gpu.py and by the child processes it starts.

    python tests/linear_family_worker.py <precision> <shape index> [<shape index> ...]

runs the table at SHAPES[index] in this process and prints one JSON line (see main()).  The A/B switches of csrc/gemm_bf16.hip
(NM_GEMM_SMALL, NM_GEMM_COALESCED) are read once per process, so the test sets them in the environment of a fresh child.

Contract under test (ops.linear's docstring):   y = (act(x . w^T + bias + pre) + residual) * [gate > 0]
"""
import functools
import hashlib
import itertools
import json
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

PARTS = ("bias", "pre", "residual", "gate")
SUBSETS = [tuple(p for i, p in enumerate(PARTS) if mask >> i & 1) for mask in range(16)]
ACTS = {"none": 0, "relu": 1, "gelu": 2}  # _lib.NM_ACT_*
TABLE = list(itertools.product(SUBSETS, ACTS))  # 48 combinations
# the bars tests/test_matcher_gpu.py holds for these kernels (test_linear, test_linear_bf16x3): max |y - fp64 reference|
BARS = {"fp32": 2e-5, "bf16x3": 5e-5}

# (M, N, K); the first four are the shapes of the A/B children
SHAPES = [(333, 256, 256), (97, 8, 128),     # split small-grid form at K = 256 / 128; M % 128 = 77 / 97; N = 8: a single 8-wide piece
          (161, 96, 256), (225, 48, 128),    # small-grid form, column tail inside a 128-chunk (inerf.GemmField's widths)
          (131, 40, 24), (33, 136, 264), (1, 8, 8),  # split ring kernel: K neither 128 nor 256, K % 16 == 8 tail, N % 128 tails, M = 1
          (70, 30, 40), (45, 100, 72)]       # N % 8 != 0: nm_linear under both settings (NB = 1; NB = 2 with a column tail)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def inputs(M, N, K):
    """fp32 CPU inputs of one shape plus the fp64 product x . w^T of the same fp32 values; made once, shared, never written to."""
    t = {"x": rnd(M, K, seed=1), "w": rnd(N, K, seed=2, scale=K**-0.5), "bias": rnd(N, seed=3), "pre": rnd(M, N, seed=4),
         "residual": rnd(M, N, seed=5)}
    gate = torch.relu(rnd(M, N, seed=6))  # a saved ReLU activation: about half exact zeros
    # planted entries, some in the last row and in the last four columns (distinct columns: N >= 8)
    for r, c in ((M - 1, N - 1), (0, 0), (M // 2, 2)):
        gate[r, c] = -0.0
    gate[M - 1, N - 3], gate[0, N - 2], gate[M // 2, 1] = -0.7, -1e-30, -3.0
    gate[M - 1, N - 4] = 1e-30
    t["gate"] = gate
    t["xw64"] = t["x"].double() @ t["w"].double().T
    return t


def reference(t, subset, act):
    """The contract in float64, in its order: `pre` before the activation, residual behind it, the gate last."""
    v = t["xw64"]
    if "bias" in subset:
        v = v + t["bias"].double()
    if "pre" in subset:
        v = v + t["pre"].double()
    if act == "relu":
        v = torch.relu(v)
    elif act == "gelu":
        v = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if "residual" in subset:
        v = v + t["residual"].double()
    if "gate" in subset:
        v = v * (t["gate"] > 0).double()
    return v


def bits(y):
    return y.contiguous().view(torch.int32)


class Runner:
    """ops.linear on the device for (subset, activation), results kept on the CPU (the gate checks compare two entries of the table)."""

    def __init__(self, t, dev, precision):
        self.t, self.precision, self.out = t, precision, {}
        self.d = {k: t[k].to(dev) for k in ("x", "w") + PARTS}

    def __call__(self, subset, act, **override):
        from nerfmatch_amd import ops

        key = (subset, act)
        if override or key not in self.out:
            kw = {p: self.d[p] for p in subset}
            kw.update(override)
            ops.LINEAR_PRECISION, keep = self.precision, ops.LINEAR_PRECISION
            try:
                y = ops.linear(self.d["x"], self.d["w"], act=ACTS[act], **kw).cpu()
            finally:
                ops.LINEAR_PRECISION = keep
            if override:
                return y
            self.out[key] = y
        return self.out[key]


def run_table(t, dev, precision, table=TABLE, digests=True):
    """-> {"err": max |y - fp64| over the table, "worst": its combination, "exact": failed bar-free checks, "digest_plain" / "digest_bias": sha256
    over the output bits of the combinations without / with a bias}."""
    run = Runner(t, dev, precision)
    zero = t["gate"] <= 0  # +0.0, -0.0 and the negative entries
    err, worst, exact = 0.0, None, []
    sha = {False: hashlib.sha256(), True: hashlib.sha256()}
    for subset, act in table:
        y = run(subset, act)
        e = (y.double() - reference(t, subset, act)).abs().max().item()
        if not e <= err:  # (a NaN anywhere wins)
            err, worst = e, "+".join(subset + (act,))
        if digests:
            sha["bias" in subset].update(bits(y).numpy().tobytes())
        if "gate" in subset:
            if bool((bits(y)[zero] != 0).any()):
                exact.append(f"{subset} {act}: an output under gate <= 0 is not +0.0")
            plain = run(tuple(p for p in subset if p != "gate"), act)
            if not torch.equal(bits(y)[~zero], bits(plain)[~zero]):
                exact.append(f"{subset} {act}: an output under gate > 0 differs from the call without the gate")
    # without bias and activation, an addend before the (absent) activation and one behind it are the same sum
    if not torch.equal(bits(run((), "none", pre=run.d["pre"])), bits(run((), "none", residual=run.d["pre"]))):
        exact.append("pre=P and residual=P differ without bias and activation")
    return {"err": err, "worst": worst, "exact": exact, "digest_plain": sha[False].hexdigest(), "digest_bias": sha[True].hexdigest()}


def main(argv):
    precision, idx = argv[0], [int(a) for a in argv[1:]]
    dev = torch.device("cuda:0")
    with torch.no_grad():
        rep = {"x".join(map(str, SHAPES[i])): run_table(inputs(*SHAPES[i]), dev, precision) for i in idx}
    torch.cuda.synchronize()
    print(json.dumps(rep))


if __name__ == "__main__":
    main(sys.argv[1:])
