"""The linear family against float64 on every kernel route: ops.linear's `pre` / `gate` epilogues (nm_linear with NB = 1 and 2, the split-bf16
small-grid and ring kernels, their coalesced and register-layout epilogues), ops.linear_t (the transposed pack), relu_bwd, the three
exact-erf GELU routes side by side, and LayerNorm at its outer widths.

    y = (act(x . w^T + bias + pre) + residual) * [gate > 0]

Other tests reach `pre` and `gate` only through inerf.GemmField, at a gradient-sized tolerance; GemmField is in turn the reference of the
fused points kernels, so a wrong row of the gate in a ragged tile or an activation on the wrong side of `pre` had nowhere to show."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import linear_family_worker as lf
from linear_family_worker import BARS, SHAPES, rnd
from nerfmatch_amd import _lib, ops

pytestmark = pytest.mark.gpu
WORKER = Path(lf.__file__).resolve()
PRECISIONS = ("fp32", "bf16x3")


def report(what, rep, bar):
    print(f"{what}: max |y - fp64| = {rep['err']:.3e} at {rep['worst']} (bar {bar:g}); exact checks failed: {rep['exact']}")


# ----------------------------------------------------------------------------------------------- 1. the epilogue truth table
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_epilogue_truth_table(gpu, built_lib, M, N, K, precision):
    """Every subset of {bias, pre, residual, gate} x {none, relu, gelu} against the contract evaluated in float64 from the same fp32 inputs.
    Bar-free: outputs under gate <= 0 (-0.0 included) are +0.0, outputs under gate > 0 (1e-30 included) are the bits of the call without
    the gate, and pre=P equals residual=P when neither bias nor activation stands between them."""
    rep = lf.run_table(lf.inputs(M, N, K), gpu, precision)
    report(f"linear {precision} {M}x{N}x{K}", rep, BARS[precision])
    assert not rep["exact"], rep["exact"]
    assert rep["err"] <= BARS[precision], (rep["err"], rep["worst"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_linear_epilogue_ring_kernel_at_k256(gpu, built_lib, precision):
    """K = 256 with more workgroups than two rounds of the chip: the split path's default route to the ring kernel (the small-grid form is
    taken up to 2 x CU count workgroups).  N = 768 is 6 column chunks; row tiles come in groups of 8, so floor(2 CUs / 48) + 1 groups
    exceed the limit; 37 rows more make the last tile ragged and leave 7 padded row tiles whose workgroups leave at once.  256 CUs:
    M = 11301.  The combinations with `pre` or `gate`, ReLU (the plain ones are test_linear_bf16x3's)."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    M, N, K = (2 * cus // 48 + 1) * 8 * 128 + 37, 768, 256
    assert -(-(-(-M // 128)) // 8) * 8 * 6 > 2 * cus
    table = [(s, "relu") for s in lf.SUBSETS if "pre" in s or "gate" in s]
    rep = lf.run_table(lf.inputs(M, N, K), gpu, precision, table, digests=False)
    report(f"linear {precision} {M}x{N}x{K}", rep, BARS[precision])
    assert not rep["exact"], rep["exact"]
    assert rep["err"] <= BARS[precision], (rep["err"], rep["worst"])


@pytest.mark.parametrize("M,N,K", [s for s in SHAPES if s[1] % 8])
def test_ragged_n_takes_nm_linear_under_both_settings(gpu, built_lib, M, N, K):
    """N % 8 != 0 is outside the split kernel's 16-byte row pieces: "bf16x3" must fall to nm_linear, i.e. return the bits of "fp32"."""
    t = lf.inputs(M, N, K)
    a, b = lf.Runner(t, gpu, "fp32"), lf.Runner(t, gpu, "bf16x3")
    differ = [(s, act) for s, act in lf.TABLE if not torch.equal(lf.bits(a(s, act)), lf.bits(b(s, act)))]
    assert not differ, differ


# ----------------------------------------------------------------------------------------------- 2. the A/B arms
def _child(env, precision="bf16x3", shapes=(0, 1, 2, 3)):
    res = subprocess.run([sys.executable, str(WORKER), precision, *map(str, shapes)], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=180)  # (interpreter + torch + HIP start-up and 4 x 50 small launches: seconds)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("env", [{"NM_GEMM_SMALL": "0", "NM_GEMM_COALESCED": "0"}, {"NM_GEMM_COALESCED": "0"}],
                         ids=["ring_kernel_register_epilogue", "small_grid_register_epilogue"])
def test_linear_epilogue_ab_arms(gpu, built_lib, env):
    """The switches are read once per process: a fresh child runs the bf16x3 table of the four small-grid shapes with the ring kernel in
    the small-grid kernel's place and / or the register-layout epilogue in the coalesced one's.  Same bars and exact checks.  That the arm
    was taken shows in the bits: the products and their order are the same on every route, so the combinations without a bias are
    bit-identical to this process's default route, while the register-layout epilogue ADDS the bias to the finished sum where the
    coalesced one starts the accumulators from it -- over the 24 bias combinations of a shape some output rounds differently."""
    rep = _child(env)
    assert set(rep) == {"x".join(map(str, s)) for s in SHAPES[:4]}
    for (M, N, K) in SHAPES[:4]:
        r = rep[f"{M}x{N}x{K}"]
        report(f"linear bf16x3 {M}x{N}x{K} {env}", r, BARS["bf16x3"])
        assert not r["exact"], r["exact"]
        assert r["err"] <= BARS["bf16x3"], (r["err"], r["worst"])
        mine = lf.run_table(lf.inputs(M, N, K), gpu, "bf16x3")
        assert r["digest_plain"] == mine["digest_plain"], "the arms differ in a combination without bias"
        assert r["digest_bias"] != mine["digest_bias"], "the child's bits are the default route's: the switch was not taken"


# ----------------------------------------------------------------------------------------------- 3. linear_t
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M,No,Ki", [(333, 256, 128), (97, 128, 256), (131, 8, 96), (45, 96, 8), (70, 3, 128)])
def test_linear_t(gpu, built_lib, M, No, Ki, precision):
    """dy (M, No) @ W (No, Ki), a layer's input gradient: nm_linear_pack_t_bf16x3 + nm_linear_bf16x3 on the split path, the cached transposed
    copy + nm_linear otherwise (No = 3: always, zero-padded to 8).  The blob / copy follows an in-place update of W (the cache key carries
    `_version`): the result is then the bits of the same call on a tensor the cache has never seen."""
    dy, w = rnd(M, No, seed=1), rnd(No, Ki, seed=2, scale=No**-0.5)
    dyg, wg = dy.to(gpu), w.to(gpu)
    ops.LINEAR_PRECISION, keep = precision, ops.LINEAR_PRECISION
    try:
        y = ops.linear_t(dyg, wg)
        wg.add_(1.0)
        y_new, y_fresh = ops.linear_t(dyg, wg), ops.linear_t(dyg, wg.clone())  # (a new tensor: nothing cached for it)
    finally:
        ops.LINEAR_PRECISION = keep
    err = (y.cpu().double() - dy.double() @ w.double()).abs().max().item()
    print(f"linear_t {precision} {M}x{No}x{Ki}: max |y - fp64| = {err:.3e} (bar {BARS[precision]:g})")
    assert err <= BARS[precision]
    assert torch.equal(y_new, y_fresh) and not torch.equal(y_new, y)
    # (and the new weights' product it is: every output moved by its row sum of dy, 1e-3 of the largest entry is far inside that)
    want = dy.double() @ (w.double() + 1.0)
    assert ((y_new.cpu().double() - want).abs().max() / want.abs().max()).item() < 1e-3


# ----------------------------------------------------------------------------------------------- 4. relu_bwd; the GELU routes
@pytest.mark.parametrize("n", [4, 1024 * 256, 1028])
def test_relu_bwd(gpu, built_lib, n):
    h, dh = torch.relu(rnd(n, seed=1)), rnd(n, seed=2)
    h[0], h[1], h[n - 1], h[n - 2] = -0.0, 1e-30, -0.0, 1e-30
    want = torch.where(h > 0, dh, torch.zeros(()))
    got = ops.relu_bwd(h.to(gpu), dh.to(gpu)).cpu()
    assert torch.equal(lf.bits(got), lf.bits(want))
    assert got[1] == dh[1] and got[n - 2] == dh[n - 2] and lf.bits(got)[0] == 0


def test_relu_bwd_refuses_a_count_that_is_no_multiple_of_4(gpu, built_lib):
    h = torch.ones(6, device=gpu)
    with pytest.raises(_lib.NerfmatchAmdError):
        ops.relu_bwd(h, h)


def test_gelu_routes_at_probe_values(gpu, built_lib):
    """The exact-erf GELU is written three times (train.hip, gemm.hip, gemm_bf16.hip).  One column of probes -- zeros of both signs, the
    linear range, the tails where 1 + erf cancels, and arguments far outside erff's table -- through ops.gelu, ops.gelu_bwd (dh = 1) and
    ops.linear(act=GELU) with an identity weight, against float64 0.5 u (1 + erf(u / sqrt 2)) and its derivative Phi(u) + u phi(u).
    Bar: 1e-6 absolute; on the split path the operand itself carries 2^-16 |u| (x = hi + lo in bf16).
    (A fourth and a fifth form, the chained kernels' polynomial gelu_erf of bf16x3.h and gelu_grad of encoder_tail_bwd.hip, see the same
    probes in test_encoder_tail_stages_gpu.py and test_fine_layer_stages_gpu.py.)"""
    probes = [0.0, -0.0, 1e-8, -1e-8, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0, 1e4]
    u = torch.tensor(probes, dtype=torch.float32).repeat(8)  # 120 values = 15 rows of the K = 8 identity product
    u64 = u.double()
    cdf = 0.5 * (1.0 + torch.erf(u64 / math.sqrt(2.0)))
    want, want_d = u64 * cdf, cdf + u64 * torch.exp(-0.5 * u64 * u64) / math.sqrt(2.0 * math.pi)
    ug = u.to(gpu)
    err = {"gelu": (ops.gelu(ug).cpu().double() - want).abs(), "gelu_bwd": (ops.gelu_bwd(ug, torch.ones_like(ug)).cpu().double() - want_d).abs()}
    for precision in PRECISIONS:
        ops.LINEAR_PRECISION, keep = precision, ops.LINEAR_PRECISION
        try:
            y = ops.linear(ug.view(-1, 8), torch.eye(8, device=gpu), act=_lib.NM_ACT_GELU)
        finally:
            ops.LINEAR_PRECISION = keep
        err[f"linear {precision}"] = (y.cpu().double().reshape(-1) - want).abs()
    for k, e in err.items():
        i = int(e.argmax())
        print(f"{k}: max |err| {e.max().item():.3e} at u = {u[i].item():g}")
    for k, e in err.items():
        bar = 1e-6 + (2.0**-16 * u64.abs() if k == "linear bf16x3" else 0.0)
        assert bool((e <= bar).all()), (k, [(probes[i % len(probes)], e[i].item()) for i in torch.nonzero(e > bar).flatten().tolist()[:8]])


# ----------------------------------------------------------------------------------------------- 5. LayerNorm widths
def _ln_case(rows, dim):
    x = rnd(rows, dim, seed=1, scale=3.0) + 0.5
    if rows > 1:
        x[rows - 1] = 2.5  # a row of constants (sums of 2.5 are exact in fp32: mean 2.5, variance 0)
    return x, 1 + 0.1 * rnd(dim, seed=2), 0.1 * rnd(dim, seed=3), rnd(rows, dim, seed=4)


def _ln64(x, g, b, eps=1e-5):
    x = x.double()
    xc = x - x.mean(-1, keepdim=True)
    return xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps) * g.double() + b.double()


@pytest.mark.parametrize("rows", [1, 3, 701])
@pytest.mark.parametrize("dim", [64, 512])
def test_layernorm_outer_widths(gpu, built_lib, rows, dim):
    """nm_layernorm / nm_layernorm2 / nm_layernorm_bwd at the narrowest and the widest instantiation (PER = 1 and 8; 128 and 256 are
    test_layernorm's and test_layernorm_backward's), at those tests' bars: 1e-5 forward, 1e-5 of the largest entry backward."""
    x, g, b, dy = _ln_case(rows, dim)
    xg, gg, bg = x.to(gpu), g.to(gpu), b.to(gpu)
    want = _ln64(x, g, b)
    y = ops.layernorm(xg, gg, bg).cpu()
    assert (y.double() - want).abs().max().item() < 1e-5
    if rows > 1:
        assert torch.equal(y[rows - 1], b)  # variance 0: the output is beta
    # the pair launch: this tensor first and second, beside a 5-row neighbour with other parameters
    x1, g1, b1 = rnd(5, dim, seed=5), 1 + 0.1 * rnd(dim, seed=6), 0.1 * rnd(dim, seed=7)
    ln0, ln1 = SimpleNamespace(weight=gg, bias=bg, eps=1e-5), SimpleNamespace(weight=g1.to(gpu), bias=b1.to(gpu), eps=1e-5)
    for (ya, yb) in (ops.layernorm_pair(xg, ln0, x1.to(gpu), ln1), ops.layernorm_pair(x1.to(gpu), ln1, xg, ln0)[::-1]):
        assert (ya.cpu().double() - want).abs().max().item() < 1e-5
        assert (yb.cpu().double() - _ln64(x1, g1, b1)).abs().max().item() < 1e-5

    x64, g64 = x.double().requires_grad_(), g.double().requires_grad_()
    b64 = b.double().requires_grad_()
    with torch.enable_grad():
        _ln64(x64, g64, b64).backward(dy.double())
    dx, dg, db = ops.layernorm_bwd(xg, gg, dy.to(gpu))

    def rel(a, ref):
        return ((a.cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-3)).item()

    assert bool(torch.isfinite(dx).all())
    # (the constant row's dx is 1 / sqrt(eps) = 316 x larger than the others': each part against its own scale)
    parts = [slice(0, rows - 1), slice(rows - 1, rows)] if rows > 1 else [slice(0, 1)]
    for p in parts:
        assert rel(dx[p], x64.grad[p]) < 1e-5
    assert rel(dg, g64.grad) < 1e-5 and rel(db, b64.grad) < 1e-5
    dx_only, none_g, none_b = ops.layernorm_bwd(xg, gg, dy.to(gpu), param_grads=False)
    assert torch.equal(dx_only, dx) and none_g is None and none_b is None


@pytest.mark.parametrize("dim", [192, 1024])
def test_layernorm_refuses_other_widths(gpu, built_lib, dim):
    """The kernels exist for 64, 128, 256 and 512 columns; another multiple of 64 is an error, not a silent no-op."""
    x, g = torch.ones(3, dim, device=gpu), torch.ones(dim, device=gpu)
    ln = SimpleNamespace(weight=g, bias=g, eps=1e-5)
    with pytest.raises(_lib.NerfmatchAmdError):
        ops.layernorm(x, g, g)
    with pytest.raises(_lib.NerfmatchAmdError):
        ops.layernorm_pair(x, ln, x, ln)
    with pytest.raises(_lib.NerfmatchAmdError):
        ops.layernorm_bwd(x, g, x)
