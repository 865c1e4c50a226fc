"""attn32_fp8_kernel (csrc/attention_fp8.hip) against an emulation of its own arithmetic (tests/attention_fp8_util.py) and against inputs
whose output is known exactly, at every edge of its 64-key tiles and its 4-slot LDS ring.  nm_attention_fp8 is called directly, so
that every shape reaches the kernel (ops._use_fp8 would send L, S <= 64 elsewhere); operands are contiguous (the strided door is pinned
to this one bit for bit in test_attention_routes_gpu.py); the workspace is filled with 0xFF bytes before each call and the output with
NaN.  The kernel's stated bounds against float64 (0.075 max|v|, 8 % rms: test_matcher_gpu.py) are printed beside the new figures."""
import pytest
import torch

import attention_fp8_util as f8
from nerfmatch_amd import _lib

pytestmark = pytest.mark.gpu


def run(gpu, c, q=None, k=None, v=None):
    """nm_attention_fp8 on the case's operands (or the given replacements) -> (B, L, C) float32 on the CPU."""
    lib = _lib.lib()
    q, k, v = (t.to(gpu).contiguous() for t in (c.q if q is None else q, c.k if k is None else k, c.v if v is None else v))
    C = 32 * c.H
    ws = torch.full((lib.nm_attention_fp8_workspace_bytes(c.B, c.S, c.H),), 0xFF, device=gpu, dtype=torch.uint8)
    out = torch.full((c.B, c.L, C), float("nan"), device=gpu)
    rc = lib.nm_attention_fp8(_lib.dptr(q), _lib.dptr(k), _lib.dptr(v), C, C, C, c.B, c.L, c.S, c.H, float(c.scale), _lib.dptr(ws, torch.uint8),
                              _lib.dptr(out), _lib.stream())
    assert rc == 0
    return out.cpu()


def worst(got, emu, allow):
    """Largest |got - emu| / allow (0 / 0 = 0: an output the emulation knows exactly and the kernel meets exactly)."""
    err = (got.double() - emu).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / allow).max().item()


@pytest.mark.parametrize("case", f8.RANDOM, ids=f8.case_id)
def test_kernel_against_the_emulation(gpu, built_lib, case):
    """|kernel - emulation| <= allow on EVERY output, allow = A_round + A_flip of attention_fp8_util.emulate: about 2^-23 (nt + 4) of the
    output's scale where no probability of the row sits on a rounding boundary of e4m3 (at least 90 % of the rows of every case), one
    e4m3 step of that probability more where one does.  The stated bounds of the kernel are four orders of magnitude wider.
    Measured on the MI355X (MEASURED below): the largest |kernel - emulation| / allow over all cases is 0.066; the largest
    |kernel - emulation| is 3.9e-7, against a kernel-to-float64 error of up to 0.029 max|v| (rms 2.5 - 5.7 % of the output's rms, the same
    figures to three digits for kernel and emulation).  With exact products summed in float64 in place of mfma_fp8 the same ratio is
    3 - 2800: see mfma_fp8 in attention_fp8_util.py for what the matrix core does to the products."""
    c = f8.random_emulated(case)
    got = run(gpu, c)
    assert torch.isfinite(got).all()
    ratio = worst(got, c.out, c.allow)
    err = (got.double() - c.out).abs()
    kmx, krms = f8.loose_figures(got, c.ref, c.v)
    emx, erms = f8.loose_figures(c.out, c.ref, c.v)
    print(f"fp8 attention {f8.case_id(case)}: max |kernel - emulation| / allow {ratio:.3f} (max |kernel - emulation| {err.max():.2e}, "
          f"{(err > 0).double().mean() * 100:.0f} % of outputs differ), flagged rows {100 * c.flagged_rows:.2f} %;  against float64: kernel max "
          f"{kmx:.4f} max|v| rms {100 * krms:.2f} %, emulation max {emx:.4f} max|v| rms {100 * erms:.2f} % (stated bounds 0.075, 8 %)")
    assert (err <= c.allow).all(), f"{(err > c.allow).sum().item()} outputs beyond the allowance, worst ratio {ratio:.3f}"


@pytest.mark.parametrize("shape", f8.COUNT, ids=f8.case_id)
def test_count_probe(gpu, built_lib, shape):
    """q = 0, one 1 per value row: every probability is exactly 1 and out = (keys of this column) / S, exact in the kernel up to the
    reciprocal, one product and v_exp_f32(0).  One key missed, or met twice, moves an output by 1 / S >= 2^-10."""
    c = f8.count_probe(*shape)
    got = run(gpu, c).double()
    err = (got - c.want).abs()
    print(f"fp8 count probe {f8.case_id(shape)}: max error {err.max():.3e} (1 / S = {1 / c.S:.3e})")
    assert (err <= 2.0 ** -20 * c.want).all()


@pytest.mark.parametrize("shape", f8.SELECT, ids=f8.case_id)
def test_select_probe(gpu, built_lib, shape):
    """Query l picks key (37 l + 5) % S with a lead of 32 log2 units: out[l] = v[that key], small integers that e4m3 holds exactly.  A
    key in the wrong place, a stale ring slot or value rows permuted against the probabilities return another row."""
    c = f8.select_probe(*shape)
    got = run(gpu, c).double()
    err = (got - c.want).abs()
    print(f"fp8 select probe {f8.case_id(shape)}: max error {err.max():.3e}")
    assert (err <= 2.0 ** -20 * 6.0).all()


DEGENERATE = (2, 70, 129, 5, (), 21, 0)


def test_degenerate_heads(gpu, built_lib):
    """A head whose V is zero (output exactly 0), a head whose K is zero (uniform softmax), a query row of zeros, and one (batch, head)
    whose K and V are 2^10 times the others': the scales are per (batch, head), so every OTHER (batch, head) returns the bits it
    returns without the inflation."""
    B, L, S, H = DEGENERATE[:4]
    base = f8.random_emulated(DEGENERATE)
    q, k, v = base.q.clone(), base.k.clone(), base.v.clone()
    head = lambda h: slice(32 * h, 32 * h + 32)
    v[:, :, head(1)] = 0.0
    k[:, :, head(2)] = 0.0
    q[:, 7] = 0.0
    k2, v2 = k.clone(), v.clone()
    k2[1, :, head(3)] *= 1024.0
    v2[1, :, head(3)] *= 1024.0
    other = torch.ones(B, L, 32 * H, dtype=torch.bool)
    other[1, :, head(3)] = False
    outs = []
    for kk, vv in ((k, v), (k2, v2)):
        f8.assert_scales_agree(q, kk, vv, H, base.scale)
        emu, allow, flagged = f8.emulate(q, kk, vv, H, base.scale)
        got = run(gpu, base, q, kk, vv)
        print(f"fp8 degenerate heads: max |kernel - emulation| / allow {worst(got, emu, allow):.3f}, flagged rows {100 * flagged:.2f} %")
        assert ((got.double() - emu).abs() <= allow).all()
        assert (got[:, :, head(1)] == 0).all()
        # uniform softmax: the mean of the value rows (as quantised: the loose bound), and the same bits for every query
        assert (got[:, :, head(2)].double() - v.double()[:, :, head(2)].mean(1, keepdim=True)).abs().max() < 0.075 * v.abs().max()
        assert torch.equal(got[:, :, head(2)], got[:, :1, head(2)].expand(B, L, 32))
        outs.append(got)
    assert torch.equal(outs[0][other], outs[1][other])
    assert not torch.equal(outs[0][~other], outs[1][~other])


@pytest.mark.parametrize("n", [-7, 5])
@pytest.mark.parametrize("case", [f8.RANDOM[11], f8.RANDOM[13]], ids=f8.case_id)
def test_power_of_two_invariance(gpu, built_lib, case, n):
    """The header's 'scaling, all powers of two (exact)': (q 2^-n, k 2^n) gives the same bits, v 2^n gives exactly 2^n times the output
    (nothing under- or overflows at n = -7, 5 with N(0,1) operands)."""
    c = f8.random_emulated(case)
    f = 2.0 ** n
    want = run(gpu, c)
    assert torch.equal(run(gpu, c, q=c.q / f, k=c.k * f), want)
    assert torch.equal(run(gpu, c, v=c.v * f), want * f)


# MEASURED on the MI355X: case, max |kernel - emulation| / allow, max |kernel - emulation|, flagged rows (the probes: within 3e-9)
#   1x33x1x3    0.000  0        0.00 %      1x129x193x8  0.025  8.6e-8  0.29 %      1x70x65x3-planted    0.035  9.7e-8  0.48 %
#   1x1x63x1    0.014  3.3e-8   0.00 %      1x70x256x3   0.022  7.3e-8  1.90 %      1x129x193x1-planted  0.016  6.0e-8  0.00 %
#   2x70x64x5   0.066  1.5e-7   0.29 %      1x1x257x8    0.006  2.2e-8  0.00 %      2x33x320x5-planted   0.051  3.9e-7  1.82 %
#   1x129x65x8  0.044  1.3e-7   0.10 %      1x129x320x1  0.019  6.2e-8  0.00 %      1x70x321x8-planted   0.032  1.9e-7  1.43 %
#   1x33x128x1  0.035  7.7e-8   0.00 %      2x70x321x5   0.014  6.0e-8  1.29 %      1x129x577x3-planted  0.018  2.4e-7  0.78 %
#   1x70x129x3  0.031  8.4e-8   0.00 %      1x33x577x3   0.008  4.2e-8  2.02 %      2x70x129x5-spread    0.026  7.0e-8  0.00 %
#   2x33x192x5  0.023  7.6e-8   0.61 %      degenerate heads 0.035, 0.026 (0.57 %)
