"""CPU: the helper of the row-reduction tests -- the slicing mirrors against hand-computed plans and the library's own workspace queries, the
probes' exactness claims in plain fp32 numpy under several summation orders, and the fp64 references against torch autograd in double."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_reduce_util as tr
from nerfmatch_amd import _lib


# (M, N, K) -> (tiles, splits, rows_per, first guess), worked out by hand from nm_linear_wgrad
FP32_PLANS = {
    (33, 64, 64): (1, 1, 64, 1), (65, 64, 64): (1, 1, 96, 1), (129, 64, 64): (1, 1, 160, 1), (257, 64, 64): (1, 2, 160, 2),
    (4097, 64, 64): (1, 15, 288, 16), (300, 4, 4): (1, 2, 160, 2), (300, 68, 132): (6, 2, 160, 2), (4800, 256, 256): (16, 15, 320, 16),
}
# (M, N, K) -> (tiles, slices, rows_per, rpw, rows of the last slice's four wavefronts, first guess), from wb_slices / nm_linear_wgrad_bf16x3
BF16X3_PLANS = {
    (1, 2, 4): (1, 1, 64, 16, (1, 0, 0, 0), 1), (17, 64, 128): (1, 1, 64, 16, (16, 1, 0, 0), 1), (49, 64, 128): (1, 1, 64, 16, (16, 16, 16, 1), 1),
    (33, 64, 128): (1, 1, 64, 16, (16, 16, 1, 0), 1), (65, 64, 128): (1, 1, 128, 32, (32, 32, 1, 0), 1),
    (193, 64, 128): (1, 1, 256, 64, (64, 64, 64, 1), 1), (257, 64, 128): (1, 2, 192, 48, (48, 17, 0, 0), 2),
    (513, 64, 128): (1, 3, 192, 48, (48, 48, 33, 0), 3), (4097, 64, 128): (1, 17, 256, 64, (1, 0, 0, 0), 17),
    (300, 70, 132): (4, 2, 192, 48, (48, 48, 12, 0), 2), (100000, 64, 128): (1, 121, 832, 208, (160, 0, 0, 0), 128),
    (100000, 4096, 4096): (2048, 1, 100032, 25008, (25008, 25008, 25008, 24976), 1),  # one partial tile set is above the 16 MiB bound: still one slice
}


def test_plans_match_hand_computed_rows():
    for shape, want in FP32_PLANS.items():
        assert tuple(tr.wgrad_plan_fp32(*shape)) == want, shape
    for shape, want in BF16X3_PLANS.items():
        assert tuple(tr.wgrad_plan_bf16x3(*shape)) == want, shape
    assert tuple(tr.col_sum_plan(1)) == (1, 1, 1) and tuple(tr.col_sum_plan(63)) == (1, 63, 1) and tuple(tr.col_sum_plan(127)) == (1, 127, 1)
    assert tuple(tr.col_sum_plan(128)) == (2, 64, 2) and tuple(tr.col_sum_plan(129)) == (2, 65, 2)
    assert tuple(tr.col_sum_plan(16385)) == (256, 65, 253) and 16385 - 252 * 65 == 5  # 256 chunks guessed, 253 launched, the last of 5 rows
    assert [tr.ln_bwd_grid(r, 256, True) for r in (1, 4, 5, 9, 17, 1025, 2053)] == [1, 1, 2, 3, 5, 256, 256]
    assert [tr.ln_bwd_grid(r, 256, False) for r in (1, 1025, 2053)] == [1, 257, 512]
    assert [tr.ln_bwd_grid(r, 304, True) for r in (4 * 304 + 1, 8 * 304 + 5)] == [304, 304]


def test_slices_cover_the_rows_once():
    """The plan's slices and wavefront quarters tile [0, M) without gap or overlap (what the kernels' m0 / m1 arithmetic assumes)."""
    for M in (1, 17, 49, 63, 64, 65, 193, 257, 300, 513, 4097, 100000):
        for N, K in ((2, 4), (64, 128), (70, 132), (768, 256)):
            p = tr.wgrad_plan_bf16x3(M, N, K)
            assert 4 * p.rpw >= p.rows_per and (p.slices - 1) * p.rows_per < M <= p.slices * p.rows_per
            assert sum(p.last_wave_rows) == M - (p.slices - 1) * p.rows_per
            if N % 4 == 0:
                q = tr.wgrad_plan_fp32(M, N, K)
                assert q.rows_per % 32 == 0 and (q.splits - 1) * q.rows_per < M <= q.splits * q.rows_per and q.splits <= q.first_guess <= 16


def test_mirrors_agree_with_the_library(built_lib):
    h = _lib.lib()
    shapes = list(BF16X3_PLANS) + list(FP32_PLANS) + [(19200, 768, 256), (1000, 70, 132), (5000, 192, 100), (40000, 8, 8), (7, 8, 8)]
    for M, N, K in shapes:
        assert h.nm_linear_wgrad_workspace_bytes(M, N, K) == tr.wgrad_workspace_bytes(M, N, K), (M, N, K)
        assert tr.wgrad_plan_bf16x3(M, N, K).slices <= tr.wgrad_plan_bf16x3(M, N, K).first_guess  # the workspace is never too small
    assert h.nm_linear_wgrad_workspace_bytes(4097, 64, 128) == 17 * 64 * 128 * 4  # more slices than the fp32 kernel's 16
    for M in (1, 3, 63, 64, 127, 128, 129, 16385, 100000):
        for N in (1, 255, 257):
            assert h.nm_col_sum_workspace_bytes(M, N) == tr.col_sum_plan(M).chunks * N * 4, (M, N)
            assert tr.col_sum_plan(M).parts <= tr.col_sum_plan(M).chunks
    assert h.nm_linear_wgrad_workspace_bytes(0, 64, 64) == 0 and h.nm_col_sum_workspace_bytes(0, 4) == 0


# ------------------------------------------------------------------------------------------------------------ exactness of the probes
def _sum_orders(terms):
    """fp32 sums of `terms` (M, ...) over axis 0 in several orders: sequential, reversed, four interleaved partial sums, slices of 48, pairwise."""
    t = terms.astype(np.float32)

    def seq(a):
        s = np.zeros(a.shape[1:], np.float32)
        for row in a:
            s = (s + row).astype(np.float32)
        return s

    out = [seq(t), seq(t[::-1])]
    out.append(((seq(t[0::4]) + seq(t[1::4])).astype(np.float32) + (seq(t[2::4]) + seq(t[3::4])).astype(np.float32)).astype(np.float32))
    out.append(seq(np.stack([seq(t[i : i + 48]) for i in range(0, len(t), 48)])))
    a = t
    while len(a) > 1:
        if len(a) % 2:
            a = np.concatenate([a, np.zeros((1,) + a.shape[1:], np.float32)])
        a = (a[0::2] + a[1::2]).astype(np.float32)
    out.append(a[0])
    return out


@pytest.mark.parametrize("probe", ["int", "a", "b"])
def test_probe_partial_sums_are_exact_in_fp32(probe):
    """Every term the split-bf16 kernel forms (hi.hi, hi.lo, lo.hi) and every partial sum of them is an fp32 number: all orders give fp64's bits."""
    M, N, K = 512, 6, 8
    dy, x = tr.wgrad_operands(M, N, K, probe)
    (dh, dl), (xh, xl) = tr.bf16_split(dy), tr.bf16_split(x)
    assert torch.equal(dh + dl, dy) and torch.equal(xh + xl, x)  # the split loses nothing
    if probe == "int":
        assert not dl.any() and not xl.any()
    elif probe == "a":
        assert not dl.any() and torch.equal(xh.abs(), torch.ones_like(x)) and torch.equal(xl.abs(), torch.full_like(x, tr.SPLIT_LO))
    else:
        assert not xl.any() and torch.equal(dh.abs(), torch.ones_like(dy)) and torch.equal(dl.abs(), torch.full_like(dy, tr.SPLIT_LO))
    assert not (dl.any() and xl.any())  # never both: lo.lo is dropped by design
    truth = tr.wgrad_ref(dy, x).numpy()
    terms = [np.einsum("mn,mk->mnk", a.numpy().astype(np.float64), b.numpy().astype(np.float64)) for a, b in ((dh, xh), (dh, xl), (dl, xh))]
    allterms = np.concatenate(terms)  # the kernel interleaves the three products; any order must do
    assert np.array_equal(allterms.astype(np.float32).astype(np.float64), allterms)
    for s in _sum_orders(allterms) + _sum_orders(allterms[np.random.default_rng(0).permutation(len(allterms))]):
        assert np.array_equal(s.astype(np.float64), truth)
    # what a dropped cross term would cost: exactly 2^-12 sum(integer operand) per output, nonzero somewhere
    if probe != "int":
        drop = terms[1 if probe == "a" else 2].sum(0)
        assert np.abs(drop).max() >= tr.SPLIT_LO and np.array_equal(drop, np.round(drop / tr.SPLIT_LO) * tr.SPLIT_LO)
    for s in _sum_orders(dy.numpy()):  # the fused db
        assert np.array_equal(s.astype(np.float64), tr.col_sum_ref(dy).numpy())


def test_integer_probe_stays_below_2_24():
    assert 16 * 10**6 < 2**24 and 4 * 10**6 + 4 < 2**24  # products up to 16, column sums up to 4 (+ a prefill of 4) over M <= 10^6 rows
    v = tr.int_probe((1000, 7), 3)
    assert v.min() == -4 and v.max() == 4 and torch.equal(v, v.round()) and torch.equal(v.to(torch.bfloat16).float(), v)
    assert torch.equal(tr.int_probe((1000, 7), 3), v) and not torch.equal(tr.int_probe((1000, 7), 4), v)


@pytest.mark.parametrize("dim", [64, 512])
def test_layernorm_probe_is_exact(dim):
    """mean 0, variance 1 and every intermediate of the backward an fp32 number: the fp32 evaluation of the kernel's formula equals fp64."""
    x, gamma, dy = tr.layernorm_probe(9, dim, seed=dim)
    assert torch.equal(x.abs(), torch.ones_like(x)) and not x.sum(-1).any() and len({tuple(r.tolist()) for r in x}) > 1
    assert gamma.min() >= 1 and gamma.max() <= 3 and dy.abs().max() <= 4
    dx, dg, db = tr.layernorm_bwd_ref(x, gamma, dy, 0.0)
    for t in (dx, dg, db):
        assert torch.equal(t.float().double(), t)
    g = dy * gamma
    for perm in (torch.arange(dim), torch.randperm(dim, generator=tr.gen(1))):  # the row sums in two orders, sequentially, in fp32
        sg, sgx = torch.zeros(9), torch.zeros(9)
        for c in perm:
            sg, sgx = sg + g[:, c], sgx + g[:, c] * x[:, c]
        dx32 = 1.0 * ((g - (sg / dim)[:, None]) - x * (sgx / dim)[:, None])
        assert torch.equal(dx32.double(), dx)


# ------------------------------------------------------------------------------------------------------------ references against autograd
def test_references_agree_with_autograd_in_double():
    with torch.enable_grad():
        g = tr.gen(5)
        M, N, K = 37, 6, 10
        x = torch.randn(M, K, generator=g, dtype=torch.float64)
        w = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(N, generator=g, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(M, N, generator=g, dtype=torch.float64)
        F.linear(x, w, b).backward(dy)
        assert torch.allclose(tr.wgrad_ref(dy, x), w.grad, rtol=1e-13, atol=1e-13) and torch.allclose(tr.col_sum_ref(dy), b.grad, rtol=1e-13, atol=1e-13)

        rows, dim = 11, 64
        x = (torch.randn(rows, dim, generator=g, dtype=torch.float64) * 3 + 0.5).requires_grad_()
        gm = (1 + 0.1 * torch.randn(dim, generator=g, dtype=torch.float64)).requires_grad_()
        bt = torch.zeros(dim, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(rows, dim, generator=g, dtype=torch.float64)
        F.layer_norm(x, (dim,), gm, bt, eps=1e-5).backward(dy)
        dx, dg, db = tr.layernorm_bwd_ref(x.detach(), gm.detach(), dy, 1e-5)
        assert torch.allclose(dx, x.grad, rtol=1e-11, atol=1e-12) and torch.allclose(dg, gm.grad, rtol=1e-11, atol=1e-12)
        assert torch.allclose(db, bt.grad, rtol=1e-13, atol=1e-13)

        f = torch.randn(rows, dim, generator=g, dtype=torch.float64)
        f[3] *= 1e-3
        f[4] *= 1e3
        f = f.requires_grad_()
        (f / (f.norm(dim=-1, keepdim=True) + 1e-6)).backward(dy)
        df, r = tr.l2norm_bwd_ref(f.detach(), dy)
        assert torch.allclose(df, f.grad, rtol=1e-10, atol=0) and torch.equal(r, f.detach().norm(dim=-1, keepdim=True))
    df0, r0 = tr.l2norm_bwd_ref(torch.zeros(2, 64), torch.ones(2, 64))  # the zero row: dy / e, finite
    assert not r0.any() and torch.equal(df0, torch.full((2, 64), 1.0 / 1e-6, dtype=torch.float64))
