"""GPU: the data-movement glue of csrc/matcher_misc.hip one kernel at a time, at ragged tiles, idle thread groups and strided arguments.

Copies are checked bit for bit against torch indexing; the only bars are those of the sine / cosine columns (the project's 1e-6 / 2e-6 against the
fp64 oracle), of the Fourier backward (per element, from the fp32 roundings of its terms) and of feature_normalize (from its two roundings)."""
import pytest
import torch

from nerfmatch_amd import _lib, ops
from nerfmatch_amd._lib import NerfmatchAmdError, dptr, stream
from oracle import matcher_oracle as mo

pytestmark = pytest.mark.gpu


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=gen(seed))


def bits_equal(a, b):
    """Same shape and the same fp32 bit patterns (so that +0.0 and -0.0 differ)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ nchw_to_tokens
@pytest.mark.parametrize("B,Cc,h,w", [(1, 1, 1, 1), (2, 33, 5, 7), (3, 32, 4, 8), (1, 65, 1, 33), (2, 40, 9, 11)])
def test_nchw_to_tokens_ragged_tiles(gpu, built_lib, B, Cc, h, w):
    """The 32x32 LDS transpose with partial tiles on both sides, B > 1, and a sine table larger than the map: one add per element, so the fp32
    torch expression is the truth bit for bit."""
    x = rnd(B, Cc, h, w, seed=1)
    assert bits_equal(ops.nchw_to_tokens(x.to(gpu)), x.flatten(-2).permute(0, 2, 1))
    for th, tw in ((h, w), (h + 3, w + 2)):
        pe = rnd(Cc, th, tw, seed=2)
        ref = (x + pe[None, :, :h, :w]).flatten(-2).permute(0, 2, 1)
        assert bits_equal(ops.nchw_to_tokens(x.to(gpu), pe.to(gpu)), ref), (th, tw)
    for th, tw in ((h - 1, w + 2), (h + 3, w - 1)):  # a table smaller than the map on either side
        if th > 0 and tw > 0:
            with pytest.raises(NerfmatchAmdError):
                ops.nchw_to_tokens(x.to(gpu), rnd(Cc, th, tw, seed=3).to(gpu))


# ------------------------------------------------------------------------------------------------------------ cat_fourier
BIG = torch.tensor([[123.456, -77.7, 301.25]])  # the large-argument points of test_tokens_pe_fourier (metres x 2^14)
CF_GRID = [(Cc, F) for Cc in (1, 8, 13, 256) for F in (1, 4, 15)]


def points(n, seed):
    return (torch.rand(n, 3, generator=gen(seed)) * 8 - 4).float()  # |x| <= 4


@pytest.mark.parametrize("Cc,F", CF_GRID)
def test_cat_fourier_layout_and_values(gpu, built_lib, Cc, F):
    for n in (1, 3, 300):
        feat, pt = rnd(n, Cc, seed=n), points(n, seed=n + 1)
        if n == 300:
            pt[:1] = BIG
            feat[1, 0] = -0.0
        ld = (Cc + 3 + 6 * F + 7) // 8 * 8
        out = ops.cat_fourier(feat.to(gpu), pt.to(gpu), F).cpu()
        assert out.shape == (n, ld)
        assert bits_equal(out[:, :Cc], feat) and bits_equal(out[:, Cc : Cc + 3], pt)
        assert bits_equal(out[:, Cc + 3 + 6 * F :], torch.zeros(n, ld - Cc - 3 - 6 * F))  # padding: exactly +0.0
        emb = mo.fourier_embed(pt.double(), F)[:, 3:]  # fp64 from the same fp32 points
        err = (out[:, Cc + 3 : Cc + 3 + 6 * F].double() - emb).abs().amax(-1)
        small = pt.abs().amax(-1) <= 4
        assert small.sum() >= n - 1
        assert err[small].max() < 1e-6
        if n == 300:
            assert not small[0] and err[0] < 2e-6


@pytest.mark.parametrize("Cc,F", CF_GRID)
def test_cat_fourier_bwd_per_element(gpu, built_lib, Cc, F):
    """d loss / d point against fp64 autograd of the oracle embedding from the fp32 points.  Per element (row, axis):
    |err| <= (F + 4) 2^-23 S,  S = |d_x| + sum_f 2^f (|d_sin| + |d_cos|):  2^f x is exact in fp32 and the sine / cosine are reduced in double, so
    each of the 2 F products carries the rounding of its factor and its own (2 x 2^-24 of its magnitude), the F differences and the F + 1
    additions one rounding each of a partial sum below S: (F/2 + 1.5) 2^-23 S in all, taken with a factor 2 of margin.  The padding columns of
    dy hold 1e30 and must not be read."""
    worst = 0.0
    for n in (1, 50):
        emb_w, ld = 3 + 6 * F, (Cc + 3 + 6 * F + 7) // 8 * 8
        pt, dy = points(n, seed=7 * n + F), rnd(n, ld, seed=Cc + n)
        dy[:, Cc + emb_w :] = 1e30
        d = dy[:, Cc : Cc + emb_w].double()
        with torch.enable_grad():
            x = pt.double().requires_grad_()
            (mo.fourier_embed(x, F) * d).sum().backward()
        sc = (2.0 ** torch.arange(F, dtype=torch.float64))[None, :, None]
        trig = d[:, 3:].reshape(n, F, 2, 3).abs().sum(2)  # |d_sin| + |d_cos| per (row, f, axis)
        S = d[:, :3].abs() + (sc * trig).sum(1)
        bar = (F + 4) * 2.0**-23 * S
        got = ops.cat_fourier_bwd(dy.to(gpu), pt.to(gpu), Cc, F).cpu().double()
        err = (got - x.grad).abs()
        worst = max(worst, (err / bar).max().item())
        assert (err <= bar).all(), f"n={n}: worst err / bar = {(err / bar).max().item():.3f}"
    print(f"cat_fourier_bwd C={Cc} F={F}: worst err / bar = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------ feature_normalize
def feature_normalize_ref(x):
    x = x.double()
    xc = x - x.mean(1, keepdim=True)
    return xc, xc / xc.norm(dim=-1).amax(-1)[:, None, None]


@pytest.mark.parametrize("B,N,D", [(1, 2, 4), (2, 20, 3), (2, 37, 96), (1, 300, 1000), (3, 5, 1024)])
def test_feature_normalize_thread_groups(gpu, built_lib, B, N, D):
    """G = 1024 / D thread groups: idle threads when D does not divide 1024 (D = 3, 96, 1000), idle groups when G > N (D = 3, 4).  x is centred
    in place within 2^-23 max|x| (the centroid is summed in fp64 and rounded once, the difference once); y within (D + 8) 2^-24 (|y| <= 1; the
    D-term fp32 norm dominates the roundings).  Each set's result is its own: the batched call equals per-set calls bit for bit."""
    G = 1024 // D
    assert {(2, 20, 3): G == 341 and G > N, (2, 37, 96): G == 10 and 1024 - G * D == 64, (1, 300, 1000): G == 1}.get((B, N, D), True)
    x = rnd(B, N, D, seed=D) * torch.tensor([1.0, 30.0, 0.01])[:B, None, None] + 0.5
    xc_ref, y_ref = feature_normalize_ref(x)
    xg = x.to(gpu)
    y = ops.feature_normalize(xg)
    ex = ((xg.cpu().double() - xc_ref).abs().amax((1, 2)) / (2.0**-23 * x.double().abs().amax((1, 2)))).max().item()
    ey = (y.cpu().double() - y_ref).abs().max().item() / ((D + 8) * 2.0**-24)
    print(f"feature_normalize ({B},{N},{D}): x err / bar = {ex:.3f}, y err / bar = {ey:.3f}")
    assert ex <= 1.0 and ey <= 1.0
    assert y.abs().max().item() <= 1.0 + 2.0**-22
    for b in range(B):
        xb = x[b : b + 1].clone().to(gpu)
        yb = ops.feature_normalize(xb)
        assert bits_equal(yb[0], y[b]) and bits_equal(xb[0], xg[b])


def test_feature_normalize_refuses_what_it_cannot_do(gpu, built_lib):
    with pytest.raises(NerfmatchAmdError):
        ops.feature_normalize(torch.zeros(1, 2, 1025, device=gpu))
    wide = rnd(2, 6, 16, seed=1).to(gpu)
    keep = wide.clone()
    for view in (wide[:, :, :8], wide.transpose(1, 2)):  # in place is the contract: no silent copy
        with pytest.raises(NerfmatchAmdError):
            ops.feature_normalize(view)
    assert torch.equal(wide, keep)


# ------------------------------------------------------------------------------------------------------------ gather_rows, assemble_matches
SLOT_CASES = [(max_k, count) for max_k in (1, 5, 257) for count in sorted({0, 1, max_k})]  # one thread block of assemble_matches is 256 slots


@pytest.mark.parametrize("dim", [3, 130])
@pytest.mark.parametrize("max_k,count", SLOT_CASES)
def test_gather_rows(gpu, built_lib, max_k, count, dim):
    """out[k] = src[ids[k]] for k < count, bit for bit; slots k >= count are not written (what ops.gather_rows documents)."""
    src = rnd(40, dim, seed=dim)
    src[0, 0] = -0.0
    ids = torch.randint(0, 40, (max_k,), generator=gen(max_k))
    ids[0] = 0
    cnt = torch.tensor([count], dtype=torch.int32, device=gpu)
    srcg, idsg = src.to(gpu), ids.to(gpu)
    got = ops.gather_rows(srcg, idsg, cnt)
    assert got.shape == (max_k, dim) and bits_equal(got[:count], src[ids[:count]])
    out = torch.full((max_k, dim), 7.0, device=gpu)
    _lib.check(_lib.lib().nm_gather_rows(dptr(srcg), dptr(idsg, torch.int64), dptr(cnt, torch.int32), max_k, dim, dptr(out), stream()), "nm_gather_rows")
    assert bits_equal(out[:count], src[ids[:count]]) and bits_equal(out[count:], torch.full((max_k - count, dim), 7.0))


def assemble_inputs(max_k, count, seed=0):
    pt2d, pt3d = rnd(50, 2, seed=seed + 1) * 100, rnd(60, 3, seed=seed + 2)
    i_ids, j_ids = torch.zeros(max_k, dtype=torch.int64), torch.zeros(max_k, dtype=torch.int64)  # (slots behind the count hold index 0)
    i_ids[:count] = torch.randint(0, 50, (count,), generator=gen(seed + 3))
    j_ids[:count] = torch.randint(0, 60, (count,), generator=gen(seed + 4))
    expec, mconf = rnd(max_k, 3, seed=seed + 5), torch.rand(max_k, generator=gen(seed + 6))
    mconf[count:] = 0.0
    for k, v in enumerate((-0.0, 1e-30, 0.0)):
        if k < max_k:
            mconf[k] = v
    return pt2d, pt3d, i_ids, j_ids, expec, mconf


def assemble_ref(pt2d, pt3d, i_ids, j_ids, expec, mconf, win, fine_ds):
    c = pt2d[i_ids]
    return c, c + ((expec[:, :2] * win) / 2) * fine_ds, pt3d[j_ids], mconf != 0  # (op for op in fp32: every intermediate rounded)


@pytest.mark.parametrize("win,fine_ds", [(5, 2), (7, 3)])
@pytest.mark.parametrize("max_k,count", SLOT_CASES)
def test_assemble_matches(gpu, built_lib, max_k, count, win, fine_ds):
    args = assemble_inputs(max_k, count, seed=max_k)
    c_ref, f_ref, p_ref, m_ref = assemble_ref(*args, win, fine_ds)
    c, f, p, m = ops.assemble_matches(*(t.to(gpu) for t in args), win, fine_ds)
    assert bits_equal(c, c_ref) and bits_equal(f, f_ref) and bits_equal(p, p_ref)
    assert m.dtype == torch.bool and torch.equal(m.cpu(), m_ref)
    assert not m_ref[0] and (max_k < 2 or m_ref[1]) and (max_k < 3 or not m_ref[2])  # -0.0 is no match, 1e-30 is one


# ------------------------------------------------------------------------------------------------------------ strided arguments
def test_strided_arguments_give_the_contiguous_bits(gpu, built_lib):
    """A column slice of a wider tensor or a transposed view gives the bits of the call on its contiguous copy."""
    n, Cc, F = 37, 13, 4
    ld = (Cc + 3 + 6 * F + 7) // 8 * 8
    feat = rnd(n, Cc + 5, seed=1).to(gpu)[:, 2 : 2 + Cc]
    pt_cols = points(n, seed=2).to(gpu).repeat(1, 2)[:, 1:4]  # a column slice
    pt_t = points(n, seed=3).T.contiguous().to(gpu).T  # a transposed view
    dy = rnd(n, ld + 3, seed=4).to(gpu)[:, 1 : 1 + ld]
    for pt in (pt_cols, pt_t):
        assert not feat.is_contiguous() and not pt.is_contiguous() and not dy.is_contiguous()
        assert bits_equal(ops.cat_fourier(feat, pt, F), ops.cat_fourier(feat.contiguous(), pt.contiguous(), F))
        assert bits_equal(ops.cat_fourier(feat.contiguous(), pt, F), ops.cat_fourier(feat.contiguous(), pt.contiguous(), F))
        assert bits_equal(ops.cat_fourier_bwd(dy, pt, Cc, F), ops.cat_fourier_bwd(dy.contiguous(), pt.contiguous(), Cc, F))

    B, h, w = 2, 5, 7
    x = rnd(B, h, w, Cc, seed=5).to(gpu).permute(0, 3, 1, 2)  # a channels-last map
    pe = rnd(Cc, h + 3, w + 4, seed=6).to(gpu)[:, 1 : h + 2, 2 : w + 3]  # a window of a larger table
    assert not x.is_contiguous() and not pe.is_contiguous()
    assert bits_equal(ops.nchw_to_tokens(x, pe), ops.nchw_to_tokens(x.contiguous(), pe.contiguous()))
    assert bits_equal(ops.nchw_to_tokens(x.contiguous(), pe), (x.cpu() + pe.cpu()[None, :, :h, :w]).flatten(-2).permute(0, 2, 1))

    K = 9
    pt2d, pt3d, i_ids, j_ids, expec, mconf = (t.to(gpu) for t in assemble_inputs(K, K, seed=7))
    views = (torch.cat([pt2d, pt2d], 1)[:, :2], pt3d.T.contiguous().T, torch.stack([i_ids, j_ids], 1)[:, 0], torch.stack([i_ids, j_ids], 1)[:, 1],
             torch.cat([expec, expec], 1)[:, 3:], torch.stack([mconf, mconf], 1)[:, 1])
    assert not any(v.is_contiguous() for v in views)
    want = ops.assemble_matches(pt2d, pt3d, i_ids, j_ids, expec, mconf, 5, 2)
    for k in range(6):  # one strided argument at a time, then all of them
        args = [pt2d, pt3d, i_ids, j_ids, expec, mconf]
        args[k] = views[k]
        got = ops.assemble_matches(*args, 5, 2)
        assert all(bits_equal(a, b) for a, b in zip(got[:3], want[:3])) and torch.equal(got[3], want[3]), k
    got = ops.assemble_matches(*views, 5, 2)
    assert all(bits_equal(a, b) for a, b in zip(got[:3], want[:3])) and torch.equal(got[3], want[3])
