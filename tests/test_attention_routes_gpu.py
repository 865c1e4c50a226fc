"""Every door into the attention kernels: the contiguous one (ops.attention / ops.attention_bwd) that the other unit tests use, and
the one the model uses (ops.attention_fused / ops.attention_bwd_fused: q, k, v as column slices of fused projection buffers, the
forward's log-sum-exp kept for the backward), at head counts where B * heads is no multiple of the 8 XCDs, and with a peaked
softmax in the backward.  Reference: tests/attention_util.py (float64, formulas written out).  All shapes are small."""
import functools
import types

import pytest
import torch

import attention_util as au
from attention_util import rel
from nerfmatch_amd import _lib, ops
from nerfmatch_amd import autograd as ag

pytestmark = pytest.mark.gpu

TILED32 = [s + (32,) for s in au.TILED]
FWD_CASES = [(s, p) for s in au.SHAPES for p in ("fp32", "bf16x3")] + [(s, "fp8") for s in au.SHAPES if s in TILED32 or s[4] == 16]
fwd_cases = pytest.mark.parametrize("shape,precision", FWD_CASES, ids=[f"{au.shape_id(s)}-{p}" for s, p in FWD_CASES])
BWD_CASES = [(s, p) for s in au.SHAPES for p in ("fp32", "bf16x3")]
bwd_cases = pytest.mark.parametrize("shape,precision", BWD_CASES, ids=[f"{au.shape_id(s)}-{p}" for s, p in BWD_CASES])
tiled_cases = pytest.mark.parametrize("shape", TILED32, ids=au.shape_id)


@pytest.fixture
def precision_switch(monkeypatch):
    """Sets ops.ATTENTION_PRECISION for the rest of the test; monkeypatch puts the old value back."""
    return lambda p: monkeypatch.setattr(ops, "ATTENTION_PRECISION", p)


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs and the float64 reference of one shape: computed once, shared, never written to."""
    B, L, S, H, D = shape
    q, k, v, d_o = (au.rnd(B, n, H * D, seed=s) for n, s in ((L, 1), (S, 2), (S, 3), (L, 4)))
    return _case(shape, q, k, v, d_o)


def _case(shape, q, k, v, d_o):
    B, L, S, H, D = shape
    scale = D**-0.5
    o, nlse, dq, dk, dv = au.reference(q, k, v, d_o, H, scale)
    return types.SimpleNamespace(B=B, L=L, S=S, H=H, D=D, dim=H * D, scale=scale, q=q, k=k, v=v, d_o=d_o, o=o, nlse=nlse, dq=dq, dk=dk, dv=dv)


@functools.lru_cache(maxsize=None)
def peaked_case(i):
    B, L, S, H, D, where, gain = au.PEAKED[i]
    c = _case((B, L, S, H, D), *au.peaked_inputs(B, L, S, H, D, where, gain, seed=11))
    _, *g32 = au.autograd_grads(c.q, c.k, c.v, c.d_o, H, c.scale, torch.float32)
    c.e32 = [rel(g, r, 0.1) for g, r in zip(g32, (c.dq, c.dk, c.dv))]
    c.max_score = au.scores_log2(c.q, c.k, H, c.scale).abs().max().item()
    return c


def layouts(c, pads=au.PADS):
    """(name, pad, q buffer, kv buffer or None, (q_col, k_col, v_col)) of every fused layout the shape allows, on the CPU."""
    for pad in pads:
        qb, kvb, cols = au.pack_cross(c.q, c.k, c.v, pad)
        yield "cross", pad, qb, kvb, cols
        if c.L == c.S:
            sb, cols = au.pack_self(c.q, c.k, c.v, pad)
            yield "self", pad, sb, None, cols


def fused_forward(c, gpu, qb, kvb, cols, want_lse=False):
    span = lambda col: (col, col + c.dim)
    return ops.attention_fused(qb.to(gpu), span(cols[0]), span(cols[1]), span(cols[2]), c.B, c.L, c.S, c.H, c.scale,
                               kv=None if kvb is None else kvb.to(gpu), want_lse=want_lse)


def fused_backward(c, gpu, qb, kvb, cols, o, nlse=None):
    """-> d_q_src, d_kv_src as attention_bwd_fused returns them."""
    qg = qb.to(gpu)
    kvg = qg if kvb is None else kvb.to(gpu)
    return ops.attention_bwd_fused(qg, cols[0], kvg, cols[1], cols[2], o, c.d_o.to(gpu), c.B, c.L, c.S, c.H, c.scale, nlse=nlse)


def slices(c, dq_src, dkv_src, cols):
    take = lambda buf, col, n: buf[:, col:col + c.dim].reshape(c.B, n, c.dim)
    return take(dq_src, cols[0], c.L), take(dkv_src, cols[1], c.S), take(dkv_src, cols[2], c.S)


def outside_slices(c, buf, cols):
    keep = torch.ones(buf.shape[1], dtype=torch.bool)
    for col in cols:
        keep[col:col + c.dim] = False
    return buf[:, keep.to(buf.device)]


def check_buffers(c, name, pad, dq_src, dkv_src, cols):
    """What attention_bwd_fused promises of the buffers it returns: the sources' layout, one buffer for self attention, nothing but
    finite values, and exactly 0.0 in every column beside the slices."""
    assert (dkv_src is dq_src) == (name == "self"), (name, pad)
    for buf, own in ((dq_src, cols if name == "self" else cols[:1]), (dkv_src, cols if name == "self" else cols[1:])):
        assert torch.isfinite(buf).all(), (name, pad)
        rest = outside_slices(c, buf, own)
        assert rest.shape[1] == (len(own) + 1) * pad and (rest == 0).all(), (name, pad)


# ------------------------------------------------------------------------------------------------------------------ forward
@fwd_cases
def test_forward_fused_door_equals_contiguous_door(gpu, built_lib, precision_switch, shape, precision):
    """Same kernel, same arithmetic, other addresses (column offsets, leading dimensions 3 dim / 2 dim / padded): the same bits, and
    finite although every column beside the slices holds NaN."""
    c = case(shape)
    precision_switch(precision)
    want = ops.attention(c.q.to(gpu), c.k.to(gpu), c.v.to(gpu), c.H, c.scale)
    assert torch.isfinite(want).all()
    for name, pad, qb, kvb, cols in layouts(c):
        got = fused_forward(c, gpu, qb, kvb, cols)
        assert got.shape == want.shape and torch.isfinite(got).all(), (name, pad)
        assert torch.equal(got, want), (name, pad, (got - want).abs().max().item())


@fwd_cases
def test_forward_against_float64(gpu, built_lib, precision_switch, shape, precision):
    """The bound of test_attention (2e-5 absolute) at head counts 1, 3, 4, 5 -- B * heads no multiple of 8 on attn32_v3_kernel and on the
    fp8 kernel, few heads on the (blocks, heads, B) grid of attn32_kernel; where the e4m3 kernel runs, the two stated bounds of
    test_attention_fp8_error_bound.
    Measured on the MI355X: fp32 <= 8.9e-7; split-bf16 <= 1.4e-5 (1x65x32x8: few keys, outputs of magnitude ~1); fp8 max <= 0.030 max|v|, rms <= 5.3 % of the
    output's."""
    c = case(shape)
    precision_switch(precision)
    out = ops.attention(c.q.to(gpu), c.k.to(gpu), c.v.to(gpu), c.H, c.scale).cpu().double()
    err = (out - c.o).abs()
    if ops._use_fp8(c.L, c.S, c.D):
        vmax, rms_ref = c.v.abs().max().item(), c.o.pow(2).mean().sqrt().item()
        print(f"fp8 {au.shape_id(shape)}: max err {err.max():.3e} = {err.max() / vmax:.4f} max|v|, rms err {err.pow(2).mean().sqrt() / rms_ref:.4f} of the output's rms")
        assert torch.isfinite(out).all()
        assert err.max() < 0.075 * vmax and err.pow(2).mean().sqrt() < 0.08 * rms_ref
    else:
        print(f"{precision} {au.shape_id(shape)}: max err {err.max():.3e}")
        assert err.max() < 2e-5


# ----------------------------------------------------------------------------------------------------------------- kept LSE
@tiled_cases
def test_kept_lse_within_derived_bound(gpu, built_lib, precision_switch, shape):
    """nlse of the split-bf16 forward against float64, per query, within au.nlse_bound (derivation there).
    Measured on the MI355X, largest error / bound over the shapes: 0.025 (1x65x32x8: error 1.3e-5); the same bits through every layout."""
    c = case(shape)
    precision_switch("bf16x3")
    assert ops.lse_supported(c.L, c.S, c.D)
    bound = au.nlse_bound(c.q, c.k, c.scale, c.H)
    first = None
    for name, pad, qb, kvb, cols in layouts(c):
        out, nlse = fused_forward(c, gpu, qb, kvb, cols, want_lse=True)
        assert nlse is not None and nlse.shape == (c.B, c.H, c.L) and nlse.dtype == torch.float32, (name, pad)
        assert torch.equal(out, fused_forward(c, gpu, qb, kvb, cols)), (name, pad)  # (keeping it does not change the output)
        if first is None:
            first = nlse
            ratio = ((nlse.cpu().double() - c.nlse).abs() / bound)
            print(f"nlse {au.shape_id(shape)}: largest error / bound {ratio.max():.3f} (error {(nlse.cpu().double() - c.nlse).abs().max():.2e})")
            assert torch.isfinite(nlse).all() and ratio.max() <= 1.0
        assert torch.equal(nlse, first), (name, pad)


@pytest.mark.parametrize("shape,precision", [(s, p) for s in TILED32 for p in ("fp32", "fp8")] + [(s, p) for s in au.SMALL for p in ("fp32", "bf16x3")],
                         ids=lambda x: x if isinstance(x, str) else au.shape_id(x))
def test_lse_not_kept_elsewhere(gpu, built_lib, precision_switch, shape, precision):
    """Only the split-bf16 tiled kernel keeps the log-sum-exp: attention_fused(want_lse=True) -> (out, None) on every other route, and
    nm_attention refuses an nlse_out there instead of leaving it unwritten.  (nm_attention_fp8 has no such argument.)"""
    c = case(shape)
    precision_switch(precision)
    assert not ops.lse_supported(c.L, c.S, c.D)
    qb, kvb, cols = au.pack_cross(c.q, c.k, c.v, 4)
    out, nlse = fused_forward(c, gpu, qb, kvb, cols, want_lse=True)
    assert nlse is None and torch.equal(out, fused_forward(c, gpu, qb, kvb, cols))
    if precision != "fp8":
        flags = ops._attn_flags()
        q, k, v = c.q.to(gpu), c.k.to(gpu), c.v.to(gpu)
        o, keep = torch.empty_like(q), torch.full((c.B, c.H, c.L), 7.0, device=gpu)
        rc = _lib.lib().nm_attention(_lib.dptr(q), _lib.dptr(k), _lib.dptr(v), c.dim, c.dim, c.dim, c.B, c.L, c.S, c.H, c.D, float(c.scale), flags,
                                     ops._attn_workspace(gpu, c.B, c.S, c.H, flags, c.L, c.D), _lib.dptr(o), _lib.dptr(keep), _lib.stream())
        assert rc == _lib.NM_ERR_UNSUPPORTED
        assert (keep == 7.0).all()


# ----------------------------------------------------------------------------------------------------------------- backward
@bwd_cases
def test_backward_fused_door_equals_contiguous_door(gpu, built_lib, precision_switch, shape, precision):
    """nlse=None: attention_bwd_fused on packed buffers gives the bits of attention_bwd, slice by slice.  Padded buffers (the zeros_like
    branch): exactly 0.0 beside the slices, no NaN anywhere.  Buffers that hold exactly the slices (the empty_like branch): every column
    within the bound of test_attention_backward of the reference gradient, so no slice column is left unwritten.  Self attention
    returns ONE buffer."""
    c = case(shape)
    precision_switch(precision)
    tol = au.bwd_tol(precision, c.L, c.S, c.D)
    o = ops.attention(c.q.to(gpu), c.k.to(gpu), c.v.to(gpu), c.H, c.scale)
    want = ops.attention_bwd(c.q.to(gpu), c.k.to(gpu), c.v.to(gpu), o, c.d_o.to(gpu), c.H, c.scale)
    errs = [rel(g, r, 0.1) for g, r in zip(want, (c.dq, c.dk, c.dv))]
    print(f"bwd {precision} {au.shape_id(shape)}: rel dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} (bound {tol:g})")
    assert max(errs) < tol
    for name, pad, qb, kvb, cols in layouts(c):
        dq_src, dkv_src = fused_backward(c, gpu, qb, kvb, cols, o)
        assert dq_src.shape == qb.shape and dkv_src.shape == (qb if kvb is None else kvb).shape, (name, pad)
        check_buffers(c, name, pad, dq_src, dkv_src, cols)
        for what, got, ref in zip(("dq", "dk", "dv"), slices(c, dq_src, dkv_src, cols), want):
            assert torch.equal(got, ref), (name, pad, what, (got - ref).abs().max().item())
        if pad == 0:  # the whole buffers, column block by column block, against the packed reference gradient
            if name == "self":
                pairs = [(dq_src, torch.cat([c.dq, c.dk, c.dv], -1).reshape(c.B * c.L, 3 * c.dim))]
            else:
                pairs = [(dq_src, c.dq.reshape(c.B * c.L, c.dim)), (dkv_src, torch.cat([c.dk, c.dv], -1).reshape(c.B * c.S, 2 * c.dim))]
            for buf, ref in pairs:
                assert buf.shape == ref.shape, name
                for col in range(0, ref.shape[1], c.dim):
                    assert rel(buf[:, col:col + c.dim], ref[:, col:col + c.dim], 0.1) < tol, (name, col)


@tiled_cases
def test_backward_with_kept_lse(gpu, built_lib, precision_switch, shape):
    """The attn32_bwd_dq_v2_kernel<true> route: the forward's nlse handed to attention_bwd_fused.  Gradients within the bound of
    test_attention_backward of the float64 reference and within twice that of the nlse=None result; the same bits through every
    layout; zeros beside the slices.  And it IS that route: nlse + 1 doubles every probability, so dq, dk, dv come out doubled
    (the kernel that rebuilds the log-sum-exp would not look at the argument).
    Measured on the MI355X (rel to the reference, floor 0.1): with the kept LSE <= 1.5e-5, rebuilt <= 1.5e-5, kept against rebuilt <= 5.4e-6 (the
    same bits at 1x65x32x8 and 1x1x65x5), the (nlse + 1) run halved <= 1.5e-5."""
    c = case(shape)
    precision_switch("bf16x3")
    tol = au.bwd_tol("bf16x3", c.L, c.S, c.D)
    refs = (c.dq, c.dk, c.dv)
    first = None
    for name, pad, qb, kvb, cols in layouts(c):
        o, nlse = fused_forward(c, gpu, qb, kvb, cols, want_lse=True)
        assert nlse is not None
        none = slices(c, *fused_backward(c, gpu, qb, kvb, cols, o), cols)
        dq_src, dkv_src = fused_backward(c, gpu, qb, kvb, cols, o, nlse=nlse)
        kept = slices(c, dq_src, dkv_src, cols)
        check_buffers(c, name, pad, dq_src, dkv_src, cols)
        if first is None:
            first = [g.clone() for g in kept]
            e_kept, e_none = [rel(g, r, 0.1) for g, r in zip(kept, refs)], [rel(g, r, 0.1) for g, r in zip(none, refs)]
            gap = [rel(a, b.cpu().double(), 0.1) for a, b in zip(kept, none)]
            doubled = slices(c, *fused_backward(c, gpu, qb, kvb, cols, o, nlse=nlse + 1.0), cols)
            e_dbl = [rel(g / 2, r, 0.1) for g, r in zip(doubled, refs)]
            print(f"kept LSE {au.shape_id(shape)}: rel dq/dk/dv kept {e_kept[0]:.2e} {e_kept[1]:.2e} {e_kept[2]:.2e}, rebuilt {e_none[0]:.2e} {e_none[1]:.2e} "
                  f"{e_none[2]:.2e}, kept vs rebuilt {max(gap):.2e}, (nlse + 1) / 2 {max(e_dbl):.2e} (bound {tol:g})")
            assert max(e_kept) < tol and max(e_none) < tol and max(gap) < 2 * tol
            assert max(e_dbl) < tol
            # and against the doubled reference directly: an ignored argument leaves half of it missing
            assert min(rel(g, r, 0.1) for g, r in zip(doubled, refs)) > 0.4
        for what, got, ref in zip(("dq", "dk", "dv"), kept, first):
            assert torch.equal(got, ref), (name, pad, what)


@tiled_cases
def test_backward_drops_lse_when_precision_moved_to_fp32(gpu, built_lib, precision_switch, shape):
    """Forward under bf16x3, switch to fp32, backward: attention_bwd_fused drops the nlse it is handed (the fp32 kernels rebuild it)
    and returns the bits of the fp32 nlse=None run."""
    c = case(shape)
    qb, kvb, cols = au.pack_cross(c.q, c.k, c.v, 4)
    precision_switch("bf16x3")
    o, nlse = fused_forward(c, gpu, qb, kvb, cols, want_lse=True)
    assert nlse is not None
    precision_switch("fp32")
    with_lse = fused_backward(c, gpu, qb, kvb, cols, o, nlse=nlse)
    without = fused_backward(c, gpu, qb, kvb, cols, o)
    assert torch.equal(with_lse[0], without[0]) and torch.equal(with_lse[1], without[1])
    assert max(rel(g, r, 0.1) for g, r in zip(slices(c, *with_lse, cols), (c.dq, c.dk, c.dv))) < au.bwd_tol("fp32", c.L, c.S, c.D)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B,L,S", [(0, 70, 33), (2, 0, 33), (2, 70, 0)])
@pytest.mark.parametrize("pad", [0, 4])
def test_backward_zero_size(gpu, built_lib, precision_switch, precision, B, L, S, pad):
    """B L == 0 or S == 0: zeroed buffers of the sources' shapes, from either allocation branch."""
    precision_switch(precision)
    H, D = 5, 32
    dim = H * D
    q, k, v = torch.ones(B, L, dim), torch.ones(B, S, dim), torch.ones(B, S, dim)
    qb, kvb, cols = au.pack_cross(q, k, v, pad, poison=1.0)
    o = d_o = torch.ones(B, L, dim, device=gpu)
    dq_src, dkv_src = ops.attention_bwd_fused(qb.to(gpu), cols[0], kvb.to(gpu), cols[1], cols[2], o, d_o, B, L, S, H, D**-0.5)
    assert dq_src.shape == qb.shape and dkv_src.shape == kvb.shape and dq_src.dtype == dkv_src.dtype == torch.float32
    assert (dq_src == 0).all() and (dkv_src == 0).all()
    if B * L == 0:  # self attention (S = L): one buffer
        sb, scols = au.pack_self(q, q, q, pad, poison=1.0)
        sg = sb.to(gpu)
        d1, d2 = ops.attention_bwd_fused(sg, scols[0], sg, scols[1], scols[2], o, d_o, B, L, L, H, D**-0.5)
        assert d1 is d2 and d1.shape == sb.shape and (d1 == 0).all()


# ------------------------------------------------------------------------------------------------------------ peaked softmax
PEAKED_CASES = [(i, r) for i, p in enumerate(au.PEAKED) for r in ("fp32", "bf16x3", "bf16x3-kept-lse") if p[4] == 32 or r != "bf16x3-kept-lse"]


@pytest.mark.parametrize("i,route", PEAKED_CASES, ids=[f"{au.shape_id(au.PEAKED[i])}-{r}" for i, r in PEAKED_CASES])
def test_backward_peaked_softmax(gpu, built_lib, precision_switch, i, route):
    """One key per chosen query with probability ~1 (scores up to +-78 in the log2 domain), planted in the first, a middle, the last and
    a ragged key tile: pass 1 of the backward has to raise its lazy running maximum after its first tile, and exp2(s - lse) of both dkv
    kernels returns values next to 1 and next to 0.  Through the fused door (pad 4), against float64.
    The bound comes from the reference alone (au.peaked_tols): e32 = rel(., ref, 0.1) of plain float32 autograd on the CPU; fp32 kernels
    max(2e-5, 4 e32), split-bf16 max(5e-5, 4 e32 + 4 ln2 2^-16 max|score|).
    Measured on the MI355X (dq / dk / dv): 
      1x70x160x8x32  e32 9.0e-7 4.4e-7 2.4e-7   fp32 3.7e-6 7.8e-7 3.5e-6   bf16x3 2.9e-4 5.6e-5 1.3e-4 (kept LSE: the same)   bound 3.2e-3
      2x129x97x5x32  e32 4.1e-7 4.0e-7 4.0e-7   fp32 2.2e-6 4.6e-7 2.3e-6   bf16x3 1.1e-4 1.6e-5 7.9e-5 (kept LSE: the same)   bound 3.3e-3
      2x49x64x5x16   e32 1.4e-6 3.3e-7 4.3e-7   the window kernel (one for both precisions) 1.6e-6 3.3e-7 4.3e-7"""
    c = peaked_case(i)
    precision = route.split("-")[0]
    precision_switch(precision)
    kept = route.endswith("kept-lse")
    assert not kept or ops.lse_supported(c.L, c.S, c.D)
    qb, kvb, cols = au.pack_cross(c.q, c.k, c.v, 4)
    o, nlse = fused_forward(c, gpu, qb, kvb, cols, want_lse=True)
    assert (nlse is not None) == ops.lse_supported(c.L, c.S, c.D)
    dq_src, dkv_src = fused_backward(c, gpu, qb, kvb, cols, o, nlse=nlse if kept else None)
    assert torch.isfinite(dq_src).all() and torch.isfinite(dkv_src).all()
    errs = [rel(g, r, 0.1) for g, r in zip(slices(c, dq_src, dkv_src, cols), (c.dq, c.dk, c.dv))]
    tols = [au.peaked_tols(e, c.max_score)[precision] for e in c.e32]
    print(f"peaked {route} {au.shape_id(au.PEAKED[i])}: e32 " + " ".join(f"{e:.2e}" for e in c.e32) + "  achieved " + " ".join(f"{e:.2e}" for e in errs) +
          "  bound " + " ".join(f"{t:.2e}" for t in tols) + f"  (max |score| {c.max_score:.1f} log2)")
    for what, e, t in zip(("dq", "dk", "dv"), errs, tols):
        assert e < t, what


@functools.lru_cache(maxsize=None)
def very_negative_case():
    B, L, S, H, D, l0, factor = au.VERY_NEGATIVE
    c = _case((B, L, S, H, D), *au.very_negative_inputs(B, L, S, H, D, l0, factor, seed=21))
    _, *g32 = au.autograd_grads(c.q, c.k, c.v, c.d_o, H, c.scale, torch.float32)
    c.e32 = [rel(g, r, 0.1) for g, r in zip(g32, (c.dq, c.dk, c.dv))]
    c.max_score = au.scores_log2(c.q, c.k, H, c.scale).abs().max().item()
    return c


@pytest.mark.parametrize("route", ["fp32", "bf16x3", "bf16x3-kept-lse"])
def test_backward_scores_all_very_negative(gpu, built_lib, precision_switch, route):
    """One query whose scores are all below -128 in the log2 domain, ragged last key tile: 2^(-lse) of that query is no fp32 number, so
    a zero-padded key past the end that reached the dS product unmasked would put inf * 0 = NaN into dq (with ordinary inputs such a
    key adds an exact 0 there: its K^T operand is zero).  Bounds as in test_backward_peaked_softmax, from float32 autograd on the CPU.
    Measured on the MI355X (dq / dk / dv): e32 4.1e-6 5.8e-6 1.2e-5; fp32 4.6e-6 6.8e-6 1.1e-5 (output 7.5e-6); split-bf16 with and
    without the kept LSE 5.0e-5 1.9e-4 3.5e-4 (bound 2.2e-2; output 5.5e-5).  Before the first-tile fix in attn32_v3_kernel and pass 1 of
    attn32_bwd_dq_v2_kernel the split-bf16 output and dq of that query were NaN (0 * 2^-max with 2^-max = inf)."""
    c = very_negative_case()
    precision = route.split("-")[0]
    precision_switch(precision)
    kept = route.endswith("kept-lse")
    qb, kvb, cols = au.pack_cross(c.q, c.k, c.v, 4)
    o, nlse = fused_forward(c, gpu, qb, kvb, cols, want_lse=True)
    assert (nlse is not None) == (precision == "bf16x3")
    # the output: 2e-5 as everywhere on the fp32 kernel; on the split-bf16 kernel the dropped lo.lo terms of a score of several hundred
    # sit in the exponent (relative 4 ln2 2^-16 max|score| in a probability, as in au.peaked_tols), times the largest |v|
    o_err, o_tol = (o.cpu().double() - c.o).abs().max().item(), 2e-5 + (au.peaked_tols(0.0, c.max_score)["bf16x3"] * c.v.abs().max().item() if precision == "bf16x3" else 0.0)
    print(f"very negative {route}: output max err {o_err:.3e} (bound {o_tol:.3e})")
    assert o_err < o_tol
    dq_src, dkv_src = fused_backward(c, gpu, qb, kvb, cols, o, nlse=nlse if kept else None)
    assert torch.isfinite(dq_src).all() and torch.isfinite(dkv_src).all()
    errs = [rel(g, r, 0.1) for g, r in zip(slices(c, dq_src, dkv_src, cols), (c.dq, c.dk, c.dv))]
    tols = [au.peaked_tols(e, c.max_score)[precision] for e in c.e32]
    print(f"very negative {route}: e32 " + " ".join(f"{e:.2e}" for e in c.e32) + "  achieved " + " ".join(f"{e:.2e}" for e in errs) +
          "  bound " + " ".join(f"{t:.2e}" for t in tols) + f"  (max |score| {c.max_score:.1f} log2)")
    for what, e, t in zip(("dq", "dk", "dv"), errs, tols):
        assert e < t, what


# ------------------------------------------------------------------------------------------------- padding workgroups
PADDED = [s for s in TILED32 if (s[0] * s[3]) % 8]


@pytest.mark.parametrize("route", ["fwd-bf16x3", "fwd-fp8", "bwd-bf16x3", "bwd-bf16x3-kept-lse"])
@pytest.mark.parametrize("shape", PADDED, ids=au.shape_id)
def test_padding_workgroups_touch_nothing(gpu, built_lib, precision_switch, shape, route):
    """map_work rounds B * heads up to a multiple of 8 and the workgroups with bh >= B * heads have to leave (attention_tile.h; written out
    by hand in attn32_v3_kernel and the fp8 kernel).  The value tests above cannot see a workgroup that stays: its (batch, head) lies
    past the end of every buffer.  Here the C entry points get buffers with room for the rounded-up count -- the real batches in front, a
    sentinel behind -- so that such a workgroup would find memory to read and write: the sentinel is intact, and the real batches hold
    the bits the ops-level call gives.  (The fp32 kernels run on a (blocks, heads, B) grid without padding.)"""
    c = case(shape)
    B, L, S, H, dim = c.B, c.L, c.S, c.H, c.dim
    bh_pad = (B * H + 7) // 8 * 8
    Bp = -(-bh_pad // H)  # batches that hold every padded (batch, head) id
    precision_switch("fp8" if route == "fwd-fp8" else "bf16x3")
    lib = _lib.lib()

    def roomy(t, fill):
        buf = torch.full((Bp,) + tuple(t.shape[1:]), fill, device=gpu, dtype=torch.float32)
        buf[:B] = t.to(gpu)
        return buf

    q, k, v, d_o = roomy(c.q, 0.0), roomy(c.k, 0.0), roomy(c.v, 0.0), roomy(c.d_o, 0.0)
    want_o, want_nlse = ops.attention_fused(q[:B].reshape(B * L, dim), (0, dim), (0, dim), (dim, 2 * dim), B, L, S, H, c.scale,
                                            kv=torch.cat([k[:B], v[:B]], -1).reshape(B * S, 2 * dim), want_lse=True)
    if route.startswith("fwd"):
        out = torch.full((Bp, L, dim), 7.0, device=gpu)
        if route == "fwd-fp8":
            assert ops._use_fp8(L, S, c.D) and want_nlse is None
            ws = torch.zeros(lib.nm_attention_fp8_workspace_bytes(Bp, S, H), device=gpu, dtype=torch.uint8)
            rc = lib.nm_attention_fp8(_lib.dptr(q), _lib.dptr(k), _lib.dptr(v), dim, dim, dim, B, L, S, H, float(c.scale), _lib.dptr(ws, torch.uint8),
                                      _lib.dptr(out), _lib.stream())
        else:
            nlse = torch.full((bh_pad, L), 7.0, device=gpu)
            ws = torch.zeros(lib.nm_attention_workspace_bytes(Bp, S, H), device=gpu, dtype=torch.uint8)
            rc = lib.nm_attention(_lib.dptr(q), _lib.dptr(k), _lib.dptr(v), dim, dim, dim, B, L, S, H, c.D, float(c.scale), _lib.NM_ATTN_BF16X3,
                                  _lib.dptr(ws, torch.uint8), _lib.dptr(out), _lib.dptr(nlse), _lib.stream())
            assert torch.equal(nlse[:B * H].reshape(B, H, L), want_nlse) and (nlse[B * H:] == 7.0).all()
        assert rc == 0
        assert torch.equal(out[:B], want_o) and (out[B:] == 7.0).all()
        return
    kept = route.endswith("kept-lse")
    nlse = None
    if kept:
        nlse = torch.zeros(bh_pad, L, device=gpu)
        nlse[:B * H] = want_nlse.reshape(B * H, L)
    o = roomy(want_o, 0.0)
    dq, dk, dv = (torch.full_like(t, 7.0) for t in (q, k, v))
    need = lib.nm_attention_bwd_workspace_bytes(Bp, L, S, H, _lib.NM_ATTN_BF16X3)
    ws = torch.zeros(need, device=gpu, dtype=torch.uint8)
    rc = lib.nm_attention_bwd(_lib.dptr(q), _lib.dptr(k), _lib.dptr(v), _lib.dptr(o), _lib.dptr(d_o), dim, dim, dim, dim, dim, B, L, S, H, c.D, float(c.scale),
                              _lib.dptr(dq), _lib.dptr(dk), _lib.dptr(dv), dim, dim, dim, _lib.NM_ATTN_BF16X3, _lib.dptr(nlse), _lib.dptr(ws, torch.uint8), need,
                              _lib.stream())
    assert rc == 0
    qb, kvb, cols = au.pack_cross(c.q, c.k, c.v, 0)
    want = slices(c, *fused_backward(c, gpu, qb, kvb, cols, want_o, nlse=want_nlse if kept else None), cols)
    for what, got, ref in zip(("dq", "dk", "dv"), (dq, dk, dv), want):
        assert torch.equal(got[:B], ref), what
        assert (got[B:] == 7.0).all(), what


# ------------------------------------------------------------------------------------------------------------ project door
@pytest.mark.parametrize("B,L,S,H", [(2, 70, 70, 5), (2, 65, 97, 5)])
def test_autograd_functions_keep_and_use_the_lse(gpu, built_lib, precision_switch, B, L, S, H):
    """autograd.py's fused attention Functions under bf16x3: the ctx holds the forward's nlse (a tensor, so the backward takes the
    kept-LSE kernels tested above) and the gradients of the fused buffers meet the bound of test_attention_backward against float64."""
    c = case((B, L, S, H, 32))
    precision_switch("bf16x3")
    tol = au.bwd_tol("bf16x3", L, S, 32)
    d_o = c.d_o.to(gpu)
    with torch.enable_grad():
        qb, kvb, cols = au.pack_cross(c.q, c.k, c.v, 0)
        qg, kvg = qb.to(gpu).requires_grad_(), kvb.to(gpu).requires_grad_()
        out = ag.attention_cross_fused(qg, kvg, B, L, S, H, c.scale)
        assert isinstance(out.grad_fn.nlse, torch.Tensor) and out.grad_fn.nlse.shape == (B, H, L)
        out.backward(d_o)
        runs = [("cross", out, slices(c, qg.grad, kvg.grad, cols))]
        if L == S:
            sb, scols = au.pack_self(c.q, c.k, c.v, 0)
            sg = sb.to(gpu).requires_grad_()
            out = ag.attention_self_fused(sg, B, L, H, c.scale)
            assert isinstance(out.grad_fn.nlse, torch.Tensor) and out.grad_fn.nlse.shape == (B, H, L)
            out.backward(d_o)
            runs.append(("self", out, slices(c, sg.grad, sg.grad, scols)))
    for name, out, grads in runs:
        assert (out.detach().cpu().double() - c.o).abs().max() < 2e-5, name
        errs = [rel(g, r, 0.1) for g, r in zip(grads, (c.dq, c.dk, c.dv))]
        print(f"autograd {name} {B}x{L}x{S}x{H}: rel dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} (bound {tol:g})")
        assert max(errs) < tol, name


def test_precision_globals_restored(gpu):
    """Last in the file: every test above set the switch through monkeypatch, so the rest of the suite sees the defaults."""
    assert ops.ATTENTION_PRECISION == "fp32" and ops.LINEAR_PRECISION == "fp32"
