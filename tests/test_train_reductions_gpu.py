"""GPU: the reductions over rows of csrc/train.hip exactly at their slice, wavefront-quarter and register-ring edges.

The indexing is carried by exact probes (tests/train_reduce_util.py): operands whose every partial sum is an fp32 number, so each output must
`torch.equal` the fp64 truth whatever the summation order -- row slices, wavefront quarters, LDS trees, the ordered partial sums and float atomics
alike.  Every case asserts, through the Python mirrors of the host's slicing, the plan it is meant to hit.  Random-float cases at the project's
existing bars keep the arithmetic covered at the same edges."""
import pytest
import torch

import train_reduce_util as tr
from nerfmatch_amd import _lib, ops
from nerfmatch_amd._lib import dptr, stream

pytestmark = pytest.mark.gpu


def assert_exact(got, ref, what):
    """torch.equal against the fp64 truth, with the place of the first difference in the message."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {ref.numel()} elements differ from fp64; first at {i}: got {got[i].item()!r}, want {ref[i].item()!r}")


def rel(a, b):
    a, b = a.detach().cpu().double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-3)).item()


class precision:
    """`with precision("bf16x3"):` -- ops.LINEAR_PRECISION for the block, restored in a finally."""

    def __init__(self, p):
        self.p = p

    def __enter__(self):
        self.keep, ops.LINEAR_PRECISION = ops.LINEAR_PRECISION, self.p

    def __exit__(self, *exc):
        ops.LINEAR_PRECISION = self.keep


# ------------------------------------------------------------------------------------------------------------ weight gradient
W0, W1, W2, W3 = (1, 0, 0, 0), (16, 1, 0, 0), (16, 16, 16, 1), (16, 16, 1, 0)
# M, N, K, fields of wgrad_plan_fp32 (None: the fp32 kernel does not take the shape), fields of wgrad_plan_bf16x3 -- the edge each row is there for
WGRAD_CASES = [
    # bf16x3: wavefronts 1..3 without rows; then wavefront 1, and then wavefront 3, holding one row
    (1, 2, 4, None, dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W0)),
    (1, 64, 128, dict(splits=1, rows_per=32), dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W0)),
    (17, 2, 4, None, dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W1)),
    (17, 64, 128, dict(splits=1, rows_per=32), dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W1)),
    (49, 2, 4, None, dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W2)),
    (49, 64, 128, dict(splits=1, rows_per=64), dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W2)),
    # fp32: the last 32-row chunk holds one row.  bf16x3: wavefront 2 holds one row (rows_per 64 / rpw 16, then 128 / 32)
    (33, 64, 64, dict(splits=1, rows_per=64), dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W3)),
    (33, 64, 128, dict(splits=1, rows_per=64), dict(slices=1, rows_per=64, rpw=16, last_wave_rows=W3)),
    (65, 64, 64, dict(splits=1, rows_per=96), dict(slices=1, rows_per=128, rpw=32, last_wave_rows=(32, 32, 1, 0))),
    (65, 64, 128, dict(splits=1, rows_per=96), dict(slices=1, rows_per=128, rpw=32, last_wave_rows=(32, 32, 1, 0))),
    # fp32: the ring of four chunks in flight wraps with one row left (five chunks)
    (129, 64, 64, dict(splits=1, rows_per=160), dict(slices=1, rows_per=192, rpw=48, last_wave_rows=(48, 48, 33, 0))),
    # bf16x3: a 48-row ring pass plus 16 per wavefront; wavefront 3 holds one row
    (193, 64, 128, dict(splits=1, rows_per=224), dict(slices=1, rows_per=256, rpw=64, last_wave_rows=(64, 64, 64, 1))),
    # the first split.  fp32: 160 + 97.  bf16x3: 192 + 65, the second slice's wavefronts 2 and 3 empty
    (257, 64, 64, dict(splits=2, rows_per=160), dict(slices=2, rows_per=192, rpw=48, last_wave_rows=(48, 17, 0, 0))),
    (257, 64, 128, dict(splits=2, rows_per=160), dict(slices=2, rows_per=192, rpw=48, last_wave_rows=(48, 17, 0, 0))),
    # bf16x3: three slices (192, 192, 129): wgrad_reduce4_kernel takes its tail loop only
    (513, 64, 128, dict(splits=3, rows_per=192), dict(slices=3, rows_per=192, rpw=48, last_wave_rows=(48, 48, 33, 0))),
    # fp32: 16 slices guessed, 15 after rounding, the last of 65 rows.  bf16x3: 17 slices, the last of one row; reduce4: four 4-groups plus a tail
    (4097, 64, 64, dict(first_guess=16, splits=15, rows_per=288), dict(first_guess=17, slices=17, rows_per=256, rpw=64, last_wave_rows=W0)),
    (4097, 64, 128, dict(first_guess=16, splits=15, rows_per=288), dict(first_guess=17, slices=17, rows_per=256, rpw=64, last_wave_rows=W0)),
    # ragged and multi-tile N and K; db comes from the first tile column only (two K tiles) and from every N tile (N = 66, 70)
    (300, 4, 4, dict(tiles=1, splits=2), dict(tiles=1, slices=2, rows_per=192)),
    (300, 60, 68, dict(tiles=2, splits=2), dict(tiles=1, slices=2, rows_per=192)),
    (300, 68, 132, dict(tiles=6, splits=2), dict(tiles=4, slices=2, rows_per=192)),
    (300, 66, 124, None, dict(tiles=2, slices=2, rows_per=192)),
    (300, 70, 132, None, dict(tiles=4, slices=2, rows_per=192)),
    (300, 62, 4, None, dict(tiles=1, slices=2, rows_per=192)),
]
WGRAD_PARAMS = [pytest.param(M, N, K, p, (f32, b16), id=f"{M}x{N}x{K}-{p}") for (M, N, K, f32, b16) in WGRAD_CASES for p in ("fp32", "bf16x3")
                if p == "bf16x3" or f32 is not None]


def assert_plan(M, N, K, prec, want):
    plan = tr.wgrad_plan_fp32(M, N, K) if prec == "fp32" else tr.wgrad_plan_bf16x3(M, N, K)
    for field, v in want.items():
        assert getattr(plan, field) == v, f"({M},{N},{K}) {prec}: the host's plan moved away from this case's edge: {field} = {getattr(plan, field)}, not {v} ({plan})"
    assert _lib.lib().nm_linear_wgrad_workspace_bytes(M, N, K) == tr.wgrad_workspace_bytes(M, N, K)


def check_all_forms_exact(dy, x, gpu, what):
    """linear_wgrad, linear_wgrad(out=prefilled), linear_wgrad_bias with and without out=(dw, db): each output equals fp64 bit for bit."""
    N, K = dy.shape[1], x.shape[1]
    dw_ref, db_ref = tr.wgrad_ref(dy, x), tr.col_sum_ref(dy)
    pw, pb = tr.int_probe((N, K), 7), tr.int_probe((N,), 8)
    dyg, xg = dy.to(gpu), x.to(gpu)
    dw = ops.linear_wgrad(dyg, xg)
    assert_exact(dw, dw_ref, f"{what} linear_wgrad")
    acc = pw.to(gpu)
    assert ops.linear_wgrad(dyg, xg, out=acc) is acc
    assert_exact(acc, pw.double() + dw_ref, f"{what} linear_wgrad(out=prefilled)")
    dw2, db2 = ops.linear_wgrad_bias(dyg, xg)
    assert_exact(dw2, dw_ref, f"{what} linear_wgrad_bias dw")
    assert_exact(db2, db_ref, f"{what} linear_wgrad_bias db")
    aw, ab = pw.to(gpu), pb.to(gpu)
    rw, rb = ops.linear_wgrad_bias(dyg, xg, out=(aw, ab))
    assert rw is aw and rb is ab
    assert_exact(aw, pw.double() + dw_ref, f"{what} linear_wgrad_bias(out=prefilled) dw")
    assert_exact(ab, pb.double() + db_ref, f"{what} linear_wgrad_bias(out=prefilled) db")
    assert torch.equal(ops.linear_wgrad(dyg, xg), dw)  # a second call gives the same bits


@pytest.mark.parametrize("M,N,K,prec,plans", WGRAD_PARAMS)
def test_wgrad_integer_probe_is_exact(gpu, built_lib, M, N, K, prec, plans):
    assert_plan(M, N, K, prec, plans[0] if prec == "fp32" else plans[1])
    dy, x = tr.wgrad_operands(M, N, K, "int", seed=M)
    with precision(prec):
        check_all_forms_exact(dy, x, gpu, f"({M},{N},{K}) {prec} integer probe:")


SPLIT_ROWS = sorted({M for (M, _, _, _, _) in WGRAD_CASES if M <= 512})  # (the split-term probes are exact up to M = 512)
assert SPLIT_ROWS == [1, 17, 33, 49, 65, 129, 193, 257, 300]


@pytest.mark.parametrize("probe", ["a", "b"])
@pytest.mark.parametrize("N,K", [(64, 128), (66, 132)])
@pytest.mark.parametrize("M", SPLIT_ROWS)
def test_wgrad_bf16x3_split_terms_are_exact(gpu, built_lib, M, N, K, probe):
    """The cross terms by name: (a) x = +-(1 + 2^-12), integer dy -- the truth holds ah.bl; (b) the mirror image -- al.bh.  A kernel without the
    term is off by exactly 2^-12 sum(integer operand)."""
    dy, x = tr.wgrad_operands(M, N, K, probe, seed=M)
    with precision("bf16x3"):
        check_all_forms_exact(dy, x, gpu, f"({M},{N},{K}) bf16x3 split probe ({probe}):")


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_wgrad_scales_by_a_power_of_two_bit_for_bit(gpu, built_lib, prec):
    """dW(2^-20 dy, x) == 2^-20 dW(dy, x): holds only if no gradient-sized value (a bf16 low part included) is flushed on the way."""
    M, N, K = 257, 64, 128
    dy, x = torch.randn(M, N, generator=tr.gen(1)).to(gpu), torch.randn(M, K, generator=tr.gen(2)).to(gpu)
    s = 2.0**-20
    with precision(prec):
        big, small = ops.linear_wgrad(dy, x), ops.linear_wgrad(dy * s, x)
        (_, db_big), (_, db_small) = ops.linear_wgrad_bias(dy, x), ops.linear_wgrad_bias(dy * s, x)
    assert big.abs().max() > 1 and torch.equal(small, big * s)
    assert torch.equal(db_small, db_big * s)


@pytest.mark.parametrize("M,N,K,prec", [(M, N, K, p) for (M, N, K, _, _) in WGRAD_CASES if M in (257, 513, 4097) for p in ("fp32", "bf16x3")])
def test_wgrad_random_floats_at_the_slice_edges(gpu, built_lib, M, N, K, prec):
    """The tolerance-based coverage of test_linear_wgrad_and_col_sum (2e-6 / 1e-5 of the largest entry, db 2e-6) at the first split, the
    tail-only reduction and the shrunken slice count."""
    dy, x = torch.randn(M, N, generator=tr.gen(1)), torch.randn(M, K, generator=tr.gen(2))
    ref, tol = tr.wgrad_ref(dy, x), (2e-6 if prec == "fp32" else 1e-5)
    with precision(prec):
        dw = ops.linear_wgrad(dy.to(gpu), x.to(gpu))
        acc = torch.ones(N, K, device=gpu)
        ops.linear_wgrad(dy.to(gpu), x.to(gpu), out=acc)
        dw2, db2 = ops.linear_wgrad_bias(dy.to(gpu), x.to(gpu))
        again = ops.linear_wgrad(dy.to(gpu), x.to(gpu))
    print(f"({M},{N},{K}) {prec}: dw {rel(dw, ref):.2e} (bar {tol:g}), db {rel(db2, tr.col_sum_ref(dy)):.2e} (bar 2e-6)")
    assert rel(dw, ref) < tol and rel(acc, ref + 1.0) < tol
    assert torch.equal(again, dw) and torch.equal(dw2, dw)
    assert rel(db2, tr.col_sum_ref(dy)) < 2e-6


# ------------------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("M", [1, 3, 5, 63, 64, 127, 128, 129, 16385])
def test_col_sum_integer_probe_is_exact(gpu, built_lib, M, N):
    """The ordered form (through ops.col_sum, fresh and onto a prefilled `out`) and the atomic nm_col_sum (accumulate 0 and 1)."""
    plan = tr.col_sum_plan(M)
    if M == 129:
        assert tuple(plan) == (2, 65, 2)  # two parts of 65 + 64 rows
    if M == 16385:
        assert tuple(plan) == (256, 65, 253) and M - 252 * 65 == 5  # 256 chunks guessed, 253 parts, the last of 5 rows
    h = _lib.lib()
    assert h.nm_col_sum_workspace_bytes(M, N) == plan.chunks * N * 4
    dy = tr.int_probe((M, N), 100 * M + N)
    ref, pre = tr.col_sum_ref(dy), tr.int_probe((N,), 9)
    dyg = dy.to(gpu)
    assert_exact(ops.col_sum(dyg), ref, "ops.col_sum")
    out = pre.to(gpu)
    assert ops.col_sum(dyg, out=out) is out
    assert_exact(out, pre.double() + ref, "ops.col_sum(out=prefilled)")
    ws = torch.empty(max(1, plan.chunks * N), device=gpu)
    for accumulate in (0, 1):
        want = ref + pre.double() * accumulate  # (accumulate 0 overwrites what `out` held)
        out = pre.to(gpu)
        _lib.check(h.nm_col_sum(dptr(dyg), M, N, accumulate, dptr(out), stream()), "nm_col_sum")
        assert_exact(out, want, f"nm_col_sum(accumulate={accumulate})")
        out = pre.to(gpu)
        _lib.check(h.nm_col_sum_ordered(dptr(dyg), M, N, accumulate, dptr(out), dptr(ws), ws.numel() * 4, stream()), "nm_col_sum_ordered")
        assert_exact(out, want, f"nm_col_sum_ordered(accumulate={accumulate})")


# ------------------------------------------------------------------------------------------------------------ LayerNorm backward
LN_PARTS = {1: 1, 4: 1, 5: 2, 9: 3, 17: 5}  # partial rows of the ordered form: sum_partials_kernel's tail loop (1, 2, 3) and 4-group + tail (5)


@pytest.mark.parametrize("rows_spec", [1, 4, 5, 9, 17, "4cu+1", "8cu+5"])
@pytest.mark.parametrize("dim", [64, 128, 256, 512])
def test_layernorm_bwd_probe_is_exact(gpu, built_lib, dim, rows_spec):
    """dx, dgamma, dbeta of the LayerNorm probe (eps = 0: mean 0, rstd 1, xh = x exactly) through the ordered form, the input-gradient-only
    form and the atomic form; the C entry points ADD onto dgamma / dbeta."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    rows = rows_spec if isinstance(rows_spec, int) else {"4cu+1": 4 * cus + 1, "8cu+5": 8 * cus + 5}[rows_spec]
    h = _lib.lib()
    parts = tr.ln_bwd_grid(rows, cus, True)
    assert h.nm_layernorm_bwd_workspace_bytes(rows, dim) == parts * 2 * dim * 4
    if isinstance(rows_spec, int):
        assert parts == LN_PARTS[rows]
    else:  # every CU has a workgroup; some wavefronts stride to a second row and others do not, with and without parameter gradients
        nw, nw_dx = 4 * parts, 4 * tr.ln_bwd_grid(rows, cus, False)  # wavefronts with / without parameter gradients
        assert parts == cus and rows % nw in (1, 5) and rows // nw == (1 if rows_spec == "4cu+1" else 2)
        assert (nw_dx >= rows) if rows_spec == "4cu+1" else (nw_dx < rows < 2 * nw_dx)
    x, gamma, dy = tr.layernorm_probe(rows, dim, seed=dim + rows)
    dx_ref, dg_ref, db_ref = tr.layernorm_bwd_ref(x, gamma, dy, 0.0)
    xg, gg, dyg = x.to(gpu), gamma.to(gpu), dy.to(gpu)

    dx, dg, db = ops.layernorm_bwd(xg, gg, dyg, eps=0.0)
    assert_exact(dx, dx_ref, "ops.layernorm_bwd dx")
    assert_exact(dg, dg_ref, "ops.layernorm_bwd dgamma")
    assert_exact(db, db_ref, "ops.layernorm_bwd dbeta")
    dx, dg, db = ops.layernorm_bwd(xg, gg, dyg, eps=0.0, param_grads=False)
    assert dg is None and db is None
    assert_exact(dx, dx_ref, "ops.layernorm_bwd(param_grads=False) dx")

    pg, pb = tr.int_probe((dim,), 11), tr.int_probe((dim,), 12)
    ws = torch.empty(parts * 2 * dim, device=gpu)
    for prefill in (False, True):
        for form in ("atomic", "ordered"):
            dg = pg.to(gpu) if prefill else torch.zeros(dim, device=gpu)
            db = pb.to(gpu) if prefill else torch.zeros(dim, device=gpu)
            dx = torch.full_like(xg, 7.0)
            if form == "atomic":
                _lib.check(h.nm_layernorm_bwd(dptr(xg), dptr(gg), dptr(dyg), rows, dim, 0.0, dptr(dx), dptr(dg), dptr(db), stream()), "nm_layernorm_bwd")
            else:
                _lib.check(h.nm_layernorm_bwd_ordered(dptr(xg), dptr(gg), dptr(dyg), rows, dim, 0.0, dptr(dx), dptr(dg), dptr(db), dptr(ws),
                                                      ws.numel() * 4, stream()), "nm_layernorm_bwd_ordered")
            what = f"nm_layernorm_bwd {form}{' onto a prefill' if prefill else ''}"
            assert_exact(dx, dx_ref, f"{what} dx")
            assert_exact(dg, dg_ref + (pg.double() if prefill else 0), f"{what} dgamma")
            assert_exact(db, db_ref + (pb.double() if prefill else 0), f"{what} dbeta")


# ------------------------------------------------------------------------------------------------------------ l2-normalise backward
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("dim", [64, 128, 256, 512])
def test_l2norm_bwd_per_row(gpu, built_lib, dim, rows):
    """df = dy / (r + e) - f (f . dy) / (r (r + e)^2) against fp64 from the fp32 inputs, row by row:  max|err| <= 1e-5 max|dy_row| / (r + 1e-6)
    -- the project's 1e-5 for this kernel on the scale of the row's first term, so that it means the same on a zero row, a row scaled by 1e-3
    and one scaled by 1e3, and does not lean on the cancellation between the two terms."""
    f, dy = torch.randn(rows, dim, generator=tr.gen(1)), torch.randn(rows, dim, generator=tr.gen(2))
    if rows >= 5:
        f[1] = 0.0
        f[2] *= 1e-3
        f[rows - 1] *= 1e3
    ref, r = tr.l2norm_bwd_ref(f, dy)
    got = ops.l2norm_bwd(f.to(gpu), dy.to(gpu)).cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().amax(-1)
    bar = 1e-5 * dy.double().abs().amax(-1) / (r[:, 0] + 1e-6)
    worst = (err / bar).max().item()
    print(f"l2norm_bwd rows={rows} dim={dim}: worst err / bar = {worst:.3f}" + (f"; zero row {(err[1] / bar[1]).item():.2e}, 1e-3 row "
          f"{(err[2] / bar[2]).item():.3f}, 1e3 row {(err[rows - 1] / bar[rows - 1]).item():.3f}" if rows >= 5 else ""))
    assert (err <= bar).all(), f"rows {(err > bar).nonzero().flatten().tolist()[:8]} above the bar (worst {worst:.3f} x)"
    if rows >= 5:  # the zero row: finite and dy / e
        assert ((got[1] - dy[1].double() * 1e6).abs().max() <= bar[1]).item()
