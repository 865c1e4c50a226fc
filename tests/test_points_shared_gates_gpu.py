"""The fine pass of the iNeRF refinement, row by row against fp64 WITH THE ROUTE'S OWN ReLU GATES (tests/points_ref_util.py): the fused pair
of csrc/nerf_points_bf16.hip and the GEMM chain (nerf/gemm_field.py) under both arithmetics.  Given the gates the backward is a linear map, so
the fp64 result is exact for every row and column and every row is held to the bar -- no share of rows is excused, g_xi0 (the path through
all eight layers, ~40 x smaller than g_xi5) is judged on its own, and the padding columns must be exactly zero.

Shapes (S = 128 fence posts): the smallest at which the tiling can go wrong -- one sample, one exact tile, a second tile of one sample, a
ragged last tile with the appearance row, and 17 tiles on an 8-unit partition stream, where the persistent loop of both kernels makes three
passes (gridDim < ntiles) and ends on a ragged tile.  Measured values: DESIGN.md section 5."""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch

from nerf_kernel_util import points_case
from nerfmatch_amd import _lib, inerf, ops
from points_ref_util import (FP32_BAR, SPLIT_BAR, decode_views_gates, field_backward64, field_forward64, heads64, pts_layer64, row_errors,
                             tapped_gates, views_width)

pytestmark = pytest.mark.gpu

SEED = 21
TAPS = (None, 0, 4, 5, 7)
#         R  Sa  app    8-unit partition stream
SHAPES = [(1, 1, False, False),    # a single sample
          (2, 64, False, False),   # one exact tile
          (3, 43, False, False),   # 129: the second tile holds one sample
          (7, 65, True, False),    # 455: ragged last tile, appearance row
          (33, 65, False, True)]   # 2145: 17 tiles on 8 workgroups -- three passes of the persistent loop, ragged last tile
IDS = [f"R{R}-Sa{Sa}{'-app' if app else ''}{'-cu8' if part else ''}" for R, Sa, app, part in SHAPES]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=IDS)


@contextlib.contextmanager
def launch_stream(part):
    """part: the project's 8-unit partition stream (kept: it lives as long as the process), a synchronize before entering and after leaving"""
    if not part:
        yield
        return
    st = _lib.partition_stream(8)
    assert _lib.lib().nm_stream_cus(st.cuda_stream) == 8
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(st):
            yield
    finally:
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def case(shape):
    """one shape's network, inputs, upstream gradients and the rays-form forward with every tap, computed once and left unchanged"""
    R, Sa, app, part = shape
    ren, rays, z, app_row, g = points_case(app, R, SEED)
    gpu, n = rays.device, R * Sa
    g4 = torch.randn(n, 4, generator=g).to(gpu)  # N(0,1) in all four columns: every row has the same scale
    w = (torch.rand(R, Sa, generator=g) * 0.5 + 0.5).to(gpu)
    g_pf = torch.randn(R, 256, generator=g).to(gpu)
    g_feats = (w.reshape(n, 1) * g_pf.repeat_interleave(Sa, 0)).contiguous()  # w_n . g_pt_feat[ray], as the backward kernel forms it
    fused = inerf.FusedField(ren.nerf_fine, gpu)
    sdf = {k: v.detach().cpu() for k, v in ren.nerf_fine.state_dict().items()}
    with launch_stream(part):
        xi, xd = inerf._encode(rays, z, Sa, app_row)
        out4, gates, feats, gate = tapped_gates(fused, rays, z, Sa, app_row)
        if part:
            assert _lib.lib().nm_stream_cus(_lib.stream()) == 8 < (n + 127) // 128
        feats = [f.cpu() for f in feats]
    return SimpleNamespace(ren=ren, rays=rays, z=z, app_row=app_row, n=n, vw=views_width(sdf), g4=g4, w=w, g_pf=g_pf, g_feats=g_feats,
                           fused=fused, sdf=sdf, xi=xi, xd=xd, out4=out4, gates=gates, feats=feats, gate=gate,
                           gate_v=decode_views_gates(gates, n))


def of_scale(got, want):
    """max |got - want| over every entry, of max(1, largest reference entry)"""
    want = want.double().cpu()
    return (got.double().cpu() - want).abs().max().item() / max(1.0, want.abs().max().item())


def check_rows(what, got, want, bar, pad_from):
    """every row of got[:, :pad_from] within `bar` of the largest entry of `want`; the columns from pad_from on exactly zero"""
    row = row_errors(got[:, :pad_from], want)
    print(f"{what}: worst row {row.max().item():.2e}  median {row.median().item():.2e} of the largest entry ({want.abs().max().item():.2e}), bar {bar:.0e}")
    assert not got[:, pad_from:].any(), f"{what}: padding columns not zero"
    return row.max().item() < bar, f"{what}: {(row >= bar).sum().item()} of {row.numel()} rows over {bar:.0e}, worst {row.max().item():.2e} (row {row.argmax().item()})"


def check_fused_backward(c, gates, tap, what):
    """nm_nerf_points_bwd_bf16x3 (tap None) / nm_nerf_points_bwd_tap_bf16x3 on `gates` against fp64 with the gates of the forward launch"""
    (g0, g5), gxd = c.fused.backward(c.g4, gates, None if tap is None else (tap, c.w, c.g_pf))
    r0, r5, rxd = field_backward64(c.sdf, c.g4, c.gate, c.gate_v, None if tap is None else (tap, c.g_feats))
    res = [check_rows(f"{what} tap {tap} g_xi0", g0, r0, SPLIT_BAR, 90), check_rows(f"{what} tap {tap} g_xi5", g5, r5, SPLIT_BAR, 90),
           check_rows(f"{what} tap {tap} g_xd", gxd, rxd, SPLIT_BAR, c.vw)]
    return [msg for ok, msg in res if not ok]


@shapes
def test_forward_teacher_forced(gpu, built_lib, shape):
    """a. Every pts layer in fp64 on the kernel's OWN previous tap (layer 0: the xi rows of nm_inerf_encode) against the kernel's tap, the
    fp64 heads on the kernel's tap 7 and the xd rows against out4: every row and column within 1e-5 of max(1, largest reference entry) --
    the bar points_pair holds one tapped layer to, here on all eight (the skip concatenation at layer 5 among them) and the density head."""
    c = case(shape)
    for l in range(8):
        err = of_scale(c.feats[l], pts_layer64(c.sdf, l, c.xi, c.feats[l - 1] if l else None))
        print(f"{IDS[SHAPES.index(shape)]} layer {l}: {err:.2e} of scale")
        assert err < 1e-5, (l, err)
    _, _, logit, sigma = heads64(c.sdf, c.feats[7], c.xd)
    e_rgb, e_sig = of_scale(c.out4[:, :3], logit), of_scale(c.out4[:, 3:], sigma)
    print(f"{IDS[SHAPES.index(shape)]} logits {e_rgb:.2e}  sigma {e_sig:.2e} of scale")
    assert e_rgb < 1e-5 and e_sig < 1e-5, (e_rgb, e_sig)


@shapes
def test_views_gates_follow_the_stated_layout(gpu, built_lib, shape):
    """b. Row 8 of the gate table, decoded by the layout stated in the kernel file, = (u > 0) of the fp64 views pre-activation on the kernel's
    own tap 7, for EVERY unit with |u| > 1e-4 max|u| (nearer to zero the kernel's rounding may decide): a wrong bit, word, half-wavefront or
    sample order fails on nearly every row."""
    c = case(shape)
    u, _, _, _ = heads64(c.sdf, c.feats[7], c.xd)
    clear = u.abs() > 1e-4 * u.abs().max()
    print(f"{IDS[SHAPES.index(shape)]}: {clear.all(1).float().mean().item():.3f} of rows have every views unit outside the margin, "
          f"{(~clear).sum().item()} units inside it")
    assert clear.float().mean().item() > 0.9  # (not vacuous)
    wrong = (c.gate_v != (u > 0)) & clear
    assert not wrong.any(), f"{wrong.sum().item()} gate bits differ from the fp64 sign, first (row, unit): {wrong.nonzero()[0].tolist()}"
    assert c.gate_v.any() and not c.gate_v.all()


@shapes
def test_fused_backward_every_row(gpu, built_lib, shape):
    """c. nm_nerf_points_bwd_bf16x3 and nm_nerf_points_bwd_tap_bf16x3 (tap 0, 4, 5, 7; w in [0.5, 1], g_pt_feat ~ N(0,1)) against fp64 with
    the kernel's own gates (layers 0 .. 7: the eight taps of the forward kernel; views layer: the decoded row 8): g_xi0, g_xi5 and g_xd
    separately, every row within 2e-4 of the tensor's largest reference entry, padding exactly zero."""
    c = case(shape)
    failed = []
    with launch_stream(shape[3]):
        for tap in TAPS:
            failed += check_fused_backward(c, c.gates, tap, f"fused {IDS[SHAPES.index(shape)]}")
    assert not failed, failed


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@shapes
def test_gemm_chain_backward_every_row(gpu, built_lib, shape, precision):
    """d. FineField.forward / backward under both arithmetics against fp64 with the gates of the chain's own saved activations, g_h entering
    at the same taps: g_xi against the reference sum g_xi0 + g_xi5, and g_xd, every row; fp32 within 2e-5, bf16x3 within 2e-4."""
    c = case(shape)
    bar = FP32_BAR if precision == "fp32" else SPLIT_BAR
    g_logit, g_sig = torch.zeros(c.n, 8, device=gpu), torch.zeros(c.n, 8, device=gpu)
    g_logit[:, :3], g_sig[:, 0] = c.g4[:, :3], c.g4[:, 3]
    failed = []
    before = ops.LINEAR_PRECISION
    ops.LINEAR_PRECISION = precision
    try:
        with launch_stream(shape[3]):
            chain = inerf.FineField(c.ren.nerf_fine, gpu)
            logit, sig, saved = chain.forward(c.xi, c.xd)
            gate, gate_v = [h.cpu() > 0 for h in saved[0]], saved[1].cpu() > 0
            for tap in TAPS:
                gxi, gxd = chain.backward(g_logit, g_sig, saved, None if tap is None else (tap, c.g_feats))
                r0, r5, rxd = field_backward64(c.sdf, c.g4, gate, gate_v, None if tap is None else (tap, c.g_feats))
                what = f"chain {precision} {IDS[SHAPES.index(shape)]} tap {tap}"
                failed += [msg for ok, msg in (check_rows(f"{what} g_xi", gxi, r0 + r5, bar, 90), check_rows(f"{what} g_xd", gxd, rxd, bar, c.vw)) if not ok]
    finally:
        ops.LINEAR_PRECISION = before
    assert not failed, failed


@shapes
def test_rows_form_forward(gpu, built_lib, shape):
    """e. nm_nerf_points_fwd_bf16x3 (FusedField.forward: xi / xd rows from memory) on the rows of nm_inerf_encode: out4 against the fp64
    network within 1e-5 of max(1, largest reference entry); out4 and the whole gate table bit-equal to the rays form's, which encodes its
    samples itself; nm_nerf_points_bwd_bf16x3 on THESE gates against fp64, every row."""
    c = case(shape)
    with launch_stream(shape[3]):
        out4, gates = c.fused.forward(c.xi, c.xd)
        ref = field_forward64(c.sdf, c.xi, c.xd)
        e_rgb, e_sig = of_scale(out4[:, :3], ref.logit), of_scale(out4[:, 3:], ref.sigma)
        print(f"rows form {IDS[SHAPES.index(shape)]}: logits {e_rgb:.2e}  sigma {e_sig:.2e} of scale")
        assert e_rgb < 1e-5 and e_sig < 1e-5, (e_rgb, e_sig)
        differ = (gates != c.gates).float().mean().item()
        print(f"rows form {IDS[SHAPES.index(shape)]}: {differ:.2e} of the gate bytes differ from the rays form's, out4 by {(out4 - c.out4).abs().max().item():.2e}")
        assert torch.equal(out4, c.out4) and torch.equal(gates, c.gates)
        failed = check_fused_backward(c, gates, None, f"rows-form gates {IDS[SHAPES.index(shape)]}")
    assert not failed, failed
