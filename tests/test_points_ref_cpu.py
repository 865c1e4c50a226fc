"""The fp64 helpers tests/test_points_shared_gates_gpu.py judges the fine field's three backward routes with (tests/points_ref_util.py),
checked without a GPU: the backward against autograd through the oracle's MLP, the reader of the gate table against a table built bit by
bit, and what a per-row bar of 2e-4 can see -- the size of a single wrong gate bit, and the split arithmetic's own error."""
import pytest
import torch

from nerfmatch_amd import synth
from oracle import nerf_oracle as no
from points_ref_util import (SPLIT_BAR, TILE, cpu_bundle, decode_views_gates, field_backward64, field_forward64, fine_state_dict, oracle_rows,
                             row_errors, split_matmul)

SEED = 21  # the synthetic fine network of the pointwise tests (nerf_kernel_util.points_case)


def case(app, R, Sa, seed=SEED):
    """(full state dict, fine network's entries, xi, xd, g4 ~ N(0,1), generator) for R seeded rays of Sa samples"""
    sd = synth.nerf_state_dict(seed=seed, app_vocab=5 if app else 0, density_bias=3.0)
    rays, z, g = cpu_bundle(R, seed)
    xi, xd = oracle_rows(rays, z, Sa, sd["embedding_a.weight"][1] if app else None)
    return sd, fine_state_dict(sd), xi, xd, torch.randn(R * Sa, 4, generator=g).double(), g


@pytest.mark.parametrize("tap", [None, 0, 4, 5, 7])
@pytest.mark.parametrize("app", [False, True])
def test_backward64_equals_autograd_through_the_oracle(app, tap):
    """field_backward64 with the gates of field_forward64 = torch autograd through oracle.nerf_oracle.nerf_mlp in fp64, to 1e-12 of each
    tensor's largest entry: with and without the appearance row, without a tap and with one at layers 0, 4, 5 (the skip layer) and 7 (next
    to the density head).  The oracle returns sigmoid(logits): its upstream gradient g is handed to the helper as g . s (1 - s)."""
    sd, sdf, xi, xd, g4, g = case(app, 3, 7)
    n = xi.shape[0]
    f = field_forward64(sdf, xi, xd)
    g_h = torch.randn(n, 256, generator=g).double() if tap is not None else None
    params = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    with torch.enable_grad():
        a, b = xi.clone().requires_grad_(True), xd.clone().requires_grad_(True)
        raw, feat = no.nerf_mlp(params, "nerf_fine", a, b[:, :27], b[:, 27:] if app else None, stop_layer=-1 if tap is None else tap)
        loss = (raw * g4).sum() + ((feat * g_h).sum() if tap is not None else 0.0)
        want_xi, want_xd = torch.autograd.grad(loss, [a, b])
    assert (raw[:, :3].detach() - torch.sigmoid(f.logit)).abs().max().item() < 1e-12 and (raw[:, 3:].detach() - f.sigma).abs().max().item() < 1e-12
    if tap is not None:
        assert torch.equal(feat.detach() > 0, f.h[tap] > 0)
    s = torch.sigmoid(f.logit)
    g4l = torch.cat([g4[:, :3] * s * (1 - s), g4[:, 3:]], 1)
    g0, g5, gxd = field_backward64(sdf, g4l, [h > 0 for h in f.h], f.hv > 0, None if tap is None else (tap, g_h))
    assert g0.shape == g5.shape == (n, 90) and gxd.shape == (n, 43 if app else 27)
    assert g0.abs().max().item() > 0 and g5.abs().max().item() > 0
    for got, want in ((g0 + g5, want_xi), (gxd, want_xd)):
        assert row_errors(got, want).max().item() < 1e-12


def build_views_row(bits):
    """the gate table whose row 8 holds bits (n, 128), every other row filled with ones: an explicit loop over (tile, wave, hh, s, ob, q, e),
    as the forward kernel's threads write it"""
    n = bits.shape[0]
    ntiles = (n + TILE - 1) // TILE
    tab = torch.full((ntiles, 9, 256, 4), -1, dtype=torch.int64)
    tab[:, 8] = 0
    for tile in range(ntiles):
        for wave in range(4):
            for hh in range(2):
                for s in range(32):
                    sample, tid = 128 * tile + 32 * wave + s, 64 * wave + 32 * hh + s
                    if sample >= n:
                        continue
                    for ob in range(4):
                        for q in range(4):
                            for e in range(4):
                                if bits[sample, 32 * ob + 8 * q + 4 * hh + e]:
                                    tab[tile, 8, tid, ob >> 1] |= 1 << (16 * (ob & 1) + 4 * q + e)
    tab = torch.where(tab >= 2**31, tab - 2**32, tab).to(torch.int32)  # (bit 31 set: the int32 of the same bits)
    return tab.reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("n", [1, 128, 129])
def test_decode_views_gates_returns_the_bits_put_in(n):
    """n = 129: the ragged second tile holds one sample"""
    bits = torch.rand(n, 128, generator=torch.Generator().manual_seed(n)) < 0.5
    bits[0, :] = True  # (bit 31 of both words set)
    table = build_views_row(bits)
    assert table.numel() == ((n + TILE - 1) // TILE) * 9 * 256 * 16
    assert torch.equal(decode_views_gates(table, n), bits)


def test_a_single_gate_flip_is_far_above_the_row_bar():
    """What one wrong gate bit in a row does to that row, per layer whose gate is flipped (0 .. 7, 8 = the views layer) and per output, of
    the output's largest entry: minimum, 5th percentile and median over the 455 rows are printed.  Where the output depends on the layer
    (g_xd: the views layer; g_xi5: layers 5 .. 7 and the views layer; g_xi0: all nine) the median must exceed ten times the per-row bar of
    the split routes -- which keeps that bar meaningful should the synthetic weights ever change."""
    sd, sdf, xi, xd, g4, g = case(True, 7, 65)
    n = xi.shape[0]
    f = field_forward64(sdf, xi, xd)
    gates, gates_v = [h > 0 for h in f.h], f.hv > 0
    base = field_backward64(sdf, g4, gates, gates_v)
    scale = [t.abs().max().item() for t in base]
    depends = {"g_xi0": range(9), "g_xi5": range(5, 9), "g_xd": range(8, 9)}
    for l in range(9):
        unit = torch.randint(0, 128 if l == 8 else 256, (n,), generator=g)
        flipped = [x.clone() for x in gates] + [gates_v.clone()]
        flipped[l][torch.arange(n), unit] ^= True
        moved = field_backward64(sdf, g4, flipped[:8], flipped[8])
        for name, a, b, sc in zip(("g_xi0", "g_xi5", "g_xd"), moved, base, scale):
            row = (a - b).abs().max(1).values / sc
            q = torch.quantile(row, torch.tensor([0.0, 0.05, 0.5], dtype=row.dtype))
            print(f"gate flip in layer {l}: {name} rows move by min {q[0]:.1e}  5 % {q[1]:.1e}  median {q[2]:.1e} of the largest entry")
            if l in depends[name]:
                assert q[2].item() > 10 * SPLIT_BAR, (l, name, q)
            else:
                assert not row.any(), (l, name)


@pytest.mark.parametrize("tap", [None, 5])
def test_split_arithmetic_model_stays_inside_the_row_bar(tap):
    """The shared-gate backward with every GEMM operand rounded to bf16 hi + bf16 lo and hi.hi + hi.lo + lo.hi summed in fp64
    (points_ref_util.split_matmul), against the exact one, per row: the arithmetic's own share of the split routes' error, independent of any
    kernel.  The model's value: worst row 1.1e-5 of the largest entry (g_xi0 without a tap; 7.6e-6 for g_xi5, 7.5e-6 for g_xd; medians
    2e-6 .. 4e-6), i.e. below 5e-5, so the bar of the split routes stays at 2e-4 and needs no allowance for the arithmetic."""
    sd, sdf, xi, xd, g4, g = case(True, 7, 65)
    n = xi.shape[0]
    f = field_forward64(sdf, xi, xd)
    gates, gates_v = [h > 0 for h in f.h], f.hv > 0
    g_h = None
    if tap is not None:
        w = torch.rand(7, 65, generator=g) * 0.5 + 0.5
        g_h = (tap, (w.reshape(n, 1) * torch.randn(7, 256, generator=g).repeat_interleave(65, 0)).float().double())
    exact = field_backward64(sdf, g4.float().double(), gates, gates_v, g_h)
    model = field_backward64(sdf, g4.float().double(), gates, gates_v, g_h, mm=split_matmul)
    for name, a, b in zip(("g_xi0", "g_xi5", "g_xd"), model, exact):
        row = row_errors(a, b)
        print(f"bf16 hi/lo model, tap {tap}: {name} worst row {row.max().item():.1e}  median {row.median().item():.1e} of the largest entry")
        assert row.max().item() < 5e-5
