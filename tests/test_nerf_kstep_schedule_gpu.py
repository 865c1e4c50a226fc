"""The per-gap schedule of the split NeRF kernels' K-steps (csrc/nerf_split_chain.h: slot_step8 / slot_step4x2 / slot_step4 and the tables
at UnitWork) at the sizes tests/test_nerf_ring_schedule_gpu.py leaves out.  That file sizes its problems so that every workgroup runs
several tiles back to back; here the grid is SMALLER than the chip: 1, 2 and 5 tiles (a ray of 256 samples is two tiles, so S = 256 runs
2 and 6), each opened on a cold ring with no second tile behind it -- the first K-steps read operands that ring_open alone fetched, and the
last ones request slots nobody consumes.  A wrong placement (an operand read in front of the barrier that makes its slot valid, a
re-packing operation in front of the one it depends on, a unit finished too late for its MFMA) shows as wrong values, or as values
that vary from run to run.

Cases: the four pass types x {fp16x3, bf16x3} x S in {32, 64, 128, 256} x the tile counts; the Cambridge network with and without its
appearance row at S = 32 and 256 (the parity of the views layer's K-step count differs between the two); trained-like weights (synth
style "surface": the re-packing scale is not 1, activations are large) on fp16x3; the pointwise forward / backward pair of the iNeRF
refinement at one and five tiles.
Checks: every output against the fp32-MFMA kernel (csrc/nerf_fwd.hip) on the same inputs at TOL of tests/nerf_kernel_util.py (1e-4 of the
tensor's scale, the bar of the split kernels); the pointwise pair against the fp32 GEMM chain at the bars of tests/test_inerf_gpu.py;
three repeated launches bit-equal.  Seeded inputs only; every reference is computed once and never written."""
import functools

import pytest
import torch

from nerf_kernel_util import PASSES, TOL, camera_rays, compare_repeated, fence_posts, launch, network, points_bundle, points_pair
from nerfmatch_amd import inerf

pytestmark = pytest.mark.gpu
TILES = (1, 2, 5)


def _rays(S, tiles):
    """fewest rays that fill `tiles` tiles of 128 samples (at least one ray)"""
    return max(1, -(-tiles * 128 // S))


# (S, R) without repeats: S = 256 has one ray (two tiles) for both 1 and 2
SIZES = sorted({(S, _rays(S, n)) for S in (32, 64, 128, 256) for n in TILES})
# arguments of nerf_kernel_util.network
NETWORKS = {"7scenes": ("7scenes", 11), "cambridge_row": ("cambridge", 11), "cambridge_no_row": ("cambridge", 11),
            "surface": ("7scenes", 0, "surface")}  # (seed 0, the bench's trained-like leg: other seeds leave the part of space these cameras see empty)


def _network(net):
    """(renderer, appearance row or None): "7scenes", "surface" (trained-like weights), "cambridge_row", "cambridge_no_row" """
    ren, _, row = network(*NETWORKS[net])
    return ren, (None if net == "cambridge_no_row" else row)


@functools.lru_cache(maxsize=None)
def _inputs(S, R, net):
    """R rays spread over an image and their fence posts.  The "surface" network occupies about a quarter of space (synth.SURFACE_STYLE), so a
    handful of rays may all miss it: there the R rays are those of 240 candidates on which the REFERENCE kernel finds the most opacity."""
    allrays = camera_rays(2)
    if net == "surface":
        cand = allrays[7::20].contiguous()
        t = fence_posts(cand, S, 300 + S)
        acc = launch(_network(net)[0], "fine", "fp32", cand, t, tap_layer=-1, need_rgb=False, need_feat=False)["acc"]
        keep = torch.sort(torch.topk(acc, R).indices).values
        return cand[keep].contiguous(), t[keep].contiguous()
    rays = allrays[37:37 + 61 * R:61].contiguous()
    assert rays.shape[0] == R
    return rays, fence_posts(rays, S, 300 + S + R)


@functools.lru_cache(maxsize=None)
def _reference(net, S, R, name):
    ren, row = _network(net)
    out = launch(ren, "fine", "fp32", *_inputs(S, R, net), row, **PASSES[name])
    return {k: v.clone() for k, v in out.items() if v is not None}


def _launch(precision, net, S, R, name):
    ren, row = _network(net)
    return {k: v for k, v in launch(ren, "fine", precision, *_inputs(S, R, net), row, **PASSES[name]).items() if v is not None}


def _check(precision, net, S, R, name):
    assert R * S <= 6 * 128 < 128 * torch.cuda.get_device_properties(0).multi_processor_count  # fewer tiles than workgroups
    runs = [_launch(precision, net, S, R, name) for _ in range(3)]
    compare_repeated(runs, _reference(net, S, R, name), TOL, f"{precision} S {S} R {R} {name} {net}")


@pytest.mark.parametrize("name", list(PASSES))
@pytest.mark.parametrize("S,R", SIZES)
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_grids_smaller_than_the_chip(gpu, built_lib, precision, S, R, name):
    _check(precision, "7scenes", S, R, name)


@pytest.mark.parametrize("net", ["cambridge_row", "cambridge_no_row"])
@pytest.mark.parametrize("S", [32, 256])
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_views_layer_with_and_without_the_appearance_step(gpu, built_lib, precision, S, net):
    _check(precision, net, S, _rays(S, 5), "rgb_tap7")


@pytest.mark.parametrize("name", ["rgb_tap7", "rgb_tap3"])
@pytest.mark.parametrize("S,R", [(64, 1), (64, 10), (256, 3)])
def test_trained_like_weights(gpu, built_lib, S, R, name):
    """synth style "surface": operand scales other than 1 in the re-packing fma, activations of O(10)"""
    _check("fp16x3", "surface", S, R, name)


@functools.lru_cache(maxsize=None)
def _points_net(app):
    """(appearance row, the fine network as fp32 GEMM chain, the same as fused kernels), built once"""
    gpu = torch.device("cuda:0")
    ren, _, row = network("cambridge" if app else "7scenes", 41, calibrate=False)
    return row, inerf.FineField(ren.nerf_fine, gpu), inerf.FusedField(ren.nerf_fine, gpu)


SEEDS = {9: 7, 1: 37}  # bundles per ray count: 4095 and 2405 rows


@pytest.mark.parametrize("R", [1, 9])
@pytest.mark.parametrize("app", [False, True])
def test_pointwise_pair_at_one_and_five_tiles(gpu, built_lib, app, R):
    """nm_nerf_points_fwd_rays_bf16x3 / nm_nerf_points_bwd_tap_bf16x3 on 65 and 585 samples (one and five tiles, the last ragged): outputs and
    gradients at the bars of tests/test_inerf_gpu.py against the fp32 GEMM chain, repeated launches bit-equal.
    The gradient bars are statements about MANY rows: at most 5 rows in a thousand further than 2e-4 from the chain's gradient -- the rows on
    which a ReLU within rounding of zero gates differently in the two passes and carries another, equally valid sub-gradient -- and all rows
    together within 1e-2 in the L2 sense.  One row of 585 is already 1.7 in a thousand, and one such row among 65 is 1.1e-2 .. 1.7e-2 of their
    L2 norm (measured: seeded bundles of 585 samples hold 0 to 3 such rows): a single launch of these sizes cannot resolve either bar.  So
    the launch is repeated on SEEDS[R] seeded bundles and both bars are taken over all their rows (4095 and 2405: no fewer than the 2405 of
    the smallest case of test_tapped_points_kernels_vs_gemm_chain); the forward bars and bit-equal repeats hold per launch."""
    Sa, tap = 65, 3
    n = R * Sa
    assert -(-n // 128) == (1 if R == 1 else 5) and n % 128 != 0
    app_row, chain, fused = _points_net(app)
    near, err2, ref2, total = [0, 0], [0.0, 0.0], [0.0, 0.0], 0
    for seed in range(SEEDS[R]):
        rays, z, g = points_bundle(R, 1000 * R + seed)
        p = points_pair(fused, chain, rays, z, Sa, app_row, tap, g, repeats=2)
        for i, (got, want) in enumerate(p.grads):  # (bars and their reasons: test_tapped_points_kernels_vs_gemm_chain)
            row = (got - want).abs().max(1).values / want.abs().max().item()
            near[i] += int((row <= 2e-4).sum().item())  # (of this launch's largest entry: no laxer than of the largest of all)
            err2[i] += float((got - want).double().pow(2).sum())
            ref2[i] += float(want.double().pow(2).sum())
        total += n
    l2 = [(e / r) ** 0.5 for e, r in zip(err2, ref2)]
    print(f"pointwise pair app {app} R {R}: rows within 2e-4 of the chain's gradient: d xi {near[0]} / {total}, d xd {near[1]} / {total}; "
          f"all rows together, L2: d xi {l2[0]:.2e}, d xd {l2[1]:.2e}")
    assert near[0] >= 0.995 * total and near[1] >= 0.995 * total, (near, total)
    assert l2[0] < 1e-2 and l2[1] < 1e-2, l2
