"""The weight ring of the split NeRF kernels (csrc/nerf_split_chain.h: ring_request / ring_acquire_two / ring_open) under back-to-back
tiles.  A wrong schedule -- a slot requested into a ring position somebody still reads, or read before it landed -- shows as stale or
half-landed weights: wrong values that vary from run to run, and only when a workgroup runs several tiles one after the other.  So the
problems here are sized from the device: R S / 128 >= 2.5 x the CU count (every persistent workgroup runs two tiles, half of them a
third), with a ragged last tile, at every row length at which the tile takes another form (32, 64, 128, 256).

Passes: colour heads + tap 7 / + tap 3, no colour heads + tap 3 / and no feature, the zero-tail skip (which reaches the leftover pass),
and a Cambridge-style launch with an appearance row next to one without (the views layer's third extra K-step is left out when there is
no row: both ways).  Modes: fp16x3, bf16x3, fp16x1.
Checks: every output against the fp32-MFMA kernel (csrc/nerf_fwd.hip) on the same inputs at the bar of the split-kernel tests (1e-4 of the
tensor's scale, tests/nerf_kernel_util.py; fp16x1 at the 2e-3 of scale its own tests state for a smooth field), and three repeated launches
bit-equal.  The pointwise forward / backward pair of the iNeRF refinement gets the same repeat check and the references of
tests/test_inerf_gpu.py (the fp32 GEMM chain).  Seeded inputs only; networks, launches and comparisons: tests/nerf_kernel_util.py."""
import functools

import pytest
import torch

from nerf_kernel_util import KEYS, PASSES, TOL, TOL_FP16X1, camera_rays, compare_repeated, fence_posts, launch, network, points_case, points_pair
from nerfmatch_amd import inerf, ops, synth

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rays_for(S):
    """smallest ray count with R S / 128 >= 2.5 CUs, plus 21 (S = 64 on 256 CUs: 1301), odd against the rays per tile"""
    R = -(-int(2.5 * _cus() * 128) // S) + 21
    nr = max(1, 128 // S)
    return R + 1 if (nr > 1 and R % nr == 0) else R


def _network(net):
    """(renderer, appearance row or None) for "7scenes", "cambridge_row", "cambridge_no_row" (the Cambridge network launched without its row)"""
    ren, _, row = network("7scenes" if net == "7scenes" else "cambridge", 7)
    return ren, (None if net == "cambridge_no_row" else row)


@functools.lru_cache(maxsize=None)
def _inputs(S):
    """(rays, coarse fence posts, zero-tail fence posts + the resampler's flag) of one seeded bundle, on the GPU"""
    R = _rays_for(S)
    rays = camera_rays(*range(-(-R // 4800)))[:R].contiguous()
    t = fence_posts(rays, S, 100 + S)
    w = launch(_network("7scenes")[0], "coarse", "fp32", rays, t, tap_layer=-1, need_rgb=False, need_feat=False)["weights"]
    t_tail, flag = ops.resample(t, w, synth.resample_jitter((R, S + 1), 200 + S).to(rays.device), randomized=True, want_tail_flag=True)
    assert int(flag.item()) == 0  # the zero-width premise holds: the skip is taken
    return rays, t, t_tail, flag


@functools.lru_cache(maxsize=None)
def _reference(net, S, name, tail):
    """the fp32-MFMA kernel on the same inputs (the full evaluation, also for the zero-tail case); computed once per case, never written"""
    ren, row = _network(net)
    rays, t, t_tail, _ = _inputs(S)
    out = launch(ren, "fine", "fp32", rays, t_tail if tail else t, row, **PASSES[name])
    return {k: v.clone() for k, v in out.items() if v is not None}


def _launch(precision, net, S, name, tail):
    ren, row = _network(net)
    rays, t, t_tail, flag = _inputs(S)
    kw = dict(PASSES[name], zero_tail=True, tail_flag=flag) if tail else PASSES[name]
    return {k: v for k, v in launch(ren, "fine", precision, rays, t_tail if tail else t, row, **kw).items() if v is not None}


def _check(precision, net, S, name, tail=False):
    R = _rays_for(S)
    assert R * S >= 2.5 * _cus() * 128
    runs = [_launch(precision, net, S, name, tail) for _ in range(3)]
    compare_repeated(runs, _reference(net, S, name, tail), TOL_FP16X1 if precision == "fp16x1" else TOL,
                     f"{precision} S {S} R {R} {name} {net}{' zero-tail' if tail else ''}")
    if tail:
        assert float(runs[0]["weights"][:, S // 2 + 1:].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(PASSES))
@pytest.mark.parametrize("S", [32, 64, 128, 256])
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3", "fp16x1"])
def test_back_to_back_tiles(gpu, built_lib, precision, S, name):
    _check(precision, "7scenes", S, name)


@pytest.mark.parametrize("S", [32, 64, 128, 256])
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3", "fp16x1"])
def test_zero_tail_skip_and_leftover_pass(gpu, built_lib, precision, S):
    _check(precision, "7scenes", S, "rgb_tap3", tail=True)


@pytest.mark.parametrize("net", ["cambridge_row", "cambridge_no_row"])
@pytest.mark.parametrize("S", [32, 64, 128, 256])
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3", "fp16x1"])
def test_appearance_row_and_none(gpu, built_lib, precision, S, net):
    """Cambridge-style network: with the row the views layer runs its third extra K-step, without one (a zero row's products) it leaves it out"""
    _check(precision, net, S, "rgb_tap7")
    if net == "cambridge_no_row":  # no row == a row of zeros, bit for bit: the K-step left out only ever added exact zeros
        ren, _ = _network(net)
        rays, t, _, _ = _inputs(S)
        a = launch(ren, "fine", precision, rays, t, None, **PASSES["rgb_tap7"])
        b = launch(ren, "fine", precision, rays, t, torch.zeros(16, device=rays.device), **PASSES["rgb_tap7"])
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("app", [False, True])
def test_pointwise_pair(gpu, built_lib, app):
    """nm_nerf_points_fwd_rays_bf16x3 / nm_nerf_points_bwd_tap_bf16x3 over enough samples that every workgroup runs several tiles, the last
    one ragged: repeated launches bit-equal, outputs and gradients at the bars of tests/test_inerf_gpu.py against the fp32 GEMM chain"""
    Sa, tap = 65, 3
    R = -(-int(2.5 * _cus() * 128) // Sa) + 1
    n = R * Sa
    assert n % 128 != 0 and n >= 2.5 * _cus() * 128
    ren, rays, z, app_row, g = points_case(app, R, seed=31)
    p = points_pair(inerf.FusedField(ren.nerf_fine, gpu), inerf.FineField(ren.nerf_fine, gpu), rays, z, Sa, app_row, tap, g, repeats=2)
    for got, want in p.grads:  # (bars and their reasons: test_tapped_points_kernels_vs_gemm_chain)
        row = (got - want).abs().max(1).values / want.abs().max().item()
        assert (row <= 2e-4).float().mean().item() >= 0.995, (row > 2e-4).sum().item()
        assert ((got - want).norm() / want.norm()).item() < 1e-2
