"""The weight ring of the split NeRF kernels (csrc/nerf_split_chain.h: ring_request / ring_acquire_two / ring_open) under back-to-back
tiles.  A wrong schedule -- a slot requested into a ring position somebody still reads, or read before it landed -- shows as stale or
half-landed weights: wrong values that vary from run to run, and only when a workgroup runs several tiles one after the other.  So the
problems here are sized from the device: R S / 128 >= 2.5 x the CU count (every persistent workgroup runs two tiles, half of them a
third), with a ragged last tile, at every row length at which the tile takes another form (32, 64, 128, 256).

Passes: colour heads + tap 7 / + tap 3, no colour heads + tap 3 / and no feature, the zero-tail skip (which reaches the leftover pass),
and a Cambridge-style launch with an appearance row next to one without (the views layer's third extra K-step is left out when there is
no row: both ways).  Modes: fp16x3, bf16x3, fp16x1.
Checks: every output against the fp32-MFMA kernel (csrc/nerf_fwd.hip) on the same inputs at the bar of the split-kernel tests (1e-4 of the
tensor's scale, tests/test_nerf_gpu.py; fp16x1 at the 2e-3 of scale its own tests state for a smooth field), and three repeated launches
bit-equal.  The pointwise forward / backward pair of the iNeRF refinement gets the same repeat check and the references of
tests/test_inerf_gpu.py (the fp32 GEMM chain).  Seeded inputs only."""
import functools

import pytest
import torch

from nerfmatch_amd import inerf, ops, synth
from nerfmatch_amd.nerf.renderer import NerfRenderer
from test_inerf_gpu import _points_case
from test_nerf_gpu import TOL, relerr

pytestmark = pytest.mark.gpu
KEYS = ("weights", "feat", "pts", "rgb", "depth", "acc")
TOL_FP16X1 = 2e-3  # tests/test_nerf_gpu.py, test_single_product_render_error_stated: smooth field, of scale
PASSES = {
    "rgb_tap7": dict(tap_layer=7, need_rgb=True, need_feat=True),
    "rgb_tap3": dict(tap_layer=3, need_rgb=True, need_feat=True),
    "norgb_tap3": dict(tap_layer=3, need_rgb=False, need_feat=True),
    "norgb_nofeat": dict(tap_layer=-1, need_rgb=False, need_feat=False),
}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rays_for(S):
    """smallest ray count with R S / 128 >= 2.5 CUs, plus 21 (S = 64 on 256 CUs: 1301), odd against the rays per tile"""
    R = -(-int(2.5 * _cus() * 128) // S) + 21
    nr = max(1, 128 // S)
    return R + 1 if (nr > 1 and R % nr == 0) else R


@functools.lru_cache(maxsize=None)
def _network(net):
    """(renderer, appearance row or None) for "7scenes", "cambridge_row", "cambridge_no_row" (the Cambridge network launched without its row)"""
    if net == "cambridge_no_row":
        return _network("cambridge_row")[0], None
    app = net != "7scenes"
    dev = torch.device("cuda:0")
    cfg = synth.nerf_config("cambridge" if app else "7scenes", num_pts=64)
    ren = NerfRenderer(cfg, num_frames=5 if app else None, training=False, stop_layer=3)
    sd = synth.nerf_state_dict(seed=7, app_vocab=5 if app else 0, density_bias=3.0)
    ren.load_state_dict(sd, strict=True)
    ren.to(dev).eval()
    ren.calibrate(dev)  # fp16x3 operand scales from the seeded probe bundle
    return ren, (sd["embedding_a.weight"][1].contiguous().to(dev) if app else None)


@functools.lru_cache(maxsize=None)
def _inputs(S):
    """(rays, coarse fence posts, zero-tail fence posts + the resampler's flag) of one seeded bundle, on the GPU"""
    dev = torch.device("cuda:0")
    R = _rays_for(S)
    rays = torch.cat([ops.raygen(synth.intrinsics(), synth.camera_pose(q), 480, 640, dev)[0] for q in range(-(-R // 4800))])[:R].contiguous()
    t = ops.sample_coarse(rays, synth.uniform01((R, S + 1), 100 + S).to(dev), S)
    ren, _ = _network("7scenes")
    with torch.no_grad():
        w = ops.nerf_fwd(ren.nerf_coarse.packed(dev, "fp32"), rays, t, tap_layer=-1, need_rgb=False, need_feat=False)["weights"]
    t_tail, flag = ops.resample(t, w, synth.resample_jitter((R, S + 1), 200 + S).to(dev), randomized=True, want_tail_flag=True)
    assert int(flag.item()) == 0  # the zero-width premise holds: the skip is taken
    return rays, t, t_tail, flag


@functools.lru_cache(maxsize=None)
def _reference(net, S, name, tail):
    """the fp32-MFMA kernel on the same inputs (the full evaluation, also for the zero-tail case); computed once per case, never written"""
    ren, row = _network(net)
    rays, t, t_tail, _ = _inputs(S)
    with torch.no_grad():
        out = ops.nerf_fwd(ren.nerf_fine.packed(rays.device, "fp32"), rays, t_tail if tail else t, row, **PASSES[name])
    return {k: v.clone() for k, v in out.items() if v is not None}


def _launch(precision, net, S, name, tail):
    ren, row = _network(net)
    rays, t, t_tail, flag = _inputs(S)
    blob = ren.nerf_fine.packed(rays.device, precision)
    kw = dict(PASSES[name], zero_tail=True, tail_flag=flag) if tail else PASSES[name]
    with torch.no_grad():
        out = ops.nerf_fwd(blob, rays, t_tail if tail else t, row, **kw)
    if precision == "fp16x3":  # the guarded fp32 pass must not have rewritten what this file is about
        assert not blob.nm_guard.read()[0], "an fp16x3 operand saturated: the outputs are the fp32 kernel's"
    return {k: v for k, v in out.items() if v is not None}


def _check(precision, net, S, name, tail=False):
    R = _rays_for(S)
    assert R * S >= 2.5 * _cus() * 128
    ref = _reference(net, S, name, tail)
    assert float(ref["weights"].sum(-1).max()) > 0.3  # not vacuous
    runs = [_launch(precision, net, S, name, tail) for _ in range(3)]
    tol = TOL_FP16X1 if precision == "fp16x1" else TOL
    for k in KEYS:
        if k not in ref:
            assert k not in runs[0]
            continue
        err = relerr(runs[0][k].reshape(R, -1), ref[k].cpu().reshape(R, -1))
        print(f"{precision} S {S} R {R} {name} {net}{' zero-tail' if tail else ''} {k}: {err:.2e} of scale")
        assert err < tol, f"{k}: {err:.2e}"
        for again in runs[1:]:
            assert torch.equal(runs[0][k], again[k]), f"{k} differs between repeated launches"
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
        blob = ren.nerf_fine.packed(rays.device, precision)
        with torch.no_grad():
            a = ops.nerf_fwd(blob, rays, t, None, **PASSES["rgb_tap7"])
            b = ops.nerf_fwd(blob, rays, t, torch.zeros(16, device=rays.device), **PASSES["rgb_tap7"])
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
    ren, rays, z, app_row, g = _points_case(gpu, app, R, Sa, seed=31)
    chain = inerf.FineField(ren.nerf_fine, gpu)
    xi, xd = inerf._encode(rays, z, Sa, app_row)
    logit, sig, saved = chain.forward(xi, xd)
    fused = inerf.FusedField(ren.nerf_fine, gpu)
    out4, gates, feats = fused.forward_rays(rays, z, Sa, app_row, tap)
    h_ref = saved[0][tap]
    assert (feats - h_ref).abs().max().item() < 1e-5 * max(1.0, h_ref.abs().max().item())
    assert (out4[:, :3] - logit[:, :3]).abs().max().item() < 1e-5 * max(1.0, logit.abs().max().item())
    assert (out4[:, 3] - sig[:, 0]).abs().max().item() < 1e-5 * max(1.0, sig.abs().max().item())
    g_logit = torch.zeros(n, 8, device=gpu)
    g_logit[:, :3] = torch.randn(n, 3, generator=g).to(gpu) * 1e-4
    g_sig = torch.zeros(n, 8, device=gpu)
    g_sig[:, 0] = torch.randn(n, generator=g).to(gpu) * 1e-5
    w = torch.rand(R, Sa, generator=g).to(gpu) * 0.1
    g_pf = torch.randn(R, 256, generator=g).to(gpu) * 1e-3
    g_feats = (w.reshape(n, 1) * g_pf.repeat_interleave(Sa, 0)).contiguous()
    gxi_ref, gxd_ref = chain.backward(g_logit, g_sig, saved, (tap, g_feats))
    g4 = torch.cat([g_logit[:, :3], g_sig[:, :1]], 1).contiguous()
    (a0, a5), gxd = fused.backward(g4, gates, (tap, w, g_pf))
    for got, want in ((a0 + a5, gxi_ref), (gxd, gxd_ref)):  # (bars and their reasons: test_tapped_points_kernels_vs_gemm_chain)
        assert torch.isfinite(got).all()
        row = (got - want).abs().max(1).values / want.abs().max().item()
        assert (row <= 2e-4).float().mean().item() >= 0.995, (row > 2e-4).sum().item()
        assert ((got - want).norm() / want.norm()).item() < 1e-2
    for _ in range(2):
        out4_b, gates_b, feats_b = fused.forward_rays(rays, z, Sa, app_row, tap)
        assert torch.equal(out4_b, out4) and torch.equal(gates_b, gates) and torch.equal(feats_b, feats)
        (b0, b5), bxd = fused.backward(g4, gates, (tap, w, g_pf))
        assert torch.equal(b0, a0) and torch.equal(b5, a5) and torch.equal(bxd, gxd)
