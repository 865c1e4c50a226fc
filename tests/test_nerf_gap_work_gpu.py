"""The fp16x3 render kernel does part of a tile's exposed work in the idle gaps of its K-loops (csrc/nerf_split_chain.h): the weight
request of an even K-step starts behind the barrier of the K-step in front of it (request_early), the IPE operands are fetched one
K-step ahead (IpeFetch), and in a pass with colour heads whose tap is not composited early the density head is added up by the views
layer's units as they re-pack layer 7 (UnitWork<2, true>, dens_open) instead of by alpha_head -- in a kernel of its own, next to the
one that may composite a tap on layer 7 early; a unit's biases are read one unit ahead (bias_next).  None of it changes a result; this
file holds every tap layer, with and without colour heads, to the fp32-MFMA kernel on the same inputs (tap 3 also to the CPU oracle),
at the row lengths at which the along-ray scan takes another form and with ray counts that leave the last tile ragged.

The 1e-4-of-scale bar, networks, inputs and launches: tests/nerf_kernel_util.py (those of tests/test_nerf_tap7_early_gpu.py)."""
import functools

import pytest
import torch

from nerf_kernel_util import KEYS, SHAPES, TOL, coarse_run, compare, launch, oracle_bundle, styled_network, tol_for
from nerfmatch_amd import ops
from oracle import nerf_oracle as no

pytestmark = pytest.mark.gpu
SFEAT = KEYS + ("sample_feat",)


def _keys(rgb, keys=SFEAT):
    return tuple(k for k in keys if rgb or k != "rgb")


@functools.lru_cache(maxsize=None)
def _fp32(style, app, S, R, tap, rgb):
    """the fp32-MFMA kernel's outputs, once per case (both splits are held to it)"""
    return coarse_run("fp32", style, app, S, R, tap_layer=tap, need_rgb=rgb, need_feat=True, want_sample_feat=True)


@functools.lru_cache(maxsize=None)
def _oracle_tap(S, R, tap):
    """CPU oracle: the coarse network on the coarse samples with the feature tapped on layer `tap` (the oracle's own functions, composed
    as its render_rays composes them)"""
    _, sd, _ = styled_network(None, False)
    rays, _, _, t = oracle_bundle(S, R)
    o, d, view, radii = rays[:, :3], rays[:, 3:6], rays[:, 8:11], rays[:, 11:12]
    mean, var = no.frustum_gaussians(t, o, d, radii)
    x_pts = no.ipe(mean.reshape(-1, 3), var.reshape(-1, 3), 15)
    x_dir = no.dir_pe(view[:, None, :].expand(R, S, 3).reshape(-1, 3), 4)
    raw, feats = no.nerf_mlp(sd, "nerf_coarse", x_pts, x_dir, None, stop_layer=tap)
    raw, feats = raw.reshape(R, S, 4), feats.reshape(R, S, -1)
    rgb, depth, acc, w = no.composite(raw, t, d, False)
    return dict(weights=w, feat=(w[..., None] * feats).sum(-2), pts=(w[..., None] * mean).sum(-2), rgb=rgb, depth=depth, acc=acc, sample_feat=feats)


@pytest.mark.parametrize("S,R", SHAPES)
@pytest.mark.parametrize("rgb", [True, False])
@pytest.mark.parametrize("tap", range(8))
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_every_tap_layer(gpu, built_lib, precision, tap, rgb, S, R):
    """sample_feat reads back every workspace row of the tapped layer"""
    out = coarse_run(precision, None, False, S, R, tap_layer=tap, need_rgb=rgb, need_feat=True, want_sample_feat=True)
    ref = _fp32(None, False, S, R, tap, rgb)
    assert out["weights"].shape == (R, S) and out["sample_feat"].shape == (R, S, 256) and (out["rgb"] is None) == (not rgb)
    assert float(ref["weights"].sum(-1).max()) > 0.3  # not vacuous
    tol = tol_for(precision, "default")
    compare(out, ref, tol, False, f"{precision} tap {tap} rgb {rgb} S {S} R {R} vs fp32 kernel", _keys(rgb))
    if tap == 3:
        compare(out, _oracle_tap(S, R, 3), tol, False, f"{precision} tap 3 rgb {rgb} S {S} R {R} vs oracle", _keys(rgb))


def test_trained_like_weights(gpu, built_lib):
    """style="surface": activations up to ~18, densities of +-1e4 -- the fp16x3 blob carries non-trivial scales, the density vector among them"""
    S, R = 64, 3
    out = coarse_run("fp16x3", "surface", False, S, R, tap_layer=3, need_rgb=True, need_feat=True, want_sample_feat=True)
    ref = _fp32("surface", False, S, R, 3, True)
    assert float(ref["weights"].sum(-1).max()) > 0.3
    compare(out, ref, TOL, False, "surface tap 3 vs fp32 kernel", SFEAT)


def test_appearance_row(gpu, built_lib):
    """Cambridge-style state dict: the views layer has its third extra K-step (appearance row) behind the slot that ends the density sum"""
    S, R = 64, 3
    out = coarse_run("fp16x3", None, True, S, R, tap_layer=3, need_rgb=True, need_feat=True, want_sample_feat=True)
    compare(out, _fp32(None, True, S, R, 3, True), TOL, False, "appearance row tap 3 vs fp32 kernel", SFEAT)


@pytest.mark.parametrize("S,R", SHAPES)
def test_density_does_not_depend_on_the_colour_heads(gpu, built_lib, S, R):
    """With colour heads the density head is summed inside the views K-loop, without them by alpha_head behind layer 7: the same terms in
    the same order, so the raw density and the weights agree bit for bit.  (Before the in-loop sum both launches ran alpha_head, the
    same inlined expressions with contraction off: the equality held there by construction.)"""
    kw = dict(tap_layer=3, need_feat=True, want_raw=True)
    with_heads = coarse_run("fp16x3", None, False, S, R, need_rgb=True, **kw)
    without = coarse_run("fp16x3", None, False, S, R, need_rgb=False, **kw)
    assert float(without["weights"].sum(-1).max()) > 0.3
    assert torch.equal(with_heads["raw"][..., 3], without["raw"][..., 3])
    assert torch.equal(with_heads["weights"], without["weights"])


@pytest.mark.parametrize("S,R", [(64, 3), (128, 2)])
def test_leftover_pass(gpu, built_lib, S, R):
    """A fine-style row (ops.resample: the fence posts past S/2 coincide) with zero_tail and its device flag: the regular tiles evaluate
    S/2 samples per ray and a leftover pass the one that remains, through the same K-loops; every output against the same launch with
    every sample evaluated."""
    ren = styled_network(None, False)[0]
    rays, _, jit, t_c = oracle_bundle(S, R)
    w_c = launch(ren, "coarse", "fp16x3", rays, t_c, tap_layer=-1, need_rgb=False, need_feat=False)["weights"]
    t_f, flag = ops.resample(t_c.to(w_c.device), w_c, jit.to(w_c.device), want_tail_flag=True)
    assert int(flag.item()) == 0  # the premise holds: the zero-tail path is taken
    kw = dict(tap_layer=3, need_rgb=True, need_feat=True)
    full = launch(ren, "coarse", "fp16x3", rays, t_f, zero_tail=False, **kw)
    lean = launch(ren, "coarse", "fp16x3", rays, t_f, zero_tail=True, tail_flag=flag, **kw)
    assert float(full["weights"].sum(-1).max()) > 0.3
    compare(lean, full, TOL, False, f"zero tail S {S} R {R} vs every sample")
