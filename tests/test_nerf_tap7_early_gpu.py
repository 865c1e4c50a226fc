"""A tap on layer 7 in a pass with colour heads (the renderer's coarse pass: tap_layer=-1, need_rgb, need_feat) is composited by the
split kernels at the end of layer 7, straight from the registers that hold it: the compositing weights are formed in front of the
views layer and the epilogue reuses them (csrc/nerf_fwd_bf16.hip, tap7_early).  Every output of such a launch against two
independent yardsticks on the same inputs: the fp32-MFMA kernel (csrc/nerf_fwd.hip) and the CPU oracle's coarse pass.

Shapes: the row lengths at which the along-ray scan takes another form -- 32 (four rays per tile, one per wavefront), 64 (a ray across
two wavefronts), 128 (a ray across the tile), 256 (two chunks: carried transmittance, running feature, best weight across chunks), 96
(padded by ops.nerf_fwd to 128 with zero-width intervals) -- with ray counts that leave the last tile ragged.
Bars, networks, launches: tests/nerf_kernel_util.py (1e-4 of scale)."""
import functools

import pytest
import torch

from nerf_kernel_util import KEYS, SHAPES, TOL, coarse_run, compare, oracle_bundle, styled_network, tol_for
from oracle import nerf_oracle as no

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle(style, app, S, R, feat_max, white_bg):
    _, sd, row = styled_network(style, app)
    rays, t_rand, jit, _ = oracle_bundle(S, R, style)
    o = no.render_rays(sd, rays, t_rand, jit, S, S, stop_layer=3, white_bg=white_bg, app_row=None if row is None else row.cpu(),
                       feat_comb="max" if feat_max else "lin", keep_raw=True)
    ref = {k: o[f"{k}_coarse"] for k in KEYS}
    ref["raw"], ref["sample_feat"] = o["raw_coarse"], o["sfeat_coarse"]
    return ref


@pytest.mark.parametrize("white_bg", [False, True])
@pytest.mark.parametrize("feat_max", [False, True])
@pytest.mark.parametrize("S,R", SHAPES)
def test_coarse_pass_vs_fp32_kernel_and_oracle(gpu, built_lib, S, R, feat_max, white_bg):
    kw = dict(tap_layer=-1, white_bg=white_bg, need_rgb=True, need_feat=True, feat_max=feat_max)
    out = coarse_run("fp16x3", None, False, S, R, **kw)
    ref32 = coarse_run("fp32", None, False, S, R, **kw)
    assert out["weights"].shape == (R, S) and out["feat"].shape == (R, 256)
    assert float(ref32["weights"].sum(-1).max()) > 0.3  # not vacuous
    compare(out, ref32, TOL, feat_max, f"S {S} R {R} vs fp32 kernel")
    compare(out, _oracle(None, False, S, R, feat_max, white_bg), TOL, feat_max, f"S {S} R {R} vs oracle")
    # tap_layer=7 names the same layer: the same path, the same bits
    out7 = coarse_run("fp16x3", None, False, S, R, **dict(kw, tap_layer=7))
    for k in KEYS:
        assert torch.equal(out[k], out7[k]), k


@pytest.mark.parametrize("feat_max", [False, True])
@pytest.mark.parametrize("S,R", [(64, 3), (256, 2)])
def test_trained_like_weights(gpu, built_lib, S, R, feat_max):
    """style="surface": activations up to ~18, densities of +-1e4 -- the fp16x3 blob carries non-trivial scales (OFF_SCALE / OFF_DESCALE)"""
    kw = dict(tap_layer=-1, need_rgb=True, need_feat=True, feat_max=feat_max)
    out = coarse_run("fp16x3", "surface", False, S, R, **kw)
    assert float(_oracle("surface", False, S, R, feat_max, False)["weights"].sum(-1).max()) > 0.3  # not vacuous
    compare(out, coarse_run("fp32", "surface", False, S, R, **kw), TOL, feat_max, f"surface S {S} vs fp32 kernel")
    compare(out, _oracle("surface", False, S, R, feat_max, False), TOL, feat_max, f"surface S {S} vs oracle")


def test_bf16_split(gpu, built_lib):
    S, R = 64, 3
    kw = dict(tap_layer=7, need_rgb=True, need_feat=True)
    out = coarse_run("bf16x3", None, False, S, R, **kw)
    tol = tol_for("bf16x3", "default")
    compare(out, coarse_run("fp32", None, False, S, R, **kw), tol, False, "bf16x3 vs fp32 kernel")
    compare(out, _oracle(None, False, S, R, False, False), tol, False, "bf16x3 vs oracle")


@pytest.mark.parametrize("S,R", [(32, 5), (256, 2)])
def test_appearance_row(gpu, built_lib, S, R):
    """Cambridge-style state dict: appearance embedding row in the views layer, white background"""
    kw = dict(tap_layer=-1, white_bg=True, need_rgb=True, need_feat=True)
    out = coarse_run("fp16x3", None, True, S, R, **kw)
    compare(out, coarse_run("fp32", None, True, S, R, **kw), TOL, False, f"app S {S} vs fp32 kernel")
    compare(out, _oracle(None, True, S, R, False, True), TOL, False, f"app S {S} vs oracle")


def test_sample_feat_keeps_the_workspace_path(gpu, built_lib):
    """want_sample_feat (a debug output) with tap 7 and colour heads: the per-sample rows still go through the workspace; the composited
    feature must be the one the early path gives, bit for bit (same products, same reduction)"""
    S, R = 64, 3
    kw = dict(tap_layer=-1, need_rgb=True, need_feat=True, want_raw=True, want_sample_feat=True)
    out = coarse_run("fp16x3", None, False, S, R, **kw)
    keys = KEYS + ("raw", "sample_feat")
    compare(out, coarse_run("fp32", None, False, S, R, **kw), TOL, False, "sample_feat vs fp32 kernel", keys)
    compare(out, _oracle(None, False, S, R, False, False), TOL, False, "sample_feat vs oracle", keys)
    early = coarse_run("fp16x3", None, False, S, R, tap_layer=-1, need_rgb=True, need_feat=True)
    for k in KEYS:
        assert torch.equal(out[k], early[k]), k


def test_without_colour_heads(gpu, built_lib):
    """need_rgb=False with tap 7: no views layer behind layer 7, the workspace path as before"""
    S, R = 64, 3
    kw = dict(tap_layer=7, need_rgb=False, need_feat=True)
    out = coarse_run("fp16x3", None, False, S, R, **kw)
    assert out["rgb"] is None
    keys = tuple(k for k in KEYS if k != "rgb")
    compare(out, coarse_run("fp32", None, False, S, R, **kw), TOL, False, "no rgb vs fp32 kernel", keys)
    compare(out, _oracle(None, False, S, R, False, False), TOL, False, "no rgb vs oracle", keys)
    # the weights and the feature do not depend on the colour heads: the early path gives the same bits
    early = coarse_run("fp16x3", None, False, S, R, tap_layer=7, need_rgb=True, need_feat=True)
    for k in ("weights", "feat", "pts", "depth", "acc"):
        assert torch.equal(out[k], early[k]), k
