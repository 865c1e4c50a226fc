"""A tap on layer 7 in a pass with colour heads (the renderer's coarse pass: tap_layer=-1, need_rgb, need_feat) is composited by the
split kernels at the end of layer 7, straight from the registers that hold it: the compositing weights are formed in front of the
views layer and the epilogue reuses them (csrc/nerf_fwd_bf16.hip, tap7_early).  Every output of such a launch against two
independent yardsticks on the same inputs: the fp32-MFMA kernel (csrc/nerf_fwd.hip) and the CPU oracle's coarse pass.

Shapes: the row lengths at which the along-ray scan takes another form -- 32 (four rays per tile, one per wavefront), 64 (a ray across
two wavefronts), 128 (a ray across the tile), 256 (two chunks: carried transmittance, running feature, best weight across chunks), 96
(padded by ops.nerf_fwd to 128 with zero-width intervals) -- with ray counts that leave the last tile ragged.
Bars: the helper of tests/test_nerf_gpu.py and its 1e-4 of scale."""
import functools

import pytest
import torch

from nerfmatch_amd import ops, synth
from nerfmatch_amd.nerf.renderer import NerfRenderer
from oracle import nerf_oracle as no
from test_nerf_gpu import TOL, relerr, tol_for

pytestmark = pytest.mark.gpu
SHAPES = [(32, 5), (64, 3), (128, 2), (256, 2), (96, 2)]
KEYS = ("weights", "feat", "pts", "rgb", "depth", "acc")


@functools.lru_cache(maxsize=None)
def _network(style, app):
    """(renderer on the GPU with calibrated fp16x3 scales, state dict, appearance row) -- one per weight style, shared by all cases"""
    dev = torch.device("cuda:0")
    cfg = synth.nerf_config("cambridge" if app else "7scenes", num_pts=64)
    ren = NerfRenderer(cfg, num_frames=5 if app else None, training=False, stop_layer=3)
    sd = synth.nerf_state_dict(seed=0 if style else 7, app_vocab=5 if app else 0, density_bias=0.0 if style else 3.0, style=style)
    ren.load_state_dict(sd, strict=True)
    ren.to(dev).eval()
    ren.calibrate(dev)  # fp16x3 operand scales from the seeded probe bundle: the tap's descale is not 1
    return ren, sd, (sd["embedding_a.weight"][1].contiguous() if app else None)


@functools.lru_cache(maxsize=None)
def _inputs(S, R, style=None):
    # (the "surface" weights with the camera of their golden fixture, tests/golden/make_golden.py: every ray meets the surface)
    H, W, f, pose = (128, 256, 240.0, 11) if style else (128, 128, 100.0, 3)
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    rays = no.make_rays(H, W, K, synth.camera_pose(pose), ds=8)[:R].contiguous()
    t_rand, jit = synth.uniform01((R, S + 1), 100 + S), synth.resample_jitter((R, S + 1), 200 + S)
    return rays, t_rand, jit, no.sample_coarse(rays, S, t_rand)


@functools.lru_cache(maxsize=None)
def _oracle(style, app, S, R, feat_max, white_bg):
    _, sd, row = _network(style, app)
    rays, t_rand, jit, _ = _inputs(S, R, style)
    o = no.render_rays(sd, rays, t_rand, jit, S, S, stop_layer=3, white_bg=white_bg, app_row=row, feat_comb="max" if feat_max else "lin",
                       keep_raw=True)
    ref = {k: o[f"{k}_coarse"] for k in KEYS}
    ref["raw"], ref["sample_feat"] = o["raw_coarse"], o["sfeat_coarse"]
    return ref


def _run(precision, style, app, S, R, **kw):
    ren, _, row = _network(style, app)
    dev = torch.device("cuda:0")
    rays, _, _, t = _inputs(S, R, style)
    blob = ren.nerf_coarse.packed(dev, precision)
    with torch.no_grad():
        out = ops.nerf_fwd(blob, rays.to(dev), t.to(dev), None if row is None else row.to(dev), **kw)
    if precision == "fp16x3":  # the guarded fp32 pass must not have rewritten what this file is about
        assert not blob.nm_guard.read()[0], "an fp16x3 operand saturated: the outputs are the fp32 kernel's"
    return out


def _clear_winner(weights):
    """feat_comb max selects by an argmax over weights that agree to ~1e-6 between arithmetics: rays whose two best weights are further
    apart than 1e-4 (tests/test_nerf_paths_gpu.py)"""
    top2 = torch.as_tensor(weights).float().cpu().topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > 1e-4


def _compare(out, ref, tol, feat_max, what, keys=KEYS):
    clear = _clear_winner(ref["weights"]) if feat_max else None
    if feat_max:
        assert bool(clear.any()), f"{what}: no ray with a clear maximum-weight sample"
    for k in keys:
        a, b = out[k].detach().cpu().float(), torch.as_tensor(ref[k]).detach().cpu().float()
        a, b = a.reshape(b.shape[0], -1), b.reshape(b.shape[0], -1)
        if feat_max and k in ("feat", "pts"):
            a, b = a[clear], b[clear]
        err = relerr(a, b)
        print(f"{what} {k}: {err:.2e} of scale")
        assert err < tol, f"{what} {k}: {err:.2e}"


@pytest.mark.parametrize("white_bg", [False, True])
@pytest.mark.parametrize("feat_max", [False, True])
@pytest.mark.parametrize("S,R", SHAPES)
def test_coarse_pass_vs_fp32_kernel_and_oracle(gpu, built_lib, S, R, feat_max, white_bg):
    kw = dict(tap_layer=-1, white_bg=white_bg, need_rgb=True, need_feat=True, feat_max=feat_max)
    out = _run("fp16x3", None, False, S, R, **kw)
    ref32 = _run("fp32", None, False, S, R, **kw)
    assert out["weights"].shape == (R, S) and out["feat"].shape == (R, 256)
    assert float(ref32["weights"].sum(-1).max()) > 0.3  # not vacuous
    _compare(out, ref32, TOL, feat_max, f"S {S} R {R} vs fp32 kernel")
    _compare(out, _oracle(None, False, S, R, feat_max, white_bg), TOL, feat_max, f"S {S} R {R} vs oracle")
    # tap_layer=7 names the same layer: the same path, the same bits
    out7 = _run("fp16x3", None, False, S, R, **dict(kw, tap_layer=7))
    for k in KEYS:
        assert torch.equal(out[k], out7[k]), k


@pytest.mark.parametrize("feat_max", [False, True])
@pytest.mark.parametrize("S,R", [(64, 3), (256, 2)])
def test_trained_like_weights(gpu, built_lib, S, R, feat_max):
    """style="surface": activations up to ~18, densities of +-1e4 -- the fp16x3 blob carries non-trivial scales (OFF_SCALE / OFF_DESCALE)"""
    kw = dict(tap_layer=-1, need_rgb=True, need_feat=True, feat_max=feat_max)
    out = _run("fp16x3", "surface", False, S, R, **kw)
    assert float(_oracle("surface", False, S, R, feat_max, False)["weights"].sum(-1).max()) > 0.3  # not vacuous
    _compare(out, _run("fp32", "surface", False, S, R, **kw), TOL, feat_max, f"surface S {S} vs fp32 kernel")
    _compare(out, _oracle("surface", False, S, R, feat_max, False), TOL, feat_max, f"surface S {S} vs oracle")


def test_bf16_split(gpu, built_lib):
    S, R = 64, 3
    kw = dict(tap_layer=7, need_rgb=True, need_feat=True)
    out = _run("bf16x3", None, False, S, R, **kw)
    tol = tol_for("bf16x3", "default")
    _compare(out, _run("fp32", None, False, S, R, **kw), tol, False, "bf16x3 vs fp32 kernel")
    _compare(out, _oracle(None, False, S, R, False, False), tol, False, "bf16x3 vs oracle")


@pytest.mark.parametrize("S,R", [(32, 5), (256, 2)])
def test_appearance_row(gpu, built_lib, S, R):
    """Cambridge-style state dict: appearance embedding row in the views layer, white background"""
    kw = dict(tap_layer=-1, white_bg=True, need_rgb=True, need_feat=True)
    out = _run("fp16x3", None, True, S, R, **kw)
    _compare(out, _run("fp32", None, True, S, R, **kw), TOL, False, f"app S {S} vs fp32 kernel")
    _compare(out, _oracle(None, True, S, R, False, True), TOL, False, f"app S {S} vs oracle")


def test_sample_feat_keeps_the_workspace_path(gpu, built_lib):
    """want_sample_feat (a debug output) with tap 7 and colour heads: the per-sample rows still go through the workspace; the composited
    feature must be the one the early path gives, bit for bit (same products, same reduction)"""
    S, R = 64, 3
    kw = dict(tap_layer=-1, need_rgb=True, need_feat=True, want_raw=True, want_sample_feat=True)
    out = _run("fp16x3", None, False, S, R, **kw)
    keys = KEYS + ("raw", "sample_feat")
    _compare(out, _run("fp32", None, False, S, R, **kw), TOL, False, "sample_feat vs fp32 kernel", keys)
    _compare(out, _oracle(None, False, S, R, False, False), TOL, False, "sample_feat vs oracle", keys)
    early = _run("fp16x3", None, False, S, R, tap_layer=-1, need_rgb=True, need_feat=True)
    for k in KEYS:
        assert torch.equal(out[k], early[k]), k


def test_without_colour_heads(gpu, built_lib):
    """need_rgb=False with tap 7: no views layer behind layer 7, the workspace path as before"""
    S, R = 64, 3
    kw = dict(tap_layer=7, need_rgb=False, need_feat=True)
    out = _run("fp16x3", None, False, S, R, **kw)
    assert out["rgb"] is None
    keys = tuple(k for k in KEYS if k != "rgb")
    _compare(out, _run("fp32", None, False, S, R, **kw), TOL, False, "no rgb vs fp32 kernel", keys)
    _compare(out, _oracle(None, False, S, R, False, False), TOL, False, "no rgb vs oracle", keys)
    # the weights and the feature do not depend on the colour heads: the early path gives the same bits
    early = _run("fp16x3", None, False, S, R, tap_layer=7, need_rgb=True, need_feat=True)
    for k in ("weights", "feat", "pts", "depth", "acc"):
        assert torch.equal(out[k], early[k]), k
