"""The sample math the NeRF kernels share (csrc/nerf_sample.h) gives the SAME BITS in the fp32-MFMA render kernel and the split ones.

A NeRF whose weight matrices are all zero and whose biases are not: every layer's output is its bias, the raw density is the density
head's bias (1.5) in every arithmetic -- the fp16x3 kernel pre-scales by powers of two only, which is exact -- so the `weights` output
depends on nothing but the fence posts, |d| and the compositing (alpha, transmittance factor, the segmented scan, the cross-wavefront
factor and the carry between 128-sample chunks): exactly the code the kernels inline from the one header.  torch.equal between
nm_nerf_fwd, nm_nerf_fwd_bf16x3 and nm_nerf_fwd_fp16x3, with R = 5 rays (the last tile is ragged) at every row length at which the scan
takes another form.  Two passes each: colour heads + tap 7 (the split kernels form the weights in front of the views layer) and neither
colour heads nor feature (they form them in the epilogue).  Stratified fence posts from a fixed seed; no zero-tail skip.

What this does NOT test: the scan's correctness.  All three kernels inline the same helpers, so an error in the header shows in all of
them alike and they still agree; this file catches a call site that drifts from the others (a re-typed formula, another barrier
placement, another carry).  The values themselves are pinned by the oracle comparisons of tests/test_nerf_gpu.py."""
import functools

import pytest
import torch

from nerf_kernel_util import camera_rays, fence_posts, launch, renderer_for
from nerfmatch_amd import synth

pytestmark = pytest.mark.gpu
R = 5
PASSES = (dict(tap_layer=7, need_rgb=True, need_feat=True), dict(tap_layer=-1, need_rgb=False, need_feat=False))


@functools.lru_cache(maxsize=None)
def _bias_only_nerf():
    sd = synth.nerf_state_dict(seed=11)
    for k in sd:
        if k.startswith("nerf_") and k.endswith(".weight"):
            sd[k] = torch.zeros_like(sd[k])
        if k.endswith("alpha_linear.bias"):
            sd[k] = torch.full_like(sd[k], 1.5)
    rays = camera_rays(2)
    return renderer_for("7scenes", sd, calibrate=False), rays[:: rays.shape[0] // R][:R].contiguous()  # five rays spread over the image


@pytest.mark.parametrize("S", [32,    # four rays per tile, 32-lane segments
                               64,    # whole-wavefront segments
                               128,   # the cross-wavefront factor
                               256])  # two chunks: the carried transmittance
def test_compositing_weights_bit_equal_across_kernels(S):
    ren, rays = _bias_only_nerf()
    t = fence_posts(rays, S, 300 + S)
    for kw in PASSES:
        w = {p: launch(ren, "coarse", p, rays, t, **kw)["weights"] for p in ("fp32", "bf16x3", "fp16x3")}  # (launch: the fp16x3 guard did not fire)
        acc = w["fp32"].sum(1)
        print(f"S={S} {kw}: weights in [{w['fp32'].min().item():.3e}, {w['fp32'].max().item():.3e}], per-ray sums {acc.tolist()}")
        assert (w["fp32"] > 0).float().mean() > 0.9 and (acc > 0.05).all() and (acc < 1.0).all()  # (not vacuous: real transmittances)
        for p in ("bf16x3", "fp16x3"):
            diff = (w[p] != w["fp32"]).sum().item()
            assert torch.equal(w[p], w["fp32"]), (p, S, kw, f"{diff} of {w[p].numel()} weights differ")
