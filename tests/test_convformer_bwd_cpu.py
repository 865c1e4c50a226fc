"""CPU: the float64 gradient restatement of the ConvFormer backward tests against torch autograd of the plain-torch module, and the
argument validation of the backward entry points."""
import ctypes as C

import pytest
import torch

import convformer_bwd_util as bu
import convformer_util as cu
from nerfmatch_amd import _lib
from nerfmatch_amd.modules.convformer import ConvFormerStages


@pytest.mark.parametrize("kind,shape", [("c2f", (2, 3, 26, 38)), ("coarse", (1, 3, 32, 40))])
def test_restatement_matches_autograd_of_the_torch_module(kind, shape):
    state, img, cots, ref = bu.case(kind, shape)
    m = ConvFormerStages(**cu.MS, out_stages=(0, 1)) if kind == "c2f" else ConvFormerStages(**cu.MINI, out_stages=(1,))
    m.load_state_dict(state, strict=True)
    m.double()
    with torch.enable_grad():
        maps = m._forward_torch(img.double())
        sum((o * c.double()).sum() for o, c in zip(maps, cots)).backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert set(grads) == set(ref) == set(cu.expected_shapes())
    assert all(g is not None for g in grads.values())
    errs = bu.grad_errors(grads, ref)
    worst = max(errs, key=errs.get)
    print(f"{kind} {shape}: worst {worst} {errs[worst]:.2e}")
    assert errs[worst] <= 1e-12  # two float64 evaluations of one formula: a few thousand roundings of 1.1e-16
    for k, (g, scale) in ref.items():
        assert (scale is None) == (not k.endswith((".scale", ".bias")) or "act" not in k)
        if scale is not None:
            assert scale >= float(g.abs()) > 0


def test_stage0_only_reference_leaves_stage1_out():
    state, img, _, _ = bu.case("c2f", (2, 3, 26, 38))
    cot = bu.cotangents([cu.case("c2f", (2, 3, 26, 38))[2].shape])[0]
    ref = bu.reference_grads(state, img, cu.MS, cot, None)
    assert ref and not [k for k in ref if k.startswith("stages_1.")]


def test_argument_validation_without_gpu(built_lib):
    """Bad arguments are refused before anything is enqueued, so no device is needed."""
    h = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_char * 512)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    q, r, s = (C.c_void_p(p.value + o) for o in (64, 128, 192))
    off = C.c_void_p(p.value + 4)
    ARG, UNSUP, WS = 1, _lib.NM_ERR_UNSUPPORTED, 4  # (NM_ERR_ARG, NM_ERR_UNSUPPORTED, NM_ERR_WORKSPACE)
    big = 1 << 20
    # nm_dwconv7_nhwc_bwd_input(dy, w49c, x, act_scale, B, H, W, C, dx, dscale_dbias, workspace, workspace_bytes, stream)
    f = h.nm_dwconv7_nhwc_bwd_input
    assert f(null, q, null, null, 1, 4, 4, 64, r, null, null, 0, null) == ARG
    assert f(p, null, null, null, 1, 4, 4, 64, r, null, null, 0, null) == ARG
    assert f(p, q, null, null, 1, 4, 4, 64, null, null, null, 0, null) == ARG
    assert f(p, q, s, null, 1, 4, 4, 64, r, null, null, 0, null) == ARG      # x without the scale
    assert f(p, q, null, s, 1, 4, 4, 64, r, null, null, 0, null) == ARG      # the scale without x
    assert f(p, q, null, null, 1, 4, 4, 64, r, s, s, big, null) == ARG       # scalar sums without the activation
    assert f(p, q, null, null, 1, 4, 4, 64, p, null, null, 0, null) == ARG   # in place on dy
    assert f(p, q, r, s, 1, 4, 4, 64, r, null, null, 0, null) == ARG         # in place on x
    assert f(off, q, null, null, 1, 4, 4, 64, r, null, null, 0, null) == ARG
    assert f(p, q, null, null, 1, 4, 4, 64, off, null, null, 0, null) == ARG
    assert f(p, q, off, s, 1, 4, 4, 64, r, null, null, 0, null) == ARG
    assert f(p, q, null, null, 1, 0, 4, 64, r, null, null, 0, null) == ARG
    assert f(p, q, null, null, 1, 4, 4, 96, r, null, null, 0, null) == UNSUP
    assert f(p, q, null, null, 1, 8193, 4, 64, r, null, null, 0, null) == UNSUP
    assert f(p, q, s, s, 1, 4, 4, 64, r, s, null, 0, null) == WS
    assert f(p, q, s, s, 1, 4, 4, 64, r, s, s, h.nm_dwconv7_nhwc_bwd_input_workspace_bytes(1, 4, 4, 64) - 1, null) == WS
    assert h.nm_dwconv7_nhwc_bwd_input_workspace_bytes(2, 17, 33, 64) == 2 * (2 * 2 * 3 * 2) * 4
    assert h.nm_dwconv7_nhwc_bwd_input_workspace_bytes(1, 4, 4, 96) == 0
    # nm_dwconv7_nhwc_bwd_weight(dy, x, act_scale, act_bias, B, H, W, C, dw49c, workspace, workspace_bytes, stream)
    f = h.nm_dwconv7_nhwc_bwd_weight
    assert f(null, q, null, null, 1, 4, 4, 64, r, s, big, null) == ARG
    assert f(p, null, null, null, 1, 4, 4, 64, r, s, big, null) == ARG
    assert f(p, q, null, null, 1, 4, 4, 64, null, s, big, null) == ARG
    assert f(p, q, s, null, 1, 4, 4, 64, r, s, big, null) == ARG             # one activation pointer without the other
    assert f(p, q, null, null, 1, 4, 4, 64, p, s, big, null) == ARG          # in place
    assert f(p, q, null, null, 1, 4, 4, 64, q, s, big, null) == ARG
    assert f(off, q, null, null, 1, 4, 4, 64, r, s, big, null) == ARG
    assert f(p, off, null, null, 1, 4, 4, 64, r, s, big, null) == ARG
    assert f(p, q, null, null, 1, 4, 4, 64, off, s, big, null) == ARG
    assert f(p, q, null, null, 1, 4, 4, 64, r, off, big, null) == ARG
    assert f(p, q, null, null, 1, 4, 4, 96, r, s, big, null) == UNSUP
    assert f(p, q, null, null, 1, 4, 4, 1088, r, s, big, null) == UNSUP
    assert f(p, q, null, null, 1, 4, 4, 64, r, null, 0, null) == WS
    assert f(p, q, null, null, 1, 4, 4, 64, r, s, 49 * 64 * 4 - 1, null) == WS
    assert h.nm_dwconv7_nhwc_bwd_weight_workspace_bytes(2, 17, 33, 64) == 2 * 3 * 49 * 64 * 4
    # nm_star_relu_bwd(x, dy, scale, n, dx, dscale_dbias, workspace, workspace_bytes, stream)
    f = h.nm_star_relu_bwd
    assert f(null, q, s, 4, r, null, null, 0, null) == ARG
    assert f(p, null, s, 4, r, null, null, 0, null) == ARG
    assert f(p, q, null, 4, r, null, null, 0, null) == ARG
    assert f(p, q, s, 4, null, null, null, 0, null) == ARG
    assert f(p, q, s, 0, r, null, null, 0, null) == ARG
    assert f(p, q, s, 4, p, null, null, 0, null) == ARG                      # in place
    assert f(p, q, s, 4, q, null, null, 0, null) == ARG
    assert f(off, q, s, 4, r, null, null, 0, null) == ARG
    assert f(p, off, s, 4, r, null, null, 0, null) == ARG
    assert f(p, q, s, 4, off, null, null, 0, null) == ARG
    assert f(p, q, s, 4, r, s, null, 0, null) == WS
    assert f(p, q, s, 4, r, s, s, 7, null) == WS
    assert h.nm_star_relu_bwd_workspace_bytes(1) == 8 and h.nm_star_relu_bwd_workspace_bytes(0) == 0
    assert h.nm_star_relu_bwd_workspace_bytes((1 << 20) + 3) == 2 * 128 * 4
    # nm_conv_patches_bwd(drows, layout, B, C, H, W, k, stride, pad, ld, dx, stream)
    f = h.nm_conv_patches_bwd
    assert f(null, 1, 1, 128, 8, 8, 3, 2, 1, 1152, q, null) == ARG
    assert f(p, 1, 1, 128, 8, 8, 3, 2, 1, 1152, null, null) == ARG
    assert f(p, 1, 1, 128, 8, 8, 3, 2, 1, 1152, p, null) == ARG              # in place
    assert f(p, 2, 1, 128, 8, 8, 3, 2, 1, 1152, q, null) == ARG
    assert f(off, 1, 1, 128, 8, 8, 3, 2, 1, 1152, q, null) == ARG
    assert f(p, 1, 1, 128, 8, 8, 3, 2, 1, 1152, off, null) == ARG
    assert f(p, 1, 1, 128, 8, 8, 3, 2, 1, 1150, q, null) == ARG              # ld: no multiple of 8
    assert f(p, 1, 1, 128, 8, 8, 3, 2, 1, 1144, q, null) == ARG              # ld below k k C
    assert f(p, 1, 1, 128, 2, 2, 7, 1, 0, 6272, q, null) == ARG              # image smaller than the kernel
    assert f(p, 0, 1, 128, 8, 8, 3, 2, 1, 1152, q, null) == UNSUP            # not channel-last
    assert f(p, 0, 1, 3, 8, 8, 7, 2, 3, 152, q, null) == UNSUP
    assert f(p, 1, 1, 6, 8, 8, 3, 2, 1, 56, q, null) == UNSUP                # C % 4
    assert f(p, 1, 1, 128, 8, 8, 9, 2, 1, 10368, q, null) == UNSUP
