"""CPU: the arithmetic of the backbone's fp16 inference walk, measured on its float64 emulation (tests/convformer_f16_util.py), and the
switch that selects the walk -- validation, default, and the way from the matcher's config to the module."""
import ctypes as C

import pytest
import torch

import convformer_f16_util as fu
import convformer_util as cu
from nerfmatch_amd import _lib, synth
from nerfmatch_amd.matcher import NeRFMatcherCoarse, NeRFMatcherMS
from nerfmatch_amd.modules import init_backbone, init_backbone_8_2
from nerfmatch_amd.modules.convformer import ConvFormerMS, ConvFormerStages

CASES = [("c2f", (1, 3, 64, 64), 0), ("c2f", (2, 3, 40, 56), 1)]


@pytest.mark.parametrize("kind,shape,seed", CASES)
def test_fp16_costs_little_more_than_tf32_and_far_less_than_bf16(kind, shape, seed):
    """Why the 16-bit format of the walk is fp16.  Against the float64 maps, in relative rms error:
      * the fp16 walk (operands AND stored intermediates rounded) stays within 1.5 x of rounding the GEMM operands alone to fp16's 11-bit
        significand -- TF32's, i.e. the error the reference accepts on its own hardware (measured 1.16-1.24 x when the mode was proposed;
        1.5 is the project's margin over a recorded value);
      * bf16 in the same places costs more than 4 x the fp16 walk's error (measured 8 x)."""
    _, _, f_ref, c_ref = cu.case(kind, shape, seed)
    err = {}
    for variant in ("fp16", "tf32", "bf16"):
        f, c = fu.emulated(kind, shape, seed, variant)
        err[variant] = (fu.rel_rms(f, f_ref), fu.rel_rms(c, c_ref))
        print(f"emulation {kind} {shape} seed {seed} {variant:>5}: rel. rms fine {err[variant][0]:.3e} coarse {err[variant][1]:.3e}; "
              f"max of scale fine {cu.scaled_err(f, f_ref):.3e} coarse {cu.scaled_err(c, c_ref):.3e}")
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(c).all())
    for i, name in enumerate(("fine", "coarse")):
        print(f"  {name}: fp16 / tf32 = {err['fp16'][i] / err['tf32'][i]:.3f}, bf16 / fp16 = {err['bf16'][i] / err['fp16'][i]:.2f}")
        assert err["fp16"][i] <= 1.5 * err["tf32"][i], name
        assert err["bf16"][i] > 4.0 * err["fp16"][i], name


def test_inference_precision_default_and_validation():
    m = ConvFormerStages(2, 3, 4, (0, 1))
    assert m.inference_precision == "same"
    m.inference_precision = "fp16"
    assert m.inference_precision == "fp16"
    for bad in ("bf16", "fp32", "FP16", None, 16):
        with pytest.raises(ValueError):
            m.inference_precision = bad
        with pytest.raises(ValueError):
            ConvFormerStages(2, 3, 4, (0, 1), bad)
    assert m.inference_precision == "fp16"  # (a refused value changes nothing)
    assert m.overflow_events() == 0        # nothing ran: nothing counted, and no device is touched
    assert "inference_precision" not in "".join(m.state_dict())  # the switch and its counter are no part of the checkpoint


def test_init_backbone_passes_the_precision_through():
    assert init_backbone_8_2("convformer").model.inference_precision == "same"
    assert init_backbone("convformer").inference_precision == "same"
    ms = init_backbone_8_2("convformer", precision="fp16")
    assert isinstance(ms, ConvFormerMS) and ms.model.inference_precision == "fp16"
    assert init_backbone("convformer384", downsample=8, precision="fp16").inference_precision == "fp16"
    for make in (init_backbone_8_2, init_backbone):
        with pytest.raises(ValueError):
            make("convformer", precision="bf16")
        with pytest.raises(ValueError):
            make("stub", precision="fp16")  # the stand-in has one arithmetic
        make("stub", precision="same")


@pytest.mark.parametrize("kind", ["c2f", "coarse"])
def test_matcher_config_selects_the_precision(kind):
    cls = NeRFMatcherMS if kind == "c2f" else NeRFMatcherCoarse
    stages = lambda m: m.backbone.model if kind == "c2f" else m.backbone
    assert stages(cls(synth.matcher_config(kind, backbone="convformer"))).inference_precision == "same"
    cfg = synth.matcher_config(kind, backbone="convformer")
    cfg.backbone_precision = "fp16"
    assert stages(cls(cfg)).inference_precision == "fp16"
    cfg.backbone_precision = "half"
    with pytest.raises(ValueError):
        cls(cfg)


def test_host_tensors_take_the_plain_torch_path_whatever_the_precision():
    state, img, _, _ = cu.case("c2f", (1, 3, 64, 64))
    outs = []
    for precision in ("same", "fp16"):
        m = init_backbone_8_2("convformer", precision=precision)
        m.model.load_state_dict(state, strict=True)
        outs.append(m.eval()(img[:, :, :32, :32]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_benchmark_flag():
    from nerfmatch_amd.benchmark_nerfmatch import build_parser

    p = build_parser()
    assert not hasattr(p.parse_args([]), "backbone_precision")  # not given: the checkpoint's own setting holds
    assert p.parse_args(["--backbone_precision", "fp16"]).backbone_precision == "fp16"
    with pytest.raises(SystemExit):
        p.parse_args(["--backbone_precision", "bf16"])


def test_argument_validation_without_gpu(built_lib):
    """Bad arguments are refused before anything is enqueued, so this is safe without a device."""
    h = _lib.lib()
    ARG, UNSUP = 1, _lib.NM_ERR_UNSUPPORTED
    null = C.c_void_p(0)
    buf = (C.c_char * 512)()
    base = (C.addressof(buf) + 15) & ~15
    p, q, off = C.c_void_p(base), C.c_void_p(base + 256), C.c_void_p(base + 8)
    assert h.nm_linear_blob_bytes_f16(128, 128) == 4 * 8192 and h.nm_linear_blob_bytes_f16(129, 152) == 2 * 5 * 8192
    assert h.nm_linear_blob_bytes_f16(0, 8) == 0
    # nm_linear_f16(x, blob, bias, star_scale, star_bias, residual, M, N, K, out_f16, y, overflow, stream)
    f = h.nm_linear_f16
    assert f(null, p, null, null, null, null, 4, 8, 8, 1, q, null, null) == ARG
    assert f(p, null, null, null, null, null, 4, 8, 8, 1, q, null, null) == ARG
    assert f(p, p, null, null, null, null, 4, 8, 8, 1, null, null, null) == ARG
    assert f(p, p, null, null, null, null, 0, 8, 8, 1, q, null, null) == ARG
    assert f(p, p, null, p, null, null, 4, 8, 8, 1, q, null, null) == ARG      # StarReLU: scale and bias, both or neither
    assert f(p, p, null, null, null, p, 4, 8, 8, 1, q, null, null) == ARG      # a residual needs fp32 output
    assert f(p, p, null, null, null, null, 4, 8, 8, 2, q, null, null) == ARG
    assert f(off, p, null, null, null, null, 4, 8, 8, 1, q, null, null) == ARG  # 16-byte pieces
    assert f(p, p, null, null, null, null, 4, 8, 12, 1, q, null, null) == UNSUP
    assert f(p, p, null, null, null, null, 4, 12, 8, 0, q, null, null) == UNSUP
    assert h.nm_linear_pack_f16(null, 8, 8, p, null) == ARG and h.nm_linear_pack_f16(p, 8, 0, p, null) == ARG
    # nm_layernorm_f16(x, gamma, beta, rows, dim, eps, y, overflow, stream)
    g = h.nm_layernorm_f16
    assert g(null, p, p, 4, 128, 1e-6, q, null, null) == ARG and g(p, p, p, 4, 128, 1e-6, null, null, null) == ARG
    assert g(p, p, p, 0, 128, 1e-6, q, null, null) == ARG
    assert g(p, p, p, 4, 64, 1e-6, q, null, null) == UNSUP and g(p, p, p, 4, 192, 1e-6, q, null, null) == UNSUP
    # nm_dwconv7_nhwc_f16(x, w49c, act_scale, act_bias, B, H, W, C, y, overflow, stream)
    d = h.nm_dwconv7_nhwc_f16
    assert d(null, p, null, null, 1, 4, 4, 64, q, null, null) == ARG and d(p, p, null, null, 1, 4, 4, 64, p, null, null) == ARG
    assert d(p, p, p, null, 1, 4, 4, 64, q, null, null) == ARG
    assert d(off, p, null, null, 1, 4, 4, 64, q, null, null) == ARG
    assert d(p, p, null, null, 1, 4, 4, 32, q, null, null) == UNSUP
    # nm_conv_patches_f16(x, layout, B, C, H, W, k, stride, pad, ld, rows, overflow, stream)
    c = h.nm_conv_patches_f16
    assert c(null, 0, 1, 3, 8, 8, 7, 2, 3, 152, q, null, null) == ARG and c(p, 2, 1, 3, 8, 8, 7, 2, 3, 152, q, null, null) == ARG
    assert c(p, 0, 1, 3, 8, 8, 7, 2, 3, 150, q, null, null) == ARG      # ld = 150: no multiple of 8
    assert c(p, 0, 1, 3, 8, 8, 7, 2, 3, 144, q, null, null) == ARG      # ld below k k C
    assert c(p, 1, 1, 128, 8, 8, 3, 2, 1, 1152, off, null, null) == ARG  # the rows are written in 16-byte words
    assert c(off, 1, 1, 128, 8, 8, 3, 2, 1, 1152, q, null, null) == ARG  # fp16 pixels are read in 16-byte words
    assert c(p, 1, 1, 12, 8, 8, 3, 2, 1, 112, q, null, null) == UNSUP    # channel-last fp16 input: C % 8
