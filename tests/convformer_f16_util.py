"""float64 emulation of the ConvFormer backbone's fp16 inference walk, on the CPU, working straight from a state dict.
It shares no code with the module under test; it restates the walk's arithmetic:

    * the residual stream, LayerNorm statistics, every sum, biases, norm weights, StarReLU's scalars, the depthwise weights: exact here
      (float64 stands in for the kernels' fp32);
    * rounded by `rop` (operands): every GEMM's weight matrix, the image values gathered into the stem's patch rows, every LayerNorm
      output that feeds a GEMM;
    * rounded by `rst` (storage): pwconv1's output, the depthwise convolution's output, StarReLU(fc1 . ...) -- the activation on the
      unrounded sum, then ONE rounding;
    * pwconv2, fc2, the stem and the downsample convolution write the stream unrounded; the stem's norm makes the stream and is not rounded.

The two roundings are parameters, so that one code gives the three variants the tests compare:
    fp16       rop = rst = to_f16      the walk
    TF32-like  rop = to_f16, rst = id  an 11-bit significand on GEMM operands only: what torch's default `cudnn.allow_tf32 = True` gives the
                                       reference's convolutions on its own hardware
    bf16       rop = rst = to_bf16
to_f16 is torch's conversion: round to nearest even, overflow to infinity, no saturation."""
import torch
import torch.nn.functional as F

import convformer_util as cu


def to_f16(x):
    return x.to(torch.float16).to(torch.float64)


def to_bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def ident(x):
    return x


VARIANTS = {"fp16": (to_f16, to_f16), "tf32": (to_f16, ident), "bf16": (to_bf16, to_bf16)}


def _ln(x, w):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + cu.EPS) * w.view(1, -1, 1, 1)


def _star(x, sd, name):
    return sd[f"{name}.scale"] * torch.clamp(x, min=0) ** 2 + sd[f"{name}.bias"]


def _block(x, sd, b, rop, rst):
    t = rst(F.conv2d(rop(_ln(x, sd[f"{b}.norm1.weight"])), rop(sd[f"{b}.token_mixer.pwconv1.weight"])))
    t = _star(t, sd, f"{b}.token_mixer.act1")  # (applied to the stored value on its way into the depthwise sums, unrounded)
    t = rst(F.conv2d(t, sd[f"{b}.token_mixer.dwconv.weight"], padding=3, groups=t.shape[1]))
    x = x + F.conv2d(rop(t), rop(sd[f"{b}.token_mixer.pwconv2.weight"]))  # (rop of a stored value: the identity in the walk itself)
    t = F.conv2d(rop(_ln(x, sd[f"{b}.norm2.weight"])), rop(sd[f"{b}.mlp.fc1.weight"]))
    t = rst(_star(t, sd, f"{b}.mlp.act"))
    return x + F.conv2d(rop(t), rop(sd[f"{b}.mlp.fc2.weight"]))


def emulate(state, img, stem_stride, stem_pad, down_stride, rop=to_f16, rst=to_f16):
    """(stage-0 map, stage-1 map) in float64 under the roundings (rop, rst), from fp32 weights (keys without prefix) and an fp32 image."""
    sd = {k: v.detach().cpu().double() for k, v in state.items()}
    x = F.conv2d(rop(img.detach().cpu().double()), rop(sd["stem.conv.weight"]), sd["stem.conv.bias"], stride=stem_stride, padding=stem_pad)
    x = _ln(x, sd["stem.norm.weight"])
    for i in range(cu.DEPTHS[0]):
        x = _block(x, sd, f"stages_0.blocks.{i}", rop, rst)
    f = x
    x = F.conv2d(rop(_ln(x, sd["stages_1.downsample.norm.weight"])), rop(sd["stages_1.downsample.conv.weight"]),
                 sd["stages_1.downsample.conv.bias"], stride=down_stride, padding=1)
    for i in range(cu.DEPTHS[1]):
        x = _block(x, sd, f"stages_1.blocks.{i}", rop, rst)
    return f, x


def rel_rms(got, ref):
    """|got - ref|_2 / |ref|_2"""
    return float((got.detach().cpu().double() - ref).norm() / ref.norm())


_EMUL = {}


def emulated(kind, shape, seed=0, variant="fp16"):
    """emulate() on cu.case(kind, shape, seed), computed once per (case, variant) and shared by the tests that need it."""
    key = (kind, tuple(shape), seed, variant)
    if key not in _EMUL:
        state, img, _, _ = cu.case(kind, shape, seed)
        _EMUL[key] = emulate(state, img, **(cu.MS if kind == "c2f" else cu.MINI), rop=VARIANTS[variant][0], rst=VARIANTS[variant][1])
    return _EMUL[key]
