"""float64 restatement of the ConvFormer stem and stages 0-1 (the architecture table of nerfmatch_amd/modules/convformer.py) with
torch.nn.functional on the CPU, working straight from a state dict: the reference of the backbone tests.  It shares no code with the
module under test.  TOL is the project's bar (tests/test_nerf_gpu.py: 1e-4 of the tensor's scale max(1, max|reference|))."""
import torch
import torch.nn.functional as F

from nerfmatch_amd import synth

TOL = 1e-4
EPS = 1e-6
DEPTHS = (3, 12)
MS = dict(stem_stride=2, stem_pad=3, down_stride=4)    # the multi-scale model's patched strides
MINI = dict(stem_stride=4, stem_pad=2, down_stride=2)  # timm's own


def _ln(x, w):
    """weight-only LayerNorm over the channels of an NCHW map"""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w.view(1, -1, 1, 1)


def _star(x, sd, name):
    return sd[f"{name}.scale"] * torch.clamp(x, min=0) ** 2 + sd[f"{name}.bias"]


def _block(x, sd, b):
    t = F.conv2d(_ln(x, sd[f"{b}.norm1.weight"]), sd[f"{b}.token_mixer.pwconv1.weight"])
    t = _star(t, sd, f"{b}.token_mixer.act1")
    t = F.conv2d(t, sd[f"{b}.token_mixer.dwconv.weight"], padding=3, groups=t.shape[1])
    x = x + F.conv2d(t, sd[f"{b}.token_mixer.pwconv2.weight"])
    t = F.conv2d(_ln(x, sd[f"{b}.norm2.weight"]), sd[f"{b}.mlp.fc1.weight"])
    return x + F.conv2d(_star(t, sd, f"{b}.mlp.act"), sd[f"{b}.mlp.fc2.weight"])


def reference_maps(state, img, stem_stride, stem_pad, down_stride):
    """(stage-0 map, stage-1 map) in float64 from fp32 weights (keys without prefix) and an fp32 image, all on the CPU."""
    sd = {k: v.detach().cpu().double() for k, v in state.items()}
    x = F.conv2d(img.detach().cpu().double(), sd["stem.conv.weight"], sd["stem.conv.bias"], stride=stem_stride, padding=stem_pad)
    x = _ln(x, sd["stem.norm.weight"])
    for i in range(DEPTHS[0]):
        x = _block(x, sd, f"stages_0.blocks.{i}")
    f = x
    x = F.conv2d(_ln(x, sd["stages_1.downsample.norm.weight"]), sd["stages_1.downsample.conv.weight"], sd["stages_1.downsample.conv.bias"],
                 stride=down_stride, padding=1)
    for i in range(DEPTHS[1]):
        x = _block(x, sd, f"stages_1.blocks.{i}")
    return f, x


def expected_shapes():
    """name -> shape of every tensor of the parameter tree (no prefix)."""
    out = {"stem.conv.weight": (128, 3, 7, 7), "stem.conv.bias": (128,), "stem.norm.weight": (128,),
           "stages_1.downsample.norm.weight": (128,), "stages_1.downsample.conv.weight": (256, 128, 3, 3),
           "stages_1.downsample.conv.bias": (256,)}
    for s, (d, depth) in enumerate(zip((128, 256), DEPTHS)):
        for i in range(depth):
            b = f"stages_{s}.blocks.{i}"
            out.update({f"{b}.norm1.weight": (d,), f"{b}.norm2.weight": (d,),
                        f"{b}.token_mixer.pwconv1.weight": (2 * d, d, 1, 1), f"{b}.token_mixer.act1.scale": (1,),
                        f"{b}.token_mixer.act1.bias": (1,), f"{b}.token_mixer.dwconv.weight": (2 * d, 1, 7, 7),
                        f"{b}.token_mixer.pwconv2.weight": (d, 2 * d, 1, 1), f"{b}.mlp.fc1.weight": (4 * d, d, 1, 1),
                        f"{b}.mlp.act.scale": (1,), f"{b}.mlp.act.bias": (1,), f"{b}.mlp.fc2.weight": (d, 4 * d, 1, 1)})
    return out


def image(shape, seed=11):
    """A normalised-image-like input: N(0, 1) from torch's CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32)


_CASES = {}


def case(kind, shape, seed=0):
    """(state without prefix, img, float64 stage-0 map, float64 stage-1 map), computed once per (kind, shape, seed) and shared by the
    tests that need it; kind "c2f" = the multi-scale strides, "coarse" = the Mini model's."""
    key = (kind, tuple(shape), seed)
    if key not in _CASES:
        state = synth.backbone_state_dict(seed, "coarse")
        img = image(shape)
        f, c = reference_maps(state, img, **(MS if kind == "c2f" else MINI))
        _CASES[key] = (state, img, f, c)
    return _CASES[key]


def scaled_err(got, ref):
    """max |got - ref| / max(1, max|ref|)"""
    return float((got.detach().cpu().double() - ref).abs().max() / max(1.0, float(ref.abs().max())))
