"""ConvFormer image backbone: the stem and stages 0-1 of timm's convformer_b36 / caformer_b36, inference on the HIP kernels.

The reference builds `timm.create_model(..., features_only=True, out_indices=[0, 1])` and patches three strides
(nerfmatch/modules/__init__.py:14-113).  In both model families these stages are MetaFormer blocks whose token mixer is a separable
convolution (CAFormer's attention lives in stages 2-3, which the reference never builds):

    stem            Conv2d(3 -> 128, k 7, bias) then LayerNorm over channels (weight only, eps 1e-6)
    stages_0        3 blocks at 128 channels                                          -> the fine map
    stages_1        downsample = LayerNorm(128) then Conv2d(128 -> 256, k 3, padding 1, bias); 12 blocks at 256 channels -> the coarse map
    block at d      x = x + pwconv2(dwconv7x7(StarReLU(pwconv1(LN(x)))))   pwconv1 d -> 2d, depthwise on 2d, pwconv2 2d -> d, no biases
                    x = x + fc2(StarReLU(fc1(LN(x))))                      fc1 d -> 4d, fc2 4d -> d, no biases
    StarReLU        scale * relu(x)**2 + bias with two learnable 1-element tensors

Parameter names are those of timm's flattened feature network (`stem.conv.weight`, `stages_1.blocks.3.token_mixer.dwconv.weight`, ...):
a reference checkpoint's `backbone.*` tensors load with strict=True.  timm itself is not a dependency and parity against timm's own
module is not pinned by a test; the architecture above is the specification.

Two arithmetics compute it, the first on two operation sets:
  * the kernel walk (`_forward_kernels`): channel-last rows through linear / layernorm and the four kernels of csrc/convformer.hip.
    Device tensors without autograd run it on `ops.*` (`_INFERENCE`), a chunk of images at a time.  Device tensors inside
    `autograd.training()` with a trainable parameter run the same walk on the Functions of nerfmatch_amd/autograd.py, whose backward
    is csrc/convformer_bwd.hip and the GEMM / LayerNorm backward kernels: the whole batch in one piece (the ordered
    parameter-gradient sums run over the batch), every block's intermediates kept.  With `inference_precision = "fp16"` (opt-in) inference
    runs the walk on a third set, `_fp16_ops`: fp16 GEMM operands and intermediates around an fp32 residual stream;
  * host tensors, an image that requires grad, torch's grad mode outside `autograd.training()`, or `train_native = False` -- the same
    architecture with torch.nn.functional (the behaviour without a GPU, and the yardstick of scripts/perf_backbone_train.py).
Parameters require grad by default, so a DIRECT call `backbone(img)` on the device under torch's default grad mode takes the plain-torch
path: wrap inference in `torch.no_grad()` (the matchers do the equivalent themselves: they record only inside autograd.training()).
"""
import warnings
from types import SimpleNamespace

import torch
from torch import nn
import torch.nn.functional as F

from .. import autograd as ag
from .. import ops

DIMS = (128, 256)
DEPTHS = (3, 12)
EPS = 1e-6
STEM_LD = 152        # 7 * 7 * 3 = 147 patch columns, padded to the GEMM's K granularity

# The operation sets of the kernel walk.  Recording: the module nerfmatch_amd.autograd itself.  Inference: ops.* under the same names
# and signatures, StarReLU in place and conv_patches returning its rows only.
_INFERENCE = SimpleNamespace(linear=ops.linear, layernorm=ops.layernorm, dwconv7_nhwc=ops.dwconv7_nhwc, conv_weight_rows=ops.conv_weight_rows,
                             star_relu=lambda x, scale, bias: ops.star_relu(x, scale, bias, inplace=True),
                             conv_patches=lambda *args: ops.conv_patches(*args)[0])
PRECISIONS = ("same", "fp16")


def _fp16_ops(events):
    """The third operation set: the fp16 inference walk (`inference_precision = "fp16"`) on the overflow counter `events`.
    The residual stream stays fp32 rows: the GEMMs that end a branch (a residual) or a convolution (a bias) write fp32, and so does the stem's
    norm, whose output IS the stream (`stream_norm`).  Every other GEMM, every other LayerNorm, the depthwise convolution and the patch
    gathers store fp16, and the channel MLP's StarReLU rides fc1's epilogue (`star`), so the set has no star_relu."""
    def linear(x, weight, bias=None, residual=None, star=None):
        wide = residual is not None or bias is not None
        return ops.linear_f16(x, weight, bias, residual, star, torch.float32 if wide else torch.float16, events)
    return SimpleNamespace(linear=linear, stream_norm=ops.layernorm, conv_weight_rows=ops.conv_weight_rows,
                           layernorm=lambda *args: ops.layernorm_f16(*args, events=events),
                           dwconv7_nhwc=lambda *args: ops.dwconv7_nhwc_f16(*args, events=events),
                           conv_patches=lambda *args: ops.conv_patches_f16(*args, events=events)[0])


class _Conv(nn.Module):
    """Holder of a convolution's parameters under timm's names (the arithmetic lives in ConvFormerStages)."""

    def __init__(self, cin, cout, k, bias, groups=1):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin // groups, k, k))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)


class _ChannelNorm(nn.Module):
    """LayerNorm over channels without a bias."""

    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))


class _StarReLU(nn.Module):
    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1))
        self.bias = nn.Parameter(torch.zeros(1))


class _SepConv(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.pwconv1 = _Conv(dim, 2 * dim, 1, False)
        self.act1 = _StarReLU()
        self.dwconv = _Conv(2 * dim, 2 * dim, 7, False, groups=2 * dim)
        self.pwconv2 = _Conv(2 * dim, dim, 1, False)


class _Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = _Conv(dim, 4 * dim, 1, False)
        self.act = _StarReLU()
        self.fc2 = _Conv(4 * dim, dim, 1, False)


class _Block(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm1 = _ChannelNorm(dim)
        self.token_mixer = _SepConv(dim)
        self.norm2 = _ChannelNorm(dim)
        self.mlp = _Mlp(dim)


class _Stem(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = _Conv(3, DIMS[0], 7, True)
        self.norm = _ChannelNorm(DIMS[0])


class _Downsample(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm = _ChannelNorm(DIMS[0])
        self.conv = _Conv(DIMS[0], DIMS[1], 3, True)


class _Stage(nn.Module):
    def __init__(self, dim, depth, downsample):
        super().__init__()
        if downsample:
            self.downsample = _Downsample()
        self.blocks = nn.ModuleList([_Block(dim) for _ in range(depth)])


def _star_relu(x, act):
    return act.scale * torch.relu(x) ** 2 + act.bias


def _channel_norm(x, norm):
    """LayerNorm over the channels of an NCHW map."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), norm.weight, None, EPS).permute(0, 3, 1, 2)


class ConvFormerStages(nn.Module):
    """forward(img (B,3,H,W) fp32) -> list of the maps of `out_stages` in that order, each NCHW: stage 0 (B,128,.,.), stage 1
    (B,256,.,.); sizes follow conv arithmetic floor((n + 2p - k) / s) + 1 at the stem (k 7) and the downsample (k 3, padding 1).
    No norm on the returned maps."""

    def __init__(self, stem_stride, stem_pad, down_stride, out_stages, inference_precision="same"):
        super().__init__()
        self.inference_precision = inference_precision
        self.stem_stride, self.stem_pad, self.down_stride = int(stem_stride), int(stem_pad), int(down_stride)
        self.out_stages = tuple(int(s) for s in out_stages)
        if not self.out_stages or any(s not in (0, 1) for s in self.out_stages):
            raise ValueError(f"out_stages {out_stages}: stages 0 and 1 exist")
        self.stem = _Stem()
        self.stages_0 = _Stage(DIMS[0], DEPTHS[0], False)
        self.stages_1 = _Stage(DIMS[1], DEPTHS[1], True)
        # Native path: images go through in chunks so that the widest intermediate -- fc1's output, 4 d floats per pixel of a stage -- stays
        # under this many bytes (one image per chunk at the least).  Results do not depend on it: every kernel's arithmetic is per row / pixel.
        self.chunk_bytes = 512 << 20
        # Training inside autograd.training() records through the HIP forward / backward kernels; False: through torch.nn.functional.
        self.train_native = True

    # ---- inference arithmetic -------------------------------------------------------------------------------------------------------
    @property
    def inference_precision(self):
        """"same": the inference walk on ops.linear's arithmetic (ops.LINEAR_PRECISION), fp32 rows throughout.  "fp16" (opt-in): the walk on
        the fp16 operation set -- fp16 GEMM operands and intermediates, fp32 residual stream, statistics and accumulation.
        Device tensors outside autograd only: recording inside autograd.training() and the plain-torch path ignore it."""
        return self._inference_precision

    @inference_precision.setter
    def inference_precision(self, value):
        if value not in PRECISIONS:
            raise ValueError(f"ConvFormerStages.inference_precision must be one of {PRECISIONS}, got {value!r}")
        self._inference_precision = value

    def _events(self, dev):
        """This module's overflow counter on `dev` (a device int32; not a buffer: it is no part of the state dict)."""
        cache = self.__dict__.setdefault("_f16_events", {})
        if dev not in cache:
            cache[dev] = ops.f16_events(dev)
        return cache[dev]

    def overflow_events(self):
        """Values the fp16 walk has stored as infinity (or NaN) from a finite fp32 value since the module was built, over all devices it ran
        on.  fp16 conversions do not saturate, so an activation beyond 65504 shows in the returned maps as inf / NaN; this count says that the
        conversions are where it came from.  Synchronises the device: a diagnostic, not part of a pass."""
        return sum(int(c.item()) for c in self.__dict__.get("_f16_events", {}).values())

    # ---- loading -------------------------------------------------------------------------------------------------------------------
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # timm's blocks at these stages have neither layer scale nor residual scale; a dict that carries them describes another network
        bad = [k for k in state_dict if k.startswith(prefix) and (".layer_scale" in k or ".res_scale" in k)]
        if bad:
            raise RuntimeError(f"ConvFormerStages: layer-scale / residual-scale tensors are not part of stages 0-1: {bad[:4]}")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ---- plain torch (host tensors; autograd) ---------------------------------------------------------------------------------------
    def _block_torch(self, x, blk):
        tm, mlp = blk.token_mixer, blk.mlp
        t = F.conv2d(_channel_norm(x, blk.norm1), tm.pwconv1.weight)
        t = F.conv2d(_star_relu(t, tm.act1), tm.dwconv.weight, None, 1, 3, 1, t.shape[1])
        x = x + F.conv2d(t, tm.pwconv2.weight)
        t = F.conv2d(_channel_norm(x, blk.norm2), mlp.fc1.weight)
        return x + F.conv2d(_star_relu(t, mlp.act), mlp.fc2.weight)

    def _forward_torch(self, img):
        x = F.conv2d(img, self.stem.conv.weight, self.stem.conv.bias, self.stem_stride, self.stem_pad)
        x = _channel_norm(x, self.stem.norm)
        for blk in self.stages_0.blocks:
            x = self._block_torch(x, blk)
        maps = {0: x}
        if 1 in self.out_stages:
            ds = self.stages_1.downsample
            x = F.conv2d(_channel_norm(x, ds.norm), ds.conv.weight, ds.conv.bias, self.down_stride, 1)
            for blk in self.stages_1.blocks:
                x = self._block_torch(x, blk)
            maps[1] = x
        return [maps[s].contiguous() for s in self.out_stages]

    # ---- HIP kernels ------------------------------------------------------------------------------------------------------------------
    def _zeros(self, dim, dev):
        """nm_layernorm's beta operand for the bias-free norms."""
        cache = self.__dict__.setdefault("_zero_beta", {})
        z = cache.get((dim, dev))
        if z is None:
            z = cache[(dim, dev)] = torch.zeros(dim, device=dev, dtype=torch.float32)
        return z

    def _block(self, K, x, blk, shape):
        """One block on the operation set K.  x: rows (n*h*w, d) of the channel-last map `shape` = (n, h, w)."""
        tm, mlp = blk.token_mixer, blk.mlp
        d = x.shape[1]
        zero = self._zeros(d, x.device)
        t = K.linear(K.layernorm(x, blk.norm1.weight, zero, EPS), tm.pwconv1.weight.view(2 * d, d))
        t = K.dwconv7_nhwc(t.view(*shape, 2 * d), tm.dwconv.weight, tm.act1.scale, tm.act1.bias)
        x = K.linear(t.view(-1, 2 * d), tm.pwconv2.weight.view(d, 2 * d), residual=x)
        t = K.layernorm(x, blk.norm2.weight, zero, EPS)
        if hasattr(K, "star_relu"):
            t = K.star_relu(K.linear(t, mlp.fc1.weight.view(4 * d, d)), mlp.act.scale, mlp.act.bias)
        else:  # (the fp16 set: the activation is fc1's epilogue)
            t = K.linear(t, mlp.fc1.weight.view(4 * d, d), star=(mlp.act.scale, mlp.act.bias))
        return K.linear(t, mlp.fc2.weight.view(d, 4 * d), residual=x)

    def _forward_kernels(self, img, recording):
        """The one walk over the kernels: stem -> stage 0 -> downsample -> stage 1 on channel-last rows.  Inference and recording run
        this same sequence on their operation sets, so the recorded maps have the inference bits."""
        img = img.contiguous()
        B, _, H, W = img.shape
        dev = img.device
        h0, w0 = (ops.conv_out_size(n, 7, self.stem_stride, self.stem_pad) for n in (H, W))
        if h0 < 1 or w0 < 1:
            raise ValueError(f"ConvFormerStages: a {H}x{W} image is smaller than the stem's kernel")
        h1, w1 = (ops.conv_out_size(n, 3, self.down_stride, 1) for n in (h0, w0))
        hw = {0: (h0, w0), 1: (h1, w1)}
        if recording:  # the whole batch in one piece (the ordered parameter-gradient sums run over the batch); the maps are Function outputs
            K, step, outs = ag, B, {}

            def emit(s, x, b0):
                outs[s] = ag.nhwc_to_nchw(x)
        else:          # a chunk of images at a time, each chunk's planes written straight into the preallocated maps
            fp16 = self.inference_precision == "fp16"
            per_image = max(h0 * w0 * 4 * DIMS[0], h1 * w1 * 4 * DIMS[1]) * (2 if fp16 else 4)
            K, step = _fp16_ops(self._events(dev)) if fp16 else _INFERENCE, max(1, int(self.chunk_bytes) // per_image)
            outs = {s: torch.empty(B, DIMS[s], *hw[s], device=dev, dtype=torch.float32) for s in set(self.out_stages)}

            def emit(s, x, b0):
                ops.nhwc_to_nchw(x, out=outs[s][b0:b0 + x.shape[0]])
        ds = self.stages_1.downsample
        stream_norm = getattr(K, "stream_norm", K.layernorm)  # (the stem's norm makes the residual stream: fp32 on every set)
        for b0 in range(0, B, step):
            n = min(step, B - b0)
            rows = K.conv_patches(img[b0:b0 + n], 7, self.stem_stride, self.stem_pad, STEM_LD)
            x = K.linear(rows, K.conv_weight_rows(self.stem.conv.weight, STEM_LD), self.stem.conv.bias)
            del rows
            x = stream_norm(x, self.stem.norm.weight, self._zeros(DIMS[0], dev), EPS)
            for blk in self.stages_0.blocks:
                x = self._block(K, x, blk, (n, h0, w0))
            if 0 in self.out_stages:
                emit(0, x.view(n, h0, w0, DIMS[0]), b0)
            if 1 not in self.out_stages:
                continue
            t = K.layernorm(x, ds.norm.weight, self._zeros(DIMS[0], dev), EPS)
            rows = K.conv_patches(t.view(n, h0, w0, DIMS[0]), 3, self.down_stride, 1, 9 * DIMS[0], True)
            x = K.linear(rows, K.conv_weight_rows(ds.conv.weight, 9 * DIMS[0]), ds.conv.bias)
            del rows, t
            for blk in self.stages_1.blocks:
                x = self._block(K, x, blk, (n, h1, w1))
            emit(1, x.view(n, h1, w1, DIMS[1]), b0)
        return [outs[s] for s in self.out_stages]

    def _records_grad(self, img):
        return torch.is_grad_enabled() and (img.requires_grad or any(p.requires_grad for p in self.parameters()))

    def forward(self, img):
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"ConvFormerStages: expected an image batch (B,3,H,W), got {tuple(img.shape)}")
        img = img.to(torch.float32)
        if img.is_cuda and self.train_native and ag.is_training() and not img.requires_grad and any(p.requires_grad for p in self.parameters()):
            return self._forward_kernels(img, recording=True)
        if not img.is_cuda or self._records_grad(img):
            return self._forward_torch(img)
        return self._forward_kernels(img, recording=False)


class ConvFormerMS(nn.Module):
    """The multi-scale wrapper (the reference's MetaFormer_MS): `.model` holds the stages with the stem at stride 2 / padding 3 and the
    downsample at stride 4; forward(img) -> (cfeat (B,256,H/8,W/8), ffeat (B,128,H/2,W/2))."""

    def __init__(self, inference_precision="same"):
        super().__init__()
        self.feat_dim = [DIMS[1], DIMS[0]]
        self.model = ConvFormerStages(2, 3, 4, (0, 1), inference_precision)

    def forward(self, img):
        ffeat, cfeat = self.model(img)
        return cfeat, ffeat


_PRETRAINED_WARNED = [False]


def pretrained_notice(name):
    """`pretrained=True` (every shipped config says so): nothing is downloaded; the weights come from the checkpoint."""
    if not _PRETRAINED_WARNED[0]:
        _PRETRAINED_WARNED[0] = True
        warnings.warn(f"nerfmatch_amd: backbone '{name}' with pretrained=True -- ImageNet weights are not fetched; the backbone is "
                      "initialised at random and takes its weights from the matcher checkpoint (or load_timm_state_dict)")


def load_timm_state_dict(backbone, state_dict):
    """Load a full timm convformer_b36 / caformer_b36 state dict (keys `stem.*`, `stages.N.*`, `head.*`) that the caller already has
    into a backbone built here (a ConvFormerStages or the multi-scale wrapper): `stages.N.` becomes `stages_N.`, stages 2-3 and the
    classifier head are ignored, any other unknown key raises, and so does a missing one."""
    model = backbone.model if isinstance(backbone, ConvFormerMS) else backbone
    want = model.state_dict()
    sd, unknown = {}, []
    for k, v in state_dict.items():
        if k.startswith(("stages.2.", "stages.3.", "head.")):
            continue
        parts = k.split(".")
        kk = f"stages_{parts[1]}." + ".".join(parts[2:]) if parts[0] == "stages" and len(parts) > 2 else k
        if kk not in want:
            unknown.append(k)
        sd[kk] = v
    if unknown:
        raise KeyError(f"load_timm_state_dict: keys that are not part of the stem or stages 0-1 of a ConvFormer-B36: {unknown[:8]}")
    model.load_state_dict(sd, strict=True)
    return backbone
