"""Image backbones.

The reference uses timm's ConvFormer/CAFormer-B36 patched to emit 1/8 and 1/2 resolution maps
(nerfmatch/modules/__init__.py:14-113): the stem and stages 0-1 of that network, which modules/convformer.py builds on the
HIP kernels (names 'convformer', 'convformer384', 'caformer', 'caformer384'; timm is not needed).  The OUTPUT CONTRACT:
    init_backbone_8_2(...)  -> module with .feat_dim == [256, 128], forward(img) -> (cfeat (B,256,H/8,W/8),
                                                                                    ffeat (B,128,H/2,W/2))
    init_backbone(...)      -> module with .feat_dim == 256,        forward(img) -> cfeat (B,256,H/8,W/8) or, as timm's
                                                                                    feature networks do, the one-element list [cfeat]
`backbone="stub"` selects a small deterministic torch stand-in with that contract (synthetic benchmarks, tests)."""
import torch
from torch import nn
import torch.nn.functional as F


class StubBackbone(nn.Module):
    """Deterministic stand-in: average pooling + fixed random 1x1 projections (PCG64 seeded)."""

    def __init__(self, coarse_dim=256, fine_dim=128, two_scales=True, seed=7):
        super().__init__()
        import numpy as np

        rng = np.random.default_rng(seed)
        self.two_scales = two_scales
        self.register_buffer("wc", torch.from_numpy(rng.standard_normal((coarse_dim, 3 * 16, 1, 1)).astype("float32")) / 3.0, persistent=False)
        self.register_buffer("wf", torch.from_numpy(rng.standard_normal((fine_dim, 3 * 4, 1, 1)).astype("float32")) / 2.0, persistent=False)
        self.feat_dim = [coarse_dim, fine_dim] if two_scales else coarse_dim

    def forward(self, img):
        # 1x1 projections as plain contractions (a conv2d would send MIOpen into its solver search on every fresh process)
        c = torch.einsum("oc,bchw->bohw", self.wc[:, :, 0, 0], F.pixel_unshuffle(F.avg_pool2d(img, 2), 4)).contiguous()
        if not self.two_scales:
            return c
        f = torch.einsum("oc,bchw->bohw", self.wf[:, :, 0, 0], F.pixel_unshuffle(img, 2)).contiguous()
        return c, f


class PrecomputedBackbone(nn.Module):
    """Returns feature maps computed elsewhere (parity tests start from the backbone's outputs)."""

    def __init__(self, outs, feat_dim):
        super().__init__()
        self.outs, self.feat_dim = outs, feat_dim

    def forward(self, img):
        return self.outs


_CONVFORMER = ("convformer", "convformer384", "caformer", "caformer384")


def _convformer_name(name):
    """True for the four names the native ConvFormer stages serve; the FPN variants (BatchNorm, bilinear upsampling; no shipped config
    selects them) and anything else are refused."""
    if name in _CONVFORMER:
        return True
    if isinstance(name, str) and name.endswith("_fpn") and name[:-4] in _CONVFORMER:
        raise NotImplementedError(f"backbone '{name}': the FPN head of the reference's MetaFormer_MS is not part of this build "
                                  f"(use '{name[:-4]}', which every shipped config selects)")
    raise NotImplementedError(f"backbone '{name}' is not known: the native backbones are {_CONVFORMER} (stem and stages 0-1 of timm's "
                              "ConvFormer/CAFormer-B36, modules/convformer.py) and 'stub'; or pass a module via model.backbone = ...")


def _stub_precision(precision):
    """The stand-in has one arithmetic: "same" passes, anything else is refused like an unknown value (ValueError)."""
    if precision != "same":
        raise ValueError(f"backbone 'stub' has no inference precision {precision!r}: \"fp16\" is a mode of the native ConvFormer stages")


def init_backbone_8_2(backbone="stub", pretrained=False, precision="same"):
    """precision: ConvFormerStages.inference_precision ("same", or the opt-in "fp16" inference walk)."""
    if backbone == "stub":
        _stub_precision(precision)
        return StubBackbone(two_scales=True)
    _convformer_name(backbone)
    from .convformer import ConvFormerMS, pretrained_notice

    if pretrained:
        pretrained_notice(backbone)
    return ConvFormerMS(precision)


def init_backbone(backbone="stub", pretrained=False, downsample=8, precision="same"):
    if backbone == "stub":
        _stub_precision(precision)
        return StubBackbone(two_scales=False)
    _convformer_name(backbone)
    if downsample != 8:
        raise ValueError(f"init_backbone: downsample {downsample}: the native ConvFormer stages end at 1/8 resolution")
    from .convformer import ConvFormerStages, pretrained_notice

    if pretrained:
        pretrained_notice(backbone)
    m = ConvFormerStages(4, 2, 2, (1,), precision)
    m.feat_dim = 256
    return m
