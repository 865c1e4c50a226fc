"""float64 restatement of the ConvFormer stem and stages 0-1 WITH gradients, on the CPU, from convformer_util._ln and the architecture
table of nerfmatch_amd/modules/convformer.py: the reference of the backbone's backward tests.  It shares no code with the module.

Every StarReLU's 1-element `scale` and `bias` is expanded to a per-element leaf, so that both the scalar's gradient (the sum of the
leaf's gradient) and its cancellation-free scale (the sum of the absolute values) are available."""
import torch
import torch.nn.functional as F

import convformer_util as cu


def cotangents(shapes, seed=5):
    """Fixed N(0, 1) cotangents, one per returned map."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, dtype=torch.float32) for s in shapes]


class _Tape:
    def __init__(self, state):
        self.p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in state.items()}
        self.leaves = {}

    def star(self, x, name):
        for part in ("scale", "bias"):
            self.leaves[f"{name}.{part}"] = self.p[f"{name}.{part}"].detach().expand(x.shape).clone().requires_grad_(True)
        return self.leaves[f"{name}.scale"] * torch.clamp(x, min=0) ** 2 + self.leaves[f"{name}.bias"]

    def block(self, x, b):
        p = self.p
        t = F.conv2d(cu._ln(x, p[f"{b}.norm1.weight"]), p[f"{b}.token_mixer.pwconv1.weight"])
        t = self.star(t, f"{b}.token_mixer.act1")
        t = F.conv2d(t, p[f"{b}.token_mixer.dwconv.weight"], padding=3, groups=t.shape[1])
        x = x + F.conv2d(t, p[f"{b}.token_mixer.pwconv2.weight"])
        t = F.conv2d(cu._ln(x, p[f"{b}.norm2.weight"]), p[f"{b}.mlp.fc1.weight"])
        return x + F.conv2d(self.star(t, f"{b}.mlp.act"), p[f"{b}.mlp.fc2.weight"])

    def maps(self, img, stem_stride, stem_pad, down_stride, stage1=True):
        p = self.p
        x = F.conv2d(img.detach().cpu().double(), p["stem.conv.weight"], p["stem.conv.bias"], stride=stem_stride, padding=stem_pad)
        x = cu._ln(x, p["stem.norm.weight"])
        for i in range(cu.DEPTHS[0]):
            x = self.block(x, f"stages_0.blocks.{i}")
        f = x
        if not stage1:
            return f, None
        x = F.conv2d(cu._ln(x, p["stages_1.downsample.norm.weight"]), p["stages_1.downsample.conv.weight"],
                     p["stages_1.downsample.conv.bias"], stride=down_stride, padding=1)
        for i in range(cu.DEPTHS[1]):
            x = self.block(x, f"stages_1.blocks.{i}")
        return f, x


def reference_grads(state, img, strides, cot_f, cot_c):
    """name -> (float64 gradient, abs-sum) of <stage-0 map, cot_f> + <stage-1 map, cot_c> (either cotangent may be None).  abs-sum: for
    the 1-element StarReLU parameters the sum of |per-element contribution|, None for every other tensor.  A parameter that the
    cotangents do not reach (stage 1 without cot_c) is absent."""
    tape = _Tape(state)
    with torch.enable_grad():  # (the suite runs under no_grad)
        f, c = tape.maps(img, stage1=cot_c is not None, **strides)
        loss = 0.0
        if cot_f is not None:
            loss = loss + (f * cot_f.double()).sum()
        if cot_c is not None:
            loss = loss + (c * cot_c.double()).sum()
        loss.backward()
    out = {}
    for k, v in tape.p.items():
        if k in tape.leaves:
            g = tape.leaves[k].grad
            out[k] = (g.sum().reshape(1), float(g.abs().sum()))
        elif v.grad is not None:
            out[k] = (v.grad, None)
    return out


_CASES = {}


def case(kind, shape, seed=0):
    """(state, img, cotangents in the order of the module's outputs, reference_grads), once per (kind, shape, seed): "c2f" returns
    (stage 0, stage 1) at the multi-scale strides, "coarse" the stage-1 map at the Mini model's."""
    key = (kind, tuple(shape), seed)
    if key not in _CASES:
        state, img, f, c = cu.case(kind, shape, seed)
        if kind == "c2f":
            cots = cotangents([f.shape, c.shape])
            ref = reference_grads(state, img, cu.MS, cots[0], cots[1])
        else:
            cots = cotangents([c.shape])
            ref = reference_grads(state, img, cu.MINI, None, cots[0])
        _CASES[key] = (state, img, cots, ref)
    return _CASES[key]


def grad_errors(named_grads, ref):
    """name -> error of a gradient against reference_grads' entry: max|g - ref| / max(1, max|ref|) for tensors (convformer_util.scaled_err),
    |g - sum| / sum|contribution| for the 1-element StarReLU parameters."""
    errs = {}
    for k, g in named_grads.items():
        r, scale = ref[k]
        if scale is None:
            errs[k] = cu.scaled_err(g.reshape(r.shape), r)
        else:
            errs[k] = float((g.detach().cpu().double().reshape(1) - r).abs() / scale)
    return errs
