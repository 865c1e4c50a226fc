"""Test helper (not product code): the fp16 mixed-precision NeRF training step (NerfRenderer.train_precision = "f16") emulated
on the CPU in float64.  Sampling, compositing and the losses are nerf_train_util's; the MLP is replaced by one whose operands are rounded to
fp16 at exactly the sites where the kernels store fp16:
  forward    the packed weights, the encodings xi / xd (appearance row included), every stored activation (the eight hidden layers, the
             feature layer, the views layer); the density / rgb heads stay unrounded (the kernels store them as fp32)
  backward   every stored gradient row g as fp16(g * scale) / scale: d loss / d (rgb logits, sigma) as they enter the chain, the gradient at
             every ReLU layer's pre-activation (gated by the STORED activation > 0, then rounded), at the feature layer's output, and the
             density head's product towards layer 7 (the kernels' fp16 residual) before it is added
Each site is a straight-through autograd.Function.  A value rounds float64 -> float32 -> fp16 (the kernels round an fp32 accumulator once).
With rounding=False every site is the identity and the step is nerf_train_util.train_step's."""
import torch
import torch.nn.functional as F

import nerf_train_util as ntu
from oracle import nerf_oracle as no


def r16(x):
    return x.to(torch.float32).to(torch.float16).to(x.dtype)


def make_sites(scale, rounding=True):
    """-> (round_st, act, feat_site, grad_site) for one loss scale"""
    rnd = r16 if rounding else (lambda x: x)
    rg = (lambda g: r16(g * scale) / scale) if rounding else (lambda g: g)

    class RoundST(torch.autograd.Function):  # a stored operand: rounded, the gradient passes
        @staticmethod
        def forward(ctx, x):
            return rnd(x)

        @staticmethod
        def backward(ctx, g):
            return g

    class Act(torch.autograd.Function):  # h = fp16(relu(z)); g_z = fp16 row of g_h * [h > 0]
        @staticmethod
        def forward(ctx, z):
            h = rnd(torch.relu(z))
            ctx.save_for_backward(h)
            return h

        @staticmethod
        def backward(ctx, g):
            (h,) = ctx.saved_tensors
            return rg(g * (h > 0))

    class Feat(torch.autograd.Function):  # the feature layer: stored activation, stored gradient row, no gate
        @staticmethod
        def forward(ctx, z):
            return rnd(z)

        @staticmethod
        def backward(ctx, g):
            return rg(g)

    class GradRow(torch.autograd.Function):  # identity forwards; the gradient is a stored fp16 row
        @staticmethod
        def forward(ctx, z):
            return z.clone()

        @staticmethod
        def backward(ctx, g):
            return rg(g)

    return RoundST.apply, Act.apply, Feat.apply, GradRow.apply


def make_mlp(scale, rounding=True):
    """nerf_oracle.nerf_mlp's signature, with the rounding sites of the fp16 walk"""
    st, act, feat_site, grad_row = make_sites(float(scale), rounding)

    def mlp(params, prefix, x_pts, x_dirs, x_app=None, stop_layer=-1, skips=(4,)):
        w = lambda name: st(params[f"{prefix}.{name}.weight"])
        b = lambda name: params[f"{prefix}.{name}.bias"]
        xi = st(x_pts)
        xd = st(torch.cat([x_dirs] + ([x_app] if x_app is not None else []), -1))
        h = xi
        for i in range(8):
            h = act(F.linear(h, w(f"pts_linears.{i}"), b(f"pts_linears.{i}")))
            last = h
            if i in skips:
                h = torch.cat([xi, h], -1)
        sigma = grad_row(F.linear(grad_row(last), w("alpha_linear"), b("alpha_linear")))
        feat = feat_site(F.linear(last, w("feature_linear"), b("feature_linear")))
        v = act(F.linear(torch.cat([feat, xd], -1), w("views_linears.0"), b("views_linears.0")))
        rgb = torch.sigmoid(grad_row(F.linear(v, w("rgb_linear"), b("rgb_linear"))))
        return torch.cat([rgb, sigma], -1), last

    return mlp


class _Oracle:
    """nerf_oracle with the MLP replaced"""

    def __init__(self, mlp):
        self.nerf_mlp = mlp

    def __getattr__(self, name):
        return getattr(no, name)


def train_step(*a, scale=65536.0, rounding=True, **kw):
    """nerf_train_util.train_step (same arguments and result) on the emulated fp16 walk under loss scale `scale`."""
    keep = ntu.no
    ntu.no = _Oracle(make_mlp(scale, rounding))
    try:
        return ntu.train_step(*a, **kw)
    finally:
        ntu.no = keep
