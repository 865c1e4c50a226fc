"""Training-mode rendering and losses of a NeRF scene model (reference: NerfRenderer.render_rays with validation=False,
nerfmatch/nerf/renderer.py:182-295; compute_nerf_metrics, nerfmatch/utils/metrics.py:59-96; NerfTrainer.training_step,
nerfmatch/nerf_trainer.py:140-158).

One coarse -> fine render with gradients towards the parameters of both networks and the appearance table:
  sampling    ops.sample_coarse, ops.resample on the coarse pass's (noisy) compositing weights -- as at inference, no gradient
              (render_utils.py:299-310, :581-597: randomized, under no_grad, stop_grad)
  encoding    nm_nerf_train_encode: xi (n,96) | xd (n,48) with the appearance row of every ray's own id (renderer.py:225)
  MLP         the GEMM chain of gemm_field.FineField on the live parameters: forward through ops.linear (`pre` joins the skip / view inputs),
              dX through ops.linear on the transposed weights with the `gate` epilogue, dW and db through ops.linear_wgrad_bias, in the
              arithmetic ops.LINEAR_PRECISION selects.  The weight gradients of the two layers with a concatenated input are two GEMMs
              written into the column blocks of the reference-shaped gradient; padded columns / head rows are dropped
  per ray     nm_nerf_composite4(_bwd) (gemm_field.composite: density noise, either background), nm_nerf_distortion(_bwd), nm_nerf_photo_loss,
              nm_nerf_app_grad (fixed summation order)
Rays are processed in chunks whose saved activations stay below `chunk_bytes`; weight gradients accumulate over the chunks.

RenderArgs.precision == "f16" (NerfRenderer.train_precision) swaps the MLP for Chain16: fp16 encodings, activations and
gradient rows, one fp16 MFMA product per K-step (ops.linear_chain_f16, ops.linear_wgrad_f16), the backward pass on RenderArgs.loss_scale
times the loss; the gradients that leave TrainRender are unscaled fp32 either way.  Non-finite fp16 stores are counted into
RenderArgs.events (device int32[2]: forward, backward)."""
import ctypes as C

import torch
import torch.nn.functional as F

from .. import ops
from .._lib import check, dptr, lib, stream
from .gemm_field import XD, XI, FineField, _new, composite, composite_bwd

SAVED_FLOATS = XI + XD + 8 * 256 + 256 + 128  # per sample: the inputs, the eight hidden layers, the feature and the views layer
HEAD = ("alpha_linear", "feature_linear", "views_linears.0", "rgb_linear")


def net_parameters(net):
    """The 24 parameters of one NeRF in the order the autograd function takes them: pts_linears 0..7 (weight, bias), then the heads."""
    ps = []
    for l in range(8):
        ps += [net.pts_linears[l].weight, net.pts_linears[l].bias]
    for mod in (net.alpha_linear, net.feature_linear, net.views_linears[0], net.rgb_linear):
        ps += [mod.weight, mod.bias]
    return ps


# ---- kernel wrappers -------------------------------------------------------------------------------------------------------------------
def encode(rays, t, ray_id=None, table=None, var_scale=-1.0, status=None, ray_id_host=None, dtype=torch.float32):
    """-> xi (R*S, 96), xd (R*S, 48).  ray_id: int64 (R,) on the device; ray_id_host: the same ids on the host (checked there).
    dtype torch.float16: the same values rounded once (nm_nerf_train_encode_f16)."""
    R, S = t.shape[0], t.shape[1] - 1
    xi, xd = (torch.empty(R * S, c, device=rays.device, dtype=dtype) for c in (XI, XD))
    hp = C.c_void_p(0)
    if ray_id_host is not None:
        ray_id_host = ray_id_host.to(torch.int64).contiguous()
        hp = C.c_void_p(ray_id_host.data_ptr())
    V = 0 if table is None else table.shape[0]
    name = "nm_nerf_train_encode" if dtype == torch.float32 else "nm_nerf_train_encode_f16"
    check(getattr(lib(), name)(dptr(rays), dptr(t), R, S, dptr(ray_id, torch.int64), hp, dptr(table), V, float(var_scale), dptr(xi, dtype),
                               dptr(xd, dtype), dptr(status, torch.int32), stream()), name)
    return xi, xd


def g4_split_f16(g4, scale, events=None):
    """g4 (n,4) fp32 -> fp16(scale * g4) as the backward chain's two zero-padded operands g_logit (n,8), g_sig (n,8) (nm_nerf_g4_split_f16)."""
    n = g4.shape[0]
    g_logit, g_sig = (torch.empty(n, 8, device=g4.device, dtype=torch.float16) for _ in range(2))
    if n:
        check(lib().nm_nerf_g4_split_f16(dptr(g4), n, float(scale), dptr(g_logit, torch.float16), dptr(g_sig, torch.float16),
                                         dptr(events, torch.int32), stream()), "nm_nerf_g4_split_f16")
    return g_logit, g_sig


def _distortion(t, t_is_s, weights, want_mean=True):
    R, S, dev = t.shape[0], t.shape[1] - 1, t.device
    ws = torch.empty(lib().nm_nerf_distortion_workspace_bytes(), dtype=torch.uint8, device=dev)
    s = None if t_is_s else torch.empty_like(t)
    per_ray = None if weights is None else _new(R, dev=dev)
    mean = _new(1, dev=dev) if weights is not None and want_mean else None
    check(lib().nm_nerf_distortion(dptr(t), int(t_is_s), dptr(weights), R, S, dptr(ws, torch.uint8), dptr(s), dptr(per_ray), dptr(mean), stream()),
          "nm_nerf_distortion")
    return s, per_ray, mean


def t_to_s(t):
    """s (R,S+1) of the fence posts t with near / far = the minimum / maximum over the whole batch (render_utils.py:618-636)."""
    return _distortion(t.contiguous(), False, None)[0]


def distortion_bwd(s, weights, scale=1.0):
    g = torch.empty_like(weights)
    check(lib().nm_nerf_distortion_bwd(dptr(s), dptr(weights), weights.shape[0], weights.shape[1], float(scale), dptr(g), stream()),
          "nm_nerf_distortion_bwd")
    return g


def app_grad(g_xd_a, g_xd_b, ray_id, R, S, g_table):
    g_ray = _new(R, 16, dev=g_table.device)
    check(lib().nm_nerf_app_grad(dptr(g_xd_a), dptr(g_xd_b), dptr(ray_id, torch.int64), R, S, g_table.shape[0], dptr(g_ray), dptr(g_table), stream()),
          "nm_nerf_app_grad")
    return g_table


class _Distortion(torch.autograd.Function):
    """weight * distortion_loss(s, weights) (metrics.py:448-465); the gradient reaches the weights only (s comes from the samplers)."""

    @staticmethod
    def forward(ctx, s, weights, weight):
        s, weights = s.contiguous(), weights.contiguous()
        _, per_ray, mean = _distortion(s, True, weights)
        ctx.save_for_backward(s, weights)
        ctx.weight = float(weight)
        return mean.reshape(()) * ctx.weight

    @staticmethod
    def backward(ctx, up):
        s, weights = ctx.saved_tensors
        return None, distortion_bwd(s, weights, ctx.weight) * up, None


class _PhotoLoss(torch.autograd.Function):
    """-> (coarse_weight * mse_c + mse_f, mse_c, mse_f) with mse = 0.5 mean(mask (rgb - gt)^2); the first output carries the gradient."""

    @staticmethod
    def forward(ctx, rgb_c, rgb_f, gt, mask, coarse_weight):
        R, dev = rgb_c.shape[0], rgb_c.device
        rgb_c, rgb_f, gt = rgb_c.contiguous(), rgb_f.contiguous(), gt.to(torch.float32).contiguous()
        mask = None if mask is None else mask.to(torch.float32).reshape(-1).contiguous()
        if gt.shape != (R, 3) or rgb_f.shape != (R, 3) or (mask is not None and mask.numel() != R):
            raise ValueError(f"photometric loss: rgb {tuple(rgb_c.shape)} / {tuple(rgb_f.shape)}, gt {tuple(gt.shape)}, mask {None if mask is None else mask.numel()}")
        acc = torch.empty(2, dtype=torch.float64, device=dev)
        g_c, g_f = _new(R, 3, dev=dev), _new(R, 3, dev=dev)
        check(lib().nm_nerf_photo_loss(dptr(rgb_c), dptr(rgb_f), dptr(gt), dptr(mask), float(coarse_weight), R, dptr(acc, torch.float64), dptr(g_c),
                                       dptr(g_f), stream()), "nm_nerf_photo_loss")
        ctx.save_for_backward(g_c, g_f)
        mse = acc.to(torch.float32)
        ctx.mark_non_differentiable(mse)
        return (acc[0] * float(coarse_weight) + acc[1]).to(torch.float32), mse

    @staticmethod
    def backward(ctx, up, _):
        g_c, g_f = ctx.saved_tensors
        return g_c * up, g_f * up, None, None, None


def training_metrics(preds, rgb_gt, mask_loss=None, cnfg_loss=None):
    """compute_nerf_metrics(validation_mode=False) (metrics.py:59-96) of a training render on the fused loss kernels: the same keys and
    values as utils.metrics.compute_nerf_metrics, `loss` differentiable towards rgb_coarse, rgb_fine and weights_fine."""
    from ..utils.metrics import mse2psnr

    total, mse = _PhotoLoss.apply(preds["rgb_coarse"], preds["rgb_fine"], rgb_gt, mask_loss, float(getattr(cnfg_loss, "coarse_weight", 1.0)))
    out = {"rgb_coarse_mse": mse[0], "rgb_coarse_psnr": mse2psnr(mse[0]), "rgb_fine_mse": mse[1], "rgb_fine_psnr": mse2psnr(mse[1])}
    reg = getattr(cnfg_loss, "ray_reg_weight", None)
    if "s_fine" in preds and reg:
        total = total + _Distortion.apply(preds["s_fine"], preds["weights_fine"], float(reg))
    out["loss"] = total
    return out


# ---- the MLP as a GEMM chain on the live parameters ----------------------------------------------------------------------------------------
class _Params:
    """state_dict() of one NeRF from its 24 parameter tensors (net_parameters order): what FineField packs its operands from"""

    def __init__(self, P):
        names = [f"pts_linears.{l}.{k}" for l in range(8) for k in ("weight", "bias")] + [f"{m}.{k}" for m in HEAD for k in ("weight", "bias")]
        self.sd = dict(zip(names, P))

    def state_dict(self):
        return self.sd


class Chain(FineField):
    """FineField (the padded GEMM operands of one NeRF and their transposes) on the CURRENT values of the network's 24 parameters
    (net_parameters order, detached; built once per step), with a forward pass that also keeps the feature layer and a backward pass that
    adds the weight / bias gradients of a chunk of samples into `grads`."""

    def __init__(self, P):
        super().__init__(_Params(P), P[0].device)
        self.app = P[20].shape[1] - 283

    def forward(self, xi, xd):
        """-> out4 (n,4) = rgb logits | raw sigma, saved activations."""
        logit, sig, h, feat, hv = self.layers(xi, xd)
        return torch.cat([logit[:, :3], sig[:, :1]], 1), (xi, xd, h, feat, hv)

    @staticmethod
    def new_grads(dev):
        z = lambda *s: torch.zeros(*s, device=dev)
        g = dict(W=[z(256, XI)] + [z(256, 256) for _ in range(7)], b=[z(256) for _ in range(8)], W5x=z(256, XI), Wa=z(8, 256), ba=z(8),
                 Wf=z(256, 256), bf=z(256), Wvf=z(128, 256), Wvd=z(128, XD), bv=z(128), Wr=z(8, 128), br=z(8))
        return g

    def backward(self, g4, saved, grads, want_g_xd=False):
        """g4 (n,4) = d loss / d out4 of one chunk: adds the chunk's dW / db into `grads`; -> d loss / d xd (n,48) when asked for (the
        appearance columns).  d loss / d xi is not formed: nothing upstream of the encodings takes a gradient."""
        lin, wgb, wg = ops.linear, ops.linear_wgrad_bias, ops.linear_wgrad
        xi, xd, h, feat, hv = saved
        g_logit, g_sig = F.pad(g4[:, :3], (0, 5)).contiguous(), F.pad(g4[:, 3:4], (0, 7)).contiguous()
        wgb(g_logit, hv, out=(grads["Wr"], grads["br"]))
        dy_v = lin(g_logit, self.WrT, gate=hv)
        wgb(dy_v, feat, out=(grads["Wvf"], grads["bv"]))
        wg(dy_v, xd, out=grads["Wvd"])
        g_xd = lin(dy_v, self.WvdT) if want_g_xd else None
        g_feat = lin(dy_v, self.WvfT)
        wgb(g_feat, h[7], out=(grads["Wf"], grads["bf"]))
        wgb(g_sig, h[7], out=(grads["Wa"], grads["ba"]))
        g = lin(g_feat, self.WfT, residual=lin(g_sig, self.WaT), gate=h[7])
        for l in range(7, 0, -1):
            wgb(g, h[l - 1], out=(grads["W"][l], grads["b"][l]))
            if l == 5:
                wg(g, xi, out=grads["W5x"])
            g = lin(g, self.WT[l], gate=h[l - 1])
        wgb(g, xi, out=(grads["W"][0], grads["b"][0]))
        return g_xd

    def finish(self, grads):
        """the accumulated operand gradients in the shapes of the 24 parameters (padding dropped, column blocks joined)"""
        out = []
        for l in range(8):
            w = grads["W"][l]
            if l == 0:
                w = w[:, :90].contiguous()
            elif l == 5:
                w = torch.cat([grads["W5x"][:, :90], w], 1)
            out += [w, grads["b"][l]]
        out += [grads["Wa"][:1].contiguous(), grads["ba"][:1].contiguous(), grads["Wf"], grads["bf"]]
        out += [torch.cat([grads["Wvf"], grads["Wvd"][:, : 27 + self.app]], 1), grads["bv"]]
        out += [grads["Wr"][:3].contiguous(), grads["br"][:3].contiguous()]
        return out


class Chain16(Chain):
    """Chain in the fp16 mixed-precision arithmetic: fp16 encodings, activations and gradient rows, weights rounded to fp16
    as they are packed, one MFMA product per K-step with fp32 accumulation; the two layers with a concatenated input are one launch with a
    two-source K loop; the heads store fp32.  The backward pass runs on `scale` times the loss and hands back unscaled fp32 gradients
    (alpha = 1 / scale in the weight-gradient launches and the one product towards xd).  ev_f / ev_b: device int32[1] counters of the
    forward / backward stores that were not finite."""

    def __init__(self, P, ev_f=None, ev_b=None):
        FineField.__init__(self, _Params(P), P[0].device, transposes=False)
        self.app = P[20].shape[1] - 283
        self.ev_f, self.ev_b = ev_f, ev_b

    def forward(self, xi, xd):
        lin, ev = ops.linear_chain_f16, self.ev_f
        h = [lin(xi, self.W[0], self.b[0], relu=True, events=ev)]
        for l in range(1, 8):
            x2, w2 = (xi, self.W5x) if l == 5 else (None, None)
            h.append(lin(h[-1], self.W[l], self.b[l], x2=x2, weight2=w2, relu=True, events=ev))
        sig = lin(h[7], self.Wa, self.ba, out_dtype=torch.float32)
        feat = lin(h[7], self.Wf, self.bf, events=ev)
        hv = lin(feat, self.Wvf, self.bv, x2=xd, weight2=self.Wvd, relu=True, events=ev)
        logit = lin(hv, self.Wr, self.br, out_dtype=torch.float32)
        return torch.cat([logit[:, :3], sig[:, :1]], 1), (xi, xd, h, feat, hv)

    def backward(self, g4, saved, grads, want_g_xd=False, scale=1.0):
        ev, inv = self.ev_b, 1.0 / float(scale)
        lin = lambda dy, w, **kw: ops.linear_chain_f16(dy, w, transposed=True, events=ev, **kw)
        wg = lambda dy, x, dw, db=None: ops.linear_wgrad_f16(dy, x, out=(dw, db), alpha=inv, bias=db is not None)
        xi, xd, h, feat, hv = saved
        g_logit, g_sig = g4_split_f16(g4.contiguous(), scale, ev)
        wg(g_logit, hv, grads["Wr"], grads["br"])
        dy_v = lin(g_logit, self.Wr, gate=hv)
        wg(dy_v, feat, grads["Wvf"], grads["bv"])
        wg(dy_v, xd, grads["Wvd"])
        g_xd = lin(dy_v, self.Wvd, alpha=inv, out_dtype=torch.float32) if want_g_xd else None
        g_feat = lin(dy_v, self.Wvf)
        wg(g_feat, h[7], grads["Wf"], grads["bf"])
        wg(g_sig, h[7], grads["Wa"], grads["ba"])
        g = lin(g_feat, self.Wf, residual=lin(g_sig, self.Wa), gate=h[7])
        for l in range(7, 0, -1):
            wg(g, h[l - 1], grads["W"][l], grads["b"][l])
            if l == 5:
                wg(g, xi, grads["W5x"])
            g = lin(g, self.W[l], gate=h[l - 1])
        wg(g, xi, grads["W"][0], grads["b"][0])
        return g_xd


class RenderArgs:
    """The non-tensor-parameter inputs of one training render (everything that carries no gradient)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class TrainRender(torch.autograd.Function):
    """(args, 24 coarse parameters, 24 fine parameters[, appearance table]) -> rgb_coarse, depth_coarse, rgb_fine, depth_fine, weights_fine,
    s_fine, t_coarse, t_fine, weights_coarse.  Differentiable: rgb_coarse, rgb_fine, weights_fine (what the reference's loss reads)."""

    @staticmethod
    def forward(ctx, a, *params):
        P = [p.detach() for p in params]
        table = P[48] if len(P) > 48 else None
        f16 = getattr(a, "precision", "same") == "f16"
        if f16:
            ev = a.events
            nets = (Chain16(P[:24], ev[0:1], ev[1:2]), Chain16(P[24:48], ev[0:1], ev[1:2]))
        else:
            nets = (Chain(P[:24]), Chain(P[24:48]))
        rays, S = a.rays, a.S
        R = rays.shape[0]
        step = max(1, int(a.chunk_rays))
        chunks = [(lo, min(R, lo + step)) for lo in range(0, R, step)]

        def run(net, t):
            out4, saved = [], []
            for lo, hi in chunks:
                ids = None if a.ray_id is None else a.ray_id[lo:hi]
                ids_host = None if a.ray_id_host is None else a.ray_id_host[lo:hi]
                xi, xd = encode(rays[lo:hi], t[lo:hi], ids, table, a.var_scale, a.status, ids_host, torch.float16 if f16 else torch.float32)
                o, sv = net.forward(xi, xd)
                out4.append(o)
                saved.append(sv)
            return (out4[0] if len(out4) == 1 else torch.cat(out4, 0)), saved

        t_c = ops.sample_coarse(rays, a.t_rand, S)
        out4_c, saved_c = run(nets[0], t_c)
        rgb_c, depth_c, _, w_c = composite(out4_c, t_c, rays, a.noise_coarse, a.noise_std, a.white_bg)
        t_f = ops.resample(t_c, w_c, a.jitter, a.padding, True, jitter_scale=a.jitter_scale)
        out4_f, saved_f = run(nets[1], t_f)
        rgb_f, depth_f, _, w_f = composite(out4_f, t_f, rays, a.noise_fine, a.noise_std, a.white_bg)
        s_f = t_to_s(t_f)
        ctx.a, ctx.nets, ctx.chunks, ctx.has_table = a, nets, chunks, table is not None
        ctx.saved = [saved_c, saved_f]
        ctx.save_for_backward(out4_c, t_c, out4_f, t_f, *params)  # (the parameters: autograd then refuses a backward after an in-place update)
        ctx.mark_non_differentiable(depth_c, depth_f, s_f, t_c, t_f, w_c)
        return rgb_c, depth_c, rgb_f, depth_f, w_f, s_f, t_c, t_f, w_c

    @staticmethod
    def backward(ctx, g_rgb_c, _gdc, g_rgb_f, _gdf, g_w_f, *_):
        a, nets = ctx.a, ctx.nets
        out4_c, t_c, out4_f, t_f = ctx.saved_tensors[:4]
        table = ctx.saved_tensors[4 + 48] if ctx.has_table else None
        rays, S, dev = a.rays, a.S, a.rays.device
        zero = lambda g: torch.zeros(rays.shape[0], 3, device=dev) if g is None else g
        g4 = [composite_bwd(out4_c, t_c, rays, zero(g_rgb_c), None, a.noise_coarse, a.noise_std, a.white_bg),
              composite_bwd(out4_f, t_f, rays, zero(g_rgb_f), g_w_f, a.noise_fine, a.noise_std, a.white_bg)]
        grads = [Chain.new_grads(dev), Chain.new_grads(dev)]
        g_table = torch.zeros_like(table) if table is not None else None
        for k, (lo, hi) in enumerate(ctx.chunks):
            g_xd = []
            for i in (0, 1):
                kw = dict(scale=a.loss_scale) if isinstance(nets[i], Chain16) else {}
                g_xd.append(nets[i].backward(g4[i][lo * S:hi * S], ctx.saved[i][k], grads[i], want_g_xd=table is not None, **kw))
                ctx.saved[i][k] = None  # (a chunk's activations are released as soon as its gradients are in)
            if table is not None:
                app_grad(g_xd[0], g_xd[1], None if a.ray_id is None else a.ray_id[lo:hi], hi - lo, S, g_table)
        out = [None] + nets[0].finish(grads[0]) + nets[1].finish(grads[1])
        if table is not None:
            out.append(g_table)
        return tuple(out)


def chunk_rays_for(S, chunk_bytes, elem_size=4):
    """rays per chunk such that one chunk's saved activations of one network (elem_size bytes each: 4, or 2 in the fp16 walk) stay below
    chunk_bytes"""
    return max(1, int(chunk_bytes) // (S * SAVED_FLOATS * int(elem_size)))
