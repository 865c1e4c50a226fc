"""One NeRF MLP as a chain of GEMMs on padded operands, and the wavefront-per-ray compositing of its output rows: what the iNeRF pose
refinement (inerf.py) and scene training (nerf/train_render.py) share.  Rows: xi (n, XI) = IPE | padding, xd (n, XD) = direction PE |
appearance | padding (csrc/nerf_sample.h's write_sample_rows), out4 (n, 4) = rgb logits | raw sigma."""
import torch

from .. import ops
from .._lib import check, dptr, lib, stream

XI, XD = 96, 48


def _new(*shape, dev):
    return torch.empty(*shape, device=dev, dtype=torch.float32)


class FineField:
    """A NeRF as padded GEMM operands: forward weights and their transposes (for the backward GEMMs), cached per
    renderer.  Layers with a concatenated input are split into two GEMMs joined through the `pre` addend of nm_linear:
    layer 5 = relu(xi . W5x^T + h4 . W5h^T + b), views = relu(feature . Wvf^T + xd . Wvd^T + b); xi has 96 columns
    (90 IPE + padding), xd 48 (27 dir PE + 16 appearance + padding); the density / rgb heads are padded to 8 outputs.
    The ReLU derivatives of the backward pass are the `gate` of the same epilogue (no elementwise passes)."""

    def __init__(self, nerf_fine, dev, transposes=True):
        sd = {k: v.detach().to(dev, torch.float32) for k, v in nerf_fine.state_dict().items()}
        z = lambda *s: torch.zeros(*s, device=dev)

        def padded(w, cols):
            out = z(w.shape[0], cols)
            out[:, : w.shape[1]] = w
            return out.contiguous()

        W = [sd[f"pts_linears.{l}.weight"].contiguous() for l in range(8)]
        self.b = [sd[f"pts_linears.{l}.bias"].contiguous() for l in range(8)]
        self.W5x, W[5] = padded(W[5][:, :90], XI), W[5][:, 90:].contiguous()
        W[0] = padded(W[0], XI)
        self.W = W
        self.Wa, self.ba = z(8, 256), z(8)
        self.Wa[:1] = sd["alpha_linear.weight"]
        self.ba[:1] = sd["alpha_linear.bias"]
        self.Wf, self.bf = sd["feature_linear.weight"].contiguous(), sd["feature_linear.bias"].contiguous()
        wv = sd["views_linears.0.weight"]  # (128, 256 + 27 [+ 16])
        self.Wvf, self.Wvd, self.bv = wv[:, :256].contiguous(), padded(wv[:, 256:], XD), sd["views_linears.0.bias"].contiguous()
        self.Wr, self.br = z(8, 128), z(8)
        self.Wr[:3] = sd["rgb_linear.weight"]
        self.br[:3] = sd["rgb_linear.bias"]
        if not transposes:  # (the fp16 training walk packs its transposed operands straight from the stored tensors)
            return
        t = lambda w: w.t().contiguous()
        self.WT = [t(w) for w in W]
        self.W5xT, self.WaT, self.WfT, self.WvfT, self.WvdT, self.WrT = t(self.W5x), t(self.Wa), t(self.Wf), t(self.Wvf), t(self.Wvd), t(self.Wr)

    def layers(self, xi, xd):
        """xi (n,96), xd (n,48) -> rgb logits (n,8), raw sigma (n,8) (columns 0..2 / 0) and every activation: the eight hidden layers h,
        the feature layer, the views layer.  12 launches."""
        lin = ops.linear
        h = [lin(xi, self.W[0], self.b[0], act=1)]
        for l in range(1, 8):
            h.append(lin(h[-1], self.W[l], self.b[l], act=1, pre=lin(xi, self.W5x) if l == 5 else None))
        sig = lin(h[7], self.Wa, self.ba)
        feat = lin(h[7], self.Wf, self.bf)
        hv = lin(feat, self.Wvf, self.bv, act=1, pre=lin(xd, self.Wvd))
        logit = lin(hv, self.Wr, self.br)
        return logit, sig, h, feat, hv

    def forward(self, xi, xd):
        """-> rgb logits (n,8), raw sigma (n,8), the activations backward() reads."""
        logit, sig, h, _, hv = self.layers(xi, xd)
        return logit, sig, (h, hv)

    def backward(self, g_logit, g_sig, saved, g_h=None):
        """d loss / d logits, d loss / d sigma -> d loss / d xi (n,96), d loss / d xd (n,48).  g_h = (layer, d loss / d h[layer])
        adds a gradient arriving at one layer's (post-ReLU) activations from outside the network: the tapped features."""
        lin = ops.linear
        h, hv = saved
        tap, g_tap = g_h if g_h is not None else (-1, None)
        g_hv = lin(g_logit, self.WrT, gate=hv)
        g_xd = lin(g_hv, self.WvdT)
        g_sig_h = lin(g_sig, self.WaT, residual=g_tap if tap == 7 else None)
        g = lin(lin(g_hv, self.WvfT), self.WfT, residual=g_sig_h, gate=h[7])
        g_xi_skip = None
        for l in range(7, 0, -1):
            if l == 5:
                g_xi_skip = lin(g, self.W5xT)
            g = lin(g, self.WT[l], residual=g_tap if tap == l - 1 else None, gate=h[l - 1])
        g_xi = lin(g, self.WT[0], residual=g_xi_skip)
        return g_xi, g_xd


def composite(out4, t, rays, noise=None, noise_std=0.0, white_bg=False, S_act=None, depth_acc=True):
    """out4 (R * S_act, 4), fence posts t (R, S + 1) -> rgb (R,3), depth (R), acc (R) (None when not wanted), weights (R, S_act); one
    wavefront per ray (nm_nerf_composite4).  S_act: the leading samples of a ray that out4 holds (None = all S)."""
    R, S, dev = t.shape[0], t.shape[1] - 1, t.device
    Sa = S if S_act is None else int(S_act)
    rgb, w = _new(R, 3, dev=dev), _new(R, Sa, dev=dev)
    depth, acc = (_new(R, dev=dev), _new(R, dev=dev)) if depth_acc else (None, None)
    check(lib().nm_nerf_composite4(dptr(out4), dptr(t), dptr(rays), dptr(noise), float(noise_std), int(bool(white_bg)), R, S, Sa, dptr(rgb),
                                   dptr(depth), dptr(acc), dptr(w), stream()), "nm_nerf_composite4")
    return rgb, depth, acc, w


def composite_bwd(out4, t, rays, g_rgb, g_weights=None, noise=None, noise_std=0.0, white_bg=False, S_act=None, want_g_d=False):
    """-> g4 (n, 4) = d loss / d (logits, sigma); with want_g_d: (g4, g_d (R,3) = d loss / d rays[:, 3:6] through |d|)."""
    R, S = t.shape[0], t.shape[1] - 1
    Sa = S if S_act is None else int(S_act)
    g4 = torch.empty_like(out4)
    g_d = _new(R, 3, dev=t.device) if want_g_d else None
    g_rgb = g_rgb.contiguous()
    g_weights = None if g_weights is None else g_weights.contiguous()
    check(lib().nm_nerf_composite4_bwd(dptr(out4), dptr(t), dptr(rays), dptr(noise), float(noise_std), int(bool(white_bg)), dptr(g_rgb),
                                       dptr(g_weights), R, S, Sa, dptr(g4), dptr(g_d), stream()), "nm_nerf_composite4_bwd")
    return (g4, g_d) if want_g_d else g4
