"""Test helper (not product code): one NeRF training step composed from the oracle's primitives in plain torch, dtype selectable.

Follows NerfRenderer.render_rays(validation=False) (nerfmatch/nerf/renderer.py:182-295), volume_render_radiance_field with the
training-time density noise (nerf/render_utils.py:176-230), t_to_s with g's in-place eps (:618-636) and compute_nerf_metrics
(nerfmatch/utils/metrics.py:59-96, :448-465).  The samplers run without gradient, as in the reference."""
import torch

from oracle import nerf_oracle as no

NETS = ("nerf_coarse", "nerf_fine")


def t_to_s(t):
    """(g(t) - g(near)) / (g(far) - g(near)) with g(x) = 1 / (x + 1e-6) adding its eps IN PLACE: `near` has the eps once in the numerator
    and twice in the denominator (the tensor `t` itself ends up shifted too, which nothing reads afterwards)."""
    eps = 1e-6
    near, far = t.min(), t.max()
    tt = t + eps
    n1 = near + eps
    f1 = far + eps
    n2 = n1 + eps
    return (1 / tt - 1 / n1) / (1 / f1 - 1 / n2)


def lossfun_distortion(s, w):
    ut = (s[..., 1:] + s[..., :-1]) / 2
    dut = torch.abs(ut[..., :, None] - ut[..., None, :])
    inter = torch.sum(w * torch.sum(w[..., None, :] * dut, dim=-1), dim=-1)
    intra = torch.sum(w**2 * (s[..., 1:] - s[..., :-1]), dim=-1) / 3
    return inter + intra


def encode(rays, t, ray_id=None, table=None, var_scale=-1.0):
    """-> x_pts (n,90), x_dir (n,27), x_app (n,16) or None: the inputs of nerf_mlp for every sample of every ray."""
    o, d, view, radii = rays[:, :3], rays[:, 3:6], rays[:, 8:11], rays[:, 11:12]
    mean, var = no.frustum_gaussians(t, o, d, radii)
    if var_scale > 0:
        var = var_scale * var
    R, S = mean.shape[:2]
    x_pts = no.ipe(mean.reshape(-1, 3), var.reshape(-1, 3), 15)
    x_dir = no.dir_pe(view[:, None, :].expand(R, S, 3).reshape(-1, 3), 4)
    x_app = None
    if table is not None:
        ids = torch.ones(R, dtype=torch.long) if ray_id is None else ray_id
        x_app = table[ids][:, None, :].expand(R, S, table.shape[1]).reshape(R * S, -1)
    return x_pts, x_dir, x_app


def train_step(*a, **kw):
    """_train_step with gradients enabled (the suite runs every test under no_grad)."""
    with torch.enable_grad():
        return _train_step(*a, **kw)


def _train_step(sd, rays, gt, t_rand=None, jitter=None, noise_coarse=None, noise_fine=None, noise_std=0.0, white_bg=False, ray_id=None,
               mask=None, coarse_weight=1.0, ray_reg_weight=0.0, var_scale=-1.0, t_coarse=None, t_fine=None, dtype=torch.float64,
               backward=True):
    """sd: state dict (reference key names); `embedding_a.weight` present = appearance on.  t_coarse / t_fine given: those fence posts are
    used instead of the samplers' (the gradient is then evaluated at another implementation's samples).
    -> dict(preds, loss, metrics, grads {name: d loss / d parameter}, t_coarse, t_fine, weights_coarse)."""
    cast = lambda x: None if x is None else x.detach().to(dtype)
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    table = P.get("embedding_a.weight")
    rays, gt, mask = cast(rays), cast(gt), cast(mask)
    S = (t_rand if t_rand is not None else t_coarse).shape[1] - 1
    d = rays[:, 3:6]
    preds, w = {}, None
    out = {}
    for key in ("coarse", "fine"):
        with torch.no_grad():
            if key == "coarse":
                t = cast(t_coarse) if t_coarse is not None else no.sample_coarse(rays, S, cast(t_rand))
            else:
                t = cast(t_fine) if t_fine is not None else no.resample(t, w.detach(), cast(jitter), padding=0.01, randomized=True)
            x_pts, x_dir, _ = encode(rays, t, var_scale=var_scale)
        x_app = None
        if table is not None:
            ids = torch.ones(rays.shape[0], dtype=torch.long) if ray_id is None else ray_id
            x_app = table[ids][:, None, :].expand(-1, S, -1).reshape(rays.shape[0] * S, -1)
        raw, _ = no.nerf_mlp(P, f"nerf_{key}", x_pts, x_dir, x_app)
        raw = raw.reshape(rays.shape[0], S, 4)
        noise = noise_coarse if key == "coarse" else noise_fine
        if noise is not None and noise_std > 0:
            raw = torch.cat([raw[..., :3], (raw[..., 3] + cast(noise) * noise_std)[..., None]], -1)
        rgb, depth, acc, w = no.composite(raw, t, d, white_bg)
        preds[f"rgb_{key}"], preds[f"depth_{key}"] = rgb, depth
        out[f"t_{key}"], out[f"weights_{key}"] = t, w
    preds["s_fine"], preds["weights_fine"] = t_to_s(out["t_fine"]), w
    m = 1 if mask is None else mask.reshape(-1, 1)
    mse_c = 0.5 * (m * (preds["rgb_coarse"] - gt) ** 2).mean()
    mse_f = 0.5 * (m * (preds["rgb_fine"] - gt) ** 2).mean()
    loss = mse_c * coarse_weight + mse_f
    dist = torch.mean(lossfun_distortion(preds["s_fine"], preds["weights_fine"]))
    if ray_reg_weight:
        loss = loss + dist * ray_reg_weight
    metrics = dict(rgb_coarse_mse=mse_c, rgb_fine_mse=mse_f, rgb_coarse_psnr=-10 * torch.log10(mse_c), rgb_fine_psnr=-10 * torch.log10(mse_f),
                   distortion=dist, loss=loss)
    grads = {}
    if backward:
        names = [k for k in P if k.startswith(NETS) or k == "embedding_a.weight"]
        gs = torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)
        grads = {k: (torch.zeros_like(P[k]) if g is None else g).detach() for k, g in zip(names, gs)}
    out.update(preds={k: v.detach() for k, v in preds.items()}, loss=loss.detach(), metrics={k: v.detach() for k, v in metrics.items()}, grads=grads)
    return out


def net_l2(got, want, net):
    """relative L2 distance of all gradient tensors of one network (names starting with `net`) taken as one vector"""
    num = sum(float(((got[k].double() - want[k].double()) ** 2).sum()) for k in want if k.startswith(net))
    den = sum(float((want[k].double() ** 2).sum()) for k in want if k.startswith(net))
    return (num / den) ** 0.5
