"""What the tests of the NeRF render kernels share (imported by name, like pnp_util / supervision_util): the bars and their vocabulary,
seeded networks, ray and fence-post sources, the one launch of ops.nerf_fwd on a renderer's packed blob, the of-scale comparison, and the
forward / backward check of the pointwise kernel pair.  No fixture, no hook, no test; nothing here touches a GPU at import.

A test file keeps, as data, WHICH network, camera, slice of rays and seeds it uses; how they are built is here, once.

Networks that look alike and are not: `network(..., calibrate=False)` leaves the fp16x3 operand scales neutral (NeRF.packed: "scaled
weights, activations as they are"), so its fp16x3 blob holds other numbers than the calibrated network of the same seed.  The files that
always launched uncalibrated networks (test_nerf_paths_gpu, test_nerf_sample_math_gpu, the pointwise cases) keep doing so; they are cached
apart from the calibrated ones."""
import functools
from types import SimpleNamespace

import torch

from conftest import abs_bound
from nerfmatch_amd import inerf, ops, synth
from nerfmatch_amd.nerf.renderer import NerfRenderer
from oracle import nerf_oracle as no

DEV = torch.device("cuda:0")

# ----------------------------------------------------------------------------------------------- bars and vocabulary
TOL = 1e-4  # anything through the 8-layer MLP, of the tensor's scale max(1, max|reference|) (tests/test_nerf_gpu.py)
TOL_FP16X1 = 2e-3  # tests/test_nerf_gpu.py, test_single_product_render_error_stated: smooth field, of scale
SPLIT = ["fp16x3", "bf16x3"]  # the two operand splits of the 16-bit matrix-core kernel (fp16x3 = the default parity arithmetic)
KEYS = ("weights", "feat", "pts", "rgb", "depth", "acc")
PASSES = {
    "rgb_tap7": dict(tap_layer=7, need_rgb=True, need_feat=True),
    "rgb_tap3": dict(tap_layer=3, need_rgb=True, need_feat=True),
    "norgb_tap3": dict(tap_layer=3, need_rgb=False, need_feat=True),
    "norgb_nofeat": dict(tap_layer=-1, need_rgb=False, need_feat=False),
}
# (weights seed, pose seed) of the trained-like fixtures tests/golden/nerf_surf_w*_p*.npz
SURFACE_SEEDS = [(1, 21), (1, 22), (2, 23), (2, 24), (3, 25), (3, 26), (4, 27), (4, 28), (5, 29), (5, 30)]


def maxdiff(a, b):
    return (a.detach().cpu().float() - torch.as_tensor(b).float()).abs().max().item()


def relerr(a, b, what=None):
    """max |a - b| in units of the reference tensor's scale max(1, max|b|).  With `what`: the ABSOLUTE maximum is also held to its
    recorded bound (conftest.abs_bound: 1.5 x the value measured when tests/golden/abs_bounds.json was made) -- an of-scale bar alone
    could hide a drift on the trained-like fixtures, whose scales are 20 (activations) to 1e4 (densities)."""
    b = torch.as_tensor(b).float()
    d = maxdiff(a, b)
    if what is not None:
        abs_bound(what, d)
    return d / max(1.0, b.abs().max().item() if b.numel() else 1.0)


def tol_for(precision, case):
    """1e-4 everywhere, with ONE stated exception (round 3 finding): the bf16 split (16 mantissa bits) on the trained-like
    "surface" fixture -- densities of +-1e4 come out ~0.25 off, compositing weights up to 7e-4, rendered features 1.4e-4 of
    scale.  It is no longer the default; its bound there is 2e-3 and the measured values are printed."""
    return 2e-3 if (precision == "bf16x3" and case.startswith("surface")) else TOL


# ----------------------------------------------------------------------------------------------- networks
def make_renderer(fx, gpu, S=None):
    """the renderer of a golden fixture (tests/golden/nerf_*.npz), on the fp32 kernel"""
    app = bool(fx["app"])
    cfg = synth.nerf_config("cambridge" if app else "7scenes", num_pts=S or fx["S"], img_wh=(fx["W"], fx["H"]))
    ren = NerfRenderer(cfg, num_frames=5 if app else None, training=False, stop_layer=fx["stop_layer"])
    style = str(fx["style"]) if "style" in fx and str(fx["style"]) else None
    sd = synth.nerf_state_dict(seed=int(fx["weights_seed"]), app_vocab=5 if app else 0, density_bias=float(fx["density_shift"]) if (style and "density_shift" in fx) else (0.0 if style else 3.0), style=style)
    ren.load_state_dict(sd, strict=True)
    ren.precision = "fp32"  # the tests of the split kernels switch it explicitly (the class default is "fp16x3")
    return ren.to(gpu).eval(), sd


def renderer_for(scene, sd, calibrate):
    """eval-mode renderer on the GPU for a "7scenes" / "cambridge" state dict; calibrate: fp16x3 operand scales from the seeded probe bundle"""
    app = scene == "cambridge"
    ren = NerfRenderer(synth.nerf_config(scene, num_pts=64), num_frames=5 if app else None, training=False, stop_layer=3)
    ren.load_state_dict(sd, strict=True)
    ren.to(DEV).eval()
    if calibrate:
        ren.calibrate(DEV)
    return ren


@functools.lru_cache(maxsize=None)
def _network(scene, seed, style, density_bias, calibrate):
    app = scene == "cambridge"
    sd = synth.nerf_state_dict(seed=seed, app_vocab=5 if app else 0, density_bias=density_bias, style=style)
    return renderer_for(scene, sd, calibrate), sd, (sd["embedding_a.weight"][1].contiguous().to(DEV) if app else None)


def network(scene, seed, style=None, density_bias=None, calibrate=True):
    """(renderer, state dict, appearance row 1 on the GPU or None), built once per argument set and shared by every file that asks for it.
    density_bias: 3.0 for the smooth synth field, 0.0 with a weight style ("surface" brings its own) unless given.  A Cambridge network
    launched WITHOUT its row is this renderer with None for the row, not another build."""
    return _network(scene, seed, style, float((0.0 if style else 3.0) if density_bias is None else density_bias), calibrate)


# ----------------------------------------------------------------------------------------------- rays and fence posts
@functools.lru_cache(maxsize=None)
def camera_rays(*poses):
    """source 1, on the GPU: ops.raygen on the 480 x 640 synth camera at synth.camera_pose(q), 4800 rays per pose, poses concatenated"""
    return torch.cat([ops.raygen(synth.intrinsics(), synth.camera_pose(q), 480, 640, DEV)[0] for q in poses])


@functools.lru_cache(maxsize=None)
def oracle_rays(H, W, f, pose, ds):
    """source 2, on the CPU: the oracle's make_rays for an H x W pinhole camera of focal length f, every ds-th pixel"""
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    return no.make_rays(H, W, K, synth.camera_pose(pose), ds=ds).contiguous()


def fence_posts(rays, S, u):
    """stratified coarse fence posts of either source (rays on the GPU: ops.sample_coarse; on the CPU: the oracle's);
    u: the (R, S + 1) uniforms on the CPU, or the seed of synth.uniform01 for them"""
    if isinstance(u, int):
        u = synth.uniform01((rays.shape[0], S + 1), u)
    return ops.sample_coarse(rays, u.to(DEV), S) if rays.is_cuda else no.sample_coarse(rays, S, u)


# the coarse-pass files (tap7_early, gap_work, dma_gaps): row lengths at which the along-ray scan takes another form -- 32 (four rays per
# tile), 64 (a ray across two wavefronts), 128 (across the tile), 256 (two chunks), 96 (padded to 128) --, ray counts that leave a ragged tile
SHAPES = [(32, 5), (64, 3), (128, 2), (256, 2), (96, 2)]


def styled_network(style, app):
    """network() of the coarse-pass files: the smooth field at seed 7, a weight style ("surface") at seed 0"""
    return network("cambridge" if app else "7scenes", 0 if style else 7, style)


@functools.lru_cache(maxsize=None)
def oracle_bundle(S, R, style=None):
    """(rays, uniforms, resampling jitter, coarse fence posts) on the CPU for the first R rays of the coarse-pass files' camera"""
    # (the "surface" weights with the camera of their golden fixture, tests/golden/make_golden.py: every ray meets the surface)
    H, W, f, pose = (128, 256, 240.0, 11) if style else (128, 128, 100.0, 3)
    rays = oracle_rays(H, W, f, pose, 8)[:R].contiguous()
    t_rand, jit = synth.uniform01((R, S + 1), 100 + S), synth.resample_jitter((R, S + 1), 200 + S)
    return rays, t_rand, jit, fence_posts(rays, S, t_rand)


# ----------------------------------------------------------------------------------------------- launch and compare
def launch(ren, which, precision, rays, t, row=None, **kw):
    """ops.nerf_fwd on ren.nerf_coarse / ren.nerf_fine (which = "coarse" / "fine") packed for `precision`; CPU inputs go to the GPU"""
    blob = getattr(ren, f"nerf_{which}").packed(DEV, precision)
    with torch.no_grad():
        out = ops.nerf_fwd(blob, rays.to(DEV), t.to(DEV), None if row is None else row.to(DEV), **kw)
    if precision == "fp16x3":  # the guarded fp32 pass must not have rewritten what the caller is about
        assert not blob.nm_guard.read()[0], "an fp16x3 operand saturated: the outputs are the fp32 kernel's"
    return out


def coarse_run(precision, style, app, S, R, **kw):
    """the coarse half of styled_network(style, app) on oracle_bundle(S, R, style)"""
    ren, _, row = styled_network(style, app)
    rays, _, _, t = oracle_bundle(S, R, style)
    return launch(ren, "coarse", precision, rays, t, row, **kw)


def clear_winner(weights):
    """feat_comb max selects by an argmax over weights that agree to ~1e-6 between arithmetics: rays whose two best weights are closer
    than that may pick another sample in the two arithmetics -- the rays whose two best weights are further apart than 1e-4"""
    top2 = torch.as_tensor(weights).float().cpu().topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > 1e-4


def compare(out, ref, tol, feat_max, what, keys=KEYS):
    """every key of `out` within tol of the scale of `ref` (relerr), printed; feat_max: feat and pts on the clear winners only"""
    clear = clear_winner(ref["weights"]) if feat_max else None
    if feat_max:
        assert bool(clear.any()), f"{what}: no ray with a clear maximum-weight sample"
    for k in keys:
        a, b = out[k].detach().cpu().float(), torch.as_tensor(ref[k]).detach().cpu().float()
        a, b = a.reshape(b.shape[0], -1), b.reshape(b.shape[0], -1)
        if feat_max and k in ("feat", "pts"):
            a, b = a[clear], b[clear]
        err = relerr(a, b)
        print(f"{what} {k}: {err:.2e} of scale")
        assert err < tol, f"{what} {k}: {err:.2e}"


def check_repeats(runs, keys):
    """repeated launches of one case: the same bits in every output"""
    for k in keys:
        for again in runs[1:]:
            assert torch.equal(runs[0][k], again[k]), f"{k} differs between repeated launches"


def compare_repeated(runs, ref, tol, what):
    """a case of the schedule files: `runs` = the outputs (those that are not None) of repeated launches of one split kernel, `ref` = the
    fp32-MFMA kernel's on the same inputs"""
    assert float(ref["weights"].sum(-1).max()) > 0.3  # not vacuous
    keys = tuple(k for k in KEYS if k in ref)
    assert set(runs[0]) & set(KEYS) == set(keys)  # an output the reference does not have, the split kernel does not have either
    compare(runs[0], ref, tol, False, what, keys)
    check_repeats(runs, keys)


# ----------------------------------------------------------------------------------------------- pointwise kernel pair (iNeRF)
def points_bundle(R, seed):
    """R seeded rays, their 129 fence posts (on the GPU) and the generator that made them, for further draws"""
    S = 128
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g) * 0.2
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.full((R, 1), 0.01), torch.ones(R, 1), d, torch.full((R, 1), 0.002)], -1).to(DEV).contiguous()
    z = torch.sort(torch.rand(R, S + 1, generator=g) * 0.9 + 0.05, dim=-1).values.to(DEV).contiguous()
    return rays, z, g


def points_case(app, R, seed):
    """rays / fence posts of a small bundle + the (uncalibrated) network whose fine half the GEMM chain and the fused kernels evaluate"""
    ren, _, app_row = network("cambridge" if app else "7scenes", seed, calibrate=False)
    rays, z, g = points_bundle(R, seed)
    return ren, rays, z, app_row, g


def points_pair(fused, chain, rays, z, Sa, app_row, tap, g, repeats):
    """nm_nerf_points_fwd_rays_bf16x3 with a tap / nm_nerf_points_bwd_tap_bf16x3 (inerf.FusedField) against the fp32 GEMM chain
    (inerf.FineField) on the first Sa samples of every ray, once: tapped activations and outputs at 1e-5 of scale, then d loss / d (xi, xd)
    for seeded upstream gradients drawn from g, one of them entering at the tapped layer as w_n . g_pt_feat[ray]; `repeats` further
    launches of both kernels give the same bits.  The gradients are returned finite and unjudged: their bars are statements about many
    rows (test_tapped_points_kernels_vs_gemm_chain) and belong to the caller."""
    R, gpu = rays.shape[0], rays.device
    n = R * Sa
    xi, xd = inerf._encode(rays, z, Sa, app_row)
    logit, sig, saved = chain.forward(xi, xd)
    out4, gates, feats = fused.forward_rays(rays, z, Sa, app_row, tap)
    h_ref = saved[0][tap]
    assert feats.shape == (n, 256)
    assert (feats - h_ref).abs().max().item() < 1e-5 * max(1.0, h_ref.abs().max().item())
    assert (out4[:, :3] - logit[:, :3]).abs().max().item() < 1e-5 * max(1.0, logit.abs().max().item())
    assert (out4[:, 3] - sig[:, 0]).abs().max().item() < 1e-5 * max(1.0, sig.abs().max().item())
    g_logit = torch.zeros(n, 8, device=gpu)
    g_logit[:, :3] = torch.randn(n, 3, generator=g).to(gpu) * 1e-4
    g_sig = torch.zeros(n, 8, device=gpu)
    g_sig[:, 0] = torch.randn(n, generator=g).to(gpu) * 1e-5
    w = torch.rand(R, Sa, generator=g).to(gpu) * 0.1
    g_pf = torch.randn(R, 256, generator=g).to(gpu) * 1e-3
    g_feats = (w.reshape(n, 1) * g_pf.repeat_interleave(Sa, 0)).contiguous()
    gxi_ref, gxd_ref = chain.backward(g_logit, g_sig, saved, (tap, g_feats))
    g4 = torch.cat([g_logit[:, :3], g_sig[:, :1]], 1).contiguous()
    (a0, a5), gxd = fused.backward(g4, gates, (tap, w, g_pf))
    gxi = a0 + a5
    assert torch.isfinite(gxi).all() and torch.isfinite(gxd).all()
    for _ in range(repeats):
        out4_b, gates_b, feats_b = fused.forward_rays(rays, z, Sa, app_row, tap)
        assert torch.equal(out4_b, out4) and torch.equal(gates_b, gates) and torch.equal(feats_b, feats)
        (b0, b5), bxd = fused.backward(g4, gates, (tap, w, g_pf))
        assert torch.equal(b0, a0) and torch.equal(b5, a5) and torch.equal(bxd, gxd)
    return SimpleNamespace(out4=out4, gates=gates, feats=feats, h_ref=h_ref, g4=g4, w=w, g_pf=g_pf,
                           grads=((gxi, gxi_ref), (gxd, gxd_ref)))
