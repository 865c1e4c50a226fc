"""CPU: pins the oracle (oracle/) to golden vectors produced by the reference itself
(tests/golden/make_golden.py).  Tolerances: the oracle uses the same torch-CPU kernels as the
reference, so everything is expected to agree to ~1e-6 (bit-exact for indices)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from nerfmatch_amd import synth
from oracle import nerf_oracle as no
from oracle import matcher_oracle as mo

NERF_CASES = ["r32_s32", "r128_s64_app", "r32_s32_last", "surface_r512_s128", "surface_r256_s64_app"]


def close(a, b, tol=1e-6):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= tol * max(1.0, b.abs().max().item() if b.numel() else 1.0), err


def nerf_params(fx):
    style = str(fx["style"]) if "style" in fx and str(fx["style"]) else None
    return synth.nerf_state_dict(seed=int(fx["weights_seed"]), app_vocab=5 if fx["app"] else 0, density_bias=float(fx["density_shift"]) if (style and "density_shift" in fx) else (0.0 if style else 3.0),
                                 style=style)


@pytest.mark.parametrize("case", NERF_CASES)
def test_rays(case):
    fx = load_golden(f"nerf_{case}")
    rays = no.make_rays(fx["H"], fx["W"], fx["K"], fx["c2w_norm"], ds=8)
    close(rays, fx["rays"], 1e-6)


def test_far_fallback():
    fx = load_golden("nerf_far_fallback")
    rays = no.make_rays(fx["H"], fx["W"], fx["K"], fx["c2w"], ds=8)
    assert torch.all(rays[:, 7] == 1.0)
    close(rays, fx["rays"], 1e-6)


@pytest.mark.parametrize("case", NERF_CASES)
def test_sampling_and_encoding(case):
    fx = load_golden(f"nerf_{case}")
    rays, S, n = fx["rays"], fx["S"], fx["sub_rays"]
    t = no.sample_coarse(rays, S, fx["t_rand"])
    close(t, fx["t_coarse"], 0)
    mean, var = no.frustum_gaussians(t, rays[:, :3], rays[:, 3:6], rays[:, 11:12])
    close(mean[:n], fx["mean_coarse"], 0)
    close(var[:n], fx["var_coarse"], 0)
    close(no.ipe(mean[:n].reshape(-1, 3), var[:n].reshape(-1, 3), 15), fx["ipe_coarse"], 0)
    close(no.dir_pe(rays[:, 8:11], 4), fx["dir_pe"], 0)
    t2 = no.resample(fx["t_coarse"], fx["comp_weights"], fx["jitter"])
    close(t2, fx["t_fine"], 0)
    mean2, var2 = no.frustum_gaussians(t2, rays[:, :3], rays[:, 3:6], rays[:, 11:12])
    close(mean2[:n], fx["mean_fine"], 0)
    close(var2[:n], fx["var_fine"], 0)
    # quirk 2 of SURVEY 8a: about half of the re-sampled fence posts collapse onto the last edge
    frac_last = (t2 == t2[:, -1:]).float().mean().item()
    assert 0.3 < frac_last < 0.6
    assert torch.all(t2[:, 1:] >= t2[:, :-1])


@pytest.mark.parametrize("case", NERF_CASES)
def test_mlp_and_composite(case):
    fx = load_golden(f"nerf_{case}")
    p = nerf_params(fx)
    rays, S, n = fx["rays"], fx["S"], fx["sub_rays"]
    view = rays[:n, 8:11][:, None, :].expand(n, S, 3).reshape(-1, 3)
    app = fx["app_row"].view(1, -1).expand(n * S, -1) if fx["app"] else None
    raw_f, feat_f = no.nerf_mlp(p, "nerf_fine", fx["ipe_coarse"], no.dir_pe(view, 4), app, stop_layer=fx["stop_layer"])
    raw_c, feat_c = no.nerf_mlp(p, "nerf_coarse", fx["ipe_coarse"], no.dir_pe(view, 4), app, stop_layer=-1)
    close(raw_f, fx["mlp_raw_fine"], 1e-6)
    close(feat_f, fx["mlp_feat_fine"], 1e-6)
    close(raw_c, fx["mlp_raw_coarse"], 1e-6)
    close(feat_c, fx["mlp_feat_coarse"], 1e-6)
    assert (raw_c[:, 3] > 0).float().mean() > 0.2  # the fixture is not vacuous: densities are active


@pytest.mark.parametrize("case", NERF_CASES)
def test_render_rays_and_novel_view(case):
    fx = load_golden(f"nerf_{case}")
    p = nerf_params(fx)
    kw = dict(stop_layer=fx["stop_layer"], white_bg=bool(fx["white_bg"]), app_row=fx["app_row"] if fx["app"] else None)
    out = no.render_rays(p, fx["rays"], fx["t_rand"], fx["jitter"], fx["S"], fx["S"], keep_raw=True, **kw)
    close(out["weights_coarse"], fx["comp_weights"], 1e-6)
    close(out["rgb_coarse"], fx["comp_rgb"], 1e-6)
    close(out["depth_coarse"], fx["comp_depth"], 1e-6)
    close(out["t_fine"], fx["t_fine"], 1e-6)
    for k in ("feat_coarse", "pts_coarse", "rgb_coarse", "depth_coarse", "feat_fine", "pts_fine", "rgb_fine", "depth_fine"):
        close(out[k], fx[f"pred_{k}"], 2e-6)
    assert out["weights_fine"].sum(-1).max() > 0.5
    if "fine_weights" in fx:  # the trained-like fixture also carries the fine pass's weights
        close(out["weights_fine"], fx["fine_weights"], 1e-6)
        close(out["acc_fine"], fx["fine_acc"], 1e-6)
    nv = no.render_novel_view(p, (fx["H"], fx["W"]), fx["K"], fx["c2w"], fx["unnorm"], fx["t_rand"], fx["jitter"],
                              fx["S"], fx["S"], **kw)
    close(nv["rays"], fx["rays"], 1e-6)
    close(nv["pt3d"], fx["nv_pt3d"], 2e-6)
    close(nv["pt_feat"], fx["nv_pt_feat"], 2e-6)
    close(nv["im_pred"], fx["nv_im_pred"], 2e-6)


def test_surface_fixture_is_trained_like():
    """The round-3 fixture really is a different numerical regime: hidden activations of O(10),
    densities in the thousands, opacity saturating within a few coarse samples, peaked fine weights."""
    fx = load_golden("nerf_surface_r512_s128")
    assert fx["rays"].shape[0] == 512 and int(fx["S"]) == 128
    assert fx["mlp_feat_coarse"].abs().max() > 10 and fx["mlp_feat_fine"].abs().max() > 4
    assert fx["mlp_raw_coarse"][:, 3].max() > 1000 and fx["mlp_raw_coarse"][:, 3].min() < -1000
    w = fx["comp_weights"]
    assert w.sum(-1).mean() > 0.99  # opaque scene
    assert (w > 0.01).sum(-1).float().median() <= 4  # alpha reaches 1 within 2-4 coarse samples
    assert w.max(-1)[0].median() > 0.5
    assert fx["pred_feat_coarse"].abs().max() > 10


# ----------------------------------------------------------------------------- matcher
def test_matcher_rows():
    fx = load_golden("matcher_c2f")
    p = synth.matcher_state_dict("c2f", seed=int(fx["weights_seed"]))
    c, h, w = fx["cfeat"].shape[1:]
    close(mo.sine_pe_table(c, h, w), fx["pe_table"], 0)
    close(mo.fourier_embed(fx["pt3d"]), fx["fourier_pt3d"], 0)
    close(mo.encoder_layer(p, "pt_sa.layers.0", fx["enc_self_in"]), fx["enc_self_out"], 1e-6)
    close(mo.encoder_layer(p, "coarse_former", fx["enc_self_in"], fx["pt_feat"]), fx["enc_cross_out"], 1e-6)
    close(mo.pixel_grid(w * 8, h * 8), fx["pt2d"][0], 0)


def test_lsa_layer():
    fx = load_golden("matcher_lsa")
    import numpy as np
    rng = np.random.default_rng(int(fx["weights_seed"]))
    sd = {}
    synth._encoder_layer(sd, rng, "L", 128)
    sd["L.attention.attend.scale"] = fx["scale"] if torch.is_tensor(fx["scale"]) else torch.tensor(fx["scale"])
    close(mo.encoder_layer(sd, "L", fx["x"], None, heads=8, att_type="lsa"), fx["y"], 1e-6)


@pytest.mark.parametrize("tag,mutual,thr,masked", [("mut", True, 0.0, False), ("nomut", False, 0.0, False),
                                                     ("mask", True, 0.0, True), ("thr", True, None, False),
                                                     ("empty", True, 0.5, False)])
def test_c2f_forward(tag, mutual, thr, masked):
    fx = load_golden("matcher_c2f")
    p = synth.matcher_state_dict("c2f", seed=int(fx["weights_seed"]))
    cfg = synth.matcher_config("c2f")
    thr = fx["thr"] if thr is None else thr
    imm = fx["im_mask_partial"] if masked else None
    ptm = fx["pt_mask_partial"] if masked else None
    out = mo.c2f_forward_match(p, cfg, fx["cfeat"], fx["ffeat"], fx["pt_feat"], fx["pt3d"], imm, ptm, mutual, thr)
    b, i, j = out["match_ids"]
    assert torch.equal(b, fx[f"{tag}_b_ids"]) and torch.equal(i, fx[f"{tag}_i_ids"]) and torch.equal(j, fx[f"{tag}_j_ids"])
    close(out["mconf"], fx[f"{tag}_mconf"], 1e-6)
    close(out["expec_f"], fx[f"{tag}_expec_f"], 1e-5)
    asm = mo.c2f_assemble(out, fx["pt2d"], fx["pt3d"])
    close(asm["mpt2d_f"], fx[f"{tag}_mpt2d_f"], 1e-5)
    close(asm["mpt2d_c"], fx[f"{tag}_mpt2d_c"], 0)
    close(asm["mpt3d"], fx[f"{tag}_mpt3d"], 0)
    if tag in ("mut", "mask"):
        close(out["conf_matrix"], fx[f"{tag}_conf"], 1e-6)
        close(out["im_cfeat"], fx[f"{tag}_im_cfeat"], 1e-6)
    if tag == "mut":
        close(out["im_tokens"].shape, out["im_tokens"].shape)


@pytest.mark.parametrize("tag,mutual,thr,masked", [("mut", True, 0.0, False), ("nomut", False, 0.0, False),
                                                     ("mask", True, 0.0, True), ("thr", True, None, False)])
def test_c2f_forward_peaked(tag, mutual, thr, masked):
    """Peaked-confidence regime, 320 x 352 tokens, run through the reference (tests/golden/matcher_peaked.npz)."""
    fx = load_golden("matcher_peaked")
    p = synth.matcher_state_dict("c2f", seed=int(fx["weights_seed"]), temperature=float(fx["temperature"]), style="aligned")
    cfg = synth.matcher_config("c2f")
    thr = float(fx["thr"]) if thr is None else thr
    imm = fx["im_mask_partial"] if masked else None
    ptm = fx["pt_mask_partial"] if masked else None
    out = mo.c2f_forward_match(p, cfg, fx["cfeat"], fx["ffeat"], fx["pt_feat"], fx["pt3d"], imm, ptm, mutual, thr)
    b, i, j = out["match_ids"]
    assert torch.equal(b, fx[f"{tag}_b_ids"]) and torch.equal(i, fx[f"{tag}_i_ids"]) and torch.equal(j, fx[f"{tag}_j_ids"])
    close(out["mconf"], fx[f"{tag}_mconf"], 1e-6)
    close(out["expec_f"], fx[f"{tag}_expec_f"], 1e-5)
    asm = mo.c2f_assemble(out, fx["pt2d"], fx["pt3d"])
    close(asm["mpt2d_f"], fx[f"{tag}_mpt2d_f"], 1e-5)
    close(asm["mpt3d"], fx[f"{tag}_mpt3d"], 0)
    if tag in ("mut", "mask"):
        close(out["conf_matrix"], fx[f"{tag}_conf"], 1e-6)
    if tag == "mut":  # the regime: >= 60 % of the rows are mutual matches whose row maximum is >= 0.2
        conf = fx["mut_conf"][0]
        M = conf.shape[0]
        assert len(i) >= 0.6 * M and (conf.max(1)[0] >= 0.2).float().mean() >= 0.6
        assert (fx["perm"][i] == j).sum() >= 0.85 * int(fx["n_plant"])


@pytest.mark.parametrize("tag,mutual", [("mut", True), ("nomut", False)])
def test_coarse_forward_peaked(tag, mutual):
    fx, fxc = load_golden("matcher_peaked"), load_golden("matcher_peaked_coarse")
    p = synth.matcher_state_dict("coarse", temperature=float(fxc["temperature"]))
    out = mo.coarse_forward_match(p, fx["cfeat"], fx["pt_feat"], mutual=mutual)
    b, i, j = out["match_ids"]
    assert torch.equal(b, fxc[f"{tag}_b_ids"]) and torch.equal(i, fxc[f"{tag}_i_ids"]) and torch.equal(j, fxc[f"{tag}_j_ids"])
    close(out["mconf"], fxc[f"{tag}_mconf"], 1e-6)
    if mutual:
        close(out["conf_matrix"], fxc["conf"], 1e-6)


@pytest.mark.parametrize("tag,mutual", [("mut", True), ("nomut", False)])
def test_coarse_forward(tag, mutual):
    fx = load_golden("matcher_coarse")
    p = synth.matcher_state_dict("coarse")
    out = mo.coarse_forward_match(p, fx["cfeat"], fx["pt_feat"], mutual=mutual)
    b, i, j = out["match_ids"]
    assert torch.equal(b, fx[f"{tag}_b_ids"]) and torch.equal(i, fx[f"{tag}_i_ids"]) and torch.equal(j, fx[f"{tag}_j_ids"])
    close(out["mconf"], fx[f"{tag}_mconf"], 1e-6)
    if mutual:
        close(out["conf_matrix"], fx["conf"], 1e-6)


@pytest.mark.parametrize("tag", ["7s", "cam_decay"])
def test_inerf_refinement_trajectory(tag):
    """oracle/inerf_oracle.py against the reference's own inerf_refinement (poses after every Adam step)."""
    from oracle import inerf_oracle as io
    from nerfmatch_amd import synth

    fx = load_golden(f"inerf_{tag}")
    app = bool(fx["app"])
    sd = synth.nerf_state_dict(seed=int(fx["weights_seed"]), app_vocab=5 if app else 0, density_bias=3.0)
    app_row = sd["embedding_a.weight"][1] if app else None
    un = fx["unnorm"]
    pose0 = un.inverse() @ fx["c2w_est0"]
    image = fx["image"][0].permute(1, 2, 0)
    n = int(fx["num_optim"])
    poses, losses = io.refine(sd, fx["K"], int(fx["H"]), int(fx["W"]), image, pose0, list(fx["t_rands"][:n]), list(fx["jitters"][:n]),
                              lrate=float(fx["lrate"]), lrdecay=bool(fx["lrdecay"]), app_row=app_row)
    got = torch.stack([un @ p for p in poses])
    want = fx["poses"]
    got = got[-want.shape[0]:]  # (with lr decay only the final pose is stored)
    assert (got - want).abs().max().item() < 2e-5
    assert all(np.isfinite(losses))


def test_inerf_match_loss_trajectory():
    """The `use_match_loss` branch (nerfmatch_evaluator.py:420-441): pose gradients of every step and the trajectory against
    the reference's own run (tests/golden/inerf_match.npz)."""
    from oracle import inerf_oracle as io
    from nerfmatch_amd import synth

    fx = load_golden("inerf_match")
    assert int(fx["use_match_loss"]) == 1
    seed = int(fx["weights_seed"])
    sd = synth.nerf_state_dict(seed=seed, app_vocab=0, density_bias=3.0)
    un = fx["unnorm"]
    pose0 = un.inverse() @ fx["c2w_est0"]
    n = int(fx["num_optim"])
    R = (int(fx["H"]) // 8) * (int(fx["W"]) // 8)
    match = dict(p=synth.matcher_state_dict("c2f", seed=seed), cfg=synth.matcher_config("c2f"), cfeat=fx["cfeat"], ffeat=fx["ffeat"], unnorm=un,
                 im_mask=torch.ones(1, R, dtype=torch.bool), pt_mask=torch.ones(1, R, dtype=torch.bool))
    grads = []
    poses, losses = io.refine(sd, fx["K"], int(fx["H"]), int(fx["W"]), fx["image"][0].permute(1, 2, 0), pose0, list(fx["t_rands"][:n]),
                              list(fx["jitters"][:n]), lrate=float(fx["lrate"]), match=match, grads=grads)
    want_g = fx["pose_grads"]
    # the matcher's Fourier features reach 2^14 x world coordinate: ONE ulp on the rendered points moves this gradient by
    # ~6e-3 of its size (measured), so only the first step -- identical inputs -- is comparable tightly; later steps start
    # from poses that differ in the last bit
    for j in range(n):
        scale = want_g[j].abs().max().item()
        assert (grads[j] - want_g[j]).abs().max().item() < (1e-5 if j == 0 else 2e-2) * scale, (j, grads[j], want_g[j])
    got = torch.stack([un @ p for p in poses])
    assert (got - fx["poses"]).abs().max().item() < 1e-4, (got - fx["poses"]).abs().max()
    # the matching term is not a rounding error of the photometric one
    g_photo = []
    io.refine(sd, fx["K"], int(fx["H"]), int(fx["W"]), fx["image"][0].permute(1, 2, 0), pose0, list(fx["t_rands"][:1]), list(fx["jitters"][:1]),
              lrate=float(fx["lrate"]), grads=g_photo)
    assert (g_photo[0] - want_g[0]).abs().max().item() > 1e-2 * want_g[0].abs().max().item()


def test_inerf_match_loss_trajectory_coarse_model():
    """Round 6: the matching term through the coarse-only model class (the reference's call works for either class,
    nerfmatch_evaluator.py:429-441; tests/golden/inerf_match_coarse.npz: synth.matcher_variant("coarse_full"))."""
    from oracle import inerf_oracle as io

    fx = load_golden("inerf_match_coarse")
    seed = int(fx["weights_seed"])
    sd = synth.nerf_state_dict(seed=seed, app_vocab=0, density_bias=3.0)
    un = fx["unnorm"]
    pose0 = un.inverse() @ fx["c2w_est0"]
    n = int(fx["num_optim"])
    R = (int(fx["H"]) // 8) * (int(fx["W"]) // 8)
    cfg, p = synth.matcher_variant("coarse_full", seed)
    match = dict(p=p, cfg=cfg, cfeat=fx["cfeat"], ffeat=None, unnorm=un, im_mask=torch.ones(1, R, dtype=torch.bool), pt_mask=torch.ones(1, R, dtype=torch.bool))
    grads = []
    poses, losses = io.refine(sd, fx["K"], int(fx["H"]), int(fx["W"]), fx["image"][0].permute(1, 2, 0), pose0, list(fx["t_rands"][:n]),
                              list(fx["jitters"][:n]), lrate=float(fx["lrate"]), match=match, grads=grads)
    want_g = fx["pose_grads"]
    for j in range(n):
        scale = want_g[j].abs().max().item()
        assert (grads[j] - want_g[j]).abs().max().item() < (1e-5 if j == 0 else 2e-2) * scale, (j, grads[j], want_g[j])
    got = torch.stack([un @ q for q in poses])
    assert (got - fx["poses"]).abs().max().item() < 1e-4, (got - fx["poses"]).abs().max()


def test_training_oracle_vs_reference_step():
    """The training oracle (losses, GT-padded match sampling, autograd gradients over the restated forward) against the
    reference's own training step (tests/golden/matcher_train.npz)."""
    import numpy as np

    from nerfmatch_amd import synth
    from oracle import train_oracle as to

    fx = load_golden("matcher_train")
    cfg = synth.matcher_config("c2f")
    with torch.enable_grad():
        p = {k: v.clone().requires_grad_() for k, v in synth.matcher_state_dict("c2f", seed=int(fx["weights_seed"])).items()}
        cfeat, ffeat, ptf = (fx[k].clone().requires_grad_() for k in ("cfeat", "ffeat", "pt_feat"))
        np.random.seed(int(fx["np_seed"]))
        out = to.c2f_train_step(p, cfg, cfeat, ffeat, ptf, fx["pt3d"], fx["pt2d"], fx["pt2d_proj"], fx["conf_gt"], fx["im_mask"], fx["pt_mask"])
        out["loss"].backward()
    assert abs(float(out["coarse_loss"]) - float(fx["coarse_loss"])) < 1e-6
    assert abs(float(out["fine_loss"]) - float(fx["fine_loss"])) < 1e-5
    ids = out["preds"]["match_ids"]
    assert torch.equal(ids[0], fx["b_ids"]) and torch.equal(ids[1], fx["i_ids"]) and torch.equal(ids[2], fx["j_ids"])
    assert out["preds"]["pred_num"] == int(fx["pred_num"])
    assert (cfeat.grad - fx["g_cfeat"]).abs().max() < 1e-6 * max(1.0, fx["g_cfeat"].abs().max().item())
    assert (ptf.grad - fx["g_pt_feat"]).abs().max() < 1e-6
    n = 0
    for key in fx:
        if key.startswith("gs__"):
            g = p[key[4:].replace("__", ".")].grad.flatten()
            mine = g if g.numel() <= 512 else g[::97]
            assert (mine - fx[key]).abs().max() <= 1e-5 * max(fx[key].abs().max().item(), 1e-3), key
            n += 1
    assert n >= 65


@pytest.mark.parametrize("tag,mutual", [("mut", True), ("nomut", False)])
def test_multi_pair_oracle_vs_reference(tag, mutual):
    """Top-k reference frames (forward_multi_pair, c2f_trainer.py:371-427 / coarse_trainer.py:290-336): the oracle's
    per-frame loop concatenated frame-major equals the reference's own run (B = 2 queries x k = 3 point sets)."""
    fx = load_golden("matcher_multipair")
    B, k, N = fx["pt3d"].shape[:3]
    p = synth.matcher_state_dict("c2f", seed=int(fx["weights_seed"]))
    cfg = synth.matcher_config("c2f")
    outs = []
    coarse = []
    for f in range(k):
        pr = mo.c2f_forward_match(p, cfg, fx["cfeat"], fx["ffeat"], fx["pt_feat"][:, f], fx["pt3d"][:, f], fx["im_mask"], fx["pt_mask"][:, f],
                                  mutual=mutual)
        b_ids, i_ids, j_ids = pr["match_ids"]
        mpt2d_c = fx["pt2d"][b_ids, i_ids]
        outs.append(dict(m_bids=b_ids, mpt2d_c=mpt2d_c, mpt3d=fx["pt3d"][:, f][b_ids, j_ids], mconf=pr["mconf"],
                         mpt2d_f=mpt2d_c + pr["expec_f"][:, :2] * 5 / 2 * 2))
        pc = mo.coarse_forward_match(synth.matcher_state_dict("coarse", seed=int(fx["weights_seed"])), fx["cfeat"], fx["pt_feat"][:, f],
                                     fx["im_mask"], fx["pt_mask"][:, f], mutual=mutual)
        coarse.append(pc)
    cat = lambda key: torch.cat([o[key] for o in outs])
    assert torch.equal(cat("m_bids"), fx[f"c2f_{tag}_m_bids"])
    close(cat("mpt3d"), fx[f"c2f_{tag}_mpt3d"], 0)
    close(cat("mpt2d_c"), fx[f"c2f_{tag}_mpt2d_c"], 0)
    close(cat("mconf"), fx[f"c2f_{tag}_mconf"], 1e-6)
    close(cat("mpt2d_f"), fx[f"c2f_{tag}_mpt2d_f"], 1e-6)
    for key, idx in (("b_ids", 0), ("i_ids", 1), ("j_ids", 2)):
        assert torch.equal(torch.cat([c["match_ids"][idx] for c in coarse]), fx[f"coarse_{tag}_{key}"])
    close(torch.cat([c["mconf"] for c in coarse]), fx[f"coarse_{tag}_mconf"], 1e-6)


def test_scene_cache_frame_oracle_vs_reference():
    """One frame of the scene-feature cache (nerf_evaluator.py:340-372): oracle render of the frame's ray bundle with the
    frame's appearance id, points un-normalised, colours clamped -- against the reference's predict + cache arithmetic."""
    fx = load_golden("scene_cache_frame")
    sd = synth.nerf_state_dict(seed=int(fx["weights_seed"]), app_vocab=5, density_bias=3.0)
    S = int(fx["S"])
    out = no.render_rays(sd, fx["rays"], fx["t_rand"], fx["jitter"], S, S, stop_layer=3, white_bg=True,
                         app_row=sd["embedding_a.weight"][int(fx["ts"][0])])
    close(no.unnormalize_points(out["pts_fine"], fx["unnorm"]), fx["frame_pt3d"], 1e-6)
    close(out["feat_fine"], fx["frame_pt_feat"], 1e-6)
    close(out["rgb_fine"].clamp(0, 1), fx["frame_pt_color"], 1e-6)


def test_fine_sample_count_is_ignored_by_the_mip_resampler():
    """coarse_nerf.num_pts = 32, fine_nerf.num_pts = 64: the reference's fine pass still has 32 samples (render_utils.py:299-309,
    :594-597; the fixture's generator asserted equality with the (32, 32) run).  The oracle reproduces that."""
    fx = load_golden("nerf_fine_count_c32_f64")
    sd = synth.nerf_state_dict(seed=int(fx["weights_seed"]), density_bias=3.0)
    out = no.render_rays(sd, fx["rays"], fx["t_rand"], fx["jitter"], int(fx["S_coarse"]), int(fx["S_fine"]), stop_layer=3)
    for k in ("feat_fine", "pts_fine", "rgb_fine", "depth_fine", "feat_coarse"):
        assert (out[k] - fx[f"pred_{k}"]).abs().max().item() < 1e-5, k


def test_post_norm_encoder_layer_oracle_vs_reference():
    """Round 5: the reference's post-norm layer (attention.py:209-221), self and cross attention."""
    import numpy as np
    from nerfmatch_amd import synth
    from oracle import matcher_oracle as mo

    fx = load_golden("matcher_postnorm")
    rng = np.random.default_rng(int(fx["weights_seed"]))
    for mode in ("self", "cross"):
        sd = {}
        synth._encoder_layer(sd, rng, "L", 256, cross=False)
        y = mo.encoder_layer_post_norm(sd, "L", fx[f"{mode}_x"], fx["cross_c"] if mode == "cross" else None)
        assert float((y - fx[f"{mode}_y"]).abs().max()) < 2e-6, mode


@pytest.mark.parametrize("name", synth.MATCHER_VARIANTS)
def test_option_envelope_oracle_vs_reference(name):
    """Round 6: option values beyond the shipped yamls (pt_ftype pe3d / pt3d + pt_proj, pt_pe_type "id", PE in front of the
    self-attention, pt_feat_norm) -- the oracle's general extract_pt_feat against the reference's own model classes
    (tests/golden/matcher_envelope.npz)."""
    fx = load_golden("matcher_envelope")
    cfg, p = synth.matcher_variant(name, int(fx["weights_seed"]))
    pf = (fx["feat128"] if name == "nerf128_id" else fx["feat256"]).clone()
    pt3d = fx["pt3d"].clone()
    close(mo.extract_pt_feat(p, cfg, pf.clone(), pt3d.clone()), fx[f"{name}_pt_tokens"], 2e-6)
    if name == "coarse_norm":
        out = mo.coarse_forward_match_cfg(p, cfg, fx["cfeat"], pf, pt3d, mutual=True)
        close(pt3d, fx[f"{name}_pt3d_after"], 1e-6)  # centred in place, like the reference's batch
        close(pf, fx[f"{name}_pt_feat_after"], 1e-6)
    else:
        out = mo.c2f_forward_match(p, cfg, fx["cfeat"], fx["ffeat"], pf, pt3d, mutual=True)
        close(out["expec_f"], fx[f"{name}_expec_f"], 1e-5)
        asm = mo.c2f_assemble(out, fx["pt2d"], pt3d)
        close(asm["mpt2d_f"], fx[f"{name}_mpt2d_f"], 1e-5)
        close(asm["mpt3d"], fx[f"{name}_mpt3d"], 0)
    b, i, j = out["match_ids"]
    assert torch.equal(i, fx[f"{name}_i_ids"]) and torch.equal(j, fx[f"{name}_j_ids"]) and len(i) > 5
    close(out["mconf"], fx[f"{name}_mconf"], 1e-6)
    close(out["conf_matrix"], fx[f"{name}_conf"], 1e-6)


@pytest.mark.parametrize("name", synth.FINE_VARIANTS)
def test_fine_envelope_oracle_vs_reference(name):
    """Fine-stage option values beyond the shipped yamls (window sides 3 / 4 / 7 / 8, 256-d fine features, 0 / 2 fine layers, lsa): the
    oracle against the reference's own NeRFMatcherMS (tests/golden/matcher_fine_envelope.npz) -- forward on the batch of 2 pairs and on
    pair 0 alone, the reference's float64 evaluation, and the GT-padded training step's windows."""
    fx = load_golden("matcher_fine_envelope")
    cfg, p = synth.fine_variant(name, int(fx["weights_seed"]))
    for pre, sl in (("", slice(0, 2)), ("p0_", slice(0, 1))):
        args = (fx["cfeat"][sl], fx["ffeat"][sl], fx["pt_feat"][sl].clone(), fx["pt3d"][sl].clone(), fx["im_mask"][sl], fx["pt_mask"][sl])
        out = mo.c2f_forward_match(p, cfg, *args, mutual=True)
        b, i, j = out["match_ids"]
        t = f"{name}_fwd_{pre}"
        assert torch.equal(b, fx[t + "b_ids"]) and torch.equal(i, fx[t + "i_ids"]) and torch.equal(j, fx[t + "j_ids"]) and len(i) > 20
        close(out["mconf"], fx[t + "mconf"], 1e-6)
        close(out["expec_f"], fx[t + "expec_f"], 1e-5)
        asm = mo.c2f_assemble(out, fx["pt2d"][sl], fx["pt3d"][sl], win_sz=cfg.win_sz)
        close(asm["mpt2d_f"], fx[t + "mpt2d_f"], 1e-5)
        close(asm["mpt3d"], fx[t + "mpt3d"], 0)
        # the reference in float64 found the same matches; the oracle in float64 agrees with it to rounding
        t64 = f"{name}_f64_{pre}"
        assert torch.equal(i, fx[t64 + "i_ids"]) and torch.equal(j, fx[t64 + "j_ids"])
        torch.set_default_dtype(torch.float64)
        try:
            o64 = mo.c2f_forward_match({k: v.double() for k, v in p.items()}, cfg, *(a.double() if a.is_floating_point() else a for a in args),
                                       mutual=True)
        finally:
            torch.set_default_dtype(torch.float32)
        assert torch.equal(o64["match_ids"][1], i) and torch.equal(o64["match_ids"][2], j)
        close(o64["expec_f"], fx[t64 + "expec_f"], 1e-12)
    # windows hang off the map: corner tokens are among the matches
    h, w = fx["cfeat"].shape[-2:]
    assert {0, w - 1, (h - 1) * w, h * w - 1} <= set(fx[f"{name}_fwd_i_ids"].tolist())
    # training step: the same GT-padded windows from the same numpy draws
    np.random.seed(int(fx["np_seed"]))
    out = mo.c2f_forward_match(p, cfg, fx["cfeat"], fx["ffeat"], fx["pt_feat"].clone(), fx["pt3d"].clone(), fx["im_mask"], fx["pt_mask"],
                               conf_gt=fx["conf_gt"])
    t = f"{name}_trn_"
    b, i, j = out["match_ids"]
    assert torch.equal(b, fx[t + "b_ids"]) and torch.equal(i, fx[t + "i_ids"]) and torch.equal(j, fx[t + "j_ids"])
    assert out["pred_num"] == int(fx[t + "pred_num"])
    close(out["expec_f"], fx[t + "expec_f"], 1e-5)
