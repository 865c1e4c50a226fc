"""GPU: nm_pnp_ransac (csrc/pnp.hip) through pnp_gpu.solve_pnp_batch and the evaluator's solver="gpu", against the float64 restatement
tests/pnp_util.py (written from the papers; the reference calls third-party solvers and has no counterpart).

Two measured bounds, from the restatement alone (no kernel involved; recorded in pnp_util.py, re-measured by test_pnp_cpu.py::test_recorded_bounds,
DESIGN.md section 3.8b):
  HYP_BOUND_PX  = 4 x 5.22e-3 px: the largest residual of a restatement hypothesis' own three sample points after its K [R | t] is rounded
                  to float32, over the 540 hypotheses of the scenes of HYP_RUNS (a few ill-conditioned samples with a point close to the
                  camera set it; the median is 2.3e-5 px, the 99th percentile 5.4e-4 px); x 4 for the kernel's different operation order.
  POSE_BOUND    = 4 x (3.28e-6 deg, 1.35e-7 scene units): the distance between the restatement's refinement run in float32 and in float64
                  from the same winning hypothesis on the sigma = 0.5 px scene of pose_scenes().
"""
import numpy as np
import pytest
import torch

import pnp_util as pu
from nerfmatch_amd import pnp_gpu
from nerfmatch_amd.utils.metrics import POSE_THRES

pytestmark = pytest.mark.gpu

HYP_BOUND_PX = 4 * pu.HYP_RESIDUAL_F32_PX
POSE_BOUND = (4 * pu.LM_F32_VS_F64[0], 4 * pu.LM_F32_VS_F64[1])
T_THRES, R_THRES = min(t for v in POSE_THRES.values() for t, _ in v) / 100.0, min(r for v in POSE_THRES.values() for _, r in v)  # 5 cm (scene unit: m), 5 deg
SEED = 5


def hyp_scene(n):
    return pu.make_scene(n, sigma=0.5, outlier_frac=0.3 if n >= 63 else 0.0, seed=100 + n)


HYP_RUNS = (((4, 5, 63, 65), 64), ((300,), 256), ((1100,), 64))  # (match counts of the batch, n_hyps): Q = 4 and Q = 1


def pose_scenes():
    return [pu.make_scene(300, 0.0, 0.0, seed=31), pu.make_scene(300, 0.0, 0.5, seed=32), pu.make_scene(300, 0.0, 0.8, seed=33),
            pu.make_scene(300, 0.5, 0.5, seed=34)]


def run(scenes, gpu, **kw):
    """One solve_pnp_batch call over the scenes as a batch (host counts)."""
    cat = lambda k, w: torch.from_numpy(np.concatenate([s[k].reshape(-1, w) for s in scenes]).astype(np.float32)).to(gpu)
    K = torch.from_numpy(np.stack([s["K"] for s in scenes])).to(gpu)
    out = pnp_gpu.solve_pnp_batch(cat("pt2d", 2), cat("pt3d", 3), [len(s["pt2d"]) for s in scenes], K, want_inliers=True, **kw)
    torch.cuda.synchronize()
    return out


def split(t, scenes):
    return torch.split(t, [len(s["pt2d"]) for s in scenes])


@pytest.fixture(scope="module")
def hyp_runs(gpu, built_lib):
    """[(scene, hyp_pose (n_hyps, 12) float64, hyp_count (n_hyps,), restatement P list, restatement flags, sample indices)]"""
    rows = []
    for counts, n_hyps in HYP_RUNS:
        scenes = [hyp_scene(n) for n in counts]
        w2c, n_inl, mask, (hp, hc) = run(scenes, gpu, n_hyps=n_hyps, seed=SEED, study=True)
        for q, s in enumerate(scenes):
            n = len(s["pt2d"])
            idx = [pu.sample_indices(SEED, h, n) for h in range(n_hyps)]
            ref = [pu.hypothesis(s["pt2d"], s["pt3d"], s["K"], i) for i in idx]
            rows.append(dict(scene=s, P=hp[q].cpu().numpy().astype(np.float64).reshape(n_hyps, 3, 4), count=hc[q].cpu().numpy(), idx=idx,
                             ref_P=[r[0] for r in ref], flag=[bool(r[1]) for r in ref], w2c=w2c[q].cpu().numpy(), n_inl=int(n_inl[q])))
    return rows


def test_hypotheses_fit_their_samples(hyp_runs):
    """1. every finite hypothesis reprojects its own three sample points (indices from the restatement's hash) within HYP_BOUND_PX; the set
    of finite hypotheses is the restatement's, except for samples the restatement flags as degenerate -- at most 2 % of them."""
    total = flagged = 0
    worst = 0.0
    for r in hyp_runs:
        s = r["scene"]
        for h, idx in enumerate(r["idx"]):
            total += 1
            fin = bool(np.all(np.isfinite(r["P"][h])))
            assert fin or bool(np.all(np.isnan(r["P"][h])))  # all or nothing
            if r["flag"][h]:
                flagged += 1
            else:
                assert fin == (r["ref_P"][h] is not None), (len(s["pt2d"]), h, idx)
            if fin:
                res = pu.residuals_P(r["P"][h], s["pt2d"][idx[:3]], s["pt3d"][idx[:3]])
                worst = max(worst, float(res.max()))
    print(f"{total} hypotheses, {flagged} flagged degenerate by the restatement, worst own-sample residual {worst:.3e} px (bound {HYP_BOUND_PX:.3e})")
    assert flagged <= 0.02 * total
    assert worst <= HYP_BOUND_PX


def test_counts_equal_the_float64_recount(hyp_runs):
    """2. hyp_count against the float64 recount under the GPU's own hyp_pose: they may differ by at most the number of the query's points
    whose float64 residual lies within 1e-3 px of the threshold."""
    slack_used = 0
    for r in hyp_runs:
        s = r["scene"]
        for h in range(len(r["idx"])):
            if not np.all(np.isfinite(r["P"][h])):
                assert r["count"][h] == 0
                continue
            res = pu.residuals_P(r["P"][h], s["pt2d"], s["pt3d"])
            want, near = int(np.sum(res <= 1.0)), int(np.sum(np.abs(res - 1.0) <= 1e-3))
            assert abs(int(r["count"][h]) - want) <= near, (len(s["pt2d"]), h, int(r["count"][h]), want, near)
            slack_used += abs(int(r["count"][h]) - want)
    print(f"counts off by {slack_used} in total (all inside the 1e-3 px band)")


def test_winner_is_the_argmax_of_the_key(gpu, hyp_runs):
    """3. with refine_iters = 0 the returned pose is the orthonormalised K^-1 P of the hypothesis that maximises (count << 32) | (~h)."""
    i = 0
    for counts, n_hyps in HYP_RUNS:
        scenes = [hyp_scene(n) for n in counts]
        w2c, n_inl, _ = run(scenes, gpu, n_hyps=n_hyps, seed=SEED, refine_iters=0)
        for q, s in enumerate(scenes):
            r = hyp_runs[i]
            i += 1
            win = int(np.argmax([pu.win_key(c, h) for h, c in enumerate(r["count"])]))
            if r["count"][win] < 4:
                assert int(n_inl[q]) < 4
                continue
            R, t = pu.pose_from_P(r["P"][win], s["K"].astype(np.float64))
            got = w2c[q].cpu().numpy()
            assert np.abs(got[:3, :3] - R).max() < 1e-6 and np.abs(got[:3, 3] - t).max() < 1e-6 * max(1.0, np.abs(t).max()), (len(s["pt2d"]), win)


def test_pose_against_truth_and_the_restatement(gpu, built_lib):
    """4. sigma = 0 with 0 / 50 / 80 % outliers: the inlier mask is the true inlier set; sigma = 0.5 px with 50 %: the pose stays within
    POSE_BOUND of the restatement's float64 refinement from the same winning hypothesis.  Every pose is inside the tightest POSE_THRES bin."""
    scenes = pose_scenes()
    w2c, n_inl, mask, (hp, hc) = run(scenes, gpu, n_hyps=256, seed=SEED, study=True)
    masks = split(mask, scenes)
    for q, s in enumerate(scenes):
        got = w2c[q].cpu().numpy().astype(np.float64)
        dR, dt = pu.c2w_err(s["R"], s["t"], got[:3, :3], got[:3, 3])
        print(f"scene {q}: {int(n_inl[q])} inliers of {int(s['inlier'].sum())} true, error to the truth {dR:.2e} deg / {dt:.2e}")
        assert dR < R_THRES and dt < T_THRES
        if q < 3:
            assert np.array_equal(masks[q].cpu().numpy(), s["inlier"]) and int(n_inl[q]) == int(s["inlier"].sum())
        else:
            counts = hc[q].cpu().numpy()
            win = int(np.argmax([pu.win_key(c, h) for h, c in enumerate(counts)]))
            K = s["K"].astype(np.float64)
            R0, t0 = pu.pose_from_P(hp[q, win].cpu().numpy().astype(np.float64).reshape(3, 4), K)
            R, t, m = pu.lm_refine(R0, t0, s["pt2d"], s["pt3d"], K, 1.0, 10)
            eR, et = pu.pose_distance(R, t, got[:3, :3], got[:3, 3])
            rR, rt = pu.c2w_err(s["R"], s["t"], R, t)
            print(f"  to the restatement: {eR:.2e} deg / {et:.2e} (bound {POSE_BOUND[0]:.1e} / {POSE_BOUND[1]:.1e}); restatement to the truth {rR:.2e} / {rt:.2e}")
            assert eR <= POSE_BOUND[0] and et <= POSE_BOUND[1]
            assert rR < R_THRES and rt < T_THRES
            assert int(np.sum(m != masks[q].cpu().numpy())) == 0


def test_batch_invariance(gpu, built_lib):
    """5. match counts (0, 3, 300, 1100), different scenes and intrinsics: every query's pose, inlier count and mask are the same bits alone,
    in the batch, in the reversed batch and on a second call; another seed gives other hypotheses."""
    scenes = [pu.make_scene(0, seed=50), pu.make_scene(3, seed=51), pu.make_scene(300, 0.5, 0.5, seed=52), pu.make_scene(1100, 0.5, 0.3, seed=53)]
    kw = dict(n_hyps=64, seed=SEED, study=True)
    w2c, n_inl, mask, (hp, hc) = run(scenes, gpu, **kw)
    assert n_inl.tolist()[:2] == [0, 0] and int(n_inl[2]) > 100 and int(n_inl[3]) > 500
    masks = split(mask, scenes)
    for q, s in enumerate(scenes):
        a_w2c, a_inl, a_mask, (a_hp, a_hc) = run([s], gpu, **kw)
        assert torch.equal(a_w2c[0], w2c[q]) and torch.equal(a_inl[0], n_inl[q]) and torch.equal(a_mask, masks[q])
        assert torch.equal(a_hc[0], hc[q]) and torch.equal(a_hp[0].view(torch.int32), hp[q].view(torch.int32))
    r_w2c, r_inl, r_mask, _ = run(scenes[::-1], gpu, **kw)
    r_masks = split(r_mask, scenes[::-1])
    for q in range(4):
        assert torch.equal(r_w2c[3 - q], w2c[q]) and torch.equal(r_inl[3 - q], n_inl[q]) and torch.equal(r_masks[3 - q], masks[q])
    b_w2c, b_inl, b_mask, (b_hp, _) = run(scenes, gpu, **kw)
    assert torch.equal(b_w2c, w2c) and torch.equal(b_inl, n_inl) and torch.equal(b_mask, mask) and torch.equal(b_hp.view(torch.int32), hp.view(torch.int32))
    _, _, _, (c_hp, _) = run(scenes, gpu, n_hyps=64, seed=SEED + 1, study=True)
    assert not torch.equal(c_hp[2:].view(torch.int32), hp[2:].view(torch.int32))
    # the same batch through sorted per-match query ids (offsets built on the device)
    bids = torch.cat([torch.full((len(s["pt2d"]),), q, dtype=torch.int64) for q, s in enumerate(scenes)]).to(gpu)
    cat = lambda k, w: torch.from_numpy(np.concatenate([s[k].reshape(-1, w) for s in scenes]).astype(np.float32)).to(gpu)
    i_w2c, i_inl, i_mask = pnp_gpu.solve_pnp_batch(cat("pt2d", 2), cat("pt3d", 3), bids, torch.from_numpy(np.stack([s["K"] for s in scenes])).to(gpu),
                                                   n_hyps=64, seed=SEED, want_inliers=True)
    assert torch.equal(i_w2c, w2c) and torch.equal(i_inl, n_inl) and torch.equal(i_mask, mask)


def test_degenerate_inputs(gpu, built_lib):
    """6. fewer than 4 matches, only outliers, identical 3-D points, points behind the camera, and center_subpixel."""
    base = pu.make_scene(65, 0.0, 0.0, seed=60)
    rng = np.random.default_rng(61)
    few = {**base, "pt2d": base["pt2d"][:3], "pt3d": base["pt3d"][:3]}
    outl = {**base, "pt2d": np.stack([rng.uniform(0, 640, 65), rng.uniform(0, 480, 65)], 1).astype(np.float32)}
    same = {**base, "pt3d": np.repeat(base["pt3d"][:1], 65, axis=0)}
    # 40 good matches + 25 whose 3-D point is mirrored through the camera centre: the same pixel, negative depth
    c = -base["R"].T @ base["t"]
    behind = {**base, "pt3d": base["pt3d"].copy()}
    behind["pt3d"][40:] = (2 * c - base["pt3d"][40:].astype(np.float64)).astype(np.float32)
    scenes = [few, outl, same, behind]
    w2c, n_inl, mask, (hp, hc) = run(scenes, gpu, n_hyps=64, seed=SEED, study=True)
    masks = split(mask, scenes)
    assert int(n_inl[0]) == 0 and torch.equal(w2c[0], torch.eye(4, device=gpu)) and not masks[0].any() and torch.isnan(hp[0]).all()
    assert int(n_inl[1]) <= 8 and int(hc[1].max()) <= 8  # 3 sample points + a few chance hits
    assert torch.isnan(hp[2]).all() and int(n_inl[2]) == 0 and torch.equal(w2c[2], torch.eye(4, device=gpu)) and not masks[2].any()
    assert int(n_inl[3]) == 40 and masks[3][:40].all() and not masks[3][40:].any()
    got = w2c[3].cpu().numpy().astype(np.float64)
    dR, dt = pu.c2w_err(base["R"], base["t"], got[:3, :3], got[:3, 3])
    assert dR < 1e-3 and dt < 1e-4
    assert (hc[3] <= 40).all()  # no hypothesis counts a point behind its camera: the 25 mirrored points project onto their pixels
    # center_subpixel == adding 0.5 px to the input (an fp32 add in both)
    shifted = {**base, "pt2d": (torch.from_numpy(base["pt2d"]) + 0.5).numpy()}
    a = run([base], gpu, n_hyps=64, seed=SEED, center_subpixel=True)
    b = run([shifted], gpu, n_hyps=64, seed=SEED)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    c0 = run([base], gpu, n_hyps=64, seed=SEED)
    assert not torch.equal(c0[0], a[0])
    # the per-query wrapper used by _solve_pnp
    R, t, inl = pnp_gpu.solve_pnp(torch.from_numpy(base["pt2d"]), torch.from_numpy(base["pt3d"]).to(gpu), torch.from_numpy(base["K"]), rthres=1, n_hyps=64)
    assert R.shape == (3, 3) and t.shape == (3,) and len(inl) == 65 and np.abs(R - base["R"]).max() < 1e-4
    assert pnp_gpu.solve_pnp(torch.zeros(3, 2), torch.zeros(3, 3, device=gpu), torch.eye(3)) is None


# ----------------------------------------------------------------------------------------------- 7. the evaluator
def _make_batch(H, W, q):
    """The synthetic-scene batch of tests/test_evaluator_gpu.py (restated)."""
    from nerfmatch_amd import synth

    unnorm = synth.unnorm_scene()
    M = (H // 8) * (W // 8)
    ys, xs = torch.meshgrid(torch.arange(H // 8), torch.arange(W // 8), indexing="ij")
    g = torch.Generator().manual_seed(q)
    return dict(image=torch.randn(1, 3, H, W, generator=g), im_mask=torch.ones(1, M, dtype=torch.bool), K=synth.intrinsics(H, W, 120.0)[None],
                c2w=(unnorm @ synth.camera_pose(q))[None], rc2w=(unnorm @ synth.camera_pose(q + 100))[None],
                pt2d=(torch.stack([xs, ys], -1) * 8 + 4).float().reshape(1, M, 2), unnorm_scene=unnorm[None])


def _stack(batches):
    return {k: torch.cat([b[k] for b in batches]) for k in batches[0]}


def _evaluator_and_renderer(gpu, H, W):
    from argparse import Namespace

    from nerfmatch_amd import synth
    from nerfmatch_amd.modules import StubBackbone
    from nerfmatch_amd.nerf.renderer import NerfRenderer
    from nerfmatch_amd.nerfmatch_evaluator import NeRFMatchEvaluator

    ev = NeRFMatchEvaluator(Namespace(model=synth.matcher_config("c2f"), exp=Namespace(seed=1), data=Namespace()))
    ev.model.load_state_dict(synth.matcher_state_dict("c2f"), strict=False)
    ev.model.backbone = StubBackbone().to(gpu)
    ren = NerfRenderer(synth.nerf_config("7scenes", num_pts=32, img_wh=(W, H)), training=False, stop_layer=3)
    ren.load_state_dict(synth.nerf_state_dict(seed=0, density_bias=3.0))
    return ev, ren.to(gpu).eval()


def _within_bin(c2w_est, c2w):
    from nerfmatch_amd.utils.metrics import pose_err

    R_err, t_err = pose_err(c2w, c2w_est)
    return R_err < R_THRES and t_err < T_THRES


def test_evaluator_solver_gpu(gpu, built_lib):
    H, W = 96, 128
    ev, ren = _evaluator_and_renderer(gpu, H, W)
    # eval_match_pose on points rendered at the query pose, with the ground-truth correspondences
    singles = [_make_batch(H, W, q) for q in range(4)]
    for Q in (1, 4):
        b = _stack(singles[:Q])
        o = ren.render_novel_views((H, W), b["K"][0], b["c2w"], b["unnorm_scene"][0], gpu, want_im_pred=False)
        b.update(pt3d=o["pt3d"], pt_feat=o["pt_feat"])
        res = ev.eval_match_pose(b, solver="gpu", match_oracle=True)
        res = [res] if Q == 1 else res
        assert isinstance(res, list) and len(res) == Q
        for q, (c2w_est, R_err, t_err, n) in enumerate(res):
            assert isinstance(c2w_est, torch.Tensor) and c2w_est.shape == (4, 4) and c2w_est.dtype == torch.float32 and not c2w_est.is_cuda
            assert isinstance(n, int) and n >= 4 and isinstance(float(R_err), float) and isinstance(float(t_err), float)
            assert _within_bin(c2w_est, singles[q]["c2w"][0]) and R_err < R_THRES and t_err < T_THRES
    # the two-iteration loop; query 1 sees fewer than 4 matches (all but three image cells masked out)
    b = _stack(singles[:3])
    b["im_mask"][1] = False
    b["im_mask"][1, 20:23] = True
    calls = []
    render_into = ev._render_into
    ev._render_into = lambda batch, renderer, poses, unnorm, **kw: (calls.append((len(poses), kw.get("queries"))), render_into(batch, renderer, poses, unnorm, **kw))[1]
    out = ev.eval_batch(b, renderer=ren, iters=2, solver="gpu", match_oracle=True, query2query=True, cache_iters=True)
    del ev.__dict__["_render_into"]
    assert [c[1] for c in calls if c[1] is not None] == [[0, 2]]  # iteration 1 re-renders the two queries that have a pose, from it
    assert len(out["iter_t_errs"]) == len(out["iter_R_errs"]) == 3 and all(len(t) == 2 for t in out["iter_t_errs"])
    assert isinstance(out["c2w_est"], list) and len(out["c2w_est"]) == 3 and len(out["c2w_ests"]) == 3
    assert out["c2w_ests"][1] is None and float(out["R_err"][1]) == float("inf") and float(out["t_err"][1]) == float("inf") and out["num_matches"][1] <= 3
    assert all(float(v) == float("inf") for v in out["iter_t_errs"][1])
    for q in (0, 2):
        assert out["c2w_ests"][q].shape == (4, 4) and _within_bin(out["c2w_ests"][q], singles[q]["c2w"][0])
        assert float(out["iter_t_errs"][q][-1]) < T_THRES and float(out["iter_R_errs"][q][-1]) < R_THRES and out["num_matches"][q] >= 4


def _matched_batch(gpu, ren, singles, H, W):
    """The batch a matcher pass needs: the queries' own fields plus points rendered at the query poses, on the device."""
    b = _stack(singles)
    o = ren.render_novel_views((H, W), b["K"][0], b["c2w"], b["unnorm_scene"][0], gpu, want_im_pred=False)
    return dict(image=b["image"].to(gpu), im_mask=b["im_mask"].to(gpu), pt2d=b["pt2d"].to(gpu), pt3d=o["pt3d"], pt_feat=o["pt_feat"],
                pt_mask=torch.ones_like(o["pt3d"][..., 0]), K=b["K"], c2w=b["c2w"])


def _check_against_direct_solve(res, b, ids, pt2d, pt3d, Q):
    """What the evaluator returned for the batch against solve_pnp_batch on the same match list."""
    res = [res] if Q == 1 else res
    w2c, n_inl, _ = pnp_gpu.solve_pnp_batch(pt2d, pt3d, ids, b["K"][:Q], num_queries=Q)
    counts = torch.bincount(ids.cpu(), minlength=Q).tolist()
    assert len(res) == Q
    for q, (c2w_est, R_err, t_err, n) in enumerate(res):
        assert n == counts[q]
        if int(n_inl[q]) < 4:
            assert c2w_est is None and float(R_err) == float("inf") and float(t_err) == float("inf")
        else:
            assert torch.equal(c2w_est, torch.linalg.inv(w2c[q].cpu()))
    return counts


def test_evaluator_solver_gpu_on_the_matcher_s_own_lists(gpu, built_lib):
    """solver="gpu" without the oracle: the fine match list with the host counts, the same list through its per-match query ids (no
    "match_counts", and a list cut shorter than the counts say), and the coarse-only model's (match_ids, pt2d, pt3d)."""
    from argparse import Namespace

    from nerfmatch_amd import synth
    from nerfmatch_amd.modules import StubBackbone
    from nerfmatch_amd.nerfmatch_evaluator import NeRFMatchEvaluator

    H, W = 96, 128
    ev, ren = _evaluator_and_renderer(gpu, H, W)
    singles = [_make_batch(H, W, q) for q in range(2)]
    for Q in (1, 2):
        b = _matched_batch(gpu, ren, singles[:Q], H, W)
        res = ev.eval_match_pose(b, solver="gpu", mutual=True)
        assert "match_counts" in b and sum(int(c) for c in b["match_counts"]) == len(b["mpt2d_f"]) > 0
        counts = _check_against_direct_solve(res, b, b["m_bids"], b["mpt2d_f"], b["mpt3d"], Q)
        assert counts == [int(c) for c in b["match_counts"]]
    # the id route: no host counts; and a list shorter than the host counts (as a pred_mask filter leaves it)
    no_counts = {k: v for k, v in b.items() if k != "match_counts"}
    assert [r[3] for r in ev._poses_from_matches(no_counts, "gpu", 1, False)] == counts
    cut = dict(b, mpt2d_f=b["mpt2d_f"][:-5], mpt3d=b["mpt3d"][:-5], m_bids=b["m_bids"][:-5])
    _check_against_direct_solve(ev._poses_from_matches(cut, "gpu", 1, False), b, cut["m_bids"], cut["mpt2d_f"], cut["mpt3d"], 2)
    # the coarse-only model
    evc = NeRFMatchEvaluator(Namespace(model=synth.matcher_config("coarse"), exp=Namespace(seed=1), data=Namespace()))
    evc.model.load_state_dict(synth.matcher_state_dict("coarse"), strict=False)
    evc.model.backbone = StubBackbone(two_scales=False).to(gpu)
    assert evc.coarse_only
    b = _matched_batch(gpu, ren, singles, H, W)
    res = evc.eval_match_pose(b, solver="gpu", mutual=True)
    bid, i2d, i3d = b["match_ids"]
    assert len(bid) > 0
    _check_against_direct_solve(res, b, bid, b["pt2d"][bid, i2d], b["pt3d"].reshape(2, -1, 3)[bid, i3d], 2)
