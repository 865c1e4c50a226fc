"""Host-side evaluation statistics used by the evaluators (numpy / tiny torch ops on K-element lists; not on the hot path).

Restated from the reference's definitions (nerfmatch/utils/metrics.py): scene-dependent pose thresholds :27-42, validation
PSNR of `compute_nerf_metrics` :59-96, the two-view pose metrics `compute_nerf_pose_metrics` :99-218 (on the device up to the
poses), `cal_error_auc` :340-352, `pose_recall` :355-356, `pose_err` :359-369, `summarize_pose_statis` :545-595, `average_pose_metrics` :598-606 -- the evaluators return / print the same quantities, so
result files written here and by the reference are interchangeable."""
import math
from argparse import Namespace

import numpy as np
import torch

# (translation cm, rotation deg) thresholds following DSAC* (reference :27-42)
POSE_THRES = {
    "GreatCourt": [(5, 45)], "KingsCollege": [(5, 38)], "OldHospital": [(5, 22)], "ShopFacade": [(5, 15)], "StMarysChurch": [(5, 35)],
    "chess": [(5, 5)], "fire": [(5, 5)], "heads": [(5, 5)], "office": [(5, 5)], "pumpkin": [(5, 5)], "redkitchen": [(5, 5)], "stairs": [(5, 5)],
}


def pose_err(gt_pose, est_pose):
    """(rotation error in degrees, translation error) between two c2w poses; the Rodrigues norm of R_est R_gt^T the
    reference takes (cv2.Rodrigues) is the rotation angle."""
    gt_pose, est_pose = torch.as_tensor(gt_pose).double().cpu(), torch.as_tensor(est_pose).double().cpu()
    t_err = float(torch.norm(gt_pose[:3, 3] - est_pose[:3, 3]))
    rel = est_pose[:3, :3] @ gt_pose[:3, :3].T
    cos = max(-1.0, min(1.0, (float(torch.trace(rel)) - 1.0) / 2.0))
    return math.degrees(math.acos(cos)), t_err


def pose_recall(r_errs, t_errs, r_thres, t_thres):
    return ((np.array(r_errs) < r_thres) & (np.array(t_errs) < t_thres)).mean() * 100


def cal_error_auc(errors, thresholds):
    if len(errors) == 0:
        return np.zeros(len(thresholds))
    n = len(errors)
    errors = np.append([0.0], np.sort(errors))
    recalls = np.arange(n + 1) / n
    aucs = []
    for thres in thresholds:
        last = np.searchsorted(errors, thres)
        rcs = np.append(recalls[:last], recalls[last - 1])
        ers = np.append(errors[:last], thres)
        aucs.append(np.sum((ers[1:] - ers[:-1]) * (rcs[1:] + rcs[:-1]) / 2.0) / thres)  # trapezoid rule (np.trapz)
    return np.array(aucs) * 100


def summarize_pose_statis(statis, pose_thres=(1, 2, 5, 10), auc_thres=(1, 2, 5, 10), t_unit="?", t_scale=1, print_out=True):
    printf = print if print_out else (lambda *_: None)
    if isinstance(statis, dict):
        statis = Namespace(**statis)
    pose_thres = [(th, th) if np.isscalar(th) else tuple(th) for th in pose_thres]
    r_errs, t_errs = np.asarray(statis.R_err, dtype=np.float64), t_scale * np.asarray(statis.t_err, dtype=np.float64)
    printf(f"\nSamples: {len(r_errs)} t_unit={t_unit} t_scale={t_scale}")
    if "num_matches" in statis:
        printf(f"Mean matches: {np.mean(statis.num_matches):.0f}")
    t_med, r_med = np.median(t_errs), np.median(r_errs)
    printf(f"Median Error: {t_med:.1f}/{r_med:.1f} {t_unit}/deg")
    pose_rec = np.array([pose_recall(r_errs, t_errs, rth, tth) for rth, tth in pose_thres])
    printf(f"Recall@{pose_thres}{t_unit}/deg: {pose_rec}%")
    printf(f"AUC@{list(auc_thres)}{t_unit}/deg: {cal_error_auc(np.maximum(t_errs, r_errs), auc_thres)}%")
    summary = {"t_med": t_med, "r_med": r_med, "recall": pose_rec[0]}
    if "match_time" in statis:
        summary["match_time"] = float(np.mean(statis.match_time) * 1000)
        printf(f"Avg match time: {summary['match_time']:.1f}ms")
    return summary


def average_pose_metrics(metr_all, print_out=True):
    avg = {k: float(np.mean([m[k] for m in metr_all])) for k in metr_all[0]}
    if print_out:
        print(f"\nAverage metrics of {len(metr_all)} (scene) caches:")
        print(f"Median pose error(cm/deg): {avg['t_med']:.1f}/{avg['r_med']:.1f}")
        print(f"Recall(%): {avg['recall']:.1f}")
    return avg


def mse2psnr(mse):
    return -10 * torch.log10(mse)


def lossfun_distortion(t, w):
    """iint w[i] w[j] |t[i] - t[j]| di dj per ray (reference :453-465): t (R,S+1) fence posts (or (R,S): a zero is put in front), w (R,S)."""
    if w.shape[-1] == t.shape[-1]:
        t = torch.hstack((t[:, :1] * 0, t))
    ut = (t[..., 1:] + t[..., :-1]) / 2
    dut = torch.abs(ut[..., :, None] - ut[..., None, :])
    loss_inter = torch.sum(w * torch.sum(w[..., None, :] * dut, dim=-1), dim=-1)
    loss_intra = torch.sum(w**2 * (t[..., 1:] - t[..., :-1]), dim=-1) / 3
    return loss_inter + loss_intra


def distortion_loss(s, w):
    """The distortion regulariser of mip-NeRF 360 (reference :448-450)."""
    return torch.mean(lossfun_distortion(s, w))


def compute_nerf_metrics(preds, rgb_gt, mask_loss=None, validation_mode=False, cnfg_loss=None):
    """The reference's compute_nerf_metrics (:59-96) in plain differentiable torch: 0.5 * mean(mask * (rgb - gt)^2) and its PSNR for the
    coarse and fine images (the 0.5 is the reference's), `loss` = coarse_weight * coarse + fine and, when training, + ray_reg_weight *
    distortion_loss(s_fine, weights_fine).  The mask is rounded in validation only.  (The reference's `app_coarse` term is dead code -- its
    renderer never sets that key -- and is not built.)  A training step on the GPU takes nerf.train_render.training_metrics, the same
    quantities on the fused loss kernels."""
    if mask_loss is None:
        m = 1
    else:
        m = torch.round(mask_loss) if validation_mode else mask_loss
    out = {}
    loss = 0
    if "rgb_coarse" in preds:
        mse = 0.5 * (m * (preds["rgb_coarse"] - rgb_gt) ** 2).mean()
        loss = loss + mse * getattr(cnfg_loss, "coarse_weight", 1.0)
        out["rgb_coarse_mse"], out["rgb_coarse_psnr"] = mse, mse2psnr(mse)
    if "rgb_fine" in preds:
        mse = 0.5 * (m * (preds["rgb_fine"] - rgb_gt) ** 2).mean()
        loss = loss + mse
        out["rgb_fine_mse"], out["rgb_fine_psnr"] = mse, mse2psnr(mse)
    else:
        out["rgb_fine_mse"], out["rgb_fine_psnr"] = out["rgb_coarse_mse"], out["rgb_coarse_psnr"]
    if not validation_mode:
        reg = getattr(cnfg_loss, "ray_reg_weight", None)
        if "s_fine" in preds and reg:
            loss = loss + distortion_loss(preds["s_fine"], preds["weights_fine"]) * reg
    out["loss"] = loss
    return out


def _unnormalize(pts, unnorm):
    """Normalised scene -> world, one view's points (n, 3): the reference's unnormaliz_pts (geometry.py:76-85).  Device points take
    nm_unnormalize_points; host points the reference's own statement."""
    if pts.is_cuda:
        from .. import ops

        return ops.unnormalize_points(pts.to(torch.float32).contiguous(), unnorm)
    p = pts.reshape(1, -1, 3)
    p = torch.cat([p, torch.ones_like(p[..., 0:1])], dim=-1)
    return torch.bmm(unnorm.reshape(1, 4, 4).to(p), p.transpose(-1, -2)).transpose(-1, -2)[0, :, :3]


def _pose_errs(c2w_gt, res):
    """(R_err deg, t_err) of a solver result (R, t, inliers) | None against a c2w pose; no pose: (inf, inf) (reference :202-218)."""
    if res is None:
        return math.inf, math.inf
    w2c = torch.eye(4, dtype=torch.float32)
    w2c[:3, :3] = torch.as_tensor(np.asarray(res[0], dtype=np.float32))
    w2c[:3, 3] = torch.as_tensor(np.asarray(res[1], dtype=np.float32)).reshape(3)
    return pose_err(c2w_gt, w2c.inverse())


def compute_nerf_pose_metrics(pts_fine, pt_mask, pts_feat, data, ds=8, ransac_thres=1, solver="gpu", **solver_kw):
    """The two-view pose metrics of a NeRF validation step (reference :99-177, called by NerfTrainer.log_step, nerf_trainer.py:125-133):
    how well the rendered 3-D points and the rendered point features of two views localise each other's camera.
      R_err_depth / t_err_depth   view 2's points, projected into image 1 with the true pose and truncated to integer pixels, every ds-th
                                  one from ds // 2, give image 1's pose back by PnP (and the other way round); mean of the two errors
      R_err_match / t_err_match   the same with the pixels of the cosine mutual-NN matches between the two views' point features
      match_score, num_matches    mean similarity and number of those matches
    t errors are multiplied by 100 (the reference's metres -> cm); a problem without a pose counts as inf.
    pts_fine (2 h w, 3) normalised points and pts_feat (2 n, C) of the two views in ray order; pt_mask: the boolean mask of the n rays
    whose features were kept (init_pfeat_mask()[0, ..., 0]); data: "img_idx" (two entries), "img_wh", "c2w" (1, 8, 4), "K" (1, 6, 3),
    "unnorm_scene" (1, 4, 4), as the pair dataset concatenates them.
    Taken from the reference literally, quirks included: the mask is shaped (W, H) but flattened against rays in (H, W) order, and its
    pixel coordinates are `ys, xs = where(pt_mask)` of that array; projected pixels are truncated by an int32 cast.
    Everything stays on the tensors' device up to the poses.  solver: "gpu" -- the four PnP problems (depth -> image 1, depth -> image 2,
    matches -> image 1, matches -> image 2) are ONE pnp_gpu.solve_pnp_batch call with Q = 4 (solver_kw: its n_hyps, seed, ...); "cv2" /
    "colmap" -- the wrappers of utils/pnp.py; or a callable (pt2d, pt3d, K) -> (R, t, inliers) | None, called once per problem in that
    order."""
    from .. import supervision as sup
    from .geometry import mutual_nn_matching

    nsample = len(data["img_idx"])
    if nsample != 2:
        raise ValueError(f"the pose metrics are defined for a two-view batch, this one has {nsample} view(s)")
    w, h = (int(v) for v in torch.as_tensor(data["img_wh"])[0][:2])
    dev = pts_fine.device
    c2w_gt = torch.as_tensor(data["c2w"]).detach().reshape(2, 4, 4).to("cpu", torch.float32)
    K = torch.as_tensor(data["K"]).detach().reshape(2, 3, 3).to(torch.float32)
    unnorm = torch.as_tensor(data["unnorm_scene"]).detach().to("cpu", torch.float32)
    pts = pts_fine.detach().reshape(2, h * w, 3)
    # world points, in the order the problems use them: row 0 = view 2's points (seen from image 1), row 1 = view 1's
    pt3d = torch.stack([_unnormalize(pts[1], unnorm), _unnormalize(pts[0], unnorm)])
    # part 1: reprojection + subsampling (reference :180-199)
    K_dev = K.to(dev)
    pix = sup.project_points3d(K_dev, sup.w2c_from_c2w(c2w_gt.to(dev)), pt3d).to(torch.int32)
    sub = lambda x: x.reshape(2, h, w, x.shape[-1])[:, ds // 2 :: ds, ds // 2 :: ds].reshape(2, -1, x.shape[-1])
    pt2d_depth, pt3d_depth = sub(pix), sub(pt3d)
    # part 2: mutual matches of the kept rays' features
    mask = torch.as_tensor(pt_mask).to(torch.bool)
    ys, xs = torch.where(mask)
    pts2d = torch.stack([xs, ys], dim=-1).to(dev)
    pt3d_kept = pt3d[:, mask.flatten().to(dev)]
    pfeat_1, pfeat_2 = pts_feat.detach().reshape(2, -1, pts_feat.shape[-1])
    matches, scores = mutual_nn_matching(pfeat_1, pfeat_2)
    matches = matches.to(dev)
    match_score = scores.float().mean() if scores.numel() else torch.tensor(math.nan)
    problems = [(pt2d_depth[0], pt3d_depth[0], K[0]), (pt2d_depth[1], pt3d_depth[1], K[1]),
                (pts2d[matches[:, 0]], pt3d_kept[0][matches[:, 1]], K[0]), (pts2d[matches[:, 1]], pt3d_kept[1][matches[:, 0]], K[1])]
    if solver == "gpu":
        from .. import pnp_gpu

        w2c, n_inl, _ = pnp_gpu.solve_pnp_batch(torch.cat([p[0] for p in problems]), torch.cat([p[1] for p in problems]),
                                                [len(p[0]) for p in problems], torch.stack([p[2] for p in problems]), rthres=ransac_thres, **solver_kw)
        w2c, n_inl = w2c.cpu(), n_inl.cpu()
        results = [(w2c[q, :3, :3], w2c[q, :3, 3], None) if int(n_inl[q]) >= 4 else None for q in range(4)]
    else:
        if solver in ("cv2", "colmap"):
            from . import pnp

            fn = pnp.estimate_pose if solver == "cv2" else pnp.estimate_pose_pycolmap
            solve = lambda p2, p3, Km: fn(p2, p3, Km, ransac_thres=ransac_thres, **solver_kw)
        elif callable(solver):
            solve = solver
        else:
            raise ValueError(f"solver must be 'gpu', 'cv2', 'colmap' or a callable, got {solver!r}")
        results = [solve(*p) for p in problems]
    errs = [_pose_errs(c2w_gt[q % 2], results[q]) for q in range(4)]
    return dict(R_err_depth=0.5 * (errs[0][0] + errs[1][0]), t_err_depth=0.5 * (errs[0][1] + errs[1][1]) * 100,
                R_err_match=0.5 * (errs[2][0] + errs[3][0]), t_err_match=0.5 * (errs[2][1] + errs[3][1]) * 100,
                match_score=match_score, num_matches=len(matches))

