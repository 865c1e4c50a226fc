"""ORACLE (test infrastructure, NOT product code) -- the multi-iteration localisation loop of ONE query.

A plain-Python restatement of the control flow of the reference's `NeRFMatchEvaluator.eval_batch`
(nerfmatch/nerfmatch_evaluator.py:502-629) for a batch of one query, with the renderer, the matcher, the PnP solver and
the iNeRF refinement passed in as callables.  Only tests/ may import it.

What the reference does (line numbers of nerfmatch/nerfmatch_evaluator.py):
  * start pose (:538-546): the query pose with `query2query`, the retrieved reference pose `rc2w` without cached points or
    with `retrieval_only`, else none (the cached points of the batch are matched as they are);
  * per iteration (:548):
      - `retrieval_only` (:549-551): no render, no matcher; num_matches = 0 and the errors of the current pose;
      - else (:553-586): a render from the current pose if there is one (:555-573; without one the previous points are
        matched again), the matcher, the solver -- called every iteration, whether or not an earlier one failed -- whose pose
        (None on failure) becomes the current pose, its errors (inf on failure, :216-219) and num_matches = len(matches)
        (:228); with `inerf_conf` and `cache_iters` the errors are appended to the trace here (:584-586);
      - with `inerf_conf` and a current pose (:588-610): the refinement, which appends its own inner entries to the trace
        when `cache_iters` (steps 1 .. num_optim-2, :491-493); its pose and errors are taken only if its rotation error is
        finite (:608-610);
      - with `cache_iters` the iteration's errors are appended (:612-614).
  * result (:619-627): the last iteration's errors and the traces; the final pose is the current pose.

The project's two extensions (nerfmatch_amd/nerfmatch_evaluator.py):
  * `solver="none"` (no PnP package): the solver is not called, the errors are inf, and the pose the points were
    rendered from is kept as the current pose (the reference would raise).
  * Batches of Q > 1 queries: the reference's eval_batch serves one query.  In a batch, a query whose solve failed keeps
    its old points while the others are re-rendered from their solved poses, and every query gets its own trace: a
    Q-query batch gives every query exactly the trace that query gets in a Q = 1 run, i.e. the trace of `localize`.
"""
import math

import torch

INF = float("inf")


def pose_err(gt, est):
    """(rotation error in degrees, translation error) of two c2w poses in fp64 (the reference's pose_err: the angle of
    R_est R_gt^T and the distance of the camera centres)."""
    gt, est = torch.as_tensor(gt).double(), torch.as_tensor(est).double()
    t_err = float(torch.linalg.norm(gt[:3, 3] - est[:3, 3]))
    cos = (float(torch.trace(est[:3, :3] @ gt[:3, :3].T)) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, cos)))), t_err


def start_pose(c2w, rc2w, query2query=False, cached_pt=True, retrieval_only=False):
    """reference :538-546."""
    if query2query:
        return c2w
    if (not cached_pt) or retrieval_only:
        return rc2w
    return None


def localize(c2w_gt, pose, points, iters, render, match, solve, refine=None, solver_none=False, retrieval_only=False,
             cache_iters=False, err=pose_err):
    """One query through `iters` iterations of the loop.

    c2w_gt: the query's ground-truth pose; pose: the start pose (`start_pose`) or None; points: what is matched while nothing
    has been rendered (the cached points).  render(pose) -> points; match(points) -> matches (a sequence);
    solve(matches) -> c2w | None; refine(pose) -> (c2w, R_err, t_err, inner) with `inner` the [(R_err, t_err), ...] entries
    the refinement appends to the traces when `cache_iters` (None: no refinement).

    Returns dict(renders=[(iteration, pose)], solves=[(iteration, matches, result)], refines=[(iteration, pose)],
    iter_t_errs, iter_R_errs, c2w_est, R_err, t_err, num_matches)."""
    tr = dict(renders=[], solves=[], refines=[], iter_t_errs=[], iter_R_errs=[])
    R_err = t_err = INF
    num_matches = 0
    for itr in range(iters):
        if retrieval_only:                                            # :549-551
            num_matches = 0
            R_err, t_err = err(c2w_gt, pose)
        else:
            if pose is not None:                                      # :555-573
                points = render(pose)
                tr["renders"].append((itr, pose))
            matches = match(points)                                   # :575-583 (eval_match_pose, :152-230)
            num_matches = len(matches)
            if solver_none:
                R_err = t_err = INF                                   # (extension: the rendered-from pose stays)
            else:
                res = solve(matches)
                tr["solves"].append((itr, matches, res))
                pose = res
                R_err, t_err = (INF, INF) if res is None else err(c2w_gt, res)
            if refine is not None and cache_iters:                    # :584-586
                tr["iter_t_errs"].append(t_err)
                tr["iter_R_errs"].append(R_err)
        if pose is not None and refine is not None:                   # :588-610
            tr["refines"].append((itr, pose))
            ref_pose, ref_R, ref_t, inner = refine(pose)
            if cache_iters:                                           # :491-493, inside the refinement
                for r, t in inner:
                    tr["iter_t_errs"].append(t)
                    tr["iter_R_errs"].append(r)
            if ref_R != INF:
                pose, R_err, t_err = ref_pose, ref_R, ref_t
        if cache_iters:                                               # :612-614
            tr["iter_t_errs"].append(t_err)
            tr["iter_R_errs"].append(R_err)
    tr.update(c2w_est=pose, R_err=R_err, t_err=t_err, num_matches=num_matches)
    return tr
