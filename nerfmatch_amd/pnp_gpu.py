"""Batched PnP-RANSAC on the GPU (`solver="gpu"`): 2D-3D matches of Q queries -> Q world-to-camera poses in one call of nm_pnp_ransac
(csrc/pnp.hip): hash-sampled P3P hypotheses in fp64, fp32 inlier scoring of every hypothesis against every match of its query, and a
Levenberg-Marquardt refinement of the winner with the inlier set re-evaluated each step.  A fixed number of hypotheses, no early
termination, fixed summation orders: a query gives the same bits alone, in any batch and on every run ("PnP-RANSAC").
No fallback: without the HIP library the call raises."""
import torch

from . import ops


def offsets_from_bids(m_bids, Q):
    """Sorted per-match query ids (the matcher's `m_bids`) -> (Q + 1,) int32 offsets, on the device, without a read-back."""
    bounds = torch.arange(Q + 1, device=m_bids.device, dtype=m_bids.dtype)
    return torch.searchsorted(m_bids.contiguous(), bounds).to(torch.int32)


def solve_pnp_batch(pt2d, pt3d, offsets_or_bids, K, rthres=1, n_hyps=1024, refine_iters=10, seed=0, center_subpixel=False, want_inliers=False,
                    study=False, num_queries=None):
    """pt2d (n, 2) pixels and pt3d (n, 3), grouped by query; K (Q, 3, 3) or (3, 3) for all queries.  `offsets_or_bids`: a list / tuple of
    per-query match counts on the host (`batch["match_counts"]`), or a tensor -- int32: the (Q + 1,) offsets; int64: the sorted per-match
    query ids (n,) the matcher returns as `m_bids` (Q = num_queries, or the number of intrinsics; the offsets are then built on the device).
    -> (w2c (Q, 4, 4) fp32, n_inliers (Q,) int32, inlier_mask (n,) bool | None), all on the device; with study=True a fourth element
    (hyp_pose (Q, n_hyps, 12), hyp_count (Q, n_hyps)).  n_inliers[q] < 4: query q has NO pose (fewer than four matches, or no hypothesis
    with four inliers); its w2c is the identity.  center_subpixel adds 0.5 px to the pixels, as the pycolmap wrapper does."""
    dev = pt3d.device
    pt2d = pt2d.detach().reshape(-1, 2).to(device=dev, dtype=torch.float32).contiguous()
    pt3d = pt3d.detach().reshape(-1, 3).to(torch.float32).contiguous()
    K = torch.as_tensor(K).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3, 3)
    n = pt2d.shape[0]
    if pt3d.shape[0] != n:
        raise ValueError(f"{n} pixels for {pt3d.shape[0]} points")
    host = None
    if isinstance(offsets_or_bids, (list, tuple)):
        host = [0]
        for c in offsets_or_bids:
            host.append(host[-1] + int(c))
        if host[-1] != n:
            raise ValueError(f"the match counts add up to {host[-1]}, there are {n} matches")
        Q = len(host) - 1
        offsets = torch.tensor(host, dtype=torch.int32)
        offsets = (offsets.pin_memory() if dev.type == "cuda" else offsets).to(dev, non_blocking=True)  # (a pageable copy would wait for all queued work)
    else:
        t = offsets_or_bids.to(dev).reshape(-1)
        if t.dtype == torch.int32:  # offsets
            Q, offsets = t.numel() - 1, t.contiguous()
        else:  # int64: one query id per match
            Q = int(num_queries) if num_queries is not None else K.shape[0]
            offsets = offsets_from_bids(t, Q)
    if Q < 1:
        raise ValueError("no query")
    if K.shape[0] == 1 and Q > 1:
        K = K.expand(Q, 3, 3)
    if K.shape[0] != Q:
        raise ValueError(f"{K.shape[0]} intrinsics for {Q} queries")
    pose, n_inl, mask, hyp = ops.pnp_ransac(pt2d, pt3d, offsets, K.contiguous(), thr_px=rthres, n_hyps=n_hyps, refine_iters=refine_iters, seed=seed,
                                            add_half_px=center_subpixel, want_inliers=want_inliers, study=study, offsets_host=host)
    w2c = torch.zeros(Q, 4, 4, device=dev, dtype=torch.float32)
    w2c[:, :3] = pose.view(Q, 3, 4)
    w2c[:, 3, 3] = 1.0
    out = (w2c, n_inl, None if mask is None else mask.bool())
    return out + (hyp,) if study else out


def solve_pnp(pt2d, pt3d, K, rthres=1, center_subpixel=False, **kw):
    """One query, with the return convention of the third-party wrappers in utils/pnp.py: (R (3,3), t (3,), inlier indices) as numpy
    arrays, or None when there is no pose."""
    dev = pt3d.device if isinstance(pt3d, torch.Tensor) and pt3d.is_cuda else torch.device("cuda", torch.cuda.current_device())
    pt2d, pt3d = torch.as_tensor(pt2d), torch.as_tensor(pt3d).to(dev)
    if len(pt2d) < 4:
        return None
    w2c, n_inl, mask = solve_pnp_batch(pt2d, pt3d, [len(pt2d)], torch.as_tensor(K).reshape(1, 3, 3), rthres=rthres, center_subpixel=center_subpixel,
                                       want_inliers=True, **kw)
    if int(n_inl[0]) < 4:
        return None
    w = w2c[0].cpu().numpy()
    return w[:3, :3], w[:3, 3], torch.nonzero(mask).reshape(-1).cpu().numpy()
