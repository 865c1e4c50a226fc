"""Coarse match supervision of a training batch: `pt2d_proj`, `conf_gt` and the ground-truth index triple, from the batch's geometry.

The reference builds these in its dataset classes, in numpy on the host (nerfmatch/datasets/nerfmatch_dataset.py:302-353 and :553-583
with project_points3d, nerfmatch/utils/geometry.py:119-136): a dense float32 M x N matrix per pair, three broadcast multiplies over it
and a copy to the device.  Every 3-D point projects into at most one coarse cell, so the matrix is a function of an N-vector of cell
ids (`gt_cell`); here one launch (nm_gt_supervision, csrc/supervision.hip) makes the projections, the cell ids, the dense uint8 matrix
the loss kernels read and the (b, i, j) triple in torch.where order -- the triple by a counting sort of N entries instead of a scan of
M * N bytes.

Device tensors are served by the kernel (no fallback: a missing library raises).  Host tensors take the torch path below, which
evaluates the same fp32 operations in the same order; it is the product's behaviour without a GPU and what the CPU tests compare with
the reference's numbers.

Two quirks of the reference are kept: the strict `min(cx, cy) > 0` excludes cell row 0 and cell column 0, and there is no depth test
(a point behind the camera whose flipped projection lands inside the image counts as visible).  Where the reference is undefined
(p.z == 0, a projection that is not finite) the point is invisible."""
import torch

from . import ops

MAX_CELLS = 6400  # nm_gt_supervision's LDS histogram


def w2c_from_c2w(c2w):
    """(B, 3|4, 4) camera-to-world -> (B, 3, 4) world-to-camera [R^T | -R^T t]: the closed-form inverse of a rigid transform, elementwise
    fp32 products and sums in a fixed order (the same bits on host and device; no factorisation, no host synchronisation).  The reference
    inverts the 4 x 4 matrix numerically (`qc2w.inverse()`, nerfmatch_dataset.py:262)."""
    c2w = c2w.to(torch.float32)
    Rt = c2w[..., :3, :3].transpose(-1, -2)
    t = c2w[..., :3, 3]
    tt = -((Rt[..., 0] * t[..., 0:1] + Rt[..., 1] * t[..., 1:2]) + Rt[..., 2] * t[..., 2:3])
    return torch.cat([Rt, tt[..., None]], dim=-1).contiguous()


def _project_torch(K, w2c, pt3d):
    """p = R X + t, q = p / p.z, pix = K q with every product and sum a separate fp32 operation, in the kernel's order.  -> pix (B,N,2), p.z (B,N)."""
    x, y, z = pt3d[..., 0], pt3d[..., 1], pt3d[..., 2]
    r = lambda a, c: w2c[:, a, c, None]
    p = [((r(a, 0) * x + r(a, 1) * y) + r(a, 2) * z) + r(a, 3) for a in range(3)]
    q = [p[a] / p[2] for a in range(3)]
    k = lambda a, c: K[:, a, c, None]
    pix = [(k(a, 0) * q[0] + k(a, 1) * q[1]) + k(a, 2) * q[2] for a in range(2)]
    return torch.stack(pix, dim=-1), p[2]


def _batched(K, w2c, pt3d):
    pt3d = pt3d.to(torch.float32)
    single = pt3d.dim() == 2
    if single:
        K, w2c, pt3d = K[None], w2c[None], pt3d[None]
    B = pt3d.shape[0]
    K = K.to(torch.float32).expand(B, 3, 3).contiguous()
    w2c = w2c.to(torch.float32)[..., :3, :].expand(B, 3, 4).contiguous()
    return K, w2c, pt3d.contiguous(), single


def project_points3d(K, w2c, pt3d):
    """Pixel coordinates (B, N, 2) of the points pt3d (B, N, 3) under intrinsics K (B, 3, 3) and world-to-camera w2c (B, 3|4, 4); unbatched
    arguments give (N, 2).  The torch counterpart of the reference's numpy project_points3d(K, R, t, pts3d) (utils/geometry.py:119-136);
    on device tensors one launch of nm_gt_supervision."""
    K, w2c, pt3d, single = _batched(K, w2c, pt3d)
    out = ops.gt_supervision(pt3d, K, w2c) if pt3d.is_cuda else _project_torch(K, w2c, pt3d)[0]
    return out[0] if single else out


def _supervision_torch(pt3d, K, w2c, pt_mask, im_mask, fallback, H, W, ds, M, dense):
    """The kernel's outputs with torch ops (any device; used for host tensors).  Restates nerfmatch_dataset.py:329-351."""
    B, N = pt3d.shape[:2]
    dev = pt3d.device
    pix, pz = _project_torch(K, w2c, pt3d)
    Wc, Hc = W // ds, H // ds
    cf = torch.floor(pix / float(ds))
    defined = torch.isfinite(pix).all(-1) & (pz != 0)
    # (compared as floats, like the kernel: values beyond the integer range are invisible either way)
    visible = defined & (cf[..., 0] > 0) & (cf[..., 1] > 0) & (cf[..., 0] < Wc) & (cf[..., 1] < Hc)
    c = torch.where(visible[..., None], cf, torch.zeros_like(cf)).to(torch.int64)
    i = (c[..., 0] + c[..., 1] * Wc).clamp(0, M - 1)
    valid = visible
    if pt_mask is not None:
        valid = valid & pt_mask.reshape(B, N).ne(0)
    if im_mask is not None:
        valid = valid & torch.gather(im_mask.reshape(B, M).ne(0), 1, i)
    gt_cell = torch.where(valid, i, torch.full_like(i, -1)).to(torch.int32)
    # the triple in torch.where order: ascending b, then i, then j -- a stable sort of the valid columns by (b, i)
    bj = torch.nonzero(valid)
    b_ids, j_ids = bj[:, 0], bj[:, 1]
    i_ids = i[b_ids, j_ids]
    order = torch.argsort(b_ids * M + i_ids, stable=True)
    b_ids, i_ids, j_ids = b_ids[order], i_ids[order], j_ids[order]
    counts = torch.bincount(b_ids, minlength=B)
    if fallback is not None:
        fb = torch.as_tensor(fallback, device=dev).reshape(B, 2).to(torch.int64)
        use = (counts == 0) & (fb[:, 0] >= 0) & (fb[:, 0] < M) & (fb[:, 1] >= 0) & (fb[:, 1] < N)
        eb = torch.nonzero(use)[:, 0]
        if len(eb):
            b_ids, i_ids, j_ids = torch.cat([b_ids, eb]), torch.cat([i_ids, fb[eb, 0]]), torch.cat([j_ids, fb[eb, 1]])
            order = torch.argsort(b_ids, stable=True)  # (an empty element has this one entry only)
            b_ids, i_ids, j_ids = b_ids[order], i_ids[order], j_ids[order]
            counts = counts + use.to(counts.dtype)
    conf = None
    if dense:
        conf = torch.zeros(B, M, N, dtype=torch.uint8, device=dev)
        conf[b_ids, i_ids, j_ids] = 1
    return dict(pt2d_proj=pix, gt_cell=gt_cell, conf_gt=conf, ids=(b_ids, i_ids, j_ids), counts=counts.to(torch.int32))


def supervision(pt3d, K, w2c, hw, ds=8, pt_mask=None, im_mask=None, fallback=None, dense=True, M=None):
    """pt3d (B,N,3), K (B,3,3), w2c (B,3|4,4), image size hw = (H, W) -> dict(pt2d_proj (B,N,2), gt_cell (B,N) int32, conf_gt (B,M,N) uint8
    or None, ids = (b_ids, i_ids, j_ids) int64 in torch.where(conf_gt) order, counts (B,) int32).  `fallback` (B,2) of (i, j): the single
    entry of a batch element that has none (the caller draws it, as nerfmatch_dataset.py:347-351 does); None: it stays empty.
    On device tensors: one launch and ONE read-back (the B counts, to trim the triple)."""
    H, W = int(hw[0]), int(hw[1])
    ds = int(ds)
    if ds <= 0 or H % ds or W % ds:
        raise ValueError(f"image size {H} x {W} is not a multiple of the coarse stride {ds}")
    M = (H // ds) * (W // ds) if M is None else int(M)
    if M > MAX_CELLS:
        raise ValueError(f"{M} coarse cells: the supervision kernel takes at most {MAX_CELLS}")
    K, w2c, pt3d, _ = _batched(K, w2c, pt3d)
    B, N = pt3d.shape[:2]
    if pt_mask is not None:
        pt_mask = pt_mask.reshape(B, N)
    if im_mask is not None:
        im_mask = im_mask.reshape(B, M)
    if not pt3d.is_cuda:
        return _supervision_torch(pt3d, K, w2c, pt_mask, im_mask, fallback, H, W, ds, M, dense)
    if fallback is not None:
        fallback = torch.as_tensor(fallback).reshape(B, 2).to(device=pt3d.device, dtype=torch.int32).contiguous()
    out = ops.gt_supervision(pt3d, K, w2c, pt_mask, im_mask, fallback, (H, W), ds, M, dense=dense)
    total = int(out["counts"].sum().item())  # the one read-back: np.random.choice(len(b_gt), ...) needs the length on the host anyway
    out["ids"] = tuple(t[:total] for t in out["ids"])
    return out


def coarse_supervision(data, ds=8, fallback=None, dense=True):
    """Fills a batch dict in place with its coarse supervision.  Reads data["image"] (for H, W), "K", "c2w", "pt3d" and, when present,
    "pt_mask" / "im_mask"; the multi-pair layout pt3d (B, k, n, 3) with pt_mask (B, k, n) is flattened to N = k * n (the reference
    builds the matrix before its reshape, nerfmatch_dataset.py:585-590).  Writes "conf_gt" (B, M, N) uint8 (dense=True), "pt2d_proj"
    (B, N, 2), "gt_cell" (B, N) int32 and "gt_ids" = (b_ids, i_ids, j_ids), equal to torch.where(conf_gt).  A model takes the triple
    with `model.seed_gt_ids(data["conf_gt"], data["gt_ids"])` and then never scans the matrix."""
    H, W = data["image"].shape[-2:]
    pt3d = data["pt3d"]
    B = pt3d.shape[0]
    pt3d = pt3d.reshape(B, -1, 3)
    out = supervision(pt3d, data["K"].reshape(-1, 3, 3), w2c_from_c2w(data["c2w"].reshape(B, -1, 4)), (H, W), ds=ds, pt_mask=data.get("pt_mask"),
                      im_mask=data.get("im_mask"), fallback=fallback, dense=dense)
    if dense:
        data["conf_gt"] = out["conf_gt"]
    data.update(pt2d_proj=out["pt2d_proj"], gt_cell=out["gt_cell"], gt_ids=out["ids"])
    return data


def draw_fallback(B, M, N):
    """The reference's draw for a sample without any ground-truth match (nerfmatch_dataset.py:347-351): two draws of Python's `random`,
    BOTH scaled by the number of cells; the column is clipped to the point count here (the reference would raise when it exceeds it)."""
    import random

    return [[int(random.random() * (M - 1)), min(int(random.random() * (M - 1)), N - 1)] for _ in range(B)]


def supervise_batch(model, data, ds=None):
    """What the trainers and the evaluator's oracle path do with a batch that carries geometry but no "conf_gt": build the supervision
    (with the reference's fallback draw) and hand the triple to the model.  A batch that has "conf_gt" is left exactly as it is."""
    if "conf_gt" in data or not all(k in data for k in ("K", "c2w", "pt3d", "image")):
        return data
    ds = int(ds if ds is not None else getattr(model, "coarse_ds", 8))
    H, W = data["image"].shape[-2:]
    B = data["pt3d"].shape[0]
    N = data["pt3d"].reshape(B, -1, 3).shape[1]
    coarse_supervision(data, ds=ds, fallback=draw_fallback(B, (H // ds) * (W // ds), N))
    if hasattr(model, "seed_gt_ids"):
        model.seed_gt_ids(data["conf_gt"], data["gt_ids"])
    return data
