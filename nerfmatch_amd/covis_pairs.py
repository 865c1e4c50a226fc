"""Covisibility pair lists of a scene, from its cached renders alone.

Matcher training reads a pair list: for every query frame the reference frames that see the same part of the scene
(`train_pair_txt: .../pairs-db-covis20.txt`, parsed by load_retrieval_pairs / load_topk_retrieval_pairs, nerfmatch/datasets/
data_loading.py:94-127).  The reference does not make these lists: they come from the sparse model of an SfM toolchain.  The scene
cache (scene_cache.py) already holds what the question needs: every frame's rendered 3-D points in ray order -- a depth map per frame --
and one camera row per frame.  "How many of frame j's points does frame i see" is F^2 n projections:

    cams = camera_rows(c2w, K, frame_wh, img_wh)                                  # the rows a ReferencePointBank keeps
    ids, n_pairs = covisibility_pairs(pt3d, pt_mask, cams, img_wh, k=20, depth_tol=0.05, grid_wh=(80, 60))
    write_pairs_txt("pairs-db-covis20.txt", names, None, ids)                     # a train_pair_txt
    pair_ids = pairs_dict(None, ids)                                              # or straight to ReferencePointBank.draw_ref_ids

The rule, stated once in plain torch in this file: the behaviour on host tensors and the specification the kernels (csrc/covis_pairs.hip;
no fallback) are tested against.  Inputs: pt3d (F,n,3) fp32 world points of the F cached frames in ray order, pt_mask (F,n) bool,
cams (F,21) = diag(W / w_f, H / h_f, 1) K_f | w2c rows 0..2, img_wh = (W, H); with the depth test also grid_wh = (gw, gh) with
gw gh == n (the frames' points are one per cell of a gw x gh grid over the image, row-major) and depth_tol >= 0.  The projection is
supervision._project_torch: p = R X + t, q = p / p.z, pix = K q, every product and sum a separate fp32 operation in that order, true
division, no contraction.
  1. own depth (depth test only): zself[f, r] = p.z of point (f, r) under camera f.
  2. seen: point X is seen by frame i iff pix is finite, p.z > 0, x >= 0, y >= 0, x < W, y < H -- unlike ref_bank.visibility_words and
     the supervision kernel there IS a depth-sign test: those two reproduce a quirk of the reference, a pair list must not pair frames
     that look in opposite directions.  With the depth test also: the cell c = ((int)y gh / H) gw + (int)x gw / W (integer arithmetic
     on the truncated pixel) has pt_mask[i, c] set, zq = zself[i, c] > 0 and |p.z - zq| <= depth_tol zq (one fp32 product): a point
     of j counts only where frame i's own rendered surface is at the same depth -- the occlusion test an SfM track gives for free.
  3. score[i, j] = #{ r : pt_mask[j, r] and (j, r) seen by i }, int32, for every i in `rows` (default: all frames) and every j; the
     diagonal like any other entry.  The score of a pair depends on the two frames alone.
  4. top-k: the candidates of row i are the j != i with score[i, j] >= min_score, ordered by score descending, then index ascending
     -> ids (Q,k) int32 padded with -1, n_pairs (Q,) int32.

Features are not needed: the functions work for scenes whose features do not fit on the device.  Out of scope: annotation parsing."""
import torch

from . import supervision

MAX_FRAMES = 1 << 20
MAX_POINTS = 1 << 20
MAX_K = 64
MAX_SIDE = 8192
MAX_SCORES = 1 << 31
QUERY_TILE = 32       # NM_COVIS_QUERY_TILE of include/nerfmatch_amd.h: query cameras per workgroup of nm_covis_scores


def camera_rows(c2w, K, frame_wh, img_wh):
    """One camera row per frame, (F,21) fp32 on the host: row-major diag(W / w_f, H / h_f, 1) K_f (9; nerfmatch_dataset.py:486-490) |
    rows 0..2 of the closed-form world-to-camera matrix (12; supervision.w2c_from_c2w).  c2w (F,4,4); K (F,3,3) or (3,3) at the frames'
    own resolution frame_wh (F,2) or (2,) = (width, height); img_wh = (W, H) the resolution visibility is tested at."""
    c2w = torch.as_tensor(c2w).detach().to("cpu", torch.float32)
    F = c2w.shape[0]
    c2w = c2w.reshape(F, 4, 4)
    K = torch.as_tensor(K).detach().to("cpu", torch.float32)
    K = K.expand(F, 3, 3) if K.dim() == 2 else K.reshape(F, 3, 3)
    wh = torch.as_tensor(frame_wh).detach().to("cpu", torch.float32)
    wh = wh.expand(F, 2) if wh.dim() == 1 else wh.reshape(F, 2)
    # sK @ rK in fp32 (a diagonal times a matrix: one product per entry, the same bits as the matmul)
    scale = torch.stack([int(img_wh[0]) / wh[:, 0], int(img_wh[1]) / wh[:, 1], torch.ones(F)], -1)
    sK = scale[:, :, None] * K
    return torch.cat([sK.reshape(F, 9), supervision.w2c_from_c2w(c2w).reshape(F, 12)], 1).contiguous()


# ----------------------------------------------------------------------------- the rule in plain torch
def _split(cams):
    return cams[:, :9].reshape(-1, 3, 3), cams[:, 9:].reshape(-1, 3, 4)


def self_depth(pt3d, cams):
    """Step 1: (F,n) fp32, p.z of every frame's points under its own camera."""
    K, w2c = _split(cams)
    return supervision._project_torch(K, w2c, pt3d)[1]


def _seen_torch(pt3d, pt_mask, cams, rows, img_wh, zself, grid_wh, depth_tol):
    """(Q,F,n) bool: point (j, r) is seen by frame rows[q] (step 2)."""
    F, n, _ = pt3d.shape
    Q = rows.shape[0]
    W, H = int(img_wh[0]), int(img_wh[1])
    K, w2c = _split(cams[rows])
    pix, pz = supervision._project_torch(K, w2c, pt3d.reshape(1, F * n, 3).expand(Q, F * n, 3))
    x, y = pix[..., 0], pix[..., 1]
    seen = torch.isfinite(pix).all(-1) & (pz > 0) & (x >= 0) & (y >= 0) & (x < W) & (y < H)
    if zself is not None:
        gw, gh = int(grid_wh[0]), int(grid_wh[1])
        zero = torch.zeros_like(x)
        xi, yi = torch.where(seen, x, zero).to(torch.int64), torch.where(seen, y, zero).to(torch.int64)  # truncation, of pixels inside the image
        c = (yi * gh // H) * gw + xi * gw // W
        zq = torch.gather(zself[rows], 1, c)
        tol = torch.tensor(float(depth_tol), dtype=torch.float32, device=pt3d.device)
        seen = seen & torch.gather(pt_mask[rows], 1, c) & (zq > 0) & ((pz - zq).abs() <= tol * zq)
    return seen.reshape(Q, F, n)


def _scores_torch(pt3d, pt_mask, cams, rows, img_wh, depth_tol, grid_wh, chunk=1 << 24):
    F, n, _ = pt3d.shape
    zself = None if depth_tol is None else self_depth(pt3d, cams)
    step = max(1, chunk // (F * n))  # rows per pass: about `chunk` projections
    out = [(_seen_torch(pt3d, pt_mask, cams, rows[q0 : q0 + step], img_wh, zself, grid_wh, depth_tol) & pt_mask[None]).sum(-1)
           for q0 in range(0, rows.shape[0], step)]
    return torch.cat(out).to(torch.int32)


def _topk_torch(scores, rows, k, min_score):
    """Step 4 on a score matrix (Q,F) with the frames `rows` (Q,) of its rows -> ids (Q,k) int32, n_pairs (Q,) int32."""
    Q, F = scores.shape
    j = torch.arange(F, device=scores.device)
    cand = (j[None] != rows[:, None]) & (scores >= min_score) & (scores >= 0)  # (a count is never negative: a row handed to topk_pairs may be)
    # (score, F - 1 - j) packed: distinct for distinct j, so the order of the sort is total
    key = torch.where(cand, scores.to(torch.int64) * F + (F - 1 - j)[None], torch.full((), -1, dtype=torch.int64, device=scores.device))
    key, order = torch.sort(key, dim=1, descending=True, stable=True)
    ids = torch.full((Q, k), -1, dtype=torch.int32, device=scores.device)
    m = min(k, F)
    ids[:, :m] = torch.where(key[:, :m] >= 0, order[:, :m], torch.full_like(order[:, :m], -1)).to(torch.int32)
    return ids, cand.sum(1).clamp(max=k).to(torch.int32)


# ----------------------------------------------------------------------------- arguments
def _check(pt3d, pt_mask, cams, img_wh, rows, depth_tol, grid_wh):
    if pt3d.dim() != 3 or pt3d.shape[-1] != 3 or pt3d.shape[0] < 1 or pt3d.shape[1] < 1 or pt3d.dtype != torch.float32:
        raise ValueError("pt3d must be (F,n,3) fp32 with F, n >= 1")
    F, n, _ = pt3d.shape
    if tuple(pt_mask.shape) != (F, n) or pt_mask.dtype != torch.bool:
        raise ValueError("pt_mask must be (F,n) bool")
    if tuple(cams.shape) != (F, 21) or cams.dtype != torch.float32:
        raise ValueError("cams must be (F,21) fp32: camera_rows makes them")
    if pt_mask.device != pt3d.device or cams.device != pt3d.device:
        raise ValueError("pt3d, pt_mask and cams must live on one device")
    W, H = int(img_wh[0]), int(img_wh[1])
    if min(W, H) < 1:
        raise ValueError(f"img_wh {(W, H)} must be positive")
    if F > MAX_FRAMES or n > MAX_POINTS or max(W, H) > MAX_SIDE:
        raise ValueError(f"{F} frames of {n} points at {W} x {H}: at most {MAX_FRAMES} frames, {MAX_POINTS} points and sides of {MAX_SIDE}")
    if (depth_tol is None) != (grid_wh is None):
        raise ValueError("the depth test needs both depth_tol and grid_wh")
    if depth_tol is not None:
        gw, gh = int(grid_wh[0]), int(grid_wh[1])
        if gw < 1 or gh < 1 or gw * gh != n or max(gw, gh) > MAX_SIDE:
            raise ValueError(f"grid_wh {(gw, gh)} must have gw * gh == n = {n} and sides up to {MAX_SIDE}")
        if not float(depth_tol) >= 0.0 or float(depth_tol) == float("inf"):
            raise ValueError(f"depth_tol {depth_tol} must be finite and >= 0")
        grid_wh, depth_tol = (gw, gh), float(depth_tol)
    if rows is None:
        rows_t = torch.arange(F, dtype=torch.int64)
    else:
        rows_t = torch.as_tensor(rows).detach().to("cpu", torch.int64).reshape(-1)
        if rows_t.numel() < 1 or int(rows_t.min()) < 0 or int(rows_t.max()) >= F:
            raise ValueError(f"rows must be a non-empty list of frame ids in [0, {F})")
    if rows_t.numel() > MAX_FRAMES or rows_t.numel() * F > MAX_SCORES:
        raise ValueError(f"{rows_t.numel()} rows of {F} scores: at most {MAX_FRAMES} rows and {MAX_SCORES} scores")
    return (W, H), rows_t, depth_tol, grid_wh


def _check_k(k):
    k = int(k)
    if not 0 < k <= MAX_K:
        raise ValueError(f"k = {k}: between 1 and {MAX_K}")
    return k


# ----------------------------------------------------------------------------- the public functions
def _scores(pt3d, pt_mask, cams, img_wh, rows, depth_tol, grid_wh):
    """-> scores (Q,F) int32 and the rows (Q,) on the tensors' device (int64 on the host, int32 on a GPU)"""
    img_wh, rows_t, depth_tol, grid_wh = _check(pt3d, pt_mask, cams, img_wh, rows, depth_tol, grid_wh)
    if not pt3d.is_cuda:
        return _scores_torch(pt3d, pt_mask, cams, rows_t, img_wh, depth_tol, grid_wh), rows_t
    from . import ops

    pt3d, pt_mask, cams = pt3d.contiguous(), pt_mask.contiguous(), cams.contiguous()
    rows_d = rows_t.to(torch.int32).to(pt3d.device)
    zself = None if depth_tol is None else ops.covis_self_depth(pt3d, cams, pt_mask)  # (NaN where the mask is clear: one gather per point)
    return ops.covis_scores(pt3d, pt_mask, cams, rows_d, img_wh, zself=zself, grid_wh=grid_wh, depth_tol=depth_tol), rows_d


def covisibility_scores(pt3d, pt_mask, cams, img_wh, rows=None, depth_tol=None, grid_wh=None):
    """score[q, j] = how many of frame j's masked points frame rows[q] sees (steps 1-3 of the rule in the module docstring) -> (Q,F) int32
    on the tensors' device.  rows: host frame ids (default: all frames, Q = F).  depth_tol with grid_wh = (gw, gh): the depth test.
    CUDA tensors: nm_covis_self_depth + nm_covis_scores on the current stream, no read-back; host tensors: the torch rule."""
    return _scores(pt3d, pt_mask, cams, img_wh, rows, depth_tol, grid_wh)[0]


def topk_pairs(scores, rows=None, k=20, min_score=1):
    """Step 4 on a score matrix (Q,F) int32 whose row q belongs to frame rows[q] (default: row q to frame q)
    -> ids (Q,k) int32 padded with -1, n_pairs (Q,) int32.  CUDA scores: nm_covis_topk, no read-back."""
    k = _check_k(k)
    if scores.dim() != 2 or scores.dtype != torch.int32 or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise ValueError("scores must be (Q,F) int32")
    Q, F = scores.shape
    rows_t = torch.arange(Q) if rows is None else torch.as_tensor(rows).detach().reshape(-1)
    if rows_t.numel() != Q:
        raise ValueError(f"{rows_t.numel()} rows for {Q} score rows")
    if not scores.is_cuda:
        return _topk_torch(scores, rows_t.to("cpu", torch.int64), k, int(min_score))
    from . import ops

    return ops.covis_topk(scores.contiguous(), rows_t.to(device=scores.device, dtype=torch.int32), k, int(min_score))


def covisibility_pairs(pt3d, pt_mask, cams, img_wh, rows=None, depth_tol=None, grid_wh=None, k=20, min_score=1):
    """The k most covisible frames of every frame in `rows` (the whole rule) -> ids (Q,k) int32: row q lists the frames j != rows[q] with
    score >= min_score by score descending, then index ascending, padded with -1; n_pairs (Q,) int32.  CUDA tensors take the kernels
    (three launches, nothing read back, no fallback), host tensors the torch rule."""
    k = _check_k(k)
    scores, rows_t = _scores(pt3d, pt_mask, cams, img_wh, rows, depth_tol, grid_wh)
    return topk_pairs(scores, rows_t, k, min_score)


def pairs_dict(rows, ids):
    """{query frame id: [reference frame ids in rank order]} from covisibility_pairs' ids (Q,k) and its rows (None: row q is frame q): the
    `pair_ids` whose entries ReferencePointBank.draw_ref_ids(pair_ids[q], ...) consumes.  One read-back, at set-up time."""
    ids = torch.as_tensor(ids).detach().cpu().tolist()
    rows = range(len(ids)) if rows is None else [int(r) for r in torch.as_tensor(rows).reshape(-1).tolist()]
    if len(rows) != len(ids):
        raise ValueError(f"{len(rows)} rows for {len(ids)} id rows")
    return {q: [j for j in row if j >= 0] for q, row in zip(rows, ids)}


def write_pairs_txt(path, names, rows, ids):
    """Writes the pair list as the text file the reference's load_retrieval_pairs / load_topk_retrieval_pairs parse (data_loading.py:94-127):
    one `qname rname` line per pair, the queries in row order and the references in rank order.  names: the frames' names (their
    `file_path`), one per frame of the bank, without white space.  -> the number of lines."""
    names = [str(v) for v in names]
    for name in names:
        if not name or len(name.split()) != 1:
            raise ValueError(f"frame name {name!r}: a line is split at white space")
    lines = [f"{names[q]} {names[j]}\n" for q, rids in pairs_dict(rows, ids).items() for j in rids]
    with open(path, "w") as f:
        f.writelines(lines)
    return len(lines)


def read_pairs_txt(path, qnames, rnames):
    """{query id: [reference ids in file order]} of a pair file, with the ids the positions in qnames / rnames; a line whose query or
    reference is in neither list is skipped, as the test branch of the reference's parse_multipair_ids_balanced does
    (data_loading.py:136-147).  Only the first two fields of a line count (load_topk_retrieval_pairs)."""
    qid = {str(v): i for i, v in enumerate(qnames)}
    rid = {str(v): i for i, v in enumerate(rnames)}
    out = {}
    with open(path) as f:
        for line in f:
            pair = line.split()[:2]
            if len(pair) < 2 or pair[0] not in qid:
                continue
            rids = out.setdefault(qid[pair[0]], [])
            if pair[1] in rid:
                rids.append(rid[pair[1]])
    return out
