"""Reference point sets of a matcher batch from a scene cache that lives on the GPU.

The reference side of a multi-pair sample is the 3-D points, their features and masks taken from the cached renders of the top-k
retrieved frames.  The reference builds it per query on the host (NeRFMatchMultiPair.load_ref_pts, nerfmatch/datasets/nerfmatch_dataset.py:
441-518, reader load_frame_3d, datasets/data_loading.py:36-80): k pickled files, k n stacked rows of 3 + D floats, with `sample_mode`
k projections of all k n points, a sequential co-visibility rule, a randperm draw, then a copy to the device.  A `ReferencePointBank`
keeps the cache (scene_cache.py writes it) on the device with one camera row per frame and makes a batch's sets in place:

    bank = ReferencePointBank.from_scene_dir(scene_dir, rframes, img_wh=(640, 480))
    ref_ids = [bank.draw_ref_ids(pair_ids[q], k=10, split="train") for q in queries]
    bank.fill(data, ref_ids, sample_mode="rand", sample_pts=3600)      # pt3d, pt_feat, pt_mask, rc2w, unnorm_scene
    supervision.supervise_batch(model, data)                           # conf_gt, pt2d_proj, the index triple

`sample_mode=None` is the stacked layout (B,k,n,.) of nerfmatch_dataset.py:585-590.  `sample_mode="rand"` is the rule below, stated once in
plain torch in this file: the behaviour of a bank on host tensors and the specification the kernels (csrc/ref_bank.hip; no fallback) are
tested against.

The rule of "rand" for one query with the frames f_0 .. f_{k-1}:
  1. candidates: the k n rows in row order, candidate c = s n + r = row r of frame f_s.  Bit j of a candidate's 32-bit word is set iff its
     projection into camera j satisfies x >= 0 && y >= 0 && x < W && y < H (:498) at the target resolution (W, H) = img_wh, under
     diag(W / w_j, H / h_j, 1) K_j (:486-490) and the closed-form world-to-camera matrix (supervision.w2c_from_c2w); the projection is
     supervision._project_torch: fp32, a fixed operation order, no contraction.  No depth test; a projection that is not finite sets no bit.
  2. co-visibility (:478, :499-502): visible = all; for j = 0 .. k-1 with I = |visible & bit_j| and V = |visible|: visible | bit_j if
     3 I < V, else visible & bit_j.  `decisions` bit j = 1 where the union was taken.  n_visible >= 1 always (an intersection is only
     taken with 3 I >= V >= 1).
  3. compaction: `list` = the visible candidates in ascending order, Nv = n_visible.
  4. sampling: output row q is list[perm(q mod Nv)] -- the shape of the reference's `idx.repeat(P // Nv + 1)[:P]` with the randperm
     replaced by the RayBank permutation of [0, Nv) (nerf.ray_bank.perm_params / epoch_ids), keyed by (seed, draw, sample_keys[b]): its
     seed is query_seed(seed, sample_keys[b]) and its epoch is `draw`.  The key does not depend on the position
     in the batch, so a query yields the same rows alone or inside any batch.

A bank also answers which frames see each other (`covisibility_pairs`: covis_pairs.py on the bank's own tensors), which is the pair
list `draw_ref_ids` draws from.

Out of scope: image files and annotation parsing; masks other than the ones handed to the constructor."""
import functools

import numpy as np
import torch

from . import covis_pairs, scene_cache, supervision
from .nerf.ray_bank import epoch_ids, perm_params

MAX_K = 32            # one bit per view in a 32-bit word
MAX_CANDIDATES = 1 << 20
MAX_SAMPLE_PTS = 1 << 20
MAX_FEAT_DIM = 1024


# ----------------------------------------------------------------------------- the rule in plain torch
def visibility_words(pt3d, cams, img_wh):
    """pt3d (B,N,3) candidates, cams (B,k,21) = scaled K (9) | w2c rows 0..2 (12) -> (B,N) int64 words: bit j = inside image j."""
    B, N, _ = pt3d.shape
    k = cams.shape[1]
    W, H = float(img_wh[0]), float(img_wh[1])
    K = cams[..., :9].reshape(B * k, 3, 3)
    w2c = cams[..., 9:].reshape(B * k, 3, 4)
    pix, _ = supervision._project_torch(K, w2c, pt3d[:, None].expand(B, k, N, 3).reshape(B * k, N, 3))
    x, y = pix[..., 0], pix[..., 1]
    inside = ((x >= 0) & (y >= 0) & (x < W) & (y < H)).reshape(B, k, N)
    shifts = torch.arange(k, device=pt3d.device, dtype=torch.int64)[None, :, None]
    return (inside.to(torch.int64) << shifts).sum(1)


# The reference writes `intersect.sum() < visible.sum() / 3`: an int64 count against a float32 quotient, compared in float32.
# For integers 0 <= I, V < 2^24 that is the integer test 3 I < V.  I and V are exact in float32.  With t = V / 3: if 3 divides V,
# t is an integer below 2^24, so fl(t) = t and I < t <=> 3 I < V.  Otherwise t lies at least 1/3 from the integers m = floor(t)
# and m + 1; below 2^23 neighbouring floats are at most 1/2 apart, so |fl(t) - t| <= 1/4 < 1/3 and m < fl(t) < m + 1; for an
# integer I then I < fl(t) <=> I <= m <=> I < t <=> 3 I < V.  (k n <= 2^20 here; the golden generator asserts the agreement.)
def covisible(words, k):
    """words (B,N) int64 -> dict(visible (B,N) bool, n_visible (B,) int32, decisions (B,) int32, steps (B,k,3) int64 = (I, V, union) of
    every round).  Torch ops on the words' device; nothing is read back."""
    B, N = words.shape
    visible = torch.ones(B, N, dtype=torch.bool, device=words.device)
    decisions = torch.zeros(B, dtype=torch.int64, device=words.device)
    steps = []
    for j in range(k):
        bit = ((words >> j) & 1).ne(0)
        I, V = (visible & bit).sum(1), visible.sum(1)
        union = 3 * I < V
        visible = torch.where(union[:, None], visible | bit, visible & bit)
        decisions = decisions | (union.to(torch.int64) << j)
        steps.append(torch.stack([I, V, union.to(torch.int64)], -1))
    decisions = torch.where(decisions >= 1 << 31, decisions - (1 << 32), decisions).to(torch.int32)  # (bit 31: the int32 with the same bits)
    return dict(visible=visible, n_visible=visible.sum(1).to(torch.int32), decisions=decisions, steps=torch.stack(steps, 1))


def query_seed(seed, sample_key):
    """The 32-bit seed of one query's permutations: seed ^ (sample_key * 0x85EBCA6B) -- for a fixed bank seed a bijection of the key's low
    32 bits (an odd multiplier); perm_params hashes it together with the draw."""
    return (int(seed) ^ (int(sample_key) * 0x85EBCA6B)) & 0xFFFFFFFF


@functools.lru_cache(maxsize=1 << 16)
def round_keys(seed, sample_key, draw):
    """The 4 round keys of one query's permutation (they do not depend on Nv; the width does).  Cached: an evaluation asks for the same
    (seed, query, draw) every epoch, and the keys are ~10 us of Python integer arithmetic per query."""
    return tuple(perm_params(1, query_seed(seed, sample_key), draw)[0])


def sample_slots(n_visible, rows, seed, draw, sample_key):
    """(rows,) int64: the positions in `list` of the output rows 0 .. rows-1 of one query: perm(q mod Nv)."""
    Nv = int(n_visible)
    return epoch_ids(Nv, query_seed(seed, sample_key), draw, torch.arange(rows) % Nv)


# ----------------------------------------------------------------------------- the bank
class ReferencePointBank:
    def __init__(self, pt3d, pt_feat, c2w, K, frame_wh, img_wh, pt_mask=None, unnorm_scene=None, device="cuda", seed=0):
        """pt3d (F,n,3) fp32 WORLD points of the F cached frames; pt_feat (F,n,D) fp32; c2w (F,4,4) world camera-to-world (the frames'
        `transform_matrix`); K (F,3,3) or (3,3) at the frames' own resolution frame_wh (F,2) or (2,) = (width, height); img_wh = (W, H) the
        target resolution visibility is tested at; pt_mask (F,n) bool (default: all true); unnorm_scene (4,4) only travels into the batch."""
        pt3d = torch.as_tensor(pt3d).detach().to(torch.float32)
        pt_feat = torch.as_tensor(pt_feat).detach().to(torch.float32)
        if pt3d.dim() != 3 or pt3d.shape[-1] != 3 or pt_feat.dim() != 3 or pt_feat.shape[:2] != pt3d.shape[:2] or pt3d.shape[0] < 1 or pt3d.shape[1] < 1:
            raise ValueError("pt3d must be (F,n,3) and pt_feat (F,n,D) with F, n >= 1")
        F, n, D = pt_feat.shape
        if D % 4 or not 0 < D <= MAX_FEAT_DIM:
            raise ValueError(f"feature dimension {D}: a multiple of 4 up to {MAX_FEAT_DIM} is required")
        self.F, self.n, self.D = F, n, D
        self.device = torch.device(device)
        self.seed = int(seed)
        self.img_wh = (int(img_wh[0]), int(img_wh[1]))
        if min(self.img_wh) < 1:
            raise ValueError(f"img_wh {self.img_wh} must be positive")
        c2w = torch.as_tensor(c2w).detach().to("cpu", torch.float32).reshape(F, 4, 4)
        cams = covis_pairs.camera_rows(c2w, K, frame_wh, self.img_wh)  # sK @ rK of nerfmatch_dataset.py:486-490 | w2c rows 0..2
        self.c2w_host = c2w
        self.unnorm_scene = None if unnorm_scene is None else torch.as_tensor(unnorm_scene).detach().to("cpu", torch.float32).reshape(4, 4)
        if pt_mask is None:
            pt_mask = torch.ones(F, n, dtype=torch.bool)
        pt_mask = torch.as_tensor(pt_mask)
        if tuple(pt_mask.shape) != (F, n):
            raise ValueError("pt_mask must be (F,n)")
        dev = self.device
        self.pt3d = pt3d.contiguous().to(dev)
        self.pt_feat = pt_feat.contiguous().to(dev)
        self.pt_mask = pt_mask.ne(0).contiguous().to(dev)
        self.cams = cams.to(dev)
        self.c2w = c2w.contiguous().to(dev)
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)

    @classmethod
    def from_scene_dir(cls, scene_dir, frames, img_wh, use_msk=None, **kw):
        """A bank over the cache files of `frames`: the reference's frame dictionaries (file_path, transform_matrix, intrinsics, width,
        height; nerfmatch_dataset.py:451-490), read by scene_cache.load_frame_3d under the reference's file-name rule (data_loading.py:40).
        The cache format carries no masks: use_msk must be None.  Frames whose cache differs in n or D raise."""
        from pathlib import Path

        if use_msk:
            raise ValueError("scene_cache.load_frame_3d reads no masks: pass pt_mask to the constructor instead of use_msk")
        if not len(frames):
            raise ValueError("no frames")
        pts, feats, masks, unnorm = [], [], [], None
        for fr in frames:
            name = fr["file_path"].replace("/", "_").replace(".color", "").replace(".png", "")
            p3, pf, pm, unnorm = scene_cache.load_frame_3d(Path(scene_dir) / f"{name}.npy")
            if pts and (p3.shape != pts[0].shape or pf.shape != feats[0].shape):
                raise ValueError(f"{name}.npy holds {p3.shape[0]} points of {pf.shape[-1]} features, the first frame {pts[0].shape[0]} of {feats[0].shape[-1]}")
            pts.append(np.asarray(p3, np.float32)); feats.append(np.asarray(pf, np.float32)); masks.append(np.asarray(pm, np.bool_))
        c2w = torch.tensor(np.array([fr["transform_matrix"] for fr in frames]), dtype=torch.float32)
        K = torch.tensor(np.array([fr["intrinsics"] for fr in frames]), dtype=torch.float32)
        wh = torch.tensor([[fr["width"], fr["height"]] for fr in frames], dtype=torch.float32)
        return cls(torch.from_numpy(np.stack(pts)), torch.from_numpy(np.stack(feats)), c2w, K, wh, img_wh, pt_mask=torch.from_numpy(np.stack(masks)),
                   unnorm_scene=unnorm, **kw)

    @staticmethod
    def draw_ref_ids(rids, k, split, rng=None):
        """The reference's choice of a query's frames (nerfmatch_dataset.py:446-449): split "train" draws k ids with replacement (rng: a
        numpy Generator or RandomState; default numpy's global state, as there), any other split takes rids[:k] and raises on fewer."""
        rids = [int(r) for r in rids]
        if split == "train":
            if not rids:
                raise ValueError("no reference frames to draw from")
            return [int(r) for r in (np.random if rng is None else rng).choice(rids, int(k))]
        if len(rids) < k:
            raise ValueError(f"{len(rids)} reference frames, {k} are needed")
        return rids[:k]

    def covisibility_pairs(self, k=20, depth_tol=None, ds=None, rows=None, min_score=1):
        """The k most covisible frames of every frame of the bank (or of `rows`), by the rule of covis_pairs.py on the bank's points, masks
        and camera rows -> ids (Q,k) int32 padded with -1, n_pairs (Q,) int32, on the bank's device; covis_pairs.pairs_dict(rows, ids) is the
        `pair_ids` draw_ref_ids takes its rows from.  depth_tol with ds: the depth test on the grid (W // ds, H // ds) of the frames'
        points (the coarse stride they were rendered at)."""
        if (depth_tol is None) != (ds is None):
            raise ValueError("the depth test needs both depth_tol and ds")
        grid_wh = None if ds is None else (self.img_wh[0] // int(ds), self.img_wh[1] // int(ds))
        return covis_pairs.covisibility_pairs(self.pt3d, self.pt_mask, self.cams, self.img_wh, rows=rows, depth_tol=depth_tol, grid_wh=grid_wh,
                                              k=k, min_score=min_score)

    @property
    def bad_ids(self):
        """how many frame ids the device path has clamped into the bank so far (synchronises)"""
        return int(self._bad.item())

    # ------------------------------------------------------------------------- arguments
    def _ids(self, ref_ids):
        """(B,k) int64 on the bank's device.  Ids given on the host are checked and an id outside the bank raises; ids already on the bank's
        GPU are not read back: the kernels clamp them and count them in `bad_ids`."""
        ref_ids = torch.as_tensor(ref_ids).to(torch.int64)
        if ref_ids.dim() != 2 or ref_ids.shape[0] < 1 or ref_ids.shape[1] < 1:
            raise ValueError("ref_ids must be (B,k) with B, k >= 1")
        k = ref_ids.shape[1]
        if k > MAX_K or k * self.n > MAX_CANDIDATES:
            raise ValueError(f"k = {k} views of {self.n} points: at most {MAX_K} views and {MAX_CANDIDATES} candidates per query")
        if ref_ids.device.type == "cpu" and (int(ref_ids.min()) < 0 or int(ref_ids.max()) >= self.F):
            raise ValueError(f"frame ids outside [0, {self.F})")
        return ref_ids.to(self.device).contiguous()

    def _frames(self, ref_ids):
        return ref_ids.clamp(0, self.F - 1)

    # ------------------------------------------------------------------------- the rule
    def select(self, ref_ids):
        """Steps 1-3 for the id rows ref_ids (B,k) -> dict(words (B,k n): the visibility words (int32 holding the uint32 bits on a GPU
        bank, int64 on a host bank), list (B,k n) int32: the visible candidates in ascending order, then -1, n_visible (B,) int32,
        decisions (B,) int32).  A GPU bank: two launches, nothing read back."""
        ref_ids = self._ids(ref_ids)
        if self.device.type != "cpu":
            from . import ops

            return ops.refbank_select(self.pt3d, self.cams, ref_ids, self.img_wh)
        return self._select_torch(ref_ids)

    def _select_torch(self, ref_ids):
        f = self._frames(ref_ids)
        B, k = f.shape
        N = k * self.n
        words = visibility_words(self.pt3d[f].reshape(B, N, 3), self.cams[f], self.img_wh)
        out = covisible(words, k)
        order = torch.arange(N, device=words.device).expand(B, N)
        # ascending candidates first: a stable sort of "not visible"
        lst = torch.gather(order, 1, torch.argsort((~out["visible"]).to(torch.int8), dim=1, stable=True))
        lst = torch.where(order < out["n_visible"][:, None], lst, torch.full_like(lst, -1)).to(torch.int32)
        return dict(words=words, list=lst, n_visible=out["n_visible"], decisions=out["decisions"], steps=out["steps"], visible=out["visible"])

    def _sets_torch(self, ref_ids, sample_mode, P, sample_keys, draw):
        """reference_sets in torch ops, on the bank's tensors wherever they live (the sampled mode reads n_visible back)."""
        f = self._frames(ref_ids)
        B, k = f.shape
        N = k * self.n
        if sample_mode is None:
            sel = dict(n_visible=torch.full((B,), N, dtype=torch.int32, device=f.device), decisions=torch.zeros(B, dtype=torch.int32, device=f.device))
            src = torch.arange(N, device=f.device).expand(B, N)
        else:
            sel = self._select_torch(ref_ids)
            nv = sel["n_visible"].tolist()
            slots = torch.stack([sample_slots(nv[b], P, self.seed, draw, sample_keys[b]) for b in range(B)]).to(f.device)
            src = torch.gather(sel["list"].to(torch.int64), 1, slots)
        rows = torch.gather(f, 1, src // self.n) * self.n + src % self.n
        return (self.pt3d.reshape(-1, 3)[rows], self.pt_feat.reshape(-1, self.D)[rows], self.pt_mask.reshape(-1)[rows]), sel

    def reference_sets(self, ref_ids, sample_mode=None, sample_pts=-1, sample_keys=None, draw=0, out=None):
        """The reference sets of the queries whose frames are the rows of ref_ids (B,k) -> dict(pt3d, pt_feat, pt_mask, rc2w (B,4,4),
        unnorm_scene (B,4,4) or None, n_visible (B,) int32, decisions (B,) int32).

        sample_mode=None: the stacked layout pt3d (B,k,n,3), pt_feat (B,k,n,D), pt_mask (B,k,n) of nerfmatch_dataset.py:585-590;
          n_visible = k n; rc2w is the pose of the FIRST frame of the row (:452-453).
        sample_mode="rand" with sample_pts = P > 0: pt3d (B,P,3), pt_feat (B,P,D), pt_mask (B,P) by the rule in the module docstring.
          rc2w is the pose of the LAST frame of the row -- a quirk of the reference that is kept: its visibility loop (:480-482) reuses
          the name `rc2w`, and the loop variable's last value is what :518 returns.  P <= 0 raises: the reference then returns Nv rows, a
          ragged length that no batch can hold.
        sample_keys: B host integers that key each query's permutation together with the bank's seed and `draw` (default 0 .. B-1; pass
          the query ids to make a query's rows independent of its batch).  out: (pt3d, pt_feat, pt_mask) to write into (GPU bank).
        A GPU bank: one launch (stacked) or three (rand) on the current stream, no host read-back."""
        ref_ids = self._ids(ref_ids)
        B, k = ref_ids.shape
        n, D = self.n, self.D
        if sample_mode not in (None, "rand"):
            raise ValueError(f"sample_mode must be None or 'rand', got {sample_mode!r}")
        P = k * n
        if sample_mode == "rand":
            P = int(sample_pts)
            if P <= 0:
                raise ValueError("sample_mode='rand' needs sample_pts > 0 (the reference returns a ragged n_visible rows without it)")
            if P > MAX_SAMPLE_PTS:
                raise ValueError(f"sample_pts {P} above {MAX_SAMPLE_PTS}")
        keys = list(range(B)) if sample_keys is None else [int(v) for v in sample_keys]
        if len(keys) != B:
            raise ValueError(f"{len(keys)} sample_keys for {B} queries")
        if self.device.type == "cpu":
            (p3, pf, pm), sel = self._sets_torch(ref_ids, sample_mode, P, keys, draw)
        else:
            from . import ops

            if sample_mode is None:
                sel = dict(n_visible=torch.full((B,), P, dtype=torch.int32, device=self.device),
                           decisions=torch.zeros(B, dtype=torch.int32, device=self.device))
                p3, pf, pm = ops.refbank_gather(self.pt3d, self.pt_feat, self.pt_mask, ref_ids, self._bad, P, out=out)
            else:
                sel = ops.refbank_select(self.pt3d, self.cams, ref_ids, self.img_wh)
                rk = [round_keys(self.seed, key, int(draw)) for key in keys]
                rk = torch.tensor([[v - (1 << 32) if v >= 1 << 31 else v for v in row] for row in rk], dtype=torch.int32).to(self.device, non_blocking=True)
                p3, pf, pm = ops.refbank_gather(self.pt3d, self.pt_feat, self.pt_mask, ref_ids, self._bad, P, select=sel, perm_keys=rk, out=out)
        if sample_mode is None:
            p3, pf, pm = p3.reshape(B, k, n, 3), pf.reshape(B, k, n, D), pm.reshape(B, k, n)
        rc2w = self.c2w[self._frames(ref_ids[:, 0 if sample_mode is None else -1])]
        unnorm = None if self.unnorm_scene is None else self.unnorm_scene[None].expand(B, 4, 4).clone()
        return dict(pt3d=p3, pt_feat=pf, pt_mask=pm, rc2w=rc2w, unnorm_scene=unnorm, n_visible=sel["n_visible"], decisions=sel["decisions"])

    def fill(self, data, ref_ids, **kw):
        """Writes pt3d, pt_feat, pt_mask, rc2w (and unnorm_scene, when the bank has one) of reference_sets(ref_ids, **kw) into the batch
        dictionary `data`; supervision.supervise_batch(model, data) then completes the batch."""
        out = self.reference_sets(ref_ids, **kw)
        data.update({key: out[key] for key in ("pt3d", "pt_feat", "pt_mask", "rc2w")})
        if out["unnorm_scene"] is not None:
            data["unnorm_scene"] = out["unnorm_scene"]
        return data
