"""Training and validation ray batches from frames that live on the GPU.

The reference's NerfBaseDataset (nerfmatch/datasets/nerfbase.py) expands every pixel of every training frame into a 12-float ray row,
an rgb row and an id on the CPU (`load_sample` :255-321), concatenates them into one host table (`process_train_data` :351-385) and lets
a shuffling DataLoader index it: 64 bytes of host memory per pixel and one copy per step.  A `RayBank` keeps the frames as uint8 with
one camera row per frame and produces the same rows where they are needed:

    bank = RayBank(images_u8, c2w, K, batch_rays=9216, device="cuda")
    NerfTrainer(cfg, num_frames=F).fit(bank, max_epochs=...)          # one kernel launch per training batch, no host work
    trainer.validation_step(bank.frame_batch(f))                      # one view
    trainer.validation_step(bank.pair_batch(f1, f2))                  # two views: adds the pose metrics

The rules, all from the reference:
  * pixel (x, y) of frame f has the direction [x, y, 1] . Kinv^T . R^T with INTEGER coordinates (render_utils.py:23-41); columns 3:6 of
    a ray row are the unit directions (`norm_ray_dir`, the default) or the unnormalised ones; columns 8:11 always the unit ones;
  * near = 0.01, far = the unit sphere's far intersection along the unit direction -- or exactly 1 for EVERY ray of a frame in which some
    pixel misses the sphere (the try / except of nerfbase.py:287-293): a per-frame flag, computed once when the bank is built;
  * radius = |d(x, y) - d(x, y + 1)| * 2 / sqrt(12) with d = columns 3:6; the last image row takes the value of row H - 3
    (`dx[-2:-1]`, render_utils.py:94-95), so H >= 3;
  * rgb = uint8 / 255 (torchvision's to_tensor); the `mask` key is 1 - round(mask / 255) and, with `exclude_masks`, only pixels where
    that is 1 are trained on (mask_transient, nerfbase.py:225-237).

An epoch visits every training pixel once in a shuffled order that is never materialised: position p of epoch e is pixel
`epoch_ids(N, seed, e, p)`, a keyed bijection of [0, N) that the gather kernel evaluates per ray.  Batch k of rank r in a world of w
ranks takes positions k R w + r R + [0, R): what a position yields depends neither on R nor on w; the last partial batch is dropped.

A bank on a GPU runs the HIP kernels (csrc/ray_bank.hip; no fallback).  A bank on device="cpu" takes the plain-torch statements of the
same rules below, which are also what the kernels are tested against.  The bank starts from uint8 tensors at the training resolution:
image_prep.nerf_frames resizes and blends decoded frames; decoding image files and annotation parsing stay with the caller."""
import math

import torch

from .. import dist as nmdist

NEAR_PLANE = 0.01  # nerfbase.py:297
ROUNDS = 4
_M32 = 0xFFFFFFFF


# ----------------------------------------------------------------------------- the epoch permutation
def _mix32_int(x):
    """nm_mix32 (csrc/common.h) on a Python int."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def perm_params(N, seed, epoch):
    """(round keys, half_bits) of the permutation of [0, N) for (seed, epoch).  2 * half_bits is the smallest even number of bits with
    2^bits >= N; the keys are mix(mix(mix(seed ^ 0x9E3779B9) + epoch) + k + 1), k = 0..3, in 32-bit unsigned arithmetic."""
    N = int(N)
    if not 1 <= N <= 1 << 40:
        raise ValueError(f"the permutation is defined for 1 <= N <= 2^40, got {N}")
    half_bits = ((N - 1).bit_length() + 1) // 2
    v = _mix32_int(_mix32_int((int(seed) & _M32) ^ 0x9E3779B9) + (int(epoch) & _M32))
    return [_mix32_int(v + k + 1) for k in range(ROUNDS)], half_bits


def _mul32(x, c):
    """(x * c) mod 2^32 for an int64 tensor 0 <= x < 2^32 and a constant c < 2^32, without leaving the int64 range."""
    lo = (x & 0xFFFF) * c
    hi = ((x >> 16) * c) & 0xFFFF
    return (lo + (hi << 16)) & _M32


def _mix32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def _feistel(x, keys, half_bits):
    m = (1 << half_bits) - 1
    l, r = x >> half_bits, x & m
    for key in keys:
        l, r = r, l ^ (_mix32((r + key) & _M32) & m)
    return (l << half_bits) | r


def epoch_ids(N, seed, epoch, positions):
    """The index in [0, N) at `positions` (int64 tensor on any device, every entry in [0, N)) of epoch `epoch`: a keyed bijection of
    [0, N), so the positions 0 .. N-1 of one epoch yield every index once.  A balanced Feistel network over 2 * half_bits bits with the
    32-bit mix as round function -- (l, r) -> (r, l ^ (mix(r + key) & (2^half_bits - 1))), four rounds -- re-applied while the value is
    >= N (cycle walking: the walk stays on the start point's own cycle, which contains a value below N, the start point itself; the domain
    is smaller than 4 N, so it takes fewer than 4 passes on average).  The specification nm_raybank_gather's permutation is tested against,
    and the path of a host bank."""
    pos = torch.as_tensor(positions).to(torch.int64)
    if pos.numel() and (int(pos.min()) < 0 or int(pos.max()) >= N):
        raise ValueError(f"positions outside [0, {N})")
    keys, half_bits = perm_params(N, seed, epoch)
    x = _feistel(pos, keys, half_bits)
    while True:
        out = x >= N
        if not bool(out.any()):
            return x
        x = torch.where(out, _feistel(x, keys, half_bits), x)


def batch_positions(k, batch_rays, rank=None, world_size=None):
    """(first position, count) of batch k of `rank`: k R w + r R + [0, R)."""
    if rank is None or world_size is None:
        rank, world_size = nmdist.world()
    return (k * world_size + rank) * batch_rays, batch_rays


# ----------------------------------------------------------------------------- the bank
class RayBank:
    def __init__(self, images_u8, c2w, K, ts=None, masks_u8=None, exclude_masks=True, norm_ray_dir=True, batch_rays=9216, seed=0,
                 device="cuda", unnorm_scene=None, img_idx=None, rank=None, world_size=None):
        """images_u8 (F,H,W,3) uint8; c2w (F,4,4) NORMALISED camera-to-world (the reference's cam2s_scene); K (3,3) or (F,3,3) at the
        images' resolution; ts (F,) the frames' appearance ids (seq_ind; default arange); masks_u8 (F,H,W) transient masks as loaded
        ('L' images); unnorm_scene (4,4) and img_idx (list) only travel into the validation dictionaries."""
        images_u8 = torch.as_tensor(images_u8)
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
            raise ValueError("images_u8 must be a (F,H,W,3) uint8 tensor")
        F, H, W, _ = images_u8.shape
        if H < 3:
            raise ValueError("H >= 3 is required (the last row's cone radius is that of row H-3)")
        self.F, self.H, self.W = F, H, W
        self.device = torch.device(device)
        self.norm_ray_dir, self.batch_rays, self.seed, self.epoch = bool(norm_ray_dir), int(batch_rays), int(seed), 0
        self.rank, self.world_size = nmdist.world() if rank is None or world_size is None else (int(rank), int(world_size))
        c2w = torch.as_tensor(c2w).detach().to("cpu", torch.float32).reshape(F, 4, 4)
        K = torch.as_tensor(K).detach().to("cpu", torch.float32)
        self.K = K.expand(F, 3, 3) if K.dim() == 2 else K.reshape(F, 3, 3)
        kinv = torch.linalg.inv(K)  # fp32 on the host, as ops.raygen does (one inverse for a shared K: the same bits as there)
        kinv = kinv.expand(F, 3, 3) if K.dim() == 2 else kinv.reshape(F, 3, 3)
        self.c2w_host = c2w
        self.unnorm_scene = None if unnorm_scene is None else torch.as_tensor(unnorm_scene).detach().to("cpu", torch.float32).reshape(4, 4)
        ts = torch.arange(F) if ts is None else torch.as_tensor(ts).reshape(F)
        self.seq_ind = [int(v) for v in ts]
        self.img_idx = list(range(F)) if img_idx is None else list(img_idx)
        self.img_wh = torch.tensor([[W, H]])
        dev = self.device
        self.images = images_u8.contiguous().to(dev)
        self.cams = torch.cat([kinv.reshape(F, 9), c2w[:, :3, :].reshape(F, 12)], 1).contiguous().to(dev)
        self.ts_table = ts.to(torch.int64).contiguous().to(dev)
        self.masks = None
        if masks_u8 is not None:
            masks_u8 = torch.as_tensor(masks_u8)
            if masks_u8.dtype != torch.uint8 or tuple(masks_u8.shape) != (F, H, W):
                raise ValueError("masks_u8 must be a (F,H,W) uint8 tensor")
            self.masks = masks_u8.contiguous().to(dev)
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self._grids = {}
        if dev.type == "cpu":
            self.flags = torch.stack([self._host_frame_flag(f) for f in range(F)]).to(torch.int32)
        else:
            from .. import ops

            self.flags = ops.raybank_frame_flags(self.cams, H, W)
        # the pixels an epoch visits: all of them, or (exclude_masks) those whose `mask` value is 1 -- the one synchronisation of the bank
        self.valid = None
        if self.masks is not None and exclude_masks:
            self.valid = torch.nonzero(self.masks.reshape(-1) < 128).reshape(-1).contiguous()
            if self.valid.numel() == 0:
                raise ValueError("exclude_masks leaves no pixel to train on")
        self.num_train = F * H * W if self.valid is None else int(self.valid.numel())
        self._perm = perm_params(self.num_train, self.seed, self.epoch)

    # ------------------------------------------------------------------------- the rules in plain torch (host path)
    def _host_dirs(self, f, x, y):
        """[x, y, 1] . Kinv^T . R^T of pixels (x, y) of frames f (render_utils.py:26-28, :38)"""
        cam = self.cams[f]
        kinv, rot = cam[:, :9].reshape(-1, 3, 3), cam[:, 9:].reshape(-1, 3, 4)[:, :, :3]
        pix = torch.stack([x, y, torch.ones_like(x)], -1).to(torch.float32)
        dirs = (pix[:, None, :] * kinv).sum(-1)
        return (dirs[:, None, :] * rot).sum(-1)

    @staticmethod
    def _unit(d):
        return d / d.norm(dim=-1, keepdim=True)

    def _host_sphere(self, f, v):
        """origin, o.v, v.v and the discriminant of o + t v against the unit sphere (scene_utils.py:101-120)"""
        o = self.cams[f][:, 9:].reshape(-1, 3, 4)[:, :, 3]
        od, dd, oo = (o * v).sum(-1), (v * v).sum(-1), (o * o).sum(-1)
        return o, od, dd, od * od + (1.0 - oo) * dd

    def _host_frame_flag(self, f):
        ys, xs = torch.meshgrid(torch.arange(self.H), torch.arange(self.W), indexing="ij")
        fs = torch.full((self.H * self.W,), f, dtype=torch.int64)
        disc = self._host_sphere(fs, self._unit(self._host_dirs(fs, xs.reshape(-1), ys.reshape(-1))))[3]
        return ~torch.all(disc >= 0)

    def _host_rows(self, g):
        H, W = self.H, self.W
        f, rem = g // (H * W), g % (H * W)
        y, x = rem // W, rem % W
        wd = self._host_dirs(f, x, y)
        v = self._unit(wd)
        o, od, dd, disc = self._host_sphere(f, v)
        far = torch.where(self.flags[f] != 0, torch.ones_like(od), (torch.sqrt(disc) - od) / dd)
        ya = torch.where(y == H - 1, torch.full_like(y, H - 3), y)  # the last row repeats row H-3's value
        da, db = self._host_dirs(f, x, ya), self._host_dirs(f, x, ya + 1)
        if self.norm_ray_dir:
            da, db = self._unit(da), self._unit(db)
        radius = torch.sqrt(((da - db) ** 2).sum(-1)) * 2 / math.sqrt(12)
        d = v if self.norm_ray_dir else wd
        rays = torch.cat([o, d, torch.full_like(far, NEAR_PLANE)[:, None], far[:, None], v, radius[:, None]], -1)
        rgbs = self.images.reshape(-1, 3)[g].to(torch.float32).div(255)
        mask = None if self.masks is None else 1 - torch.round(self.masks.reshape(-1)[g].to(torch.float32).div(255))[:, None]
        return rays, rgbs, self.ts_table[f], mask

    # ------------------------------------------------------------------------- batches
    @property
    def bad_ids(self):
        """how many indices the device path has clamped into its tables so far (synchronises)"""
        return int(self._bad.item())

    def _rows(self, n, ids=None, pos0=0, through_valid=False):
        """(rays, rgbs, ts, mask) of n rays: explicit ids, or the positions pos0 + [0, n) of the current epoch"""
        valid = self.valid if through_valid else None
        if self.device.type != "cpu":
            from .. import ops

            return ops.raybank_gather(self.images, self.cams, self.flags, self.ts_table, self._bad, n, ids=ids, perm=None if ids is not None else self._perm,
                                      pos0=pos0, valid=valid, masks=self.masks, norm_ray_dir=self.norm_ray_dir, near=NEAR_PLANE)
        if ids is None:
            ids = epoch_ids(self.num_train, self.seed, self.epoch, pos0 + torch.arange(n))
        return self._host_rows(ids if valid is None else valid[ids])

    def batch(self, ids, through_valid=False):
        """(rays (n,12), rgbs (n,3), ts (n,), mask (n,1) | None) of the pixels `ids` = (f H + y) W + x (through_valid: indices into the table
        of unmasked pixels instead).  Ids given on the host are checked and an id outside the table raises; ids that are already on the
        bank's GPU are not read back: the kernel clamps them into the table and counts them in `bad_ids`."""
        ids = torch.as_tensor(ids).to(torch.int64).reshape(-1)
        limit = self.num_train if through_valid and self.valid is not None else self.F * self.H * self.W
        if ids.device.type == "cpu" and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= limit):
            raise ValueError(f"ray ids outside [0, {limit})")
        return self._rows(ids.numel(), ids=ids.to(self.device).contiguous(), through_valid=through_valid)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self._perm = perm_params(self.num_train, self.seed, self.epoch)

    def __len__(self):
        return self.num_train // (self.batch_rays * self.world_size)

    def train_batch(self, k):
        """training dictionary of batch k of the current epoch (this rank's): no host synchronisation on a GPU bank"""
        pos0, n = batch_positions(k, self.batch_rays, self.rank, self.world_size)
        rays, rgbs, ts, mask = self._rows(n, pos0=pos0, through_valid=True)
        out = dict(rays=rays[None], rgbs=rgbs[None], ts=ts[None], img_wh=self.img_wh)
        if mask is not None:
            out["mask"] = mask
        return out

    def __iter__(self):
        for k in range(len(self)):
            yield self.train_batch(k)

    def _grid_ids(self, ds):
        """ids of the pixels (ds//2 + i ds, ds//2 + j ds) of frame 0 (data_downsample, nerfbase.py:239-248), on the bank's device"""
        if ds not in self._grids:
            ys, xs = torch.arange(ds // 2, self.H, ds), torch.arange(ds // 2, self.W, ds)
            self._grids[ds] = ((ys[:, None] * self.W + xs[None, :]).reshape(-1).to(self.device), (len(xs), len(ys)))
        return self._grids[ds]

    def frame_batch(self, f, ds=1):
        """validation dictionary of ONE view (load_sample, nerfbase.py:255-321): all pixels of frame f, or the ds//2::ds grid"""
        f = int(f)
        if not 0 <= f < self.F:
            raise ValueError(f"frame {f} outside [0, {self.F})")
        grid, (w, h) = self._grid_ids(int(ds))
        rays, rgbs, ts, mask = self._rows(grid.numel(), ids=grid + f * self.H * self.W)
        out = dict(rays=rays[None], rgbs=rgbs[None], ts=ts[None], seq_ind=[self.seq_ind[f]], img_idx=[self.img_idx[f]], img_wh=torch.tensor([[w, h]]),
                   K=self.K[f][None].clone(), cam2scene=self.c2w_host[f][None].clone())
        if self.unnorm_scene is not None:
            out["unnorm_scene"] = self.unnorm_scene[None].clone()
        if mask is not None:
            out["mask"] = mask
        return out

    def pair_batch(self, f1, f2, ds=1):
        """validation dictionary of TWO views (load_retrieval_pair_sample, nerfbase.py:323-349): the rows of both, c2w (1,8,4) =
        unnorm_scene @ cam2scene of both, K (1,6,3); NerfTrainer.validation_step adds the pose metrics for it"""
        if self.unnorm_scene is None:
            raise ValueError("pair_batch needs the bank's unnorm_scene (the pose metrics are measured in world units)")
        a, b = self.frame_batch(f1, ds), self.frame_batch(f2, ds)
        out = {k: torch.cat([a[k], b[k]], 1) for k in ("rays", "rgbs", "ts", "K", "img_wh")}
        out.update(img_idx=a["img_idx"] + b["img_idx"], seq_ind=a["seq_ind"] + b["seq_ind"], unnorm_scene=a["unnorm_scene"],
                   c2w=torch.cat([self.unnorm_scene @ a["cam2scene"][0], self.unnorm_scene @ b["cam2scene"][0]], 0)[None])
        if "mask" in a:
            out["mask"] = torch.cat([a["mask"], b["mask"]], 0)
        return out
