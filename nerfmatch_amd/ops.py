"""Thin torch-tensor wrappers over the C ABI (one function per entry point of include/nerfmatch_amd.h).

Everything here enqueues hand-written gfx950 kernels on torch's current stream; there is no eager
fallback.  Tensors must live on the GPU, be contiguous and fp32 (int64 / uint8 where stated)."""
import contextlib
import ctypes as C

import torch

from . import _lib
from ._lib import check, dptr, hptr, lib, stream

NEAR_PLANE = 0.01  # reference: nerfmatch/nerf/render_utils.py:72

# Measurement hook (bench.py sets it, nothing else does): callable(tag, flop) -> context manager that brackets the launches of one
# native call with HIP events on the launch stream.  None in production: the wrappers below then cost a null context.
KERNEL_PROBE = None


def _probe(tag, flop):
    return contextlib.nullcontext() if KERNEL_PROBE is None else KERNEL_PROBE(tag, flop)


def _f32(t):
    return t.to(torch.float32).contiguous()


def _mask_u8(m):
    """Mask -> contiguous uint8 device tensor (or None).  A bool mask is re-viewed, not converted: same bytes, no launch."""
    if m is None:
        return None
    m = m.contiguous()
    if m.dtype != torch.bool:  # the reference's `mask.bool()` (c2f_trainer.py:296-298): non-zero = valid
        m = m.ne(0)
    return m.view(torch.uint8)


_SIDE_STREAMS = {}


def side_stream(dev):
    """One extra (non-blocking) HIP stream per device for small transfers and checks that must not queue behind -- or lengthen -- the main
    stream's chain of dependent launches: the match counts' read-back, the parameter fingerprints."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[key]


def _scratch(cache, dev, need):
    """The (growing) uint8 scratch buffer of one kernel family, one per (device, stream): calls on one stream are serialised, calls on
    different streams must not share it.  `cache`: that family's own dict (buffers are not shared between kernels)."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        ws = cache[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    return ws


# ----------------------------------------------------------------------------- parameter fingerprints
class ParamGuard:
    """Notices parameters whose VALUES changed behind the derived copies this package keeps of them (packed / split / transposed blobs,
    host values), i.e. writes through `.data`, which change neither data_ptr nor _version -- the keys those caches use.
    check() is ONE small launch: it sums every parameter's words on the device and compares with the sums taken at the last baseline;
    `flag` (device int32[2], element 1) goes up on a mismatch.  The first check() for a given (data_ptr, _version) state of the parameters
    takes the baseline -- taken at the start of a pass, before that pass packs anything, so copies and baseline describe the same values.
    No synchronisation here: callers read `flag` where they synchronise anyway."""

    CHUNK = 4096  # words per workgroup: FP_CHUNK of csrc/capi.hip

    def __init__(self, module):
        """module: an nn.Module (every parameter of it and its children is watched; a Parameter OBJECT that is replaced later --
        load_state_dict(assign=True), `layer.weight = nn.Parameter(...)` -- is picked up: the list is validated by identity on every check)."""
        self.module = module
        self.key = None
        self.tables = None
        self.flag = None
        self._collect()

    def _collect(self):
        seen, self.slots = set(), []
        for m in self.module.modules():
            for n, p in m._parameters.items():
                if p is not None and id(p) not in seen and p.is_cuda and p.numel() > 0 and p.element_size() in (4, 8):
                    seen.add(id(p))
                    self.slots.append((m, n, p))
        self.params = [p for _, _, p in self.slots]

    def _state(self):
        for m, n, p in self.slots:
            if m._parameters.get(n) is not p:  # (a replaced Parameter object: walk the module again)
                self._collect()
                break
        return tuple([(p.data_ptr(), p._version) for p in self.params])

    def _build(self, dev):
        ptrs, words, bt, bo = [], [], [], []
        for i, p in enumerate(self.params):
            if not p.is_contiguous():
                raise _lib.NerfmatchAmdError("ParamGuard: parameters must be contiguous")
            n = p.numel() * p.element_size() // 4
            ptrs.append(p.data_ptr()); words.append(n)
            for off in range(0, n, self.CHUNK):
                bt.append(i); bo.append(off)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64).to(dev)
        self.tables = dict(ptrs=i64(ptrs), words=i64(words), bt=torch.tensor(bt, dtype=torch.int32).to(dev), bo=i64(bo), nblk=len(bt),
                           cur=torch.zeros(len(ptrs), dtype=torch.int64, device=dev), ref=torch.zeros(len(ptrs), dtype=torch.int64, device=dev),
                           ptr_key=tuple(ptrs))
        self.flag = torch.zeros(2, dtype=torch.int32, device=dev)

    def check(self):
        """Enqueue the fingerprint launch (baseline when the parameters' (data_ptr, _version) state is new) on the device's SIDE stream,
        ordered behind everything the current stream holds at this moment -- a write to a parameter enqueued there is seen -- and beside
        whatever the current stream does next: the pass's chain of dependent launches is not lengthened.  Everything of this object runs
        on that one side stream (tables, launches, reset).  Returns True when this call took a baseline."""
        state = self._state()
        if not self.params:
            return True
        dev = self.params[0].device
        side = side_stream(dev)
        here = torch.cuda.Event()
        here.record(torch.cuda.current_stream(dev))
        side.wait_event(here)
        baseline = state != self.key
        with torch.cuda.stream(side):
            if self.tables is None or self.tables["ptr_key"] != tuple(s[0] for s in state):
                self._build(dev)
                baseline = True
            self.key = state
            t = self.tables
            u64 = torch.int64
            check(lib().nm_params_fingerprint(dptr(t["ptrs"], u64), dptr(t["words"], u64), dptr(t["bt"], torch.int32), dptr(t["bo"], u64),
                                              len(self.params), t["nblk"], dptr(t["cur"], u64), dptr(t["ref"], u64), dptr(self.flag, torch.int32),
                                              int(baseline), stream()), "nm_params_fingerprint")
        return baseline

    def reset(self):
        """Forget the baseline: the next check() takes a new one (call together with dropping the derived caches)."""
        self.key = None
        if getattr(self, "flag", None) is not None:
            with torch.cuda.stream(side_stream(self.flag.device)):
                self.flag.zero_()  # (sticky on the device until the next baseline: cleared so that a reader in between sees "clean")
                self.tables["cur"].zero_()


# ----------------------------------------------------------------------------- NeRF half
def raygen(K, c2w_norm, H, W, device, ds=8, near=NEAR_PLANE, out=None, flag=None):
    """rays (R,12) on `device` for the sub-sampled pixel grid; also returns the far-fallback flag tensor.
    `out` / `flag` let a caller fill a slice of a larger (batched) ray bundle."""
    L = lib()
    kinv = torch.linalg.inv(K.detach().to("cpu", torch.float32)).contiguous()
    pose = c2w_norm.detach().to("cpu", torch.float32).contiguous()
    R = L.nm_raygen_count(int(H), int(W), int(ds))
    rays = torch.empty(R, 12, device=device, dtype=torch.float32) if out is None else out
    assert rays.shape == (R, 12)
    flag = torch.empty(1, device=device, dtype=torch.int32) if flag is None else flag
    check(L.nm_raygen(hptr(kinv), hptr(pose), int(H), int(W), int(ds), float(near), dptr(rays), dptr(flag, torch.int32), stream()), "nm_raygen")
    return rays, flag


def raygen_batch(K, c2ws_norm, H, W, device, ds=8, near=NEAR_PLANE):
    """Q normalised poses (Q,4,4) -> rays (Q*R,12) and far-fallback flags (Q,) with one launch per kernel."""
    L = lib()
    kinv = torch.linalg.inv(K.detach().to("cpu", torch.float32)).contiguous()
    poses = c2ws_norm.detach().to("cpu", torch.float32).reshape(-1, 16).contiguous()
    Q = poses.shape[0]
    R = L.nm_raygen_count(int(H), int(W), int(ds))
    rays = torch.empty(Q * R, 12, device=device, dtype=torch.float32)
    flags = torch.empty(Q, device=device, dtype=torch.int32)
    check(L.nm_raygen_batch(hptr(kinv), hptr(poses), Q, int(H), int(W), int(ds), float(near), dptr(rays), dptr(flags, torch.int32), stream()),
          "nm_raygen_batch")
    return rays, flags


def sample_coarse(rays, t_rand, S):
    R = rays.shape[0]
    assert t_rand.shape == (R, S + 1)
    t = torch.empty(R, S + 1, device=rays.device, dtype=torch.float32)
    check(lib().nm_sample_coarse(dptr(rays), dptr(t_rand), R, int(S), dptr(t), stream()), "nm_sample_coarse")
    return t


def resample(t, weights, jitter, padding=0.01, randomized=True, want_tail_flag=False, jitter_scale=1.0):
    """want_tail_flag: also return the device int32[1] flag nm_resample raises when the fence posts j > S/2 do NOT
    coincide (the premise of nerf_fwd(zero_tail=True)); pass it on as `tail_flag`.  jitter_scale: the kernel uses jitter * jitter_scale
    (one fp32 product where it reads the value: the same bits as scaling the tensor first, one launch less)."""
    R, n = t.shape
    S = n - 1
    assert weights.shape == (R, S)
    out = torch.empty_like(t)
    flag = torch.empty(1, device=t.device, dtype=torch.int32) if want_tail_flag else None
    check(lib().nm_resample(dptr(t), dptr(weights), dptr(jitter), float(jitter_scale), R, S, float(padding), int(bool(randomized)), dptr(out),
                            dptr(flag, torch.int32), stream()), "nm_resample")
    return (out, flag) if want_tail_flag else out


class Fp16Guard:
    """Safety net of one fp16x3 blob (round 4): the device status block nm_nerf_fwd_fp16x3 writes (saturation flag + range
    telemetry, int32[16]) and the fp32 blob of the same parameters for the device-side fall-back nm_nerf_fwd_guarded.  NeRF.packed
    attaches one to every fp16x3 blob (`blob.nm_guard`); nerf_fwd refuses an fp16x3 blob without one.
    ONE STREAM PER STATUS BLOCK: the guarded pass consumes the flag (completion counter status[12], event count status[11]); two guarded
    launches on different streams against the same block could clear the flag before the other has read it.  A blob -- and with it its
    guard -- is used by one stream at a time (the evaluator's render stream; give a second concurrent renderer its own NeRF.packed blob)."""

    def __init__(self, device, blob32, act_log2=None):
        self.status = torch.zeros(16, dtype=torch.int32, device=device)
        self.blob32 = blob32
        self.act_log2 = None if act_log2 is None else [int(v) for v in act_log2]

    def read(self):
        """(saturated, ranges[10]) -- SYNCHRONISES; ranges are in the scaled units of the blob (divide by 2^act_log2).
        saturated = some launch on this block hit the fp16 limit since the last reset(): bit 0 of status[0] (raised by the fp16x3
        kernel, cleared again by the guarded fp32 pass that rewrote that launch) or the sticky event count status[11]."""
        h = self.status.cpu()
        return bool(int(h[0]) & 1) or int(h[11]) > 0, h[1:11].view(torch.float32).tolist()

    def reset(self):
        self.status.zero_()


def nerf_fwd(blob, rays, t, app_row=None, tap_layer=-1, white_bg=False, var_scale=-1.0, need_rgb=True, need_feat=True,
             feat_max=False, want_raw=False, want_sample_feat=False, zero_tail=False, tail_flag=None, guard=None):
    """One fused pass.  Returns dict(weights, feat, pts, rgb, depth, acc[, raw, sample_feat]).
    zero_tail: the intervals s > S/2 have zero width (t from `resample(..., randomized=True)`), see NM_NERF_ZERO_TAIL in the
    header; same outputs, about half the work on the bf16x3 path.  `tail_flag` = the device flag of
    `resample(..., want_tail_flag=True)` for this very `t`: the kernel then checks the premise itself and evaluates every
    sample when it does not hold; without it the caller vouches for the premise.
    fp16x3 blobs run GUARDED: the kernel raises a device flag when an operand reached the fp16 limit, and a second launch
    (the fp32 kernel, which exits at once unless that flag is set) rewrites the outputs -- no host synchronisation, never a
    silently clamped result.  guard: an Fp16Guard (default: the one NeRF.packed attached to the blob)."""
    R, n = t.shape
    S_req = n - 1
    # Row lengths the kernels tile natively: 32, 64 and multiples of 128 (a tile = 128 samples = 4 wavefronts of 32).  Any other
    # `num_pts` (the reference takes any, renderer.py:86,100,196-213) runs on the next native length with the fence posts padded by
    # copies of the last one: a zero-width interval has alpha = 0, i.e. weight EXACTLY 0 and transmittance unchanged, so every output
    # is the sum the unpadded row defines plus exact zeros (cost: the padded samples still go through the MLP -- 96 -> 128: +33 %).
    S = S_req if (S_req in (32, 64) or S_req % 128 == 0) else (32 if S_req < 32 else 64 if S_req < 64 else (S_req + 127) // 128 * 128)
    if S != S_req:
        if S_req < 1:
            raise _lib.NerfmatchAmdError("nerf_fwd needs at least one interval per ray")
        t = torch.cat([t, t[:, -1:].expand(R, S - S_req)], 1).contiguous()
        zero_tail, tail_flag = False, None  # (the premise is about the second half of the REQUESTED row)
    dev = rays.device
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    out = dict(weights=new(R, S), pts=new(R, 3), depth=new(R), acc=new(R))
    out["feat"] = new(R, 256) if need_feat else None
    out["rgb"] = new(R, 3) if need_rgb else None
    out["raw"] = new(R, S, 4) if want_raw else None
    out["sample_feat"] = new(R, S, 256) if want_sample_feat else None
    flags = (0 if need_rgb else _lib.NM_NERF_SKIP_RGB) | (_lib.NM_NERF_FEAT_MAX if feat_max else 0) | (_lib.NM_NERF_ZERO_TAIL if zero_tail else 0)
    # the blob's dtype tells the kernel family: fp32 blob -> fp32 MFMA kernel, uint8 -> bf16x3 split, int16 -> fp16x3 split, float16 -> fp16x1
    common = (dptr(rays), dptr(t), dptr(app_row), R, S, int(tap_layer), int(bool(white_bg)),
              float(var_scale), flags, dptr(out["weights"]), dptr(out["feat"]), dptr(out["pts"]),
              dptr(out["rgb"]), dptr(out["depth"]), dptr(out["acc"]), dptr(out["raw"]), dptr(out["sample_feat"]))
    split = _NERF_SPLIT.get(blob.dtype)
    if split is None:
        check(lib().nm_nerf_fwd(dptr(blob), *common, stream()), "nm_nerf_fwd")
    else:
        name, guarded = split
        status = ()
        if guarded:
            g = guard if guard is not None else getattr(blob, "nm_guard", None)
            if g is None:
                raise _lib.NerfmatchAmdError("fp16x3 blob without an Fp16Guard: take it from NeRF.packed(device, 'fp16x3') (operands beyond "
                                             "+-65504 would be clamped silently)")
            status = (dptr(g.status, torch.int32),)
        ws = _nerf_workspace(dev) if (need_feat or want_sample_feat) else None
        check(getattr(lib(), name)(dptr(blob, blob.dtype), *common, dptr(ws, torch.uint8), dptr(tail_flag, torch.int32), *status, stream()), name)
        if guarded:
            check(lib().nm_nerf_fwd_guarded(dptr(g.blob32), *common, *status, stream()), "nm_nerf_fwd_guarded")
    if S != S_req:
        for k in ("weights", "raw", "sample_feat"):
            if out[k] is not None:
                out[k] = out[k][:, :S_req].contiguous()
    return out


# split-precision kernel families by blob dtype: (entry point, takes the Fp16Guard's `status` block and runs guarded)
_NERF_SPLIT = {torch.uint8: ("nm_nerf_fwd_bf16x3", False),    # NeRF.packed(device, "bf16x3")
               torch.int16: ("nm_nerf_fwd_fp16x3", True),     # fp16 hi/lo-split blob (NeRF.packed(device, "fp16x3"))
               torch.float16: ("nm_nerf_fwd_fp16x1", False)}  # single-product fp16 blob (NeRF.packed(device, "fp16x1"))
_NERF_WS = {}


def _nerf_workspace(dev):
    """Scratch of the persistent split-precision kernels."""
    return _scratch(_NERF_WS, dev, lib().nm_nerf_workspace_bytes_bf16x3())


def unnormalize_points(pts, unnorm):
    m = unnorm.detach().to("cpu", torch.float32).contiguous()
    out = torch.empty_like(pts)
    check(lib().nm_unnormalize_points(dptr(pts), hptr(m), pts.shape[0], dptr(out), stream()), "nm_unnormalize_points")
    return out


def raybank_frame_flags(cams, H, W):
    """cams (F,21) on the device (Kinv | c2w rows 0..2 per frame) -> flags (F,) int32: 1 = some pixel of the frame misses the unit sphere."""
    F = cams.shape[0]
    assert cams.shape == (F, 21)
    flags = torch.empty(F, device=cams.device, dtype=torch.int32)
    check(lib().nm_raybank_frame_flags(dptr(cams), F, int(H), int(W), dptr(flags, torch.int32), stream()), "nm_raybank_frame_flags")
    return flags


def raybank_gather(images, cams, flags, ts_table, bad, n, ids=None, perm=None, pos0=0, pos_stride=1, valid=None, masks=None, norm_ray_dir=True,
                   near=NEAR_PLANE):
    """n training rays of a ray bank (images (F,H,W,3) uint8, cams (F,21), flags (F,) int32, ts_table (F,) int64, masks (F,H,W) uint8 or None)
    -> rays (n,12), rgbs (n,3), ts (n,) int64, mask (n,1) or None.  ids: (n,) int64 device indices; or perm = (keys, half_bits) of the epoch
    permutation applied to positions pos0 + i * pos_stride.  valid: int64 table the indices go through.  bad: device int32[1] counter of
    clamped indices (add-only).  No host synchronisation."""
    F, H, W, _ = images.shape
    assert images.shape == (F, H, W, 3) and cams.shape == (F, 21) and (ids is None) != (perm is None)
    assert ids is None or ids.shape == (n,)
    n_src = F * H * W if valid is None else valid.numel()
    dev = images.device
    rays = torch.empty(n, 12, device=dev, dtype=torch.float32)
    rgbs = torch.empty(n, 3, device=dev, dtype=torch.float32)
    ts = torch.empty(n, device=dev, dtype=torch.int64)
    mask = None if masks is None else torch.empty(n, 1, device=dev, dtype=torch.float32)
    keys, half_bits = (None, 0) if perm is None else ((C.c_uint32 * 4)(*perm[0]), int(perm[1]))
    check(lib().nm_raybank_gather(dptr(images, torch.uint8), dptr(masks, torch.uint8), dptr(cams), dptr(flags, torch.int32),
                                  dptr(ts_table, torch.int64), F, H, W, dptr(ids, torch.int64), dptr(valid, torch.int64), n_src, keys, half_bits,
                                  int(pos0), int(pos_stride), int(n), int(bool(norm_ray_dir)), float(near), dptr(rays), dptr(rgbs),
                                  dptr(ts, torch.int64), dptr(mask), dptr(bad, torch.int32), stream()), "nm_raybank_gather")
    return rays, rgbs, ts, mask


def refbank_select(pt3d, cams, ref_ids, img_wh):
    """The co-visibility rule of a reference point bank (pt3d (F,n,3), cams (F,21) = scaled K | w2c rows 0..2) for the id rows ref_ids
    (B,k) int64 on the device, at the target resolution img_wh = (W, H): nm_refbank_visibility + nm_refbank_select -> words (B,k n) int32
    (the uint32 visibility words' bits), list (B,k n) int32 (the visible candidates in ascending order, then -1), n_visible (B,) int32,
    decisions (B,) int32.  No host synchronisation."""
    F, n, _ = pt3d.shape
    B, k = ref_ids.shape
    assert pt3d.shape == (F, n, 3) and cams.shape == (F, 21)
    N, dev = k * n, pt3d.device
    words = torch.empty(B, N, device=dev, dtype=torch.int32)
    lst = torch.empty(B, N, device=dev, dtype=torch.int32)
    n_visible = torch.empty(B, device=dev, dtype=torch.int32)
    decisions = torch.empty(B, device=dev, dtype=torch.int32)
    st = stream()
    check(lib().nm_refbank_visibility(dptr(pt3d), dptr(cams), dptr(ref_ids, torch.int64), F, n, B, k, int(img_wh[0]), int(img_wh[1]),
                                      dptr(words, torch.int32), st), "nm_refbank_visibility")
    check(lib().nm_refbank_select(dptr(words, torch.int32), B, k, N, dptr(lst, torch.int32), dptr(n_visible, torch.int32),
                                  dptr(decisions, torch.int32), st), "nm_refbank_select")
    return dict(words=words, list=lst, n_visible=n_visible, decisions=decisions)


def refbank_gather(pt3d, pt_feat, pt_mask, ref_ids, bad, rows, select=None, perm_keys=None, out=None):
    """nm_refbank_gather: `rows` output rows per query of a reference point bank (pt3d (F,n,3), pt_feat (F,n,D), pt_mask (F,n) bool) for
    the id rows ref_ids (B,k) int64 on the device -> pt3d (B,rows,3), pt_feat (B,rows,D), pt_mask (B,rows) bool.  select = refbank_select's
    dict with perm_keys (B,4) int32 (the round keys' bits): row q is candidate list[perm(q mod Nv)]; select=None: row q is candidate q
    (rows == k n).  bad: device int32[1] counter of clamped frame ids (add-only).  out: (pt3d, pt_feat, pt_mask) to write into."""
    F, n, D = pt_feat.shape
    B, k = ref_ids.shape
    assert pt3d.shape == (F, n, 3) and pt_mask.shape == (F, n) and (select is None) == (perm_keys is None)
    dev = pt3d.device
    if out is None:
        out = (torch.empty(B, rows, 3, device=dev), torch.empty(B, rows, D, device=dev), torch.empty(B, rows, device=dev, dtype=torch.bool))
    o3, of, om = out
    assert o3.shape == (B, rows, 3) and of.shape == (B, rows, D) and om.shape == (B, rows) and om.dtype == torch.bool
    lst, nv = (None, None) if select is None else (select["list"], select["n_visible"])
    assert select is None or (lst.shape == (B, k * n) and perm_keys.shape == (B, 4))
    check(lib().nm_refbank_gather(dptr(pt3d), dptr(pt_feat), dptr(pt_mask.view(torch.uint8), torch.uint8), dptr(ref_ids, torch.int64), F, n, D,
                                  B, k, dptr(lst, torch.int32), dptr(nv, torch.int32), dptr(perm_keys, torch.int32), int(rows), dptr(o3),
                                  dptr(of), dptr(om.view(torch.uint8), torch.uint8), dptr(bad, torch.int32), stream()), "nm_refbank_gather")
    return o3, of, om


def covis_self_depth(pt3d, cams, pt_mask=None):
    """nm_covis_self_depth: pt3d (F,n,3), cams (F,21) on the device -> zself (F,n): p.z of every frame's points under its own camera; with
    pt_mask (F,n) bool, NaN where it is false: the depth map covis_scores gathers from."""
    F, n, _ = pt3d.shape
    assert pt3d.shape == (F, n, 3) and cams.shape == (F, 21) and (pt_mask is None or (pt_mask.shape == (F, n) and pt_mask.dtype == torch.bool))
    zself = torch.empty(F, n, device=pt3d.device, dtype=torch.float32)
    mask = None if pt_mask is None else pt_mask.view(torch.uint8)
    check(lib().nm_covis_self_depth(dptr(pt3d), dptr(mask, torch.uint8), dptr(cams), F, n, dptr(zself), stream()), "nm_covis_self_depth")
    return zself


def covis_scores(pt3d, pt_mask, cams, rows, img_wh, zself=None, grid_wh=None, depth_tol=None):
    """nm_covis_scores: how many of frame j's masked points (pt3d (F,n,3), pt_mask (F,n) bool) the frames rows (Q,) int32 (device; None: all
    frames) see under cams (F,21) at img_wh = (W, H) -> scores (Q,F) int32.  zself (F,n) with grid_wh = (gw, gh) and depth_tol: the depth
    test; zself is covis_self_depth(pt3d, cams, pt_mask): the kernel reads the query frames' masks from it.  One launch, no host
    synchronisation."""
    F, n, _ = pt3d.shape
    assert pt3d.shape == (F, n, 3) and pt_mask.shape == (F, n) and pt_mask.dtype == torch.bool and cams.shape == (F, 21)
    assert (zself is None) == (grid_wh is None) == (depth_tol is None) and (zself is None or zself.shape == (F, n))
    Q = F if rows is None else rows.numel()
    gw, gh = (0, 0) if grid_wh is None else (int(grid_wh[0]), int(grid_wh[1]))
    scores = torch.empty(Q, F, device=pt3d.device, dtype=torch.int32)
    check(lib().nm_covis_scores(dptr(pt3d), dptr(pt_mask.view(torch.uint8), torch.uint8), dptr(cams), dptr(rows, torch.int32), dptr(zself), F, n, Q,
                                int(img_wh[0]), int(img_wh[1]), gw, gh, 0.0 if depth_tol is None else float(depth_tol), dptr(scores, torch.int32),
                                stream()), "nm_covis_scores")
    return scores


def covis_topk(scores, rows, k, min_score=1):
    """nm_covis_topk: scores (Q,F) int32 whose row q belongs to frame rows[q] (rows (Q,) int32 on the device; None: frame q)
    -> ids (Q,k) int32 padded with -1, n_pairs (Q,) int32.  One launch, no host synchronisation."""
    Q, F = scores.shape
    assert rows is None or rows.shape == (Q,)
    ids = torch.empty(Q, int(k), device=scores.device, dtype=torch.int32)
    n_pairs = torch.empty(Q, device=scores.device, dtype=torch.int32)
    check(lib().nm_covis_topk(dptr(scores, torch.int32), dptr(rows, torch.int32), Q, F, int(k), int(min_score), dptr(ids, torch.int32),
                              dptr(n_pairs, torch.int32), stream()), "nm_covis_topk")
    return ids, n_pairs


def image_resize_u8(src, wh, tables_x, tables_y, white_where=None, lut=None, want_u8=True):
    """nm_image_resize_u8: src (F,H,W,C) uint8 on the device, C in {1, 3} -> (uint8 (F,h,w,C) or None, float32 (F,C,h,w) or None) at
    wh = (w, h).  tables_x = (coef (ksize, w) int32 TAP-major, bounds (w, 2) int32) on the device, or None when the width stays;
    tables_y = (coef (h, ksize), bounds (h, 2)), or None when the height stays.  white_where (F,h,w) uint8: 255 where it is >= 128.
    lut (C,256) float32 on the device asks for the float output.  One launch, no host synchronisation."""
    F, H, W, Cn = src.shape
    w, h = int(wh[0]), int(wh[1])
    assert (tables_x is None) == (W == w) and (tables_y is None) == (H == h) and (want_u8 or lut is not None)
    assert white_where is None or tuple(white_where.shape) == (F, h, w)
    assert lut is None or tuple(lut.shape) == (Cn, 256)
    (cx, bx), (cy, by) = tables_x or (None, None), tables_y or (None, None)
    kx, ky = 0 if cx is None else cx.shape[0], 0 if cy is None else cy.shape[1]
    assert cx is None or (cx.shape == (kx, w) and bx.shape == (w, 2))
    assert cy is None or (cy.shape == (h, ky) and by.shape == (h, 2))
    out_u8 = torch.empty(F, h, w, Cn, device=src.device, dtype=torch.uint8) if want_u8 else None
    out_f = None if lut is None else torch.empty(F, Cn, h, w, device=src.device, dtype=torch.float32)
    check(lib().nm_image_resize_u8(dptr(src, torch.uint8), F, H, W, Cn, dptr(cx, torch.int32), dptr(bx, torch.int32), kx,
                                   dptr(cy, torch.int32), dptr(by, torch.int32), ky, h, w, dptr(white_where, torch.uint8), dptr(lut),
                                   dptr(out_u8, torch.uint8), dptr(out_f), stream()), "nm_image_resize_u8")
    return out_u8, out_f


# ----------------------------------------------------------------------------- matcher half
# Arithmetic of the nn.Linear layers: "fp32" (v_mfma_f32_32x32x2_f32, nm_linear) or "bf16x3" (bf16 MFMA on hi/lo-split
# operands, fp32-accurate, nm_linear_bf16x3).  Module-level switch like ATTENTION_PRECISION.
LINEAR_PRECISION = "fp32"
_LINEAR_BLOBS = {}
_LINEAR_LIMIT = 256   # entries per generation
_LINEAR_GRAVE = []    # the previous generation (see _linear_evict)
_LINEAR_RECENT = __import__("collections").deque(maxlen=16)  # the last blobs handed out stay allocated whatever the limit is


def _linear_evict():
    """Start a new generation of the blob cache.  The entries of the old one stay ALLOCATED until the next eviction: an op that takes
    several blobs (the encoder tail takes three) fetches their device pointers one after the other and launches afterwards -- had the
    second fetch freed the first blob (round 1-4: `_LINEAR_BLOBS.clear()`), the third one's allocation could land on its memory and the pack
    kernel would overwrite weights the launch had not consumed yet.  (Seen in round 5 as an order-dependent test failure once the suite
    had created more than 256 weight tensors; a training loop, whose parameter versions change every step, evicts every few steps.)"""
    global _LINEAR_GRAVE
    _LINEAR_GRAVE = list(_LINEAR_BLOBS.values())
    _LINEAR_BLOBS.clear()


def _linear_cached(prefix, weight, make):
    """make(w) for the detached weight, cached under prefix + (data_ptr, _version, shape, device) until the tensor changes."""
    w = weight.detach()
    key = (*prefix, w.data_ptr(), w._version, tuple(w.shape), w.device.index)
    hit = _LINEAR_BLOBS.get(key)
    if hit is None:
        made = make(w)
        if len(_LINEAR_BLOBS) >= _LINEAR_LIMIT:
            _linear_evict()
        hit = _LINEAR_BLOBS[key] = (made, w)  # keeps the source tensor alive so that its data_ptr is not reused
    _LINEAR_RECENT.append(hit)
    return hit[0]


def _pack(name, N, K):
    """make-callable of _linear_cached: the nm_linear_blob_bytes_bf16x3(N, K) blob that entry point `name` writes from the weight."""
    def make(w):
        blob = torch.empty(lib().nm_linear_blob_bytes_bf16x3(N, K), dtype=torch.uint8, device=w.device)
        wc = w.contiguous()
        check(getattr(lib(), name)(dptr(wc), N, K, dptr(blob, torch.uint8), stream()), name)
        return blob
    return make


def _linear_blob(weight):
    """Split / re-ordered copy of a weight matrix for nm_linear_bf16x3, cached until the tensor changes."""
    return _linear_cached((), weight, _pack("nm_linear_pack_bf16x3", *weight.shape))


def _linear_blob_perm(weight):
    """The same blob with the K dimension in accumulator order (nm_linear_pack_perm_bf16x3): the weights of a product whose
    input is the previous product's output still sitting in accumulator registers (nm_encoder_tail_bf16x3)."""
    return _linear_cached(("perm",), weight, _pack("nm_linear_pack_perm_bf16x3", *weight.shape))


def _linear_blob_t(weight):
    """The packed blob of weight.T made straight from the stored (N_out, K_in) tensor (nm_linear_pack_t_bf16x3): a training step, whose
    parameter versions change every step, then needs neither the transposed copy nor a second trip through the cache for it."""
    K, N = weight.shape  # stored (out = K of the product, in = N of the product): the packed matrix is (N, K)
    return _linear_cached(("packT",), weight, _pack("nm_linear_pack_t_bf16x3", N, K))


def linear_t(dy, weight):
    """dy (..., N_out) @ weight (N_out, K_in) -> (..., K_in): a linear layer's input gradient.  Split-bf16 arithmetic: nm_linear_bf16x3 on the
    transposed-pack blob; otherwise nm_linear on the cached transposed copy (ops.transposed).  N_out is the K of that product and the kernels
    slice K into 8-wide pieces: an N_out that is no multiple of 8 (a 3-wide output head) is zero-padded to the next one, on both operands."""
    No, Ki = weight.shape
    if LINEAR_PRECISION == "bf16x3" and No % 8 == 0 and Ki % 8 == 0:
        d2 = dy.reshape(-1, No).contiguous()
        y = torch.empty(d2.shape[0], Ki, device=dy.device, dtype=torch.float32)
        if d2.shape[0]:
            check(lib().nm_linear_bf16x3(dptr(d2), dptr(_linear_blob_t(weight), torch.uint8), None, None, None, None, d2.shape[0], Ki, No,
                                         _lib.NM_ACT_NONE, dptr(y), stream()), "nm_linear_bf16x3")
        return y.reshape(*dy.shape[:-1], Ki)
    if No % 8:
        pad = -No % 8  # (the zero columns add exact zeros to every sum)
        wt = _linear_cached(("Tpad",), weight, lambda w: torch.nn.functional.pad(w.t(), (0, pad)).contiguous())
        return linear(torch.nn.functional.pad(dy, (0, pad)), wt)
    return linear(dy, transposed(weight))


def transposed(weight):
    """weight.T as a contiguous tensor, cached until the tensor changes (same generations as the blobs): the dX product of a linear
    layer's backward pass, dy @ W, is nm_linear with W^T as the weight.  A fresh `.t().contiguous()` per call is a copy kernel AND a
    miss of the blob cache (a new tensor every time: one pack per layer and call); with frozen parameters -- the matching term of the
    iNeRF refinement differentiates through the matcher five times per query -- both happen once."""
    return _linear_cached(("T",), weight, lambda w: w.t().contiguous())


ENCODER_TAIL_FUSED = True  # False: the four separate launches (A/B runs, tests)


def encoder_tail_supported(dim, inner, hidden, act):
    """nm_encoder_tail_bf16x3 takes model dim = attention inner dim = FFN hidden dim = 256, GELU, split-bf16 arithmetic."""
    return ENCODER_TAIL_FUSED and LINEAR_PRECISION == "bf16x3" and dim == inner == hidden == 256 and act == _lib.NM_ACT_GELU


def encoder_tail(att, xh, w_out, norm2, ffn0, ffn2):
    """y = xh + FFN(LN2(xh + att @ w_out.T)) as ONE kernel (csrc/encoder_tail.hip).  att, xh (..., 256); norm2: nn.LayerNorm;
    ffn0 / ffn2: the two nn.Linear layers of the feed-forward network."""
    dim = xh.shape[-1]
    a2, x2 = att.reshape(-1, dim).contiguous(), xh.reshape(-1, dim).contiguous()
    y = torch.empty_like(x2)
    if x2.shape[0]:
        check(lib().nm_encoder_tail_bf16x3(dptr(a2), dptr(x2), dptr(_linear_blob(w_out), torch.uint8), dptr(_linear_blob_perm(ffn0.weight), torch.uint8),
                                           dptr(_linear_blob_perm(ffn2.weight), torch.uint8), dptr(norm2.weight), dptr(norm2.bias), dptr(ffn0.bias),
                                           dptr(ffn2.bias), x2.shape[0], dim, float(norm2.eps), dptr(y), stream()), "nm_encoder_tail_bf16x3")
    return y.reshape(xh.shape)


ENCODER_TAIL_BWD_FUSED = True  # False: the separate backward launches (A/B runs, tests)


def encoder_tail_save(att, xh, w_out, norm2, ffn0, ffn2):
    """(y, a, u): encoder_tail's y (bit-identical) plus the two intermediates encoder_tail_bwd needs, in ONE launch (nm_encoder_tail_save_bf16x3)."""
    dim = xh.shape[-1]
    a2, x2 = att.reshape(-1, dim).contiguous(), xh.reshape(-1, dim).contiguous()
    y, a, u = torch.empty_like(x2), torch.empty_like(x2), torch.empty_like(x2)
    if x2.shape[0]:
        check(lib().nm_encoder_tail_save_bf16x3(dptr(a2), dptr(x2), dptr(_linear_blob(w_out), torch.uint8), dptr(_linear_blob_perm(ffn0.weight), torch.uint8),
                                                dptr(_linear_blob_perm(ffn2.weight), torch.uint8), dptr(norm2.weight), dptr(norm2.bias), dptr(ffn0.bias),
                                                dptr(ffn2.bias), x2.shape[0], dim, float(norm2.eps), dptr(y), dptr(a), dptr(u), stream()),
              "nm_encoder_tail_save_bf16x3")
    return y.reshape(xh.shape), a, u


def encoder_tail_bwd(dy, a_pre, u_pre, w_out, norm2, ffn0, ffn2):
    """(d_att, d_xh) of y = xh + FFN(LN2(xh + att @ w_out.T)) for FROZEN parameters in ONE launch (csrc/encoder_tail_bwd.hip): a_pre / u_pre are
    the forward pass's LayerNorm-2 input and GELU input.  The blobs are those of the TRANSPOSED matrices (cached: the parameters are frozen)."""
    dim = dy.shape[-1]
    d2, a2, u2 = dy.reshape(-1, dim).contiguous(), a_pre.reshape(-1, dim).contiguous(), u_pre.reshape(-1, dim).contiguous()
    d_att, d_xh = torch.empty_like(d2), torch.empty_like(d2)
    if d2.shape[0]:
        check(lib().nm_encoder_tail_bwd_bf16x3(dptr(d2), dptr(a2), dptr(u2), dptr(_linear_blob(transposed(ffn2.weight)), torch.uint8),
                                               dptr(_linear_blob_perm(transposed(ffn0.weight)), torch.uint8),
                                               dptr(_linear_blob_perm(transposed(w_out)), torch.uint8), dptr(norm2.weight), d2.shape[0], dim,
                                               float(norm2.eps), dptr(d_att), dptr(d_xh), stream()), "nm_encoder_tail_bwd_bf16x3")
    return d_att.reshape(dy.shape), d_xh.reshape(dy.shape)


def linear(x, weight, bias=None, residual=None, act=_lib.NM_ACT_NONE, pre=None, gate=None):
    """y = (act(x @ weight.T + bias + pre) + residual) * [gate > 0] for x (..., K); weight (N, K) as stored by nn.Linear."""
    K = x.shape[-1]
    N = weight.shape[0]
    x2 = x.reshape(-1, K).contiguous()
    M = x2.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    if M == 0:
        return y.reshape(*x.shape[:-1], N)
    r2 = None if residual is None else residual.reshape(-1, N).contiguous()
    p2 = None if pre is None else pre.reshape(-1, N).contiguous()
    g2 = None if gate is None else gate.reshape(-1, N).contiguous()
    if LINEAR_PRECISION == "bf16x3" and K % 8 == 0 and N % 8 == 0:
        check(lib().nm_linear_bf16x3(dptr(x2), dptr(_linear_blob(weight), torch.uint8), dptr(bias), dptr(p2), dptr(r2), dptr(g2), M, N, K,
                                     int(act), dptr(y), stream()), "nm_linear_bf16x3")
    elif LINEAR_PRECISION in ("fp32", "bf16x3"):
        check(lib().nm_linear(dptr(x2), dptr(weight), dptr(bias), dptr(p2), dptr(r2), dptr(g2), M, N, K, int(act), dptr(y), stream()),
              "nm_linear")
    else:
        raise _lib.NerfmatchAmdError(f"LINEAR_PRECISION must be 'fp32' or 'bf16x3', got {LINEAR_PRECISION!r}")
    return y.reshape(*x.shape[:-1], N)


def layernorm(x, gamma, beta, eps=1e-5):
    dim = x.shape[-1]
    x2 = x.reshape(-1, dim).contiguous()
    y = torch.empty_like(x2)
    if x2.shape[0]:
        check(lib().nm_layernorm(dptr(x2), dptr(gamma), dptr(beta), x2.shape[0], dim, float(eps), dptr(y), stream()), "nm_layernorm")
    return y.reshape(x.shape)


def layernorm_pair(x0, ln0, x1, ln1):
    """(LN0(x0), LN1(x1)) in ONE launch (nm_layernorm2) when both have the same width -- the two pre-norms of a cross-attention layer;
    a row's arithmetic is nm_layernorm's, so the results are the same bits as two calls of `layernorm`."""
    dim = x0.shape[-1]
    if x1.shape[-1] != dim or x0.numel() == 0 or x1.numel() == 0:
        return layernorm(x0, ln0.weight, ln0.bias, ln0.eps), layernorm(x1, ln1.weight, ln1.bias, ln1.eps)
    a, b = x0.reshape(-1, dim).contiguous(), x1.reshape(-1, dim).contiguous()
    ya, yb = torch.empty_like(a), torch.empty_like(b)
    check(lib().nm_layernorm2(dptr(a), dptr(ln0.weight), dptr(ln0.bias), a.shape[0], float(ln0.eps), dptr(ya), dptr(b), dptr(ln1.weight), dptr(ln1.bias),
                              b.shape[0], float(ln1.eps), dptr(yb), dim, stream()), "nm_layernorm2")
    return ya.reshape(x0.shape), yb.reshape(x1.shape)


# Arithmetic of the two attention contractions: "fp32" (v_mfma_f32_32x32x2_f32), "bf16x3" (bf16 MFMA on hi/lo-split
# operands, fp32-accurate) or "fp8" (ONE e4m3 MFMA per product block: the THROUGHPUT configuration of BASELINE config 5, not a
# parity arithmetic; head_dim 32 sequences only, everything else falls to bf16x3).  Module-level switch so that the encoder
# modules need no extra plumbing.
ATTENTION_PRECISION = "fp32"


def _attn_flags():
    if ATTENTION_PRECISION not in ("fp32", "bf16x3", "fp8"):
        raise _lib.NerfmatchAmdError(f"ATTENTION_PRECISION must be 'fp32', 'bf16x3' or 'fp8', got {ATTENTION_PRECISION}")
    return _lib.NM_ATTN_BF16X3 if ATTENTION_PRECISION in ("bf16x3", "fp8") else 0


_ATTN_FP8_WS = {}


def _attention_fp8(qp, kp, vp_, ldq, ldk, ldv, B, L, S, heads, scale, out, dev):
    ws = _scratch(_ATTN_FP8_WS, dev, lib().nm_attention_fp8_workspace_bytes(int(B), int(S), int(heads)))
    check(lib().nm_attention_fp8(qp, kp, vp_, ldq, ldk, ldv, int(B), int(L), int(S), int(heads), float(scale), dptr(ws, torch.uint8), dptr(out),
                                 stream()), "nm_attention_fp8")


def _use_fp8(L, S, head_dim):
    return ATTENTION_PRECISION == "fp8" and head_dim == 32 and not (L <= 64 and S <= 64)


def attention(q, k, v, heads, scale):
    """q (B,L,C), k/v (B,S,C) -> (B,L,C); softmax((q*scale).k) v per head."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    B, L, Cc = q.shape
    S = k.shape[1]
    out = torch.empty_like(q)
    if B * L and _use_fp8(L, S, Cc // heads):
        _attention_fp8(dptr(q), dptr(k), dptr(v), Cc, Cc, Cc, B, L, S, heads, scale, out, q.device)
    elif B * L:
        flags = _attn_flags()
        with _probe("nm_attention_ws", 4.0 * B * L * S * Cc):
            check(lib().nm_attention(dptr(q), dptr(k), dptr(v), Cc, Cc, Cc, B, L, S, int(heads), Cc // heads, float(scale), flags,
                                     _attn_workspace(q.device, B, S, heads, flags, L, Cc // heads), dptr(out), None, stream()), "nm_attention")
    return out


_ATTN_WS = {}


def _attn_workspace(dev, B, S, heads, flags, L=None, head_dim=32):
    """Scratch for the pre-split K / V operands of the bf16x3 kernel, one (growing) buffer per (device, stream).  NULL for the
    shapes nm_attention does not route to that kernel (head dim != 32, or the <= 64-token windows of the fine stage: with
    thousands of windows the request would be ~1 GB and re-grow -- a device allocation, milliseconds -- whenever a batch had
    more matches than any before)."""
    if not (flags & _lib.NM_ATTN_BF16X3) or head_dim != 32 or (L is not None and L <= 64 and S <= 64):
        return C.c_void_p(0)
    return dptr(_scratch(_ATTN_WS, dev, lib().nm_attention_workspace_bytes(int(B), int(S), int(heads))), torch.uint8)


def lse_supported(L, S, head_dim):
    """True when the attention forward can keep the log-sum-exp for the backward pass (nm_attention's nlse_out: the split-bf16 kernel)."""
    return ATTENTION_PRECISION == "bf16x3" and head_dim == 32 and not (L <= 64 and S <= 64)


def attention_fused(qkv, q_cols, k_cols, v_cols, B, L, S, heads, scale, kv=None, want_lse=False):
    """Attention reading q / k / v as column slices of fused projection buffers.
    qkv: (B*L, ld) holding q at column offset q_cols (and k, v too when kv is None); kv: (B*S, ldkv) holding k and v.
    want_lse (training forward): -> (out, nlse) with nlse (B, heads, L) = -(log-sum-exp), log2 domain, for attention_bwd_fused -- or
    (out, None) where the kernel at hand does not keep it."""
    src_kv = qkv if kv is None else kv
    ldq, ldkv = qkv.shape[1], src_kv.shape[1]
    dim = (k_cols[1] - k_cols[0])
    out = torch.empty(B * L, dim, device=qkv.device, dtype=torch.float32)
    esz = 4
    qp = C.c_void_p(qkv.data_ptr() + q_cols[0] * esz)
    kp = C.c_void_p(src_kv.data_ptr() + k_cols[0] * esz)
    vp_ = C.c_void_p(src_kv.data_ptr() + v_cols[0] * esz)
    assert qkv.is_contiguous() and src_kv.is_contiguous() and qkv.dtype == torch.float32
    if _use_fp8(L, S, dim // heads):
        _attention_fp8(qp, kp, vp_, ldq, ldkv, ldkv, B, L, S, heads, scale, out, qkv.device)
        return (out.reshape(B, L, dim), None) if want_lse else out.reshape(B, L, dim)
    flags = _attn_flags()
    nlse = torch.empty(B, heads, L, device=qkv.device, dtype=torch.float32) if want_lse and lse_supported(L, S, dim // heads) else None
    with _probe("nm_attention_ws", 4.0 * B * L * S * dim):
        check(lib().nm_attention(qp, kp, vp_, ldq, ldkv, ldkv, B, L, S, int(heads), dim // heads, float(scale), flags,
                                 _attn_workspace(qkv.device, B, S, heads, flags, L, dim // heads), dptr(out), dptr(nlse), stream()), "nm_attention")
    return (out.reshape(B, L, dim), nlse) if want_lse else out.reshape(B, L, dim)


def projected_attention_supported(K, heads, head_dim, L, S):
    """True when attention_projected can take the projection + attention of a layer (split-bf16 arithmetic on both, head dim
    32, whole 128-column chunks per role, whole 32-key tiles)."""
    return (LINEAR_PRECISION == "bf16x3" and ATTENTION_PRECISION == "bf16x3" and head_dim == 32 and (32 * heads) % 128 == 0 and
            S % 32 == 0 and K % 8 == 0 and not (L <= 64 and S <= 64))


def attention_projected(x_q, w_q, x_kv, w_stack, B, L, S, heads, scale):
    """softmax(q k^T scale) v with the projections fused in front: the keys and values never exist as fp32 rows -- the
    projection GEMM writes them split into bf16 hi / lo parts, laid out as the MFMA operands of the attention kernel.
    Self attention: x_kv is None, x_q (B*L, K), w_stack = [Wq; Wk; Wv].  Cross attention: x_q (B*L, K) is projected with w_q
    by the plain GEMM, x_kv (B*S, K) with w_stack = [Wk; Wv]."""
    dev = x_q.device
    inner = 32 * heads
    flags = _attn_flags()
    ws = _attn_workspace(dev, B, S, heads, flags, L, 32)
    if x_kv is None:
        x2 = x_q.contiguous()
        q = torch.empty(B * L, inner, device=dev, dtype=torch.float32)
        check(lib().nm_linear_qkv_bf16x3(dptr(x2), dptr(_linear_blob(w_stack), torch.uint8), B * L, x2.shape[1], inner, int(heads), int(S),
                                         dptr(q), ws, stream()), "nm_linear_qkv_bf16x3")
    else:
        q = linear(x_q, w_q)
        x2 = x_kv.contiguous()
        check(lib().nm_linear_qkv_bf16x3(dptr(x2), dptr(_linear_blob(w_stack), torch.uint8), B * S, x2.shape[1], 0, int(heads), int(S), None, ws,
                                         stream()), "nm_linear_qkv_bf16x3")
    out = torch.empty(B * L, inner, device=dev, dtype=torch.float32)
    with _probe("attn32_v3_kernel", 4.0 * B * L * S * inner):  # exactly one launch of the attention kernel (operands pre-split by the GEMM)
        check(lib().nm_attention_presplit(dptr(q), inner, ws, int(B), int(L), int(S), int(heads), float(scale), dptr(out), stream()),
              "nm_attention_presplit")
    return out.reshape(B, L, inner)


def nchw_to_tokens(x, pe_table=None):
    """(B,C,h,w) -> (B,h*w,C), optionally adding the sine PE table (C,Hmax,Wmax)."""
    x = x.contiguous()
    if pe_table is not None:
        pe_table = pe_table.contiguous()
    B, Cc, h, w = x.shape
    y = torch.empty(B, h * w, Cc, device=x.device, dtype=torch.float32)
    th, tw = (pe_table.shape[1], pe_table.shape[2]) if pe_table is not None else (0, 0)
    check(lib().nm_add_sine_pe(dptr(x), dptr(pe_table), B, h, w, Cc, th, tw, dptr(y), stream()), "nm_add_sine_pe")
    return y


def nhwc_to_nchw(x, out=None):
    """(B,h,w,C) channel-last -> (B,C,h,w) planes (nm_nhwc_to_nchw), into `out` when given: a contiguous fp32 device tensor of that
    shape (a slice along the batch of a larger one will do); anything else raises."""
    B, h, w, Cc = x.shape
    y = torch.empty(B, Cc, h, w, device=x.device, dtype=torch.float32) if out is None else out
    assert tuple(y.shape) == (B, Cc, h, w)
    check(lib().nm_nhwc_to_nchw(dptr(x), B, h * w, Cc, dptr(y), stream()), "nm_nhwc_to_nchw")
    return y


def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv_patches(x, k, stride, pad, ld, channel_last=False):
    """The k x k patches of a strided convolution as GEMM rows (nm_conv_patches): x (B,C,H,W), or (B,H,W,C) with channel_last ->
    (B*Ho*Wo, ld), columns in (ky, kx, c) order and zero from k*k*C on; also returns (Ho, Wo)."""
    if channel_last:
        B, H, W, Cc = x.shape
    else:
        B, Cc, H, W = x.shape
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    if Ho < 1 or Wo < 1:
        raise _lib.NerfmatchAmdError(f"conv_patches: a {H}x{W} image is smaller than the {k}x{k} kernel with padding {pad}")
    rows = torch.empty(B * Ho * Wo, int(ld), device=x.device, dtype=torch.float32)
    check(lib().nm_conv_patches(dptr(x), int(bool(channel_last)), B, Cc, H, W, int(k), int(stride), int(pad), int(ld), dptr(rows), stream()),
          "nm_conv_patches")
    return rows, (Ho, Wo)


def conv_weight_rows(weight, ld):
    """A Conv2d weight (N, C, k, k) as the (N, ld) matrix that multiplies conv_patches' rows: columns in (ky, kx, c) order, zero-padded
    to ld; cached until the tensor changes, like every derived copy of a weight."""
    N = weight.shape[0]
    kkc = weight.shape[1] * weight.shape[2] * weight.shape[3]
    return _linear_cached(("convrows", int(ld)), weight,
                          lambda w: torch.nn.functional.pad(w.permute(0, 2, 3, 1).reshape(N, kkc), (0, int(ld) - kkc)).contiguous())


def dwconv_weight_taps(weight):
    """A depthwise 7x7 weight (C, 1, 7, 7) as nm_dwconv7_nhwc's tap-major (49, C) matrix, cached until the tensor changes."""
    return _linear_cached(("dwtaps",), weight, lambda w: w.reshape(w.shape[0], 49).t().contiguous())


def dwconv7_nhwc(x, weight, act_scale=None, act_bias=None, taps=None):
    """Depthwise 7x7 convolution, stride 1, zero padding 3, of channel-last x (B,H,W,C) (nm_dwconv7_nhwc); weight: the (C,1,7,7)
    parameter (or taps: its (49, C) form).  act_scale / act_bias: the two 1-element StarReLU parameters, applied to x on the way in."""
    B, H, W, Cc = x.shape
    w49 = dwconv_weight_taps(weight) if taps is None else taps
    assert tuple(w49.shape) == (49, Cc)
    y = torch.empty_like(x)
    check(lib().nm_dwconv7_nhwc(dptr(x), dptr(w49), dptr(act_scale), dptr(act_bias), B, H, W, Cc, dptr(y), stream()), "nm_dwconv7_nhwc")
    return y


def star_relu(x, scale, bias, inplace=False):
    """scale * relu(x)**2 + bias (nm_star_relu); scale, bias: 1-element device tensors."""
    if not x.is_contiguous():
        raise _lib.NerfmatchAmdError("star_relu: hand over a contiguous tensor")
    y = x if inplace else torch.empty_like(x)
    if x.numel():
        check(lib().nm_star_relu(dptr(x), dptr(scale), dptr(bias), x.numel(), dptr(y), stream()), "nm_star_relu")
    return y


# ---- the backbone's fp16 inference walk: fp16 tensors are torch.float16, `events` a device int32 tensor of one element
# (or None) onto which a kernel adds the values it stored as non-finite fp16 from a finite fp32 value
def f16_events(dev):
    """A zeroed overflow-event counter for the fp16 kernels."""
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _linear_blob_f16(weight):
    """fp16-rounded, re-ordered copy of a weight matrix for nm_linear_f16, cached until the tensor changes like the bf16x3 blobs."""
    N, K = weight.shape

    def make(w):
        blob = torch.empty(lib().nm_linear_blob_bytes_f16(N, K), dtype=torch.uint8, device=w.device)
        check(lib().nm_linear_pack_f16(dptr(w.contiguous()), N, K, dptr(blob, torch.uint8), stream()), "nm_linear_pack_f16")
        return blob
    return _linear_cached(("f16",), weight, make)


def linear_f16(x, weight, bias=None, residual=None, star=None, out_dtype=torch.float16, events=None):
    """y = star(x @ fp16(weight).T + bias) + residual for fp16 rows x (..., K) (nm_linear_f16: one fp16 MFMA product per K-step, fp32
    accumulation); weight (N, K) fp32 as stored, bias (N,) and residual (..., N) fp32.  star: StarReLU's (scale, bias) 1-element device
    tensors, applied to the fp32 accumulator.  out_dtype torch.float16 (rounded once, no saturation) or torch.float32; a residual needs
    fp32 output.  K and N multiples of 8."""
    K = x.shape[-1]
    N = weight.shape[0]
    if out_dtype not in (torch.float16, torch.float32):
        raise _lib.NerfmatchAmdError(f"linear_f16: out_dtype must be torch.float16 or torch.float32, got {out_dtype}")
    if residual is not None and out_dtype != torch.float32:
        raise _lib.NerfmatchAmdError("linear_f16: a residual is added in fp32: ask for out_dtype=torch.float32")
    x2 = x.reshape(-1, K).contiguous()
    M = x2.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=out_dtype)
    if M:
        r2 = None if residual is None else residual.reshape(-1, N).contiguous()
        sc, sb = (None, None) if star is None else star
        check(lib().nm_linear_f16(dptr(x2, torch.float16), dptr(_linear_blob_f16(weight), torch.uint8), dptr(bias), dptr(sc), dptr(sb), dptr(r2),
                                  M, N, K, int(out_dtype == torch.float16), dptr(y, out_dtype), dptr(events, torch.int32), stream()), "nm_linear_f16")
    return y.reshape(*x.shape[:-1], N)


def _linear_blob_t_f16(weight):
    """nm_linear_pack_f16's blob of weight.T made straight from the stored (N_out, K_in) fp32 tensor (nm_linear_pack_t_f16), cached under its
    own key prefix: the dX product of the fp16 training walk."""
    K, N = weight.shape  # stored (out = K of the product, in = N of the product): the packed matrix is (N, K)

    def make(w):
        blob = torch.empty(lib().nm_linear_blob_bytes_f16(N, K), dtype=torch.uint8, device=w.device)
        check(lib().nm_linear_pack_t_f16(dptr(w.contiguous()), N, K, dptr(blob, torch.uint8), stream()), "nm_linear_pack_t_f16")
        return blob
    return _linear_cached(("f16T",), weight, make)


def linear_chain_f16(x, weight, bias=None, x2=None, weight2=None, relu=False, residual=None, gate=None, alpha=1.0, transposed=False,
                     out_dtype=torch.float16, events=None):
    """y = alpha * [gate > 0] * (relu?(x @ W.T + x2 @ W2.T + bias) + residual) for fp16 rows x (M, K), x2 (M, K2) (nm_linear_chain_f16: one
    fp16 MFMA product per K-step, fp32 accumulation, the two sources in ONE K loop).  weight / weight2: fp32 as stored, rounded to fp16 when
    packed (cached); transposed=True: W = weight.T for a stored weight (K, N) -- a layer's dX product.  bias fp32 (N,), residual and gate
    fp16 (M, N).  out_dtype torch.float16 (rounded once, no saturation, non-finite stores counted into `events`) or torch.float32."""
    if out_dtype not in (torch.float16, torch.float32):
        raise _lib.NerfmatchAmdError(f"linear_chain_f16: out_dtype must be torch.float16 or torch.float32, got {out_dtype}")
    if (x2 is None) != (weight2 is None):
        raise _lib.NerfmatchAmdError("linear_chain_f16: x2 and weight2 come together")
    if transposed and x2 is not None:
        raise _lib.NerfmatchAmdError("linear_chain_f16: the transposed form takes one source")
    M, K = x.shape
    N = weight.shape[1] if transposed else weight.shape[0]
    if (weight.shape[0] if transposed else weight.shape[1]) != K:
        raise _lib.NerfmatchAmdError(f"linear_chain_f16: x has {K} columns, the weight {tuple(weight.shape)} (transposed={transposed})")
    K2 = 0
    if x2 is not None:
        K2 = x2.shape[1]
        if tuple(weight2.shape) != (N, K2) or x2.shape[0] != M:
            raise _lib.NerfmatchAmdError(f"linear_chain_f16: second source {tuple(x2.shape)} x {tuple(weight2.shape)} for {M} rows of {N}")
    for name, t in (("residual", residual), ("gate", gate)):
        if t is not None and tuple(t.shape) != (M, N):
            raise _lib.NerfmatchAmdError(f"linear_chain_f16: {name} {tuple(t.shape)} for an output of {(M, N)}")
    y = torch.empty(M, N, device=x.device, dtype=out_dtype)
    if M:
        blob = _linear_blob_t_f16(weight) if transposed else _linear_blob_f16(weight)
        blob2 = None if x2 is None else _linear_blob_f16(weight2)
        f16 = torch.float16
        check(lib().nm_linear_chain_f16(dptr(x, f16), dptr(blob, torch.uint8), K, dptr(x2, f16), dptr(blob2, torch.uint8), K2, dptr(bias),
                                        dptr(residual, f16), dptr(gate, f16), float(alpha), int(bool(relu)), M, N, int(out_dtype == f16),
                                        dptr(y, out_dtype), dptr(events, torch.int32), stream()), "nm_linear_chain_f16")
    return y


_WGRAD_F16_WS = {}


def linear_wgrad_f16_slice_rows(M):
    """Rows of one workgroup's slice of M in nm_linear_wgrad_f16 (64 up to M = 16384)."""
    return int(lib().nm_linear_wgrad_f16_slice_rows(int(M)))


def linear_wgrad_f16(dy, x, out=None, alpha=1.0, bias=True):
    """(dw, db) = alpha * (dy.T @ x, column sums of dy) for fp16 rows dy (M, N), x (M, K): fp32 accumulation, fp32 results, partial sums
    added in a fixed order (nm_linear_wgrad_f16).  out = (dw, db): both are added onto.  bias=False: db is not formed (-> None)."""
    f16 = torch.float16
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise _lib.NerfmatchAmdError(f"linear_wgrad_f16: dy has {M} rows, x {x.shape[0]}")
    acc = out is not None
    dw = out[0] if acc else torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = None if not bias else (out[1] if acc else torch.empty(N, device=dy.device, dtype=torch.float32))
    if M == 0:
        return (dw, db) if acc else (dw.zero_(), None if db is None else db.zero_())
    ws = _scratch(_WGRAD_F16_WS, dy.device, lib().nm_linear_wgrad_f16_workspace_bytes(M, N, K))
    check(lib().nm_linear_wgrad_f16(dptr(dy, f16), dptr(x, f16), M, N, K, float(alpha), int(acc), dptr(dw), dptr(db), dptr(ws, torch.uint8),
                                    ws.numel(), stream()), "nm_linear_wgrad_f16")
    return dw, db


def layernorm_f16(x, gamma, beta, eps=1e-5, events=None):
    """ops.layernorm(x, ...) rounded to fp16, bit for bit, in one kernel (nm_layernorm_f16); x fp32, dim in {128, 256, 512}."""
    dim = x.shape[-1]
    x2 = x.reshape(-1, dim).contiguous()
    y = torch.empty(x2.shape, device=x.device, dtype=torch.float16)
    if x2.shape[0]:
        check(lib().nm_layernorm_f16(dptr(x2), dptr(gamma), dptr(beta), x2.shape[0], dim, float(eps), dptr(y, torch.float16),
                                     dptr(events, torch.int32), stream()), "nm_layernorm_f16")
    return y.reshape(x.shape)


def dwconv7_nhwc_f16(x, weight, act_scale=None, act_bias=None, taps=None, events=None):
    """ops.dwconv7_nhwc on fp16 channel-last x (B,H,W,C) with an fp16 result (nm_dwconv7_nhwc_f16): the fp32 kernel's sums on the widened input,
    rounded once.  weight / taps, act_scale / act_bias: fp32, as for dwconv7_nhwc."""
    B, H, W, Cc = x.shape
    w49 = dwconv_weight_taps(weight) if taps is None else taps
    assert tuple(w49.shape) == (49, Cc)
    y = torch.empty_like(x)
    check(lib().nm_dwconv7_nhwc_f16(dptr(x, torch.float16), dptr(w49), dptr(act_scale), dptr(act_bias), B, H, W, Cc, dptr(y, torch.float16),
                                    dptr(events, torch.int32), stream()), "nm_dwconv7_nhwc_f16")
    return y


def conv_patches_f16(x, k, stride, pad, ld, channel_last=False, events=None):
    """ops.conv_patches with fp16 rows (nm_conv_patches_f16): from an fp32 image (B,C,H,W), rounded as it is gathered, or -- channel_last -- from
    fp16 rows (B,H,W,C) with C % 8 == 0, copied.  Returns (rows (B*Ho*Wo, ld) fp16, (Ho, Wo))."""
    if channel_last:
        B, H, W, Cc = x.shape
    else:
        B, Cc, H, W = x.shape
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    if Ho < 1 or Wo < 1:
        raise _lib.NerfmatchAmdError(f"conv_patches_f16: a {H}x{W} image is smaller than the {k}x{k} kernel with padding {pad}")
    rows = torch.empty(B * Ho * Wo, int(ld), device=x.device, dtype=torch.float16)
    check(lib().nm_conv_patches_f16(dptr(x, torch.float16 if channel_last else torch.float32), int(bool(channel_last)), B, Cc, H, W, int(k), int(stride),
                                    int(pad), int(ld), dptr(rows, torch.float16), dptr(events, torch.int32), stream()), "nm_conv_patches_f16")
    return rows, (Ho, Wo)


_DWCONV_BWD_INPUT_WS = {}
_DWCONV_BWD_WEIGHT_WS = {}
_STAR_RELU_BWD_WS = {}


def dwconv7_nhwc_bwd(dy, x, taps, act_scale=None, act_bias=None, need=(True, True, True)):
    """Backward of dwconv7_nhwc (nm_dwconv7_nhwc_bwd_input / _bwd_weight): dy, x (B,H,W,C), taps (49,C) ->
    (dx, dw49c (49,C) tap-major, dscale_dbias (2,)); need = which of (dx, dw49c, the two scalars) to compute, None for the others --
    dw49c alone costs one kernel, the scalars come out of the input-gradient kernel."""
    B, H, W, Cc = x.shape
    dy = _aligned16(dy.contiguous())
    assert dy.shape == x.shape and tuple(taps.shape) == (49, Cc)
    act = act_scale is not None
    dx = dw = dsb = None
    if need[0] or (act and need[2]):
        dx = torch.empty_like(x)
        ws = None
        if act and need[2]:
            dsb = torch.empty(2, device=x.device, dtype=torch.float32)
            ws = _scratch(_DWCONV_BWD_INPUT_WS, x.device, lib().nm_dwconv7_nhwc_bwd_input_workspace_bytes(B, H, W, Cc))
        check(lib().nm_dwconv7_nhwc_bwd_input(dptr(dy), dptr(taps), dptr(x) if act else None, dptr(act_scale), B, H, W, Cc, dptr(dx), dptr(dsb),
                                              dptr(ws, torch.uint8), 0 if ws is None else ws.numel(), stream()), "nm_dwconv7_nhwc_bwd_input")
    if need[1]:
        dw = torch.empty(49, Cc, device=x.device, dtype=torch.float32)
        ws = _scratch(_DWCONV_BWD_WEIGHT_WS, x.device, lib().nm_dwconv7_nhwc_bwd_weight_workspace_bytes(B, H, W, Cc))
        check(lib().nm_dwconv7_nhwc_bwd_weight(dptr(dy), dptr(x), dptr(act_scale), dptr(act_bias), B, H, W, Cc, dptr(dw), dptr(ws, torch.uint8),
                                               ws.numel(), stream()), "nm_dwconv7_nhwc_bwd_weight")
    return dx if need[0] else None, dw, dsb


def star_relu_bwd(x, dy, scale, need_params=True):
    """Backward of star_relu (nm_star_relu_bwd): -> (dx like x, dscale_dbias (2,) or None)."""
    dy = _aligned16(dy.contiguous())
    if not x.is_contiguous() or dy.shape != x.shape:
        raise _lib.NerfmatchAmdError("star_relu_bwd: x contiguous and dy of its shape")
    dx = torch.empty_like(x)
    dsb = torch.zeros(2, device=x.device, dtype=torch.float32) if need_params else None
    if x.numel():
        ws = _scratch(_STAR_RELU_BWD_WS, x.device, lib().nm_star_relu_bwd_workspace_bytes(x.numel())) if need_params else None
        check(lib().nm_star_relu_bwd(dptr(x), dptr(dy), dptr(scale), x.numel(), dptr(dx), dptr(dsb), dptr(ws, torch.uint8),
                                     0 if ws is None else ws.numel(), stream()), "nm_star_relu_bwd")
    return dx, dsb


def conv_patches_bwd(drows, shape, k, stride, pad):
    """The adjoint of conv_patches for a channel-last input of `shape` = (B,H,W,C) (nm_conv_patches_bwd): drows (B*Ho*Wo, ld) -> dx."""
    B, H, W, Cc = shape
    drows = _aligned16(drows.contiguous())
    assert drows.shape[0] == B * conv_out_size(H, k, stride, pad) * conv_out_size(W, k, stride, pad)
    dx = torch.empty(B, H, W, Cc, device=drows.device, dtype=torch.float32)
    check(lib().nm_conv_patches_bwd(dptr(drows), 1, B, Cc, H, W, int(k), int(stride), int(pad), drows.shape[1], dptr(dx), stream()),
          "nm_conv_patches_bwd")
    return dx


def feature_normalize(x):
    """x (B,N,D) is centred IN PLACE (per set b: minus the mean over its N rows); returns the centred set divided by its largest row norm
    (nm_feature_normalize; the coarse model's `pt_feat_norm` option).  x must be contiguous: a silent copy would be centred instead of the
    caller's tensor."""
    if not x.is_contiguous():
        raise _lib.NerfmatchAmdError("feature_normalize centres x in place: hand over a contiguous tensor")
    B, N, D = x.shape
    y = torch.empty_like(x)
    check(lib().nm_feature_normalize(dptr(x), B, N, D, dptr(y), stream()), "nm_feature_normalize")
    return y


def cat_fourier(feat, pt3d, num_freqs=15):
    """(n,C),(n,3) -> (n, ld) = [feat | x | sin/cos(2^f x)...] zero padded to a multiple of 8 columns."""
    feat, pt3d = feat.contiguous(), pt3d.contiguous()
    n, Cc = feat.shape
    ld = ((Cc + 3 + 6 * num_freqs + 7) // 8) * 8
    out = torch.empty(n, ld, device=feat.device, dtype=torch.float32)
    check(lib().nm_cat_fourier(dptr(feat), dptr(pt3d), n, Cc, int(num_freqs), dptr(out), stream()), "nm_cat_fourier")
    return out


def cat_fourier_bwd(dy, pt3d, C, num_freqs=15):
    """d loss / d pt3d (n,3) from the gradient dy (n, ld) of cat_fourier's output."""
    dy, pt3d = dy.contiguous(), pt3d.contiguous()
    g = torch.empty_like(pt3d)
    if pt3d.shape[0]:
        check(lib().nm_cat_fourier_bwd(dptr(dy), dptr(pt3d), pt3d.shape[0], int(C), int(num_freqs), dptr(g), stream()), "nm_cat_fourier_bwd")
    return g


_ws_cache = {}


def _match_workspace(dev, need):
    """Scratch of the matching kernels (similarity matrix + statistics), one growing buffer per (device, stream): calls on one
    stream are serialised, calls on different streams must not share it."""
    return _scratch(_ws_cache, dev, need)


def invalidate_caches():
    """Drop every derived-weight cache of this module (packed bf16x3 weight blobs).  The caches are keyed on (data_ptr,
    _version) of the source tensor; writes through `.data` (EMA updates, manual weight surgery) do not bump `_version`, so
    call this -- and `module.invalidate()` on NeRF / matcher modules -- after such writes."""
    _linear_evict()


# Arithmetic of the similarity GEMM of the dual-softmax matcher: "fp32" or "bf16x3" (cf. LINEAR_PRECISION)
MATCH_PRECISION = "fp32"


def dual_softmax_match(im, pt, scale, im_mask=None, pt_mask=None, threshold=0.0, mutual=True, want_conf=True, want_norm=False,
                       conf_out=None, defer_count=False):
    """im (M,C), pt (N,C) -> dict(i_ids, j_ids, mconf [K], conf (M,N) | None, im_norm, pt_norm).
    K is read back from the device (one 4-byte D2H copy), as the reference's torch.where does implicitly."""
    M, Cc = im.shape
    N = pt.shape[0]
    dev = im.device
    L = lib()
    need = L.nm_match_workspace_bytes(M, N, Cc)
    ws = _match_workspace(dev, need)
    conf = (conf_out if conf_out is not None else torch.empty(M, N, device=dev, dtype=torch.float32)) if want_conf else None
    assert conf is None or (conf.shape == (M, N) and conf.is_contiguous())
    imn = torch.empty(M, Cc, device=dev, dtype=torch.float32) if want_norm else None
    ptn = torch.empty(N, Cc, device=dev, dtype=torch.float32) if want_norm else None
    oi = torch.empty(M, device=dev, dtype=torch.int64)
    oj = torch.empty(M, device=dev, dtype=torch.int64)
    oc = torch.empty(M, device=dev, dtype=torch.float32)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    im_m, pt_m = _mask_u8(im_mask), _mask_u8(pt_mask)
    if MATCH_PRECISION not in ("fp32", "bf16x3"):
        raise _lib.NerfmatchAmdError(f"MATCH_PRECISION must be 'fp32' or 'bf16x3', got {MATCH_PRECISION!r}")
    flags = _lib.NM_MATCH_BF16X3 if MATCH_PRECISION == "bf16x3" else 0
    check(L.nm_dual_softmax_match(dptr(im), dptr(pt), M, N, Cc, float(scale), dptr(im_m, torch.uint8), dptr(pt_m, torch.uint8),
                                  float(threshold), int(bool(mutual)), flags, dptr(conf), dptr(imn), dptr(ptn), dptr(oi, torch.int64),
                                  dptr(oj, torch.int64), dptr(oc), dptr(cnt, torch.int32), dptr(ws, torch.uint8), C.c_size_t(need),
                                  stream()), "nm_dual_softmax_match")
    if defer_count:  # the caller reads `count` back later (one synchronisation for a whole batch) and slices itself
        return dict(i_ids=oi, j_ids=oj, mconf=oc, conf=conf, im_norm=imn, pt_norm=ptn, count=cnt)
    k = int(cnt.item())
    return dict(i_ids=oi[:k], j_ids=oj[:k], mconf=oc[:k], conf=conf, im_norm=imn, pt_norm=ptn, count=cnt)


MATCH_FUSED = True  # False: always the per-pair path that materialises the similarity matrix (A/B runs, tests)
_fused_ws = {}


def _dual_softmax_match_fused(im, pt, scale, im_mask, pt_mask, threshold, mutual):
    B, M, Cc = im.shape
    N = pt.shape[1]
    dev = im.device
    L = lib()
    need = L.nm_match_fused_workspace_bytes(B, M, N, Cc)
    ws = _scratch(_fused_ws, dev, need)
    # (one allocation for the three lists; the compaction kernel writes every slot: matches first, zeros behind the count -- the
    # single-pair path's speculative fine stage reads the first `cap` slots as indices before the count is known)
    buf = torch.empty(B * M * 20, device=dev, dtype=torch.uint8)
    oi = buf[: B * M * 8].view(torch.int64).view(B, M)
    oj = buf[B * M * 8: B * M * 16].view(torch.int64).view(B, M)
    oc = buf[B * M * 16:].view(torch.float32).view(B, M)
    cnt = torch.empty(B, device=dev, dtype=torch.int32)
    im_m, pt_m = _mask_u8(im_mask), _mask_u8(pt_mask)
    with _probe("nm_dual_softmax_match_fused", 2.0 * B * M * N * Cc):
        rc = L.nm_dual_softmax_match_fused(dptr(im), dptr(pt), B, M, N, Cc, float(scale), dptr(im_m, torch.uint8), dptr(pt_m, torch.uint8),
                                           float(threshold), int(bool(mutual)), dptr(oi, torch.int64), dptr(oj, torch.int64), dptr(oc),
                                           dptr(cnt, torch.int32), dptr(ws, torch.uint8), C.c_size_t(need), stream())
    if rc == _lib.NM_ERR_UNSUPPORTED:
        return None
    check(rc, "nm_dual_softmax_match_fused")
    return dict(i_ids=oi, j_ids=oj, mconf=oc, count=cnt, conf=None, im_norm=None, pt_norm=None)


def dual_softmax_match_batch(im, pt, scale, im_mask=None, pt_mask=None, threshold=0.0, mutual=True, want_conf=True, want_norm=False):
    """Batched form: im (B,M,C), pt (B,N,C) -> dict(i_ids, j_ids (B,M) int64, mconf (B,M), count (B,) int32 [device],
    conf (B,M,N) | None, im_norm, pt_norm).  One allocation per output for the whole batch and no per-element torch calls
    (the host issues the B kernel sequences back to back); the valid prefix of row b has count[b] entries."""
    B, M, Cc = im.shape
    N = pt.shape[1]
    dev = im.device
    L = lib()
    if MATCH_PRECISION not in ("fp32", "bf16x3"):
        raise _lib.NerfmatchAmdError(f"MATCH_PRECISION must be 'fp32' or 'bf16x3', got {MATCH_PRECISION!r}")
    flags = _lib.NM_MATCH_BF16X3 if MATCH_PRECISION == "bf16x3" else 0
    im, pt = im.contiguous(), pt.contiguous()
    if not want_conf and not want_norm and MATCH_PRECISION == "bf16x3" and MATCH_FUSED:
        # inference without the confidence matrix: the similarity never leaves the registers and the whole batch is ONE launch
        # sequence (csrc/match_fused.hip); shapes / temperatures it does not take fall through to the per-pair path below
        r = _dual_softmax_match_fused(im, pt, scale, im_mask, pt_mask, threshold, mutual)
        if r is not None:
            return r
    # (only the per-pair path needs the M x N similarity workspace -- ~92 MB at 4800^2; the fused path above never allocates it)
    need = L.nm_match_workspace_bytes(M, N, Cc)
    ws = _match_workspace(dev, need)
    conf = torch.empty(B, M, N, device=dev, dtype=torch.float32) if want_conf else None
    imn = torch.empty(B, M, Cc, device=dev, dtype=torch.float32) if want_norm else None
    ptn = torch.empty(B, N, Cc, device=dev, dtype=torch.float32) if want_norm else None
    oi = torch.zeros(B, M, device=dev, dtype=torch.int64)
    oj = torch.zeros(B, M, device=dev, dtype=torch.int64)
    oc = torch.zeros(B, M, device=dev, dtype=torch.float32)
    cnt = torch.zeros(B, device=dev, dtype=torch.int32)
    im_m, pt_m = _mask_u8(im_mask), _mask_u8(pt_mask)
    off = lambda t, b, stride: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + b * stride)
    st, wsp = stream(), dptr(ws, torch.uint8)
    for b in range(B):
        check(L.nm_dual_softmax_match(off(im, b, M * Cc * 4), off(pt, b, N * Cc * 4), M, N, Cc, float(scale), off(im_m, b, M), off(pt_m, b, N),
                                      float(threshold), int(bool(mutual)), flags, off(conf, b, M * N * 4), off(imn, b, M * Cc * 4),
                                      off(ptn, b, N * Cc * 4), off(oi, b, M * 8), off(oj, b, M * 8), off(oc, b, M * 4), off(cnt, b, 4),
                                      wsp, C.c_size_t(need), st), "nm_dual_softmax_match")
    return dict(i_ids=oi, j_ids=oj, mconf=oc, count=cnt, conf=conf, im_norm=imn, pt_norm=ptn)


_feature_nn_ws = {}


def feature_mutual_nn(desc1, desc2, threshold=None, eps=1e-9, want_nn=False):
    """nm_feature_mutual_nn: cosine mutual nearest neighbours of desc1 (N1,C) and desc2 (N2,C) -> (matches (K,2) int64, scores (K,) fp32),
    and with want_nn=True also (nn12 (N1,) int32, nn21 (N2,) int32).  Rows are normalised as f / (|f| + eps); equal similarities go to
    the lowest index; a truthy `threshold` keeps score > threshold, None / 0 keeps every mutual pair.  K is read back from the device
    (one 4-byte copy, like dual_softmax_match).  An empty side returns empty lists without a launch (nn: -1)."""
    if desc1.dim() != 2 or desc2.dim() != 2 or desc1.shape[1] != desc2.shape[1]:
        raise _lib.NerfmatchAmdError(f"feature_mutual_nn: descriptor sets of shapes {tuple(desc1.shape)} and {tuple(desc2.shape)}")
    N1, Cc = desc1.shape
    N2 = desc2.shape[0]
    dev = desc1.device
    if N1 == 0 or N2 == 0:
        out = (torch.empty(0, 2, device=dev, dtype=torch.int64), torch.empty(0, device=dev, dtype=torch.float32))
        if want_nn:
            out += (torch.full((N1,), -1, device=dev, dtype=torch.int32), torch.full((N2,), -1, device=dev, dtype=torch.int32))
        return out
    L = lib()
    need = L.nm_feature_mutual_nn_workspace_bytes(N1, N2, Cc)
    ws = _scratch(_feature_nn_ws, dev, need)
    matches = torch.empty(N1, 2, device=dev, dtype=torch.int64)
    scores = torch.empty(N1, device=dev, dtype=torch.float32)
    cnt = torch.empty(1, device=dev, dtype=torch.int32)
    nn12 = torch.empty(N1, device=dev, dtype=torch.int32) if want_nn else None
    nn21 = torch.empty(N2, device=dev, dtype=torch.int32) if want_nn else None
    use_thr = bool(threshold)  # the reference's `if threshold:`
    with _probe("nm_feature_mutual_nn", 2.0 * N1 * N2 * Cc):
        rc = L.nm_feature_mutual_nn(dptr(desc1), dptr(desc2), N1, N2, Cc, float(eps), float(threshold) if use_thr else 0.0, int(use_thr),
                                    dptr(matches, torch.int64), dptr(scores), dptr(cnt, torch.int32), dptr(nn12, torch.int32),
                                    dptr(nn21, torch.int32), dptr(ws, torch.uint8), C.c_size_t(need), stream())
    check(rc, "nm_feature_mutual_nn")
    k = int(cnt.item())
    out = (matches[:k], scores[:k])
    return out + (nn12, nn21) if want_nn else out


def fine_windows(ffeat_chw, i_ids, count, win=5, stride=4):
    """ffeat (C,Hf,Wf), i_ids (K,) int64 -> (K, win*win, C)."""
    Cc, Hf, Wf = ffeat_chw.shape
    K = i_ids.shape[0]
    out = torch.empty(K, win * win, Cc, device=ffeat_chw.device, dtype=torch.float32)
    if K:
        check(lib().nm_fine_windows(dptr(ffeat_chw), Cc, Hf, Wf, dptr(i_ids, torch.int64), dptr(count, torch.int32), K, int(win), int(stride),
                                    dptr(out), stream()), "nm_fine_windows")
    return out


def fine_windows_batch(ffeat, map_ids, i_ids, count, win=5, stride=4):
    """ffeat (B,C,Hf,Wf), map_ids / i_ids (K,) int64 -> (K, win*win, C): the window of match k comes from map map_ids[k]."""
    B, Cc, Hf, Wf = ffeat.shape
    K = i_ids.shape[0]
    out = torch.empty(K, win * win, Cc, device=ffeat.device, dtype=torch.float32)
    if K:
        check(lib().nm_fine_windows_batch(dptr(ffeat), B, Cc, Hf, Wf, dptr(map_ids, torch.int64), dptr(i_ids, torch.int64),
                                          dptr(count, torch.int32), K, int(win), int(stride), dptr(out), stream()), "nm_fine_windows_batch")
    return out


def assemble_matches(pt2d, pt3d, i_ids, j_ids, expec_f, mconf, win, fine_ds):
    """One pair's match assembly in one launch (nm_assemble_matches): -> mpt2d_c (K,2), mpt2d_f (K,2), mpt3d (K,3), pred_mask (K,) bool."""
    pt2d, pt3d, i_ids, j_ids, expec_f, mconf = (t.contiguous() for t in (pt2d, pt3d, i_ids, j_ids, expec_f, mconf))
    K, dev = i_ids.shape[0], pt2d.device
    c2, f2, p3 = (torch.empty(K, 2, device=dev), torch.empty(K, 2, device=dev), torch.empty(K, 3, device=dev))
    mask = torch.empty(K, device=dev, dtype=torch.bool)
    if K:
        check(lib().nm_assemble_matches(dptr(pt2d), dptr(pt3d), dptr(i_ids, torch.int64), dptr(j_ids, torch.int64), dptr(expec_f), dptr(mconf), K,
                                        float(win), float(fine_ds), dptr(c2), dptr(f2), dptr(p3), dptr(mask, torch.bool), stream()), "nm_assemble_matches")
    return c2, f2, p3, mask


FINE_LAYER_FUSED = True  # False: window gather + the generic layer kernels (A/B runs, tests)
FINE_STAGE_ONE_LAUNCH = True  # False: point side (nm_fine_pt_proj) and image side (nm_fine_window_layer) as two launches (A/B runs)


def fine_window_layer_supported(block, win_sz, C):
    """nm_fine_window_layer takes ONE pre-norm self-attention layer of width 128 with 8 heads of 16, bias-free attention projections, a
    GELU feed-forward 128 -> 128 -> 128 with biases, 5 x 5 windows (the shipped c2f configuration), split-bf16 arithmetic."""
    if not FINE_LAYER_FUSED or LINEAR_PRECISION != "bf16x3" or win_sz != 5 or C != 128:
        return False
    ok = block.__dict__.get("_nm_fwl_shape_ok")  # (the module's structure does not change after construction: examined once)
    if ok is None:
        ok = block.__dict__["_nm_fwl_shape_ok"] = _fine_window_layer_shape_ok(block)
    return ok


def _fine_window_layer_shape_ok(block):
    from .modules.attention import GenericEncoderLayer

    if len(block.layers) != 1:
        return False
    l = block.layers[0]
    if not isinstance(l, GenericEncoderLayer) or l.norm_type != "pre" or l.att_mode != "self":
        return False
    at, ff = l.attention, l.feedforward
    lin = (at.proj_q, at.proj_k, at.proj_v, at.proj_out[0])
    return (at.att_type == "full" and at.head_num == 8 and at.head_dim == 16 and all(m.bias is None and tuple(m.weight.shape) == (128, 128) for m in lin)
            and ff.act == _lib.NM_ACT_GELU and all(tuple(ff.layers[i].weight.shape) == (128, 128) and ff.layers[i].bias is not None for i in (0, 2))
            and tuple(l.norm1[0].weight.shape) == (128,) and tuple(l.norm2.weight.shape) == (128,))


def fine_window_layer(ffeat, map_ids, i_ids, count, block, stride=4, pt_f=None, pt_proj=None):
    """(K, 25, 128): the matches' 5 x 5 windows of `ffeat` through the block's one encoder layer, in one launch (nm_fine_window_layer).
    With pt_f (K, 128), the point-side fine features: returns FineMatching's expectation (K, 3) instead -- the layer's output is consumed
    inside the kernel and never stored.  With pt_proj = (src (rows, C0), ids (K,), lin0, lin1) the point side is computed inside too
    (nm_fine_stage: the whole fine stage in one launch)."""
    B, C, Hf, Wf = ffeat.shape
    K = i_ids.shape[0]
    want_expec = pt_f is not None or pt_proj is not None
    out = None if want_expec else torch.empty(K, 25, C, device=ffeat.device, dtype=torch.float32)
    expec = torch.empty(K, 3, device=ffeat.device, dtype=torch.float32) if want_expec else None
    if pt_f is not None:
        pt_f = pt_f.contiguous()
    p_src = p_ids = p_w0 = p_b0 = p_w1 = p_b1 = None
    p_c0 = 0
    if pt_proj is not None:
        p_src, p_ids, lin0, lin1 = pt_proj
        p_src, p_ids = p_src.contiguous(), p_ids.contiguous()
        p_c0 = p_src.shape[1]
        p_w0, p_w1 = transposed(lin0.weight), transposed(lin1.weight)
        p_b0 = None if lin0.bias is None else lin0.bias.detach()
        p_b1 = None if lin1.bias is None else lin1.bias.detach()
    if K:
        l = block.layers[0]
        at, ff, n1, n2 = l.attention, l.feedforward, l.norm1[0], l.norm2
        ffeat, map_ids, i_ids = ffeat.contiguous(), map_ids.contiguous(), i_ids.contiguous()
        ws = (at.proj_q.weight, at.proj_k.weight, at.proj_v.weight, at.proj_out[0].weight, ff.layers[0].weight, ff.layers[2].weight)
        # the six packed matrices, looked up once per parameter state (this sits between two launches of the one-query step's tail)
        vkey = (ws[0]._version, ws[1]._version, ws[2]._version, ws[3]._version, ws[4]._version, ws[5]._version, ws[0].data_ptr(), ws[5].data_ptr())
        hit = block.__dict__.get("_nm_fwl_blobs")
        # (an eviction -- invalidate_caches() after a write through .data, or the generation limit -- drops the entries: packed again then)
        if hit is None or hit[0] != vkey or any(_LINEAR_BLOBS.get(k) is None for k in hit[2]):
            blobs = [_linear_blob_perm(w) for w in ws]
            keys = [("perm", w.data_ptr(), w._version, tuple(w.shape), w.device.index) for w in ws]
            hit = block.__dict__["_nm_fwl_blobs"] = (vkey, blobs, keys)
        blobs = hit[1]
        b1, b2 = ff.layers[0].bias.detach(), ff.layers[2].bias.detach()
        u8 = torch.uint8
        check(lib().nm_fine_stage(dptr(ffeat), B, C, Hf, Wf, dptr(map_ids, torch.int64), dptr(i_ids, torch.int64), dptr(count, torch.int32), K, 5,
                                  int(stride), 8, dptr(n1.weight), dptr(n1.bias), float(n1.eps), dptr(blobs[0], u8), dptr(blobs[1], u8),
                                  dptr(blobs[2], u8), dptr(blobs[3], u8), dptr(n2.weight), dptr(n2.bias), float(n2.eps), dptr(blobs[4], u8), dptr(b1),
                                  dptr(blobs[5], u8), dptr(b2), float(at.attend.scale()), dptr(out), dptr(pt_f), dptr(p_src), dptr(p_ids, torch.int64),
                                  int(p_c0), dptr(p_w0), dptr(p_b0), dptr(p_w1), dptr(p_b1), dptr(expec), stream()), "nm_fine_stage")
    return expec if want_expec else out


FINE_PT_PROJ_FUSED = True  # False: gather + two nm_linear launches (A/B runs, tests)


def fine_pt_proj_supported(lin0, lin1):
    return (FINE_PT_PROJ_FUSED and lin1.out_features == 128 and lin1.in_features == 128 and lin0.out_features == 128
            and lin0.in_features % 4 == 0 and lin0.in_features <= 512)


def fine_pt_proj(src, ids, count, lin0, lin1):
    """out (K, 128) = lin1(lin0(src[ids])) for the first `count` slots (zeros behind them) in one launch (nm_fine_pt_proj): the point side
    of the fine stage, `pt_ffeat_proj`.  lin0 / lin1: the two nn.Linear modules; their transposed weights are cached (ops.transposed)."""
    K, dev = ids.shape[0], src.device
    out = torch.empty(K, 128, device=dev, dtype=torch.float32)
    if K:
        src, ids = src.contiguous(), ids.contiguous()
        w0t, w1t = transposed(lin0.weight), transposed(lin1.weight)
        b0 = None if lin0.bias is None else lin0.bias.detach()
        b1 = None if lin1.bias is None else lin1.bias.detach()
        check(lib().nm_fine_pt_proj(dptr(src), dptr(ids, torch.int64), dptr(count, torch.int32), K, src.shape[1], 128, dptr(w0t), dptr(b0), dptr(w1t),
                                    dptr(b1), dptr(out), stream()), "nm_fine_pt_proj")
    return out


def gather_rows(src, ids, count):
    """out[k] = src[ids[k]] for the slots k < count (a device int32); slots k >= count are NOT written: they hold whatever the fresh buffer held."""
    K, dim = ids.shape[0], src.shape[1]
    out = torch.empty(K, dim, device=src.device, dtype=torch.float32)
    if K:
        check(lib().nm_gather_rows(dptr(src), dptr(ids, torch.int64), dptr(count, torch.int32), K, dim, dptr(out), stream()), "nm_gather_rows")
    return out


def fine_expectation(pt_f, win_f, count, win=5):
    K, ww, Cc = win_f.shape
    out = torch.empty(K, 3, device=pt_f.device, dtype=torch.float32)
    if K:
        check(lib().nm_fine_expectation(dptr(pt_f), dptr(win_f), dptr(count, torch.int32), K, int(win), Cc, dptr(out), stream()), "nm_fine_expectation")
    return out


# ----------------------------------------------------------------------------- training side
_WGRAD_WS = {}


def _aligned16(t):
    """t, or a copy of it when its first element does not sit on a 16-byte boundary (a contiguous view at an odd offset into its storage)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def linear_wgrad(dy, x, out=None):
    """dw (N,K) = dy(M,N)^T @ x(M,K)  (added onto `out` when given)."""
    dy, x = _aligned16(dy.contiguous()), _aligned16(x.contiguous())
    M, N = dy.shape
    K = x.shape[1]
    dw = out if out is not None else torch.empty(N, K, device=dy.device, dtype=torch.float32)
    if M == 0:
        return dw if out is not None else dw.zero_()
    need = lib().nm_linear_wgrad_workspace_bytes(M, N, K)
    ws = _scratch(_WGRAD_WS, dy.device, need)
    if LINEAR_PRECISION == "bf16x3" and N % 2 == 0 and K % 4 == 0:  # (the arithmetic of the dX GEMMs of the same backward pass; round 6: 3 x faster than the fp32-MFMA kernel)
        check(lib().nm_linear_wgrad_bf16x3(dptr(dy), dptr(x), M, N, K, int(out is not None), dptr(dw), None, dptr(ws, torch.uint8), ws.numel(), stream()),
              "nm_linear_wgrad_bf16x3")
        return dw
    if N % 4 or K % 4:
        raise _lib.NerfmatchAmdError("linear_wgrad (fp32 kernel): N and K must be multiples of 4")
    check(lib().nm_linear_wgrad(dptr(dy), dptr(x), M, N, K, int(out is not None), dptr(dw), dptr(ws, torch.uint8), ws.numel(), stream()),
          "nm_linear_wgrad")
    return dw


def linear_wgrad_bias(dy, x, out=None):
    """(dw, db) = (dy^T @ x, column sums of dy): one launch on the split-bf16 path (dy read once), two otherwise.  out = (dw, db): both are
    added onto (the chunks of a NeRF training step)."""
    dy, x = _aligned16(dy.contiguous()), _aligned16(x.contiguous())
    M, N = dy.shape
    K = x.shape[1]
    if not (LINEAR_PRECISION == "bf16x3" and N % 2 == 0 and K % 4 == 0 and M > 0):
        if out is None:
            return linear_wgrad(dy, x), col_sum(dy)
        return linear_wgrad(dy, x, out=out[0]), col_sum(dy, out=out[1])
    acc = out is not None
    dw = out[0] if acc else torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = out[1] if acc else torch.empty(N, device=dy.device, dtype=torch.float32)
    ws = _scratch(_WGRAD_WS, dy.device, lib().nm_linear_wgrad_workspace_bytes(M, N, K))
    check(lib().nm_linear_wgrad_bf16x3(dptr(dy), dptr(x), M, N, K, int(acc), dptr(dw), dptr(db), dptr(ws, torch.uint8), ws.numel(), stream()),
          "nm_linear_wgrad_bf16x3")
    return dw, db


_COLSUM_WS = {}
_LN_BWD_WS = {}


def col_sum(dy, out=None):
    """column sums of dy (M, N) (added onto `out` when given)."""
    dy = dy.contiguous()
    M, N = dy.shape
    if out is None:
        out = torch.zeros(N, device=dy.device, dtype=torch.float32)
    if M:  # (the ordered form: partial sums added in a fixed order -- the same bits on every run)
        ws = _scratch(_COLSUM_WS, dy.device, lib().nm_col_sum_workspace_bytes(M, N))
        check(lib().nm_col_sum_ordered(dptr(dy), M, N, 1, dptr(out), dptr(ws, torch.uint8), ws.numel(), stream()), "nm_col_sum_ordered")
    return out


def gelu(u):
    u = u.contiguous()
    h = torch.empty_like(u)
    if u.numel():
        check(lib().nm_gelu(dptr(u), u.numel(), dptr(h), stream()), "nm_gelu")
    return h


def gelu_bwd(u, dh):
    u, dh = u.contiguous(), dh.contiguous()
    du = torch.empty_like(u)
    if u.numel():
        check(lib().nm_gelu_bwd(dptr(u), dptr(dh), u.numel(), dptr(du), stream()), "nm_gelu_bwd")
    return du


def relu_bwd(h, dh):
    """dh where the ReLU's output h is positive, else 0."""
    h, dh = h.contiguous(), dh.contiguous()
    du = torch.empty_like(h)
    if h.numel():
        check(lib().nm_relu_bwd(dptr(h), dptr(dh), h.numel(), dptr(du), stream()), "nm_relu_bwd")
    return du


def layernorm_bwd(x, gamma, dy, eps=1e-5, param_grads=True):
    """-> dx (like x), dgamma (dim), dbeta (dim); param_grads=False: (dx, None, None) -- no parameter-gradient reduction, no zero fills."""
    dim = x.shape[-1]
    x2, dy2 = x.reshape(-1, dim).contiguous(), dy.reshape(-1, dim).contiguous()
    dx = torch.empty_like(x2)
    dg = db = None
    if param_grads:
        dg_db = torch.zeros(2, dim, device=x.device, dtype=torch.float32)  # (one fill launch for both)
        dg, db = dg_db[0], dg_db[1]
    if x2.shape[0] and param_grads:  # (the ordered form: dgamma / dbeta summed in a fixed order -- the same bits on every run)
        ws = _scratch(_LN_BWD_WS, x.device, lib().nm_layernorm_bwd_workspace_bytes(x2.shape[0], dim))
        check(lib().nm_layernorm_bwd_ordered(dptr(x2), dptr(gamma), dptr(dy2), x2.shape[0], dim, float(eps), dptr(dx), dptr(dg), dptr(db),
                                             dptr(ws, torch.uint8), ws.numel(), stream()), "nm_layernorm_bwd_ordered")
    elif x2.shape[0]:
        check(lib().nm_layernorm_bwd(dptr(x2), dptr(gamma), dptr(dy2), x2.shape[0], dim, float(eps), dptr(dx), None, None, stream()),
              "nm_layernorm_bwd")
    return dx.reshape(x.shape), dg, db


def l2norm_bwd(f, dy):
    f, dy = f.contiguous(), dy.contiguous()
    df = torch.empty_like(f)
    if f.shape[0]:
        check(lib().nm_l2norm_bwd(dptr(f), dptr(dy), f.shape[0], f.shape[1], dptr(df), stream()), "nm_l2norm_bwd")
    return df


_ATTN_BWD_WS = {}


def attention_bwd_fused(q_src, q_col, kv_src, k_col, v_col, o, d_o, B, L, S, heads, scale, nlse=None):
    """Backward of attention_fused: q / k / v are column slices (offsets in floats) of the fused projection buffers q_src
    (B*L, ldq) and kv_src (B*S, ldkv).  Returns (d_q_src, d_kv_src) of the same shapes with the three slices filled (other
    columns zero); d_kv_src is d_q_src when both are the same buffer (self attention)."""
    dim = o.shape[-1]
    o2, d2 = o.reshape(B * L, dim).contiguous(), d_o.reshape(B * L, dim).contiguous()
    same = kv_src is q_src
    # (every column is written when the buffers hold exactly the slices: [q | k | v], or q alone beside [k | v]: no zero fill then)
    dq_src = torch.empty_like(q_src) if q_src.shape[1] == (3 * dim if same else dim) else torch.zeros_like(q_src)
    dkv_src = dq_src if same else (torch.empty_like(kv_src) if kv_src.shape[1] == 2 * dim else torch.zeros_like(kv_src))
    if B * L == 0 or S == 0:
        return dq_src.zero_(), dkv_src.zero_()
    flags = _attn_flags() if dim // heads == 32 else 0
    need = lib().nm_attention_bwd_workspace_bytes(B, L, S, int(heads), flags)
    ws = _scratch(_ATTN_BWD_WS, q_src.device, need)
    ldq, ldkv = q_src.shape[1], kv_src.shape[1]
    off = lambda t, c: C.c_void_p(t.data_ptr() + 4 * c)
    if nlse is not None and not (flags & _lib.NM_ATTN_BF16X3):
        nlse = None  # (the precision switch moved between forward and backward: the fp32 kernels rebuild the log-sum-exp themselves)
    check(lib().nm_attention_bwd(off(q_src, q_col), off(kv_src, k_col), off(kv_src, v_col), dptr(o2), dptr(d2), ldq, ldkv, ldkv, dim, dim,
                                 B, L, S, int(heads), dim // heads, float(scale), off(dq_src, q_col), off(dkv_src, k_col),
                                 off(dkv_src, v_col), ldq, ldkv, ldkv, flags, dptr(nlse), dptr(ws, torch.uint8), ws.numel(), stream()),
          "nm_attention_bwd")
    return dq_src, dkv_src


def attention_bwd(q, k, v, o, d_o, heads, scale):
    """Gradients of softmax attention: q, o, d_o (B,L,C); k, v (B,S,C) -> dq, dk, dv (arithmetic per ATTENTION_PRECISION)."""
    q, k, v, o, d_o = (t.contiguous() for t in (q, k, v, o, d_o))
    B, L, Cc = q.shape
    S = k.shape[1]
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if B * L == 0 or S == 0:
        return dq.zero_(), dk.zero_(), dv.zero_()
    flags = _attn_flags() if Cc // heads == 32 else 0
    need = lib().nm_attention_bwd_workspace_bytes(B, L, S, int(heads), flags)
    ws = _scratch(_ATTN_BWD_WS, q.device, need)
    check(lib().nm_attention_bwd(dptr(q), dptr(k), dptr(v), dptr(o), dptr(d_o), Cc, Cc, Cc, Cc, Cc, B, L, S, int(heads), Cc // heads,
                                 float(scale), dptr(dq), dptr(dk), dptr(dv), Cc, Cc, Cc, flags, None, dptr(ws, torch.uint8), ws.numel(), stream()),
          "nm_attention_bwd")
    return dq, dk, dv


def fine_windows_bwd(dwin, shape_chw, i_ids, count, win=5, stride=4, out=None):
    """Scatter-add of window gradients (K, win*win, C) into a (C,Hf,Wf) map (`out` accumulated onto when given)."""
    Cc, Hf, Wf = shape_chw
    K = i_ids.shape[0]
    d = out if out is not None else torch.zeros(Cc, Hf, Wf, device=dwin.device, dtype=torch.float32)
    if K:
        dwin = dwin.contiguous()
        check(lib().nm_fine_windows_bwd(dptr(dwin), Cc, Hf, Wf, dptr(i_ids, torch.int64), dptr(count, torch.int32), K, int(win),
                                        int(stride), dptr(d), stream()), "nm_fine_windows_bwd")
    return d


def fine_expectation_bwd(pt_f, win_f, d_expec, count, win=5):
    K, ww, Cc = win_f.shape
    d_pt, d_win = torch.empty_like(pt_f), torch.empty_like(win_f)
    if K:
        d_expec = d_expec.contiguous()
        check(lib().nm_fine_expectation_bwd(dptr(pt_f), dptr(win_f), dptr(d_expec), dptr(count, torch.int32), K, int(win), Cc,
                                            dptr(d_pt), dptr(d_win), stream()), "nm_fine_expectation_bwd")
    return d_pt, d_win


# ----------------------------------------------------------------------------- ground-truth supervision (supervision.hip)
_SUPERVISION_WS = {}


def gt_supervision(pt3d, K, w2c, pt_mask=None, im_mask=None, fallback=None, hw=None, ds=8, M=None, dense=True, triple=True):
    """nm_gt_supervision: pt3d (B,N,3), K (B,3,3), w2c (B,3,4), masks (B,N) / (B,M) or None, fallback (B,2) int32 or None.
    hw=None: projection only -> pt2d_proj (B,N,2).  Otherwise -> dict(pt2d_proj, gt_cell (B,N) int32, conf_gt (B,M,N) uint8 | None,
    ids = (b_ids, i_ids, j_ids) int64 at capacity B*N and counts (B,) int32 | None): the caller trims the triple to counts.sum()."""
    B, N = pt3d.shape[:2]
    dev = pt3d.device
    proj = torch.empty(B, N, 2, device=dev, dtype=torch.float32)
    if B * N == 0:
        raise _lib.NerfmatchAmdError("gt_supervision: empty point set")
    if hw is None:
        check(lib().nm_gt_supervision(dptr(pt3d), dptr(K), dptr(w2c), None, None, None, B, 0, N, 0, 0, 0, dptr(proj), None, None, None, None, None,
                                      None, None, 0, stream()), "nm_gt_supervision")
        return proj
    H, W = int(hw[0]), int(hw[1])
    M = (H // ds) * (W // ds) if M is None else int(M)
    cell = torch.empty(B, N, device=dev, dtype=torch.int32)
    conf = torch.empty(B, M, N, device=dev, dtype=torch.uint8) if dense else None
    ids = [torch.empty(B * N, device=dev, dtype=torch.int64) for _ in range(3)] if triple else [None] * 3
    counts = torch.empty(B, device=dev, dtype=torch.int32) if triple else None
    ws, need = None, 0
    if triple:
        need = lib().nm_gt_supervision_workspace_bytes(B, M, N)
        ws = _scratch(_SUPERVISION_WS, dev, need)
    check(lib().nm_gt_supervision(dptr(pt3d), dptr(K), dptr(w2c), dptr(_mask_u8(pt_mask), torch.uint8), dptr(_mask_u8(im_mask), torch.uint8),
                                  dptr(fallback, torch.int32), B, M, N, H, W, int(ds), dptr(proj), dptr(cell, torch.int32),
                                  dptr(conf, torch.uint8), dptr(ids[0], torch.int64), dptr(ids[1], torch.int64), dptr(ids[2], torch.int64),
                                  dptr(counts, torch.int32), dptr(ws, torch.uint8), need, stream()), "nm_gt_supervision")
    return dict(pt2d_proj=proj, gt_cell=cell, conf_gt=conf, ids=tuple(ids) if triple else None, counts=counts)


# ----------------------------------------------------------------------------- batched PnP-RANSAC (pnp.hip)
_PNP_WS = {}


def pnp_ransac(pt2d, pt3d, offsets, K, thr_px=1.0, n_hyps=1024, refine_iters=10, seed=0, add_half_px=False, want_inliers=False, study=False,
               offsets_host=None):
    """nm_pnp_ransac: pt2d (K,2), pt3d (K,3), offsets (Q+1,) int32 device, K (Q,3,3) -> pose (Q,12) fp32 [R|t] w2c, n_inliers (Q,) int32,
    inlier_mask (K,) uint8 | None, and with study=True (hyp_pose (Q,n_hyps,12), hyp_count (Q,n_hyps)) else None.  offsets_host: the same
    offsets as a list of Python ints (validated on the host before the launch) or None."""
    Q, n = K.shape[0], pt2d.shape[0]
    dev = K.device
    pose = torch.empty(Q, 12, device=dev, dtype=torch.float32)
    n_inl = torch.empty(Q, device=dev, dtype=torch.int32)
    mask = torch.empty(n, device=dev, dtype=torch.uint8) if want_inliers else None
    hyp = (torch.empty(Q, n_hyps, 12, device=dev, dtype=torch.float32), torch.empty(Q, n_hyps, device=dev, dtype=torch.int32)) if study else None
    need = lib().nm_pnp_ransac_workspace_bytes(Q, int(n_hyps))
    ws = _scratch(_PNP_WS, dev, need)
    oh = None if offsets_host is None else (C.c_int * (Q + 1))(*[int(v) for v in offsets_host])
    check(lib().nm_pnp_ransac(dptr(pt2d if n else None), dptr(pt3d if n else None), dptr(offsets, torch.int32), oh, dptr(K), Q, n, float(thr_px),
                              int(n_hyps), int(refine_iters), int(seed) & 0xFFFFFFFF, int(bool(add_half_px)), dptr(pose), dptr(n_inl, torch.int32),
                              dptr(mask, torch.uint8), dptr(hyp[0] if study else None), dptr(hyp[1] if study else None, torch.int32),
                              dptr(ws, torch.uint8), need, stream()), "nm_pnp_ransac")
    return pose, n_inl, mask, hyp
