"""Query and training images from decoded uint8 frames: Pillow-exact Lanczos resize, normalisation and white-background blending.

Every image of the reference passes `process_img` first (the matcher's query: nerfmatch/datasets/nerfmatch_dataset.py:36-61; a NeRF frame
and its background / transient masks: nerfmatch/datasets/nerfbase.py:197-237): `PIL.Image.resize(img_wh, Image.LANCZOS)` on an 8-bit image
and a few lines of arithmetic -- `/ 255`, optional ImageNet mean / std, `h w c -> c h w`, `img * (1 - round(m)) + round(m)`.  Here the
decoded frames are resized where they are used:

    image, sK = query_images(images_u8.cuda(), (480, 480), imagenet_norm=False)           # (F,3,h,w) float32, (3,3)
    fr = nerf_frames(images_u8.cuda(), (480, 480), bg_masks_u8=bg, trnz_masks_u8=trnz)     # uint8, ready for RayBank
    bank = RayBank(fr["images_u8"], c2w, fr["sK"] @ K, masks_u8=fr["masks_u8"])

Tensors on a GPU take the HIP kernel (csrc/image_prep.hip; no fallback).  Tensors on the host take `_resize_torch`, the same integer
arithmetic in torch ops on the same tables: the path of CPU-only users and the statement the kernel is tested against.  Both return
Pillow's bytes (tests/golden/image_prep.npz), so the comparisons are `torch.equal`.

The arithmetic is Pillow's Resample.c for 8 bits per channel, `reducing_gap=None`.  One axis, `in` -> `out` pixels, in float64:
    scale = in / out, fs = max(scale, 1), support = 3 fs, ksize = ceil(support) * 2 + 1; for output xx:
    center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), in) - xmin,
    w[x] = L((x + xmin - center + 0.5) * (1 / fs)) for x < n, L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3 (0 elsewhere),
    sinc(0) = 1, sinc(t) = sin(pi t) / (pi t); ww = sum of w in index order, w /= ww unless ww == 0;
    k[x] = int(w 2^22 - 0.5) for negative w, int(w 2^22 + 0.5) otherwise (int() truncates);
    pixel = clip((2^21 + sum_x k[x] src[xmin + x]) >> 22, 0, 255) in int32 with an arithmetic shift.
The horizontal pass runs first and is rounded and clipped to uint8; the vertical pass filters those bytes.  An axis that keeps its size
is not filtered.  (Pillow multiplies by the reciprocal 1 / fs where one might divide by fs; the tables follow Pillow.)

Envelope (ValueError beyond, before anything is launched): uint8 input, C in {1, 3}, every side <= 8192, a reduction of at most 8 x per
axis (ksize <= 51), any enlargement.  Decoding image files, `convert("L")` and annotation parsing stay with the caller."""
import functools
import math

import numpy as np
import torch

TILE_WH = (64, 32)   # output pixels per workgroup: NM_IMAGE_TILE_W, NM_IMAGE_TILE_H of include/nerfmatch_amd.h
MAX_SIDE = 8192
MAX_REDUCTION = 8    # per axis
MAX_KSIZE = 51       # the stated limit; 8 x gives ceil(3 * 8) * 2 + 1 = 49
PRECISION_BITS = 22  # Pillow: 32 - 8 - 2
IMAGENET_MEAN = (0.485, 0.456, 0.406)  # nerfmatch_dataset.py:53-54
IMAGENET_STD = (0.229, 0.224, 0.225)


# ----------------------------------------------------------------------------- tables
def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _lanczos3(t):
    if -3.0 <= t < 3.0:
        return _sinc(t) * _sinc(t / 3)
    return 0.0


@functools.lru_cache(maxsize=256)
def _tables(in_size, out_size):
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    coef = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos3((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        coef[xx, :n] = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]
        bounds[xx] = (xmin, n)
    return torch.from_numpy(coef), torch.from_numpy(bounds)


def _check_axis(name, in_size, out_size):
    if not 1 <= in_size <= MAX_SIDE or not 1 <= out_size <= MAX_SIDE:
        raise ValueError(f"{name} {in_size} -> {out_size}: every side must lie in [1, {MAX_SIDE}]")
    if in_size > MAX_REDUCTION * out_size:
        raise ValueError(f"{name} {in_size} -> {out_size}: a reduction of at most {MAX_REDUCTION} x per axis (ksize <= {MAX_KSIZE}) is supported")


def lanczos_tables(in_size, out_size):
    """The tables of one axis `in_size` -> `out_size`: (coef int32 (out, ksize), bounds int32 (out, 2) = (xmin, n)) as host tensors.
    Computed once per pair in float64 with math.sin (the C library's), cached and shared: do not write into them."""
    in_size, out_size = int(in_size), int(out_size)
    _check_axis("axis", in_size, out_size)
    return _tables(in_size, out_size)


@functools.lru_cache(maxsize=64)
def _device_tables(in_size, out_size, device, tap_major):
    coef, bounds = lanczos_tables(in_size, out_size)
    if tap_major:  # the horizontal pass reads tap x of 64 neighbouring columns at once
        coef = coef.t()
    return coef.contiguous().to(device), bounds.contiguous().to(device)


@functools.lru_cache(maxsize=8)
def _lut_np(channels, imagenet_norm):
    """(C,256) float32: what the reference computes for byte v of channel c -- `np.array(img) / 255.0`, then `img - mean` and `/ std` in
    float64 (nerfmatch_dataset.py:49-56), then `.float()`."""
    lut = np.repeat((np.arange(256, dtype=np.uint8) / 255.0)[None], channels, 0)
    if imagenet_norm:
        lut = lut - np.array(IMAGENET_MEAN)[:, None]
        lut = lut / np.array(IMAGENET_STD)[:, None]
    return lut.astype(np.float32)


@functools.lru_cache(maxsize=16)
def _device_lut(channels, imagenet_norm, device):
    return torch.from_numpy(_lut_np(channels, imagenet_norm)).to(device)


# ----------------------------------------------------------------------------- the arithmetic in plain torch
def _pass_torch(x, dim, in_size, out_size):
    """One pass along `dim` of an int32 tensor of bytes: int32 accumulation (as in Pillow), arithmetic shift, clip."""
    coef, bounds = lanczos_tables(in_size, out_size)
    ksize = coef.shape[1]
    shape = [1] * x.dim()
    shape[dim] = out_size
    acc = torch.full([out_size if d == dim else s for d, s in enumerate(x.shape)], 1 << (PRECISION_BITS - 1), dtype=torch.int32)
    for t in range(ksize):  # taps past a window's n have coefficient 0; their index is clamped into the axis
        idx = (bounds[:, 0].to(torch.int64) + t).clamp_(max=in_size - 1)
        acc += coef[:, t].reshape(shape) * x.index_select(dim, idx)
    return (acc >> PRECISION_BITS).clamp_(0, 255)


def _resize_torch(images, wh):
    """(F,H,W,C) uint8 host tensor -> (F,h,w,C) uint8: horizontal pass, uint8 intermediate, vertical pass; an unchanged axis is skipped."""
    w, h = wh
    x = images.to(torch.int32)
    if images.shape[2] != w:
        x = _pass_torch(x, 2, images.shape[2], w)
    if images.shape[1] != h:
        x = _pass_torch(x, 1, images.shape[1], h)
    return x.to(torch.uint8)


# ----------------------------------------------------------------------------- the public functions
def _check_images(images_u8, wh, channels=(1, 3)):
    images_u8 = torch.as_tensor(images_u8)
    if images_u8.dtype != torch.uint8:
        raise ValueError(f"images must be uint8, got {images_u8.dtype}")
    squeeze = images_u8.dim() == 3
    if squeeze:
        images_u8 = images_u8[..., None]
    if images_u8.dim() != 4 or images_u8.shape[0] < 1:
        raise ValueError("images must be (F,H,W,C) or (F,H,W) with F >= 1")
    F, H, W, C = images_u8.shape
    if C not in channels:
        raise ValueError(f"C = {C} channels: C must be in {set(channels)}")
    w, h = int(wh[0]), int(wh[1])
    _check_axis("width", W, w)
    _check_axis("height", H, h)
    return images_u8, (w, h), squeeze


def _check_white(white_where, F, wh):
    if white_where is None:
        return None
    white_where = torch.as_tensor(white_where)
    if white_where.dtype != torch.uint8 or tuple(white_where.shape) != (F, wh[1], wh[0]):
        raise ValueError(f"white_where must be a (F,h,w) = ({F},{wh[1]},{wh[0]}) uint8 tensor at the OUTPUT resolution, "
                         f"got {white_where.dtype} {tuple(white_where.shape)}")
    return white_where


def _resize(images_u8, wh, white_where, lut_key=None, want_u8=True):
    """The shared body: checked arguments -> (uint8 (F,h,w,C) or None, float32 (F,C,h,w) or None) on the images' device."""
    F, H, W, C = images_u8.shape
    w, h = wh
    dev = images_u8.device
    if dev.type == "cpu":
        out = _resize_torch(images_u8, wh)
        if white_where is not None:
            out = torch.where(white_where.to("cpu")[..., None] >= 128, torch.full_like(out, 255), out)
        out_f = None
        if lut_key is not None:
            lut = torch.from_numpy(_lut_np(*lut_key))
            out_f = torch.stack([lut[c][out[..., c].to(torch.int64)] for c in range(C)], 1)
        return (out if want_u8 else None), out_f
    from . import ops

    src = images_u8.contiguous()  # a strided view is copied, never read with wrong strides
    if src.data_ptr() % 16:       # (a view that starts inside an allocation)
        src = src.clone()
    if F > 65535:
        raise ValueError(f"{F} frames in one call: at most 65535")
    tx = None if W == w else _device_tables(W, w, dev, True)
    ty = None if H == h else _device_tables(H, h, dev, False)
    lut = None if lut_key is None else _device_lut(*lut_key, dev)
    if white_where is not None:
        white_where = white_where.to(dev).contiguous()
    return ops.image_resize_u8(src, wh, tx, ty, white_where=white_where, lut=lut, want_u8=want_u8)


def resize_lanczos_u8(images_u8, wh, white_where=None):
    """images_u8 (F,H,W,C) or (F,H,W) uint8, on a GPU or on the host -> the bytes of `Image.resize(wh, Image.LANCZOS)` of every frame,
    (F,h,w,C) or (F,h,w), on the same device; wh = (w, h).  white_where (F,h,w) uint8 at the output resolution: where it is >= 128 the
    pixel becomes 255 in every channel."""
    images_u8, wh, squeeze = _check_images(images_u8, wh)
    white_where = _check_white(white_where, images_u8.shape[0], wh)
    out, _ = _resize(images_u8, wh, white_where)
    return out[..., 0] if squeeze else out


def scale_intrinsics(src_wh, wh):
    """sK = diag(w / W, h / H, 1) as float32 (3,3): float64 quotients, then `.float()` (nerfmatch_dataset.py:41-43)."""
    return torch.from_numpy(np.diag([wh[0] / src_wh[0], wh[1] / src_wh[1], 1])).float()


def query_images(images_u8, wh, imagenet_norm=False):
    """The reference's process_img for a batch of one source size: images_u8 (F,H,W,3) uint8 -> (image float32 (F,3,h,w), sK float32
    (3,3)).  The float values go through a (3,256) table built as the reference computes them (float64 `/ 255.0`, mean / std, then
    float32), so they equal its `torch.tensor(img).float()` bit for bit."""
    images_u8, wh, _ = _check_images(images_u8, wh, channels=(3,))
    _, image = _resize(images_u8, wh, None, lut_key=(3, bool(imagenet_norm)), want_u8=False)
    return image, scale_intrinsics((images_u8.shape[2], images_u8.shape[1]), wh)


def nerf_frames(images_u8, wh, bg_masks_u8=None, trnz_masks_u8=None):
    """NeRF training / validation frames (nerfbase.py:197-237): images_u8 (F,H,W,3) and single-channel masks (F,H,W) uint8 as decoded
    -> dict(images_u8 (F,h,w,3), masks_u8 (F,h,w) or None, sK), ready for RayBank(images_u8=..., masks_u8=...).
    bg_masks_u8 is resized and the image becomes white where the resized mask is >= 128: the reference's
    `img * (1 - round(m)) + round(m)` on m = byte / 255, in bytes (no byte gives exactly 0.5, so round's half-to-even never applies).
    trnz_masks_u8 is resized and returned; RayBank applies `1 - round(mask / 255)`."""
    images_u8, wh, _ = _check_images(images_u8, wh, channels=(3,))
    F, H, W, _ = images_u8.shape

    def mask(m, name):
        m = torch.as_tensor(m)
        if m.dtype != torch.uint8 or tuple(m.shape) != (F, H, W):
            raise ValueError(f"{name} must be a (F,H,W) = ({F},{H},{W}) uint8 tensor, got {m.dtype} {tuple(m.shape)}")
        return _resize(m.to(images_u8.device)[..., None], wh, None)[0][..., 0]

    white = None if bg_masks_u8 is None else mask(bg_masks_u8, "bg_masks_u8")
    out, _ = _resize(images_u8, wh, white)
    masks = None if trnz_masks_u8 is None else mask(trnz_masks_u8, "trnz_masks_u8")
    return dict(images_u8=out, masks_u8=masks, sK=scale_intrinsics((W, H), wh))


def prepare_query_batch(batch, img_wh, imagenet_norm=False):
    """A batch that carries decoded queries `image_u8` (Q,H,W,3) uint8 and no `image` gets `image` = query_images(image_u8) and
    `K` = sK @ K (nerfmatch_dataset.py:267-268); `image_u8` stays.  Any other batch is returned as it is, the same object."""
    if "image_u8" not in batch or "image" in batch:
        return batch
    image, sK = query_images(batch["image_u8"], img_wh, imagenet_norm=imagenet_norm)
    batch["image"] = image
    if "K" in batch:
        K = torch.as_tensor(batch["K"]).to(torch.float32)
        batch["K"] = sK.to(K.device) @ K
    return batch
