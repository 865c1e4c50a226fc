"""Shared by test_image_prep_cpu.py / test_image_prep_gpu.py and tests/golden/make_golden_image_prep.py: Pillow's 8-bit Lanczos
resampler restated in plain numpy, independent of the package, the cases of tests/golden/image_prep.npz and seeded sources.

The restatement (Pillow's Resample.c, 8 bits per channel, reducing_gap=None).  One axis, `in` -> `out` pixels, float64:
    scale = in / out, fs = max(scale, 1), support = 3 fs, ksize = ceil(support) * 2 + 1
    center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), in) - xmin
    w[x] = L((x + xmin - center + 0.5) * (1 / fs)), L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3, sinc(t) = sin(pi t) / (pi t), sinc(0) = 1
    w /= sum(w) (summed in index order) unless the sum is 0; k[x] = int(w 2^22 -+ 0.5) (sign of w; truncation)
    pixel = clip((2^21 + sum k[x] src[xmin + x]) >> 22, 0, 255), int32, arithmetic shift
horizontal pass first, rounded and clipped to uint8, then the vertical pass; an axis that keeps its size is skipped."""
import math

import numpy as np

from conftest import GOLDEN

# (name, H, W, C, w, h, content): the cases of the fixture.  `wide` lies outside the package's envelope (200 -> 3 is a 66 x reduction):
# the fixture and the restatement cover it, the package must refuse it (test_image_prep_cpu.py states this); `wide8` is the same source
# at the envelope's edge, 200 -> 25.
CASES = (
    ("cambridge", 108, 192, 3, 48, 48, "noise"),   # 4 x and 2.25 x
    ("scenes7", 48, 64, 3, 48, 48, "noise"),       # vertical pass skipped
    ("tall", 64, 48, 3, 48, 48, "noise"),          # horizontal pass skipped
    ("odd", 37, 53, 3, 16, 8, "binary"),           # non-integer reductions, windows clipped at both borders
    ("enlarge", 24, 40, 1, 61, 47, "binary"),      # enlargement, ksize 7
    ("mixed", 9, 7, 3, 7, 13, "noise"),            # one axis enlarged, the other unchanged
    ("edge8", 40, 40, 3, 5, 5, "noise"),           # exactly 8 x
    ("wide", 5, 200, 3, 3, 5, "noise"),            # every window spans far more than a tile's share of the row
    ("wide8", 5, 200, 3, 25, 5, "binary"),
)
IN_ENVELOPE = tuple(c for c in CASES if c[0] != "wide")
FLOAT_CASES = tuple(c[0] for c in CASES if c[3] == 3 and c[0] != "wide")  # query_images takes three channels


def source(name, H, W, C, content, frames=1, seed=0):
    """Seeded uint8 frames (frames,H,W,C): uniform noise, or pure 0 / 255 (`binary`: the overshoot reaches the clip at both ends)."""
    g = np.random.default_rng([seed, sum(map(ord, name)), H, W, C])
    if content == "binary":
        return (g.integers(0, 2, size=(frames, H, W, C), dtype=np.uint8) * 255).astype(np.uint8)
    return g.integers(0, 256, size=(frames, H, W, C), dtype=np.uint8)


# ----------------------------------------------------------------------------- the restatement
def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _lanczos(t):
    return _sinc(t) * _sinc(t / 3) if -3.0 <= t < 3.0 else 0.0


def tables(in_size, out_size):
    """(coef int32 (out, ksize), bounds int32 (out, 2) = (xmin, n))"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    coef, bounds = np.zeros((out_size, ksize), np.int32), np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([_lanczos((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(n)], np.float64)
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = w / ww
        for x in range(n):
            v = w[x] * float(1 << 22)
            coef[xx, x] = int(v - 0.5) if w[x] < 0 else int(v + 0.5)
        bounds[xx] = (xmin, n)
    return coef, bounds


def _pass(img, axis, out_size, keep_wide=False):
    """img (..) integer array; filters `axis`.  keep_wide: no rounding, no clip -- the accumulator itself (for the study of the
    intermediate rounding below)."""
    coef, bounds = tables(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.zeros((out_size,) + src.shape[1:], np.int64)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        out[xx] = np.tensordot(coef[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
    if not keep_wide:
        out = ((out + (1 << 21)).astype(np.int32) >> 22).clip(0, 255)  # int32 accumulator (no case here wraps), arithmetic shift
    return np.moveaxis(out, 0, axis)


def resize_np(img, wh):
    """img (H,W,C) uint8 -> Pillow's Image.resize(wh, Image.LANCZOS) bytes, (h,w,C) uint8."""
    w, h = wh
    x = img
    if img.shape[1] != w:
        x = _pass(x, 1, w)
    if img.shape[0] != h:
        x = _pass(x, 0, h)
    return x.astype(np.uint8)


def resize_np_wide_intermediate(img, wh):
    """The same filter WITHOUT the uint8 intermediate: the horizontal accumulator (22 fractional bits) goes into the vertical pass
    unrounded and unclipped, one rounding at the end.  Not Pillow: it differs from it wherever the intermediate rounding matters."""
    w, h = wh
    assert img.shape[1] != w and img.shape[0] != h
    x = _pass(img, 1, w, keep_wide=True)          # value * 2^22
    y = _pass(x, 0, h, keep_wide=True)            # value * 2^44
    return ((y + (1 << 43)) >> 44).clip(0, 255).astype(np.uint8)


def lut_np(imagenet_norm):
    """(3,256) float32 of the reference's float64 arithmetic (nerfmatch_dataset.py:49-56)."""
    v = np.arange(256, dtype=np.uint8) / 255.0
    lut = np.repeat(v[None], 3, 0)
    if imagenet_norm:
        lut = (lut - np.array([0.485, 0.456, 0.406])[:, None]) / np.array([0.229, 0.224, 0.225])[:, None]
    return lut.astype(np.float32)


# ----------------------------------------------------------------------------- the fixture
_FX = {}


def fixture():
    """tests/golden/image_prep.npz as numpy arrays, loaded once per process (the tests only read it): per case `<name>_src` (H,W,C),
    `<name>_out` (h,w,C) = Pillow's bytes; per float case `<name>_f32` and `<name>_f32_norm` (3,h,w) and `<name>_sK` (3,3)."""
    if not _FX:
        z = np.load(GOLDEN / "image_prep.npz")
        _FX.update({k: np.asarray(z[k]) for k in z.files})
    return _FX
