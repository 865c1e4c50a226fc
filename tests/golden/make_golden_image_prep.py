#!/usr/bin/env python3
"""Golden vectors of the image preparation (tests/golden/image_prep.npz): Pillow's own `Image.resize(wh, Image.LANCZOS)` bytes and
the reference's float images for the cases of tests/image_prep_util.py.

    python tests/golden/make_golden_image_prep.py      # rewrites tests/golden/image_prep.npz (NM_GOLDEN_OUT=<dir>: elsewhere)

Needs Pillow, and the reference tree for the float outputs (make_golden.py's REF and stub modules): every float case is written to a PNG
file (lossless) in a temporary directory and read back through the reference's `process_img` (nerfmatch/datasets/nerfmatch_dataset.py:
36-61) with imagenet_norm False and True; its `sK` is stored too.  This file was generated that way: process_img imported (its einops
import is present here), so the three-line float64 fallback below (`/ 255.0`, `- mean`, `/ std`, `.float()`, the same lines of
process_img) was NOT used; it only runs -- and says so -- where the reference cannot be imported.  The uint8 sources are seeded noise and
0 / 255 images; only arrays are written, uint8 except the float outputs."""
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch
from PIL import Image

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import make_golden as mg  # noqa: E402
import image_prep_util as ipu  # noqa: E402


def pillow_resize(img, wh):
    pil = Image.fromarray(img[..., 0], "L") if img.shape[-1] == 1 else Image.fromarray(img, "RGB")
    out = np.asarray(pil.resize(wh, Image.LANCZOS))
    return out[..., None] if out.ndim == 2 else out


def reference_float(process_img, img, wh, norm, tmp):
    if process_img is None:
        x = np.array(Image.fromarray(img, "RGB").resize(wh, Image.LANCZOS)) / 255.0
        if norm:
            x = (x - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225])
        sK = torch.from_numpy(np.diag([wh[0] / img.shape[1], wh[1] / img.shape[0], 1])).float()
        return torch.tensor(x).permute(2, 0, 1).float().numpy(), sK.numpy()
    path = Path(tmp) / "frame.png"
    Image.fromarray(img, "RGB").save(path)
    x, sK = process_img(wh, path, imagenet_norm=norm)
    return x.numpy(), sK.numpy()


def main():
    try:
        mg.install_stubs()
        from nerfmatch.datasets.nerfmatch_dataset import process_img
        print("float outputs: the reference's process_img")
    except Exception as e:  # noqa: BLE001
        process_img = None
        print(f"float outputs: the float64 fallback ({type(e).__name__}: {e})")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, H, W, C, w, h, content in ipu.CASES:
            src = ipu.source(name, H, W, C, content)[0]
            res = pillow_resize(src, (w, h))
            assert res.shape == (h, w, C) and res.dtype == np.uint8
            assert np.array_equal(ipu.resize_np(src, (w, h)), res), f"{name}: the numpy restatement differs from Pillow"
            out[f"{name}_src"], out[f"{name}_out"] = src, res
            if name in ipu.FLOAT_CASES:
                for norm, key in ((False, "f32"), (True, "f32_norm")):
                    x, sK = reference_float(process_img, src, (w, h), norm, tmp)
                    assert x.shape == (3, h, w) and x.dtype == np.float32
                    out[f"{name}_{key}"], out[f"{name}_sK"] = x, sK
    np.savez_compressed(mg.OUT / "image_prep.npz", **out)
    print("wrote", mg.OUT / "image_prep.npz", sum(v.nbytes for v in out.values()), "bytes of arrays")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
