#!/usr/bin/env python3
"""Golden vectors of the training ray rows (tests/golden/ray_bank.npz), from the REFERENCE's own functions.

    python tests/golden/make_golden_ray_bank.py      # rewrites tests/golden/ray_bank.npz (NM_GOLDEN_OUT=<dir>: elsewhere)

Needs the reference tree (make_golden.py's REF and stub modules).  Two frames of W x H = 9 x 7 px, focal length ~10 px, one K per frame,
expanded the way NerfBaseDataset.load_sample does (nerfmatch/datasets/nerfbase.py:278-298): get_ray_dirs, get_rays_c2w,
rays_intersect_sphere inside the try / except, prepare_rays_data with comp_radii -- once with norm_ray_dir True and once False; the rgb
rows are uint8 / 255 as torchvision's to_tensor divides (`.float().div(255)`).  Only arrays are written."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402

H, W = 7, 9


def frame_rays(K, c2w, norm_ray_dir):
    from nerfmatch.nerf.render_utils import get_ray_dirs, get_rays_c2w, prepare_rays_data
    from nerfmatch.nerf.scene_utils import rays_intersect_sphere

    directions, _ = get_ray_dirs(H, W, K, return_xys=True)
    rays_o, rays_d, viewdirs = get_rays_c2w(directions, c2w)
    rays_d = viewdirs if norm_ray_dir else rays_d
    try:
        far = rays_intersect_sphere(rays_o.view(-1, 3), viewdirs.view(-1, 3), r=1).reshape(H, W, 1)
        flag = 0
    except Exception:
        far = torch.ones((H, W, 1)).float()
        flag = 1
    return prepare_rays_data(rays_o, rays_d, viewdirs, 0.01, far, comp_radii=True), flag


def main():
    from nerfmatch_amd import synth

    g = np.random.default_rng(23)
    Ks = torch.stack([synth.intrinsics(H, W, 10.0), torch.tensor([[11.0, 0.0, 4.0], [0.0, 9.5, 3.0], [0.0, 0.0, 1.0]])])
    c2w = torch.stack([synth.camera_pose(11), synth.camera_pose(12)])
    images = g.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    images.reshape(-1)[:256] =np.arange(256, dtype=np.uint8)  # every uint8 code occurs
    out = dict(K=Ks.numpy(), c2w=c2w.numpy(), images=images, rgbs=torch.from_numpy(images).reshape(-1, 3).float().div(255).numpy())
    for name, norm in (("rays_norm", True), ("rays_unnorm", False)):
        rows, flags = zip(*[frame_rays(Ks[f], c2w[f], norm) for f in range(2)])
        out[name] = torch.cat(rows, 0).numpy()
        out["flags"] = np.asarray(flags, np.int32)
    assert out["rays_norm"].shape == (2 * H * W, 12) and out["rays_norm"].dtype == np.float32
    np.savez_compressed(mg.OUT / "ray_bank.npz", **out)
    print("wrote", mg.OUT / "ray_bank.npz")


if __name__ == "__main__":
    assert mg.REF.exists(), "the reference is only present in the build container"
    mg.install_stubs()
    torch.set_num_threads(1)
    main()
