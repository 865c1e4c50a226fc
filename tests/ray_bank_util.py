"""Shared fixtures of the ray-bank tests (test_ray_bank_cpu.py, test_ray_bank_gpu.py): four frames of 24 x 32 px at a focal length of 30 px
-- small enough that the last image row's cone radius differs from its row neighbour's by 2 % -- of which the fourth lies outside the unit
sphere (far = 1 on every ray), and the oracle's rows for them, computed once."""
import functools

import numpy as np
import torch

from nerfmatch_amd import synth
from nerfmatch_amd.nerf.ray_bank import RayBank
from oracle import nerf_oracle as no

H, W, FOCAL = 24, 32, 30.0
RAY_BAR = 2e-6  # the project's bar for ray rows (tests/test_nerf_gpu.py::test_raygen)


@functools.lru_cache(None)
def poses():
    far = synth.camera_pose(7)
    far[:3, 3] = torch.tensor([3.0, 0.5, -2.0])  # outside the unit sphere: pixels that look away from it have a negative discriminant
    return torch.stack([synth.camera_pose(1), synth.camera_pose(2), synth.camera_pose(3), far])


def intrinsics():
    return synth.intrinsics(H, W, FOCAL)


def images(F=4, h=H, w=W, seed=5):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, size=(F, h, w, 3), dtype=np.uint8)
    k = min(256, img.size)
    img.reshape(-1)[:k] = np.arange(k).astype(np.uint8)  # every code of the uint8 -> float conversion occurs (in images of >= 256 bytes)
    return torch.from_numpy(img)


def masks(F=4, h=H, w=W, seed=6):
    g = np.random.default_rng(seed)
    m = g.integers(0, 256, size=(F, h, w), dtype=np.uint8)
    k = min(256, m.size)
    m.reshape(-1)[:k] = np.arange(128 - k // 2, 128 - k // 2 + k).astype(np.uint8)  # 127 / 128, the rounding boundary of round(m / 255), included
    return torch.from_numpy(m)


def bank(device, with_masks=False, **kw):
    kw.setdefault("ts", torch.tensor([3, 0, 2, 1]))
    kw.setdefault("batch_rays", 64)
    return RayBank(images(), poses(), intrinsics(), masks_u8=masks() if with_masks else None, device=device, **kw)


@functools.lru_cache(None)
def oracle_rows():
    """(4 H W, 12): the oracle's rows of every pixel of the four frames (norm_ray_dir=True); treat as read-only"""
    return torch.cat([no.make_rays(H, W, intrinsics(), p, ds=1) for p in poses()])


def all_ids(F=4, h=H, w=W):
    return torch.arange(F * h * w)


def id_images(F, h, w):
    """images whose rgb value spells the pixel's own id (little-endian bytes): recovers which pixel a gathered row came from"""
    g = torch.arange(F * h * w)
    return torch.stack([g & 255, (g >> 8) & 255, (g >> 16) & 255], -1).to(torch.uint8).reshape(F, h, w, 3)


def ids_from_rgbs(rgbs):
    c = torch.round(rgbs.detach().cpu().double() * 255).long()
    return c[:, 0] + (c[:, 1] << 8) + (c[:, 2] << 16)


def id_bank(F, h, w, device, **kw):
    """bank over id_images with simple in-sphere cameras"""
    pose = torch.stack([synth.camera_pose(20 + f) for f in range(F)])
    return RayBank(id_images(F, h, w), pose, synth.intrinsics(h, w, 30.0), device=device, **kw)
