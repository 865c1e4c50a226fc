"""GPU: nm_image_resize_u8 (csrc/image_prep.hip) through nerfmatch_amd.image_prep -- every comparison at exact equality: against Pillow's
bytes and the reference's float images (tests/golden/image_prep.npz), and against the package's host path, which test_image_prep_cpu.py
ties to Pillow.

Shapes: the golden cases (each as one frame and as frame 1 of three), output sizes one below, at and one above a tile in each direction
and 1 x 1 from a 2.5 x larger source, 0 / 255 patterns at 3 x reduction and 2 x enlargement, the largest reduction (8 x: the largest LDS
image, chunks of few staged rows), one 1080 x 1920 frame.  The golden case `wide` lies outside the package's envelope (see
test_image_prep_cpu.py) and must be refused before anything is launched."""
import numpy as np
import pytest
import torch

import image_prep_util as ipu
from nerfmatch_amd import image_prep as ip

pytestmark = pytest.mark.gpu
TW, TH = ip.TILE_WH
ENV_IDS = [c[0] for c in ipu.IN_ENVELOPE]


def _case(name):
    return next(c for c in ipu.CASES if c[0] == name)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _seeded(shape, seed):
    return _t(np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8))


def _batch_of_three(name):
    """frame 1 = the golden source, frames 0 and 2 other seeded content of the same shape"""
    _, H, W, C, w, h, content = _case(name)
    frames = _t(ipu.source(name, H, W, C, "noise", frames=3, seed=9))
    frames[1] = _t(ipu.fixture()[f"{name}_src"])
    return frames


# ----------------------------------------------------------------------------- the golden cases
@pytest.mark.parametrize("name", ENV_IDS)
def test_golden_case_equals_pillow(gpu, built_lib, name):
    _, H, W, C, w, h, _ = _case(name)
    fx = ipu.fixture()
    src, ref = _t(fx[f"{name}_src"])[None], _t(fx[f"{name}_out"])[None]
    got = ip.resize_lanczos_u8(src.to(gpu), (w, h))
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (1, h, w, C)
    print(f"{name}: bytes differing from Pillow: {int((got.cpu() != ref).sum())} of {ref.numel()}")
    assert torch.equal(got.cpu(), ref)
    frames = _batch_of_three(name)
    got3 = ip.resize_lanczos_u8(frames.to(gpu), (w, h)).cpu()
    assert torch.equal(got3[1], ref[0])                                       # the frame stride
    assert torch.equal(got3, ip.resize_lanczos_u8(frames, (w, h)))            # the other frames: the host path
    assert not torch.equal(got3[0], got3[1]) and not torch.equal(got3[2], got3[1])


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("name", ipu.FLOAT_CASES)
def test_golden_float_images_equal_the_reference(gpu, built_lib, name, norm):
    _, H, W, C, w, h, _ = _case(name)
    fx = ipu.fixture()
    ref = _t(fx[f"{name}_f32_norm" if norm else f"{name}_f32"])
    image, sK = ip.query_images(_t(fx[f"{name}_src"])[None].to(gpu), (w, h), imagenet_norm=norm)
    assert image.is_cuda and image.dtype == torch.float32 and image.shape == (1, 3, h, w) and image.is_contiguous()
    assert torch.equal(image[0].cpu(), ref) and torch.equal(sK, _t(fx[f"{name}_sK"]))
    frames = _batch_of_three(name)
    image3, _ = ip.query_images(frames.to(gpu), (w, h), imagenet_norm=norm)
    assert torch.equal(image3[1].cpu(), ref)
    assert torch.equal(image3.cpu(), ip.query_images(frames, (w, h), imagenet_norm=norm)[0])


# ----------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("w,h", [(tw, th) for tw in (TW - 1, TW, TW + 1) for th in (TH - 1, TH, TH + 1)] + [(1, 1)])
def test_output_sizes_at_the_tile_edges(gpu, built_lib, w, h):
    H, W = int(2.5 * h + 0.5), int(2.5 * w + 0.5)
    src = _seeded((2, H, W, 3), 100 * w + h)
    ref = ip.resize_lanczos_u8(src, (w, h))
    assert torch.equal(ip.resize_lanczos_u8(src.to(gpu), (w, h)).cpu(), ref)
    image, _ = ip.query_images(src.to(gpu), (w, h))
    assert torch.equal(image.cpu(), ip.query_images(src, (w, h))[0])
    one = src[..., 1].contiguous()  # C = 1, the (F,H,W) form
    assert torch.equal(ip.resize_lanczos_u8(one.to(gpu), (w, h)).cpu(), ip.resize_lanczos_u8(one, (w, h)))


@pytest.mark.parametrize("H,W,w,h", [(264, 520, TW + 1, TH + 1), (16, 520, TW + 1, 2), (300, 24, 3, TH + 6)])
def test_largest_reduction(gpu, built_lib, H, W, w, h):
    """8 x on both axes, on the width alone and on the height alone: the largest LDS image and the fewest staged rows per chunk"""
    for C in (3, 1):
        src = _seeded((1, H, W, C), H + W + C)
        assert torch.equal(ip.resize_lanczos_u8(src.to(gpu), (w, h)).cpu(), ip.resize_lanczos_u8(src, (w, h)))


# ----------------------------------------------------------------------------- saturation
def _patterns(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    checker = (((yy // 3 + xx // 3) & 1) * 255).astype(np.uint8)
    fine = (((yy + xx) & 1) * 255).astype(np.uint8)
    step = ((xx > W // 2) * 255).astype(np.uint8)
    step_y = ((yy > H // 3) * 255).astype(np.uint8)
    return _t(np.stack([checker, fine, step, step_y]))  # (4,H,W)


@pytest.mark.parametrize("H,W,w,h", [(96, 150, 50, 32), (40, 45, 90, 80)], ids=["reduce3x", "enlarge2x"])
def test_saturated_patterns(gpu, built_lib, H, W, w, h):
    """0 / 255 checkerboards and step edges: the filter's overshoot is clipped at both ends, every byte must be equal"""
    pats = _patterns(H, W)
    ref = ip.resize_lanczos_u8(pats, (w, h))
    got = ip.resize_lanczos_u8(pats.to(gpu), (w, h)).cpu()
    assert torch.equal(got, ref)
    assert int((ref[2] == 0).sum()) > 0 and int((ref[2] == 255).sum()) > 0 and int(((ref[2] > 0) & (ref[2] < 255)).sum()) > 0
    # the restatement's unclipped accumulator really leaves [0, 255] on the step edge: the clip is exercised at both ends
    coef, bounds = ipu.tables(W, w)
    row = pats[2, 0].numpy().astype(np.int64)
    acc = np.array([(coef[x, : bounds[x, 1]].astype(np.int64) * row[bounds[x, 0] : bounds[x, 0] + bounds[x, 1]]).sum() + (1 << 21) for x in range(w)]) >> 22
    assert acc.min() < 0 and acc.max() > 255
    rgb = torch.stack([pats[0], pats[2], pats[3]], -1)[None].contiguous()
    assert torch.equal(ip.resize_lanczos_u8(rgb.to(gpu), (w, h)).cpu(), ip.resize_lanczos_u8(rgb, (w, h)))


def test_the_uint8_intermediate_is_real(gpu, built_lib):
    """37x53 -> 16x8: the filter without the uint8 intermediate differs from Pillow somewhere, the kernel does not"""
    _, H, W, C, w, h, _ = _case("odd")
    fx = ipu.fixture()
    wide = ipu.resize_np_wide_intermediate(fx["odd_src"], (w, h))
    n = int((wide != fx["odd_out"]).sum())
    print(f"bytes that differ without the uint8 intermediate: {n} of {wide.size}")
    assert n > 0
    assert torch.equal(ip.resize_lanczos_u8(_t(fx["odd_src"])[None].to(gpu), (w, h))[0].cpu(), _t(fx["odd_out"]))


# ----------------------------------------------------------------------------- white_where, nerf_frames, RayBank
def test_white_where_values(gpu, built_lib):
    _, H, W, C, w, h, _ = _case("cambridge")
    fx = ipu.fixture()
    src, plain = _t(fx["cambridge_src"])[None], _t(fx["cambridge_out"])[None]
    white = torch.zeros(1, h, w, dtype=torch.uint8)
    spots = {(0, 0): 127, (0, 1): 128, (7, 5): 255, (h - 1, w - 1): 128, (h - 1, 0): 127, (20, 20): 0}
    for (y, x), v in spots.items():
        white[0, y, x] = v
    ref = plain.clone()
    for (y, x), v in spots.items():
        if v >= 128:
            ref[0, y, x] = 255
    got = ip.resize_lanczos_u8(src.to(gpu), (w, h), white_where=white.to(gpu))
    assert torch.equal(got.cpu(), ref) and torch.equal(got.cpu(), ip.resize_lanczos_u8(src, (w, h), white_where=white))
    assert torch.equal(ip.resize_lanczos_u8(src.to(gpu), (w, h), white_where=white).cpu(), ref)  # a host mask is moved
    g = np.random.default_rng(3)  # every pixel one of the four values, a size across tiles, C = 1 too
    w2, h2 = TW + 3, TH + 2
    src2 = _seeded((2, 2 * h2, 3 * w2, 3), 17)
    white2 = _t(g.choice(np.array([0, 127, 128, 255], np.uint8), size=(2, h2, w2)))
    ref2 = ip.resize_lanczos_u8(src2, (w2, h2), white_where=white2)
    assert torch.equal(ip.resize_lanczos_u8(src2.to(gpu), (w2, h2), white_where=white2.to(gpu)).cpu(), ref2)
    assert torch.equal(ref2[white2 >= 128], torch.full_like(ref2[white2 >= 128], 255))
    one = src2[..., 0].contiguous()
    assert torch.equal(ip.resize_lanczos_u8(one.to(gpu), (w2, h2), white_where=white2.to(gpu)).cpu(),
                       ip.resize_lanczos_u8(one, (w2, h2), white_where=white2))


def _nerf_inputs(F=2, H=108, W=192):
    g = np.random.default_rng(21)
    images = _seeded((F, H, W, 3), 22)
    yy, xx = np.mgrid[0:H, 0:W]
    bg = _t(np.stack([(((yy - 30 - 9 * f) ** 2 + (xx - 60) ** 2) < 900).astype(np.uint8) * 255 for f in range(F)]))
    trnz = _t(g.integers(0, 2, size=(F, H, W), dtype=np.uint8) * 255)
    return images, bg, trnz


def test_nerf_frames_and_a_ray_bank_on_them(gpu, built_lib):
    from nerfmatch_amd import synth
    from nerfmatch_amd.nerf.ray_bank import RayBank

    images, bg, trnz = _nerf_inputs()
    wh = (48, 48)
    host = ip.nerf_frames(images, wh, bg_masks_u8=bg, trnz_masks_u8=trnz)
    dev = ip.nerf_frames(images.to(gpu), wh, bg_masks_u8=bg.to(gpu), trnz_masks_u8=trnz.to(gpu))
    assert dev["images_u8"].is_cuda and dev["masks_u8"].is_cuda
    assert torch.equal(dev["images_u8"].cpu(), host["images_u8"]) and torch.equal(dev["masks_u8"].cpu(), host["masks_u8"])
    assert torch.equal(dev["sK"], host["sK"])
    white = int((host["images_u8"] == 255).all(-1).sum())
    assert 0 < white < 2 * 48 * 48  # part of every frame is blended
    only_bg = ip.nerf_frames(images.to(gpu), wh, bg_masks_u8=bg)  # host masks beside device images are moved
    assert only_bg["masks_u8"] is None and torch.equal(only_bg["images_u8"], dev["images_u8"])
    K = dev["sK"] @ synth.intrinsics(108, 192, 150.0)
    pose = torch.stack([synth.camera_pose(3), synth.camera_pose(4)])
    bank = RayBank(dev["images_u8"], pose, K, masks_u8=dev["masks_u8"], exclude_masks=False, device=gpu)
    ids = torch.tensor([0, 47, 48 * 20 + 13, 48 * 48 - 1, 48 * 48, 48 * 48 + 48 * 30 + 60 // 4, 2 * 48 * 48 - 1])
    _, rgbs, _, mask = bank.batch(ids.to(gpu))
    flat = host["images_u8"].reshape(-1, 3)
    assert torch.equal(rgbs.cpu(), flat[ids].float().div(255))
    assert torch.equal(mask.cpu()[:, 0], 1 - torch.round(host["masks_u8"].reshape(-1)[ids].float().div(255)))


# ----------------------------------------------------------------------------- full size
def test_full_size_frame(gpu, built_lib):
    src = _seeded((1, 1080, 1920, 3), 1080)
    ref = ip.resize_lanczos_u8(src, (480, 480))
    dev = src.to(gpu)
    assert torch.equal(ip.resize_lanczos_u8(dev, (480, 480)).cpu(), ref)
    image, sK = ip.query_images(dev, (480, 480), imagenet_norm=True)
    lut = _t(ipu.lut_np(True))
    assert torch.equal(image[0].cpu(), torch.stack([lut[c][ref[0, ..., c].long()] for c in range(3)]))
    assert torch.equal(sK, torch.tensor([[0.25, 0, 0], [0, 480 / 1080, 0], [0, 0, 1]], dtype=torch.float64).float())


# ----------------------------------------------------------------------------- arguments
def test_envelope_errors_come_before_any_launch(gpu, built_lib, monkeypatch):
    from nerfmatch_amd import _lib, ops

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched for a call outside the envelope")

    monkeypatch.setattr(ops, "image_resize_u8", no_launch)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=gpu)
    _, H, W, C, w, h, _ = _case("wide")
    with pytest.raises(ValueError, match="at most 8 x"):
        ip.resize_lanczos_u8(_t(ipu.fixture()["wide_src"])[None].to(gpu), (w, h))
    with pytest.raises(ValueError, match="C = 2"):
        ip.resize_lanczos_u8(u8(1, 8, 8, 2), (4, 4))
    with pytest.raises(ValueError, match="64 -> 1"):
        ip.resize_lanczos_u8(u8(1, 64, 64), (1, 1))
    with pytest.raises(ValueError, match="8193"):
        ip.resize_lanczos_u8(u8(1, 2, 8193, 1), (8193, 2))
    with pytest.raises(ValueError, match="uint8"):
        ip.resize_lanczos_u8(torch.zeros(1, 8, 8, 3, device=gpu), (4, 4))
    with pytest.raises(ValueError, match="white_where"):
        ip.resize_lanczos_u8(u8(1, 8, 8, 3), (5, 4), white_where=u8(1, 5, 4))
    monkeypatch.undo()
    # the entry point itself refuses the same shapes with NM_ERR_UNSUPPORTED (nothing is enqueued: its checks come first)
    src, out = _seeded((1, 72, 72, 3), 72).to(gpu), u8(1, 8, 8, 3)
    cx, bx = (t.to(gpu) for t in ip.lanczos_tables(64, 8))
    cxt = cx.t().contiguous()  # tap-major for the horizontal pass
    call = lambda Hs, Ws, Cs, kx, ky: _lib.lib().nm_image_resize_u8(_lib.dptr(src, torch.uint8), 1, Hs, Ws, Cs, _lib.dptr(cxt, torch.int32),
                                                                   _lib.dptr(bx, torch.int32), kx, _lib.dptr(cx, torch.int32), _lib.dptr(bx, torch.int32), ky,
                                                                   8, 8, None, None, _lib.dptr(out, torch.uint8), None, _lib.stream())
    assert call(64, 64, 2, 49, 49) == _lib.NM_ERR_UNSUPPORTED   # channels
    assert call(72, 64, 3, 49, 55) == _lib.NM_ERR_UNSUPPORTED   # 9 x
    assert call(64, 64, 3, 49, 47) == 1                         # a ksize that is not the axis' (NM_ERR_ARG)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
    assert call(64, 64, 3, 49, 49) == 0
    assert torch.equal(out.cpu(), ip.resize_lanczos_u8(src.cpu().reshape(-1)[: 64 * 64 * 3].view(1, 64, 64, 3), (8, 8)))


def test_sources_that_are_not_plain_contiguous_tensors(gpu, built_lib):
    base = _seeded((2, 60, 90, 3), 5)
    dev = base.to(gpu)
    for view in (lambda t: t[:, ::2], lambda t: t[:, :, 3:80], lambda t: t.permute(0, 2, 1, 3), lambda t: t[..., 1]):
        v = view(dev)
        assert not v.is_contiguous()
        wh = (v.shape[2] // 2, v.shape[1] // 2)
        assert torch.equal(ip.resize_lanczos_u8(v, wh).cpu(), ip.resize_lanczos_u8(view(base).contiguous(), wh))
    # contiguous, but starting one byte into an allocation: no 16-byte alignment
    buf = torch.zeros(base.numel() + 1, dtype=torch.uint8, device=gpu)
    buf[1:] = dev.reshape(-1)
    odd = buf[1:].view(2, 60, 90, 3)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 1
    assert torch.equal(ip.resize_lanczos_u8(odd, (30, 40)).cpu(), ip.resize_lanczos_u8(base, (30, 40)))
