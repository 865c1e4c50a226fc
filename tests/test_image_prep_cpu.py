"""image_prep without a GPU: the numpy restatement of Pillow's 8-bit Lanczos resampler against Pillow's bytes (tests/golden/image_prep.npz),
the package's tables against the restatement's, the package's host path against the golden outputs -- all at exact equality -- the
blending threshold, the batch glue and the envelope.

One golden case, `wide` (5x200x3 -> 3x5), reduces its width 66 x, which lies outside the envelope the package states (at most 8 x per
axis, ksize <= 51).  The fixture holds it and the restatement reproduces it; the package must refuse it and name the limit, which
test_package_refuses_the_case_outside_its_envelope asserts.  `wide8` is the same source at the envelope's edge (200 -> 25)."""
import re
from argparse import Namespace
from pathlib import Path

import numpy as np
import pytest
import torch

import image_prep_util as ipu
from nerfmatch_amd import image_prep as ip

ROOT = Path(__file__).resolve().parents[1]
CASE_IDS = [c[0] for c in ipu.CASES]
ENV_IDS = [c[0] for c in ipu.IN_ENVELOPE]


def _case(name):
    return next(c for c in ipu.CASES if c[0] == name)


def _src(name):
    """(1,H,W,C) uint8 tensor of a golden case"""
    return torch.from_numpy(ipu.fixture()[f"{name}_src"])[None]


def _out(name):
    return torch.from_numpy(ipu.fixture()[f"{name}_out"])[None]


# ----------------------------------------------------------------------------- the restatement and Pillow
@pytest.mark.parametrize("name", CASE_IDS)
def test_restatement_matches_the_golden_bytes(name):
    _, H, W, C, w, h, content = _case(name)
    fx = ipu.fixture()
    assert np.array_equal(fx[f"{name}_src"], ipu.source(name, H, W, C, content)[0])  # the fixture's sources are the seeded ones
    got = ipu.resize_np(fx[f"{name}_src"], (w, h))
    assert got.dtype == np.uint8 and np.array_equal(got, fx[f"{name}_out"])


@pytest.mark.parametrize("H,W,C,w,h,content", [(45, 80, 3, 20, 20, "noise"), (30, 41, 1, 67, 11, "binary"), (96, 33, 3, 33, 12, "binary")])
def test_restatement_matches_pillow_on_further_shapes(H, W, C, w, h, content):
    PIL = pytest.importorskip("PIL")
    from PIL import Image

    src = ipu.source("further", H, W, C, content)[0]
    pil = Image.fromarray(src[..., 0], "L") if C == 1 else Image.fromarray(src, "RGB")
    ref = np.asarray(pil.resize((w, h), Image.LANCZOS)).reshape(h, w, C)
    assert np.array_equal(ipu.resize_np(src, (w, h)), ref), PIL.__version__


def test_intermediate_rounding_is_visible_in_the_odd_case():
    """the uint8 intermediate is part of the result: keeping the horizontal pass in wider precision gives other bytes somewhere"""
    _, H, W, C, w, h, _ = _case("odd")
    fx = ipu.fixture()
    assert not np.array_equal(ipu.resize_np_wide_intermediate(fx["odd_src"], (w, h)), fx["odd_out"])


# ----------------------------------------------------------------------------- tables
def _axis_pairs():
    pairs = {(1920, 480), (1080, 480), (640, 480)}
    for _, H, W, _, w, h, _ in ipu.IN_ENVELOPE:
        pairs |= {(W, w), (H, h)}
    return sorted(pairs)


@pytest.mark.parametrize("in_size,out_size", _axis_pairs())
def test_tables_equal_the_restatement(in_size, out_size):
    coef, bounds = ip.lanczos_tables(in_size, out_size)
    rc, rb = ipu.tables(in_size, out_size)
    assert coef.dtype == torch.int32 and bounds.dtype == torch.int32
    assert coef.shape == rc.shape and np.array_equal(coef.numpy(), rc) and np.array_equal(bounds.numpy(), rb)
    assert coef.shape[1] <= ip.MAX_KSIZE and int(coef.abs().max()) < 1 << 23
    assert ip.lanczos_tables(in_size, out_size)[0] is coef  # cached


def test_tile_constants_are_the_headers():
    txt = (ROOT / "include" / "nerfmatch_amd.h").read_text()
    tw, th = (int(re.search(rf"#define {n}\s+(\d+)", txt).group(1)) for n in ("NM_IMAGE_TILE_W", "NM_IMAGE_TILE_H"))
    assert ip.TILE_WH == (tw, th)


# ----------------------------------------------------------------------------- the host path against the golden outputs
@pytest.mark.parametrize("name", ENV_IDS)
def test_host_resize_equals_pillow(name):
    _, H, W, C, w, h, _ = _case(name)
    got = ip.resize_lanczos_u8(_src(name), (w, h))
    assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got, _out(name))
    if C == 1:  # the (F,H,W) form
        assert torch.equal(ip.resize_lanczos_u8(_src(name)[..., 0], (w, h)), _out(name)[..., 0])


def test_host_resize_of_a_batch_is_frame_by_frame():
    _, H, W, C, w, h, content = _case("odd")
    frames = torch.from_numpy(ipu.source("odd", H, W, C, content, frames=3, seed=5))
    frames[1] = _src("odd")[0]
    got = ip.resize_lanczos_u8(frames, (w, h))
    assert torch.equal(got[1], _out("odd")[0]) and not torch.equal(got[0], got[1])


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("name", ipu.FLOAT_CASES)
def test_host_query_images_equal_the_reference(name, norm):
    _, H, W, C, w, h, _ = _case(name)
    fx = ipu.fixture()
    image, sK = ip.query_images(_src(name), (w, h), imagenet_norm=norm)
    ref = torch.from_numpy(fx[f"{name}_f32_norm" if norm else f"{name}_f32"])
    assert image.dtype == torch.float32 and image.shape == (1, 3, h, w) and torch.equal(image[0], ref)
    assert sK.dtype == torch.float32 and torch.equal(sK, torch.from_numpy(fx[f"{name}_sK"]))


def test_lut_is_the_references_arithmetic():
    for norm in (False, True):
        assert np.array_equal(ip._lut_np(3, norm), ipu.lut_np(norm))


def test_white_where_threshold():
    _, H, W, C, w, h, _ = _case("cambridge")
    white = torch.zeros(1, h, w, dtype=torch.uint8)
    white[0, 0, 0], white[0, 0, 1], white[0, 5, 7], white[0, h - 1, w - 1] = 127, 128, 255, 128
    got = ip.resize_lanczos_u8(_src("cambridge"), (w, h), white_where=white)
    ref = _out("cambridge").clone()
    for y, x in ((0, 1), (5, 7), (h - 1, w - 1)):
        ref[0, y, x] = 255
    assert torch.equal(got, ref)
    assert torch.equal(got[0, 0, 0], _out("cambridge")[0, 0, 0])  # 127 keeps the pixel


def _nerf_inputs(name="cambridge", frames=2):
    _, H, W, C, w, h, content = _case(name)
    images = torch.from_numpy(ipu.source(name, H, W, C, content, frames=frames, seed=3))
    images[0] = _src(name)[0]
    g = np.random.default_rng(11)
    # smooth blobs: the resized masks take values on both sides of 128 and in between
    yy, xx = np.mgrid[0:H, 0:W]
    bg = torch.from_numpy(np.stack([(((yy - 30 - 9 * f) ** 2 + (xx - 60) ** 2) < 900).astype(np.uint8) * 255 for f in range(frames)]))
    trnz = torch.from_numpy(g.integers(0, 2, size=(frames, H, W), dtype=np.uint8) * 255)
    return images, bg, trnz, (w, h)


def test_nerf_frames_host():
    images, bg, trnz, wh = _nerf_inputs()
    out = ip.nerf_frames(images, wh, bg_masks_u8=bg, trnz_masks_u8=trnz)
    m = torch.stack([torch.from_numpy(ipu.resize_np(bg[f].numpy()[..., None], wh))[..., 0] for f in range(2)])
    img = torch.stack([torch.from_numpy(ipu.resize_np(images[f].numpy(), wh)) for f in range(2)])
    assert 0 < int((m >= 128).sum()) < m.numel() and int(((m > 0) & (m < 255)).sum()) > 0
    # the reference's blend in floats (nerfbase.py:218-223) on to_tensor's values, back to bytes
    mf = torch.round(m.float().div(255))[..., None]
    blended = img.float().div(255) * (1 - mf) + mf * torch.tensor([1.0, 1.0, 1.0])
    assert torch.equal(out["images_u8"], (blended * 255).round().to(torch.uint8))
    assert torch.equal(out["images_u8"][0][m[0] < 128], _out("cambridge")[0][m[0] < 128])
    tm = torch.stack([torch.from_numpy(ipu.resize_np(trnz[f].numpy()[..., None], wh))[..., 0] for f in range(2)])
    assert torch.equal(out["masks_u8"], tm)
    assert torch.equal(out["sK"], torch.from_numpy(ipu.fixture()["cambridge_sK"]))
    plain = ip.nerf_frames(images, wh)
    assert plain["masks_u8"] is None and torch.equal(plain["images_u8"], img)


def test_nerf_frames_pass_ray_banks_argument_checks():
    """what RayBank.__init__ requires of images_u8 / masks_u8 (nerf/ray_bank.py), without building rays"""
    images, bg, trnz, (w, h) = _nerf_inputs()
    out = ip.nerf_frames(images, (w, h), bg_masks_u8=bg, trnz_masks_u8=trnz)
    im, mk = out["images_u8"], out["masks_u8"]
    assert im.dtype == torch.uint8 and im.dim() == 4 and tuple(im.shape) == (2, h, w, 3) and im.is_contiguous() and h >= 3
    assert mk.dtype == torch.uint8 and tuple(mk.shape) == (2, h, w) and mk.is_contiguous()


# ----------------------------------------------------------------------------- batch glue
def _query_batch(name="scenes7"):
    K = torch.tensor([[[525.0, 0.0, 320.0], [0.0, 525.0, 240.0], [0.0, 0.0, 1.0]]])
    return dict(image_u8=_src(name), K=K.clone(), idx=torch.tensor([4])), K


def test_prepare_query_batch_fills_image_and_scales_K():
    _, H, W, C, w, h, _ = _case("scenes7")
    batch, K = _query_batch()
    out = ip.prepare_query_batch(batch, (w, h), imagenet_norm=True)
    assert out is batch and torch.equal(batch["image"][0], torch.from_numpy(ipu.fixture()["scenes7_f32_norm"]))
    sK = torch.from_numpy(ipu.fixture()["scenes7_sK"])
    assert torch.equal(batch["K"], sK @ K) and batch["K"].shape == (1, 3, 3) and float(batch["K"][0, 0, 0]) == 525.0 * 48 / 64
    assert torch.equal(batch["idx"], torch.tensor([4]))


def test_batch_without_image_u8_is_untouched():
    image, K = torch.zeros(1, 3, 4, 4), torch.eye(3)[None]
    batch = dict(image=image, K=K)
    out = ip.prepare_query_batch(batch, (48, 48))
    assert out is batch and set(batch) == {"image", "K"} and batch["image"] is image and batch["K"] is K
    both = dict(image=image, K=K, image_u8=_src("scenes7"))  # an `image` that is already there is kept
    assert ip.prepare_query_batch(both, (48, 48)) is both and both["image"] is image and both["K"] is K


def test_evaluator_prepares_decoded_queries_from_its_data_config():
    from nerfmatch_amd.nerfmatch_evaluator import NeRFMatchEvaluator

    batch, K = _query_batch()
    ev = Namespace(config=Namespace(data=Namespace(img_wh=[48, 48], imagenet_norm=True)), device=torch.device("cpu"))
    out = NeRFMatchEvaluator._prepare_queries(ev, batch)
    assert out is batch and torch.equal(batch["image"][0], torch.from_numpy(ipu.fixture()["scenes7_f32_norm"]))
    assert torch.equal(batch["K"], torch.from_numpy(ipu.fixture()["scenes7_sK"]) @ K)
    ev.config.data = Namespace(img_wh=[48, 48])  # imagenet_norm defaults to False, as in the reference's dataset
    batch, _ = _query_batch()
    NeRFMatchEvaluator._prepare_queries(ev, batch)
    assert torch.equal(batch["image"][0], torch.from_numpy(ipu.fixture()["scenes7_f32"]))


# ----------------------------------------------------------------------------- the envelope
def test_package_refuses_the_case_outside_its_envelope():
    _, H, W, C, w, h, _ = _case("wide")
    with pytest.raises(ValueError, match="at most 8 x"):
        ip.resize_lanczos_u8(_src("wide"), (w, h))
    with pytest.raises(ValueError, match="at most 8 x"):
        ip.lanczos_tables(W, w)


def test_out_of_envelope_calls_name_the_limit():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"C = 2 channels.*\{1, 3\}"):
        ip.resize_lanczos_u8(u8(1, 8, 8, 2), (4, 4))
    with pytest.raises(ValueError, match="C = 1 channels"):
        ip.query_images(u8(1, 8, 8, 1), (4, 4))
    with pytest.raises(ValueError, match="64 -> 1.*at most 8 x"):
        ip.resize_lanczos_u8(u8(1, 64, 64, 1), (1, 1))
    with pytest.raises(ValueError, match="64 -> 1.*at most 8 x"):
        ip.lanczos_tables(64, 1)
    with pytest.raises(ValueError, match="8193.*8192"):
        ip.resize_lanczos_u8(u8(1, 2, 8193, 1), (8193, 2))
    with pytest.raises(ValueError, match="8193.*8192"):
        ip.resize_lanczos_u8(u8(1, 4, 4, 1), (4, 8193))
    with pytest.raises(ValueError, match="uint8.*float32"):
        ip.resize_lanczos_u8(torch.zeros(1, 8, 8, 3), (4, 4))
    with pytest.raises(ValueError, match=r"white_where.*\(1,4,5\)"):
        ip.resize_lanczos_u8(u8(1, 8, 8, 3), (5, 4), white_where=u8(1, 5, 4))
    with pytest.raises(ValueError, match="white_where.*uint8"):
        ip.resize_lanczos_u8(u8(1, 8, 8, 3), (5, 4), white_where=torch.zeros(1, 4, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="bg_masks_u8"):
        ip.nerf_frames(u8(2, 8, 8, 3), (4, 4), bg_masks_u8=u8(2, 4, 4))
    assert ip.resize_lanczos_u8(u8(1, 40, 40, 3), (5, 5)).shape == (1, 5, 5, 3)  # exactly 8 x is inside
