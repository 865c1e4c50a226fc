"""GPU: the four kernels of csrc/convformer.hip, the ConvFormer stages built on them, and their wiring into the matchers.

References are computed on the CPU (float64 where a tolerance is involved, tests/convformer_util.py); no test here calls a torch
device convolution."""
import warnings
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

import convformer_util as cu
from nerfmatch_amd import _lib, ops, synth
from nerfmatch_amd.matcher import NeRFMatcherCoarse, NeRFMatcherMS
from nerfmatch_amd.modules import PrecomputedBackbone, init_backbone, init_backbone_8_2
from nerfmatch_amd.modules.convformer import ConvFormerStages

pytestmark = pytest.mark.gpu

TH, TW = _lib.NM_DWCONV_TILE_H, _lib.NM_DWCONV_TILE_W


def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


@pytest.fixture
def native_only(monkeypatch):
    """The plain-torch path must not be what answers on the device."""
    def boom(self, img):
        raise AssertionError("the plain-torch path ran on a device tensor without autograd")
    monkeypatch.setattr(ConvFormerStages, "_forward_torch", boom)


# ------------------------------------------------------------------------------------------------------------------ nm_conv_patches
@pytest.mark.parametrize("layout,shape,k,s,p,ld", [(0, (2, 3, 30, 22), 7, 2, 3, 152), (0, (1, 3, 33, 37), 7, 4, 2, 152),
                                                   (1, (2, 12, 20, 128), 3, 4, 1, 1152), (1, (1, 5, 7, 128), 3, 2, 1, 1152)])
def test_conv_patches_exact(gpu, built_lib, layout, shape, k, s, p, ld):
    x = randn(shape, 5)
    nchw = x.permute(0, 3, 1, 2) if layout else x
    B, Cc, H, W = nchw.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    unf = F.unfold(nchw, k, padding=p, stride=s)  # (B, C k k, L), rows in (c, ky, kx) order
    want = unf.view(B, Cc, k, k, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(B * Ho * Wo, k * k * Cc)
    want = F.pad(want, (0, ld - k * k * Cc))
    got, hw = ops.conv_patches(x.to(gpu), k, s, p, ld, channel_last=bool(layout))
    assert hw == (Ho, Wo) and torch.equal(got.cpu(), want)
    # into a poisoned buffer: the pad columns are WRITTEN as zero
    rows = torch.full((B * Ho * Wo, ld), float("nan"), device=gpu)
    _lib.check(_lib.lib().nm_conv_patches(_lib.dptr(x.to(gpu)), layout, B, Cc, H, W, k, s, p, ld, _lib.dptr(rows), ops.stream()), "nm_conv_patches")
    assert torch.equal(rows.cpu(), want)


def test_conv_patches_times_reordered_weight_is_the_convolution(gpu, built_lib):
    """ops.conv_weight_rows orders a Conv2d weight the way the patches' columns run (float64 convolution on the CPU as the reference)."""
    x, w, b = randn((2, 3, 30, 22), 1), randn((128, 3, 7, 7), 2) * 0.1, randn((128,), 3)
    rows, (Ho, Wo) = ops.conv_patches(x.to(gpu), 7, 2, 3, 152)
    y = ops.linear(rows, ops.conv_weight_rows(w.to(gpu), 152), b.to(gpu)).view(2, Ho, Wo, 128).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3)
    assert cu.scaled_err(y, ref) <= cu.TOL


# ------------------------------------------------------------------------------------------------------------------ nm_nhwc_to_nchw
@pytest.mark.parametrize("B,hw,Cc", [(2, (1, 1), 256), (1, (4, 6), 256), (3, (13, 19), 128)])
def test_nhwc_to_nchw_exact(gpu, built_lib, B, hw, Cc):
    x = randn((B, *hw, Cc), 9)
    y = ops.nhwc_to_nchw(x.to(gpu))
    assert torch.equal(y.cpu(), x.permute(0, 3, 1, 2).contiguous())
    out = torch.full((B + 1, Cc, *hw), float("nan"), device=gpu)  # into a slice of a larger buffer: nothing behind it is touched
    ops.nhwc_to_nchw(x.to(gpu), out=out[:B])
    assert torch.equal(out[:B].cpu(), x.permute(0, 3, 1, 2)) and bool(torch.isnan(out[B]).all())


# ------------------------------------------------------------------------------------------------------------------ nm_star_relu
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 1e-20, 3e-39, -2.5, 1.5]


def same_bits_or_nan(a, b):
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros_like(a)
    return torch.equal(nan_a, nan_b) and torch.equal(torch.where(nan_a, zero, a), torch.where(nan_b, zero, b))


@pytest.mark.parametrize("n", [1, 63, 257, 2 ** 20 + 3])
@pytest.mark.parametrize("inplace", [False, True])
def test_star_relu_exact(gpu, built_lib, n, inplace):
    x = randn((n,), n) * 3
    sp = torch.tensor(SPECIALS)
    x[:min(n, len(sp))] = sp[:n]
    if n > 2 * len(sp):
        x[-len(sp):] = sp  # (the scalar tail sees them too)
    if n == 1:
        x[0] = float("nan")
    scale, bias = torch.tensor([0.83]), torch.tensor([-0.41])
    want = scale * torch.relu(x) ** 2 + bias
    xd = x.to(gpu)
    got = ops.star_relu(xd, scale.to(gpu), bias.to(gpu), inplace=inplace)
    assert (got.data_ptr() == xd.data_ptr()) == inplace
    assert same_bits_or_nan(got.cpu(), want)
    if not inplace:
        assert same_bits_or_nan(xd.cpu(), x)


def test_star_relu_signed_zero_and_small_n(gpu, built_lib):
    scale, bias = torch.tensor([1.25]).to(gpu), torch.tensor([0.0]).to(gpu)
    for n in (2, 3, 4, 5, 7, 8):
        x = torch.tensor(SPECIALS[:n])
        got = ops.star_relu(x.to(gpu), scale, bias).cpu()
        assert same_bits_or_nan(got, 1.25 * torch.relu(x) ** 2 + 0.0)


# ------------------------------------------------------------------------------------------------------------------ nm_dwconv7_nhwc
DW_SHAPES = [(1, 1, 1, 256), (2, 2, 3, 256), (2, 7, 9, 256), (1, 13, 17, 512), (1, 3, 40, 64), (1, TH, TW, 64), (1, TH + 1, TW + 1, 64),
             (2, 2 * TH + 3, TW - 1, 128)]


def dwconv_reference(x, w, scale, bias):
    """float64 result and the pointwise bound 56 2^-24 sum_taps |w| (|scale| relu(x)^2 + |bias|)  (|x| without the activation) from fp32
    inputs x (B,H,W,C), w (C,1,7,7): 49 fused steps plus the activation's three roundings, the rest room for second-order terms."""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    if scale is None:
        a, mag = xd, xd.abs()
    else:
        r2 = torch.clamp(xd, min=0) ** 2
        a, mag = scale.double() * r2 + bias.double(), scale.double().abs() * r2 + bias.double().abs()
    ref = F.conv2d(a, wd, padding=3, groups=wd.shape[0])
    bound = 56 * 2.0 ** -24 * F.conv2d(mag, wd.abs(), padding=3, groups=wd.shape[0])
    return ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", DW_SHAPES)
@pytest.mark.parametrize("act", [False, True])
def test_dwconv7_against_float64(gpu, built_lib, shape, act):
    x, w = randn(shape, 3) * 2, randn((shape[3], 1, 7, 7), 4) * 0.3
    scale, bias = (torch.tensor([0.9]), torch.tensor([-0.35])) if act else (None, None)
    ref, bound = dwconv_reference(x, w, scale, bias)
    got = ops.dwconv7_nhwc(x.to(gpu), w.to(gpu), None if scale is None else scale.to(gpu), None if bias is None else bias.to(gpu))
    err = (got.cpu().double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"dwconv7 {shape} act={act}: max err {float(err.max()):.2e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all())


def test_dwconv7_border_rule_exact_integers(gpu, built_lib):
    """x = 0, w = 1, scale = 1, bias = 1: every in-image tap is worth 1, every padded one 0 (the padding comes behind the activation)."""
    x, w = torch.zeros(1, 9, 9, 64, device=gpu), torch.ones(64, 1, 7, 7, device=gpu)
    one = torch.ones(1, device=gpu)
    y = ops.dwconv7_nhwc(x, w, one, one).cpu()
    assert bool((y[0, 0, 0] == 16).all()) and bool((y[0, 8, 8] == 16).all())
    assert bool((y[0, 0, 4] == 28).all()) and bool((y[0, 4, 8] == 28).all())
    assert bool((y[0, 4, 4] == 49).all())
    rows = torch.tensor([4, 5, 6, 7, 7, 7, 6, 5, 4.0])
    assert torch.equal(y[0, :, :, 0], rows[:, None] * rows[None, :])
    assert bool((ops.dwconv7_nhwc(x, w).cpu() == 0).all())  # without the activation the same image is all zeros


@pytest.mark.parametrize("act", [False, True])
def test_dwconv7_no_bleed_between_images(gpu, built_lib, act):
    H, W, Cc = TH + 2, 5, 64
    w = (randn((Cc, 1, 7, 7), 8)).to(gpu)
    sb = (torch.tensor([0.9], device=gpu), torch.tensor([-0.35], device=gpu)) if act else (None, None)
    pair = torch.zeros(2, H, W, Cc, device=gpu)
    pair[1] = 1e3
    both = ops.dwconv7_nhwc(pair, w, *sb)
    alone = ops.dwconv7_nhwc(pair[:1].contiguous(), w, *sb)
    assert torch.equal(both[:1], alone)
    assert torch.equal(both[1:], ops.dwconv7_nhwc(pair[1:].contiguous(), w, *sb))


# ------------------------------------------------------------------------------------------------------------------ whole backbone
def load_ms(state, gpu):
    m = init_backbone_8_2("convformer")
    m.model.load_state_dict(state, strict=True)
    return m.to(gpu).eval()


def load_mini(state, gpu):
    m = init_backbone("convformer", downsample=8)
    m.load_state_dict(state, strict=True)
    return m.to(gpu).eval()


@pytest.mark.parametrize("kind,shape", [("c2f", (2, 3, 32, 48)), ("c2f", (2, 3, 26, 38)), ("coarse", (2, 3, 64, 72))])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_backbone_against_float64(gpu, built_lib, native_only, monkeypatch, kind, shape, precision):
    monkeypatch.setattr(ops, "LINEAR_PRECISION", precision)
    state, img, f_ref, c_ref = cu.case(kind, shape)
    if kind == "c2f":
        cfeat, ffeat = load_ms(state, gpu)(img.to(gpu))
        assert tuple(ffeat.shape) == tuple(f_ref.shape) and ffeat.is_contiguous()
        ef = cu.scaled_err(ffeat, f_ref)
        print(f"backbone {kind} {shape} {precision}: ffeat err {ef:.2e} of scale (max|ref| {float(f_ref.abs().max()):.1f})")
        assert ef <= cu.TOL
    else:
        out = load_mini(state, gpu)(img.to(gpu))
        assert isinstance(out, list) and len(out) == 1
        cfeat = out[0]
    assert tuple(cfeat.shape) == tuple(c_ref.shape) and cfeat.is_contiguous()
    ec = cu.scaled_err(cfeat, c_ref)
    print(f"backbone {kind} {shape} {precision}: cfeat err {ec:.2e} of scale (max|ref| {float(c_ref.abs().max()):.1f})")
    assert ec <= cu.TOL


def test_backbone_batch_invariance(gpu, built_lib, native_only):
    """Image q of a batch gives the bits of q alone, also when the chunk budget forces one image per chunk."""
    state = cu.case("c2f", (2, 3, 32, 48))[0]
    m = load_ms(state, gpu)
    img = cu.image((3, 3, 32, 48), seed=4).to(gpu)
    cfeat, ffeat = m(img)
    m.model.chunk_bytes = 1
    c1, f1 = m(img)
    assert torch.equal(c1, cfeat) and torch.equal(f1, ffeat)
    m.model.chunk_bytes = 512 << 20
    for q in range(3):
        cq, fq = m(img[q:q + 1])
        assert torch.equal(cq[0], cfeat[q]) and torch.equal(fq[0], ffeat[q]), q


@pytest.mark.parametrize("kind,shape", [("c2f", (3, 3, 33, 37)), ("coarse", (3, 3, 37, 41))])
def test_backbone_odd_sides_one_image_per_chunk(gpu, built_lib, native_only, kind, shape):
    """H W odd: image q of the batch starts 3 H W floats in, which is no multiple of 16 bytes for q = 1, 2 -- the chunked forward hands
    such slices to the stem's patch gather.  One image per chunk against float64, against the unchunked batch, against q alone, and for a
    whole batch that itself sits at an odd float offset of its buffer."""
    assert (shape[2] * shape[3]) % 4 and (3 * shape[2] * shape[3]) % 4
    state, img, f_ref, c_ref = cu.case(kind, shape)
    m = load_ms(state, gpu) if kind == "c2f" else load_mini(state, gpu)
    st = m.model if kind == "c2f" else m
    x = img.to(gpu)
    maps = lambda out: {"c": out[0], "f": out[1]} if kind == "c2f" else {"c": out[0]}
    whole = maps(m(x))
    st.chunk_bytes = 1
    single = maps(m(x))
    errs = {k: cu.scaled_err(v, c_ref if k == "c" else f_ref) for k, v in single.items()}
    print(f"backbone {kind} {shape}, one image per chunk: " + ", ".join(f"{k}feat err {e:.2e}" for k, e in errs.items()))
    assert all(e <= cu.TOL for e in errs.values())
    for k in whole:
        assert torch.equal(single[k], whole[k]), k
    for q in range(shape[0]):
        alone = maps(m(x[q:q + 1]))  # (a view: its data pointer is the slice's)
        for k in whole:
            assert torch.equal(alone[k][0], whole[k][q]), (k, q)
    buf = torch.empty(x.numel() + 1, device=gpu)
    shifted = buf[1:].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    st.chunk_bytes = 512 << 20
    for k, v in maps(m(shifted)).items():
        assert torch.equal(v, whole[k]), k


def test_conv_patches_nchw_slice_at_any_float(gpu, built_lib):
    """The NCHW gather reads single floats: a batch slice 3 * 33 * 37 floats into its buffer is taken as it is."""
    x = randn((3, 3, 33, 37), 6)
    xd = x.to(gpu)
    for q in (1, 2):
        assert xd[q:q + 1].data_ptr() % 16
        got, (Ho, Wo) = ops.conv_patches(xd[q:q + 1], 7, 2, 3, 152)
        unf = F.unfold(x[q:q + 1], 7, padding=3, stride=2)
        want = F.pad(unf.view(1, 3, 7, 7, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(Ho * Wo, 147), (0, 5))
        assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------------------------ wiring
def matcher_inputs(gpu, B, n, seed=31):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, 64, 64, generator=g)
    pt_feat = torch.relu(torch.randn(B, n, 256, generator=g))
    pt3d = torch.randn(B, n, 3, generator=g) * 2
    return img.to(gpu), pt_feat.to(gpu), pt3d.to(gpu)


def make_matcher(kind, backbone, gpu):
    cls = NeRFMatcherMS if kind == "c2f" else NeRFMatcherCoarse
    m = cls(synth.matcher_config(kind, backbone=backbone))
    res = m.load_state_dict(synth.matcher_state_dict(kind), strict=False)
    assert not res.unexpected_keys
    if backbone != "stub":
        m.backbone.load_state_dict(synth.backbone_state_dict(0, kind), strict=True)
    return m.to(gpu).eval()


@pytest.mark.parametrize("kind", ["c2f", "coarse"])
def test_matcher_runs_the_native_backbone(gpu, built_lib, native_only, kind):
    """The matcher built with backbone='convformer' returns the bits of the same matcher fed the native backbone's maps."""
    img, pt_feat, pt3d = matcher_inputs(gpu, 1, 64)
    m = make_matcher(kind, "convformer", gpu)
    got = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)
    outs = m.backbone(img)
    fed = make_matcher(kind, "stub", gpu)
    fed.backbone = PrecomputedBackbone(tuple(outs) if kind == "c2f" else outs[0], [256, 128] if kind == "c2f" else 256)
    want = fed.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)
    for a, b in zip(got["match_ids"], want["match_ids"]):
        assert torch.equal(a, b)
    keys = ("conf_matrix", "mconf", "im_cfeat", "pt_cfeat") + (("expec_f",) if kind == "c2f" else ())
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["conf_matrix"]).all())


@pytest.mark.parametrize("kind", ["c2f", "coarse"])
def test_matcher_inference_stays_native_with_grad_mode_on(gpu, built_lib, native_only, kind):
    """Parameters require grad by default and callers do not always wrap inference in no_grad: the matcher records autograd only inside
    autograd.training(), so its backbone call stays on the kernels (native_only raises otherwise) and returns the no_grad bits."""
    img, pt_feat, pt3d = matcher_inputs(gpu, 1, 64)
    m = make_matcher(kind, "convformer", gpu)
    want = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"]
    with torch.enable_grad():
        assert any(p.requires_grad for p in m.backbone.parameters())
        got = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"]
    assert torch.equal(got, want) and not got.requires_grad


def test_stale_backbone_weights_are_noticed(gpu, built_lib, native_only):
    """A write through `.data` changes neither data_ptr nor _version, the keys of the cached (49, C) copy; the matcher's parameter
    fingerprint covers the backbone, so the next pass repeats on fresh copies and its result moves."""
    img, pt_feat, pt3d = matcher_inputs(gpu, 1, 64)
    m = make_matcher("c2f", "convformer", gpu)
    first = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"].clone()
    again = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"]
    assert torch.equal(first, again)
    m.backbone.model.stages_0.blocks[0].token_mixer.dwconv.weight.data.mul_(1.5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        second = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"]
    assert not torch.equal(first, second)
    assert any("modified in place" in str(x.message) for x in w)
    fresh = make_matcher("c2f", "convformer", gpu)
    fresh.backbone.model.stages_0.blocks[0].token_mixer.dwconv.weight.data.mul_(1.5)
    assert torch.equal(second, fresh.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"])


def test_reference_checkpoint_loads_with_its_backbone(gpu, built_lib, tmp_path):
    """Hyper-parameters as the shipped yamls write them (backbone 'convformer384', pretrained: true) and `model.backbone.model.*`
    tensors: load_nerfmatch_from_ckpt leaves no backbone key over, and the weights are the checkpoint's."""
    from nerfmatch_amd.nerfmatch_evaluator import load_nerfmatch_from_ckpt

    cfg = synth.matcher_config("c2f", backbone="convformer384")
    cfg.pretrained = True
    bsd = synth.backbone_state_dict(2, "c2f")
    msd = {f"model.{k}": v for k, v in synth.matcher_state_dict("c2f").items()}
    msd.update({f"model.backbone.{k}": v for k, v in bsd.items()})
    hp = vars(Namespace(model=cfg, exp=Namespace(seed=1), data=Namespace()))
    torch.save(dict(state_dict=msd, hyper_parameters=hp, epoch=1, global_step=2), tmp_path / "m.ckpt")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev = load_nerfmatch_from_ckpt(str(tmp_path / "m.ckpt"))
    assert isinstance(ev.model.backbone.model, ConvFormerStages)
    for k, v in bsd.items():
        assert torch.equal(ev.model.backbone.state_dict()[k].cpu(), v), k
    msd["model.backbone.model.stages_0.blocks.0.layer_scale1.scale"] = torch.ones(128)
    torch.save(dict(state_dict=msd, hyper_parameters=hp, epoch=1, global_step=2), tmp_path / "bad.ckpt")
    with pytest.raises(RuntimeError):
        load_nerfmatch_from_ckpt(str(tmp_path / "bad.ckpt"))
