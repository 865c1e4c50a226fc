"""GPU: the kernels of the backbone's fp16 inference walk (nm_linear_f16, nm_layernorm_f16, nm_dwconv7_nhwc_f16, nm_conv_patches_f16), the
walk built on them (`inference_precision = "fp16"`), its loud overflow, and its wiring into the matchers.

References are computed on the CPU in float64 (tests/convformer_util.py, tests/convformer_f16_util.py); the exact tests compare with the
fp32 kernels' results rounded by torch."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import convformer_f16_util as fu
import convformer_util as cu
from nerfmatch_amd import _lib, ops, synth
from nerfmatch_amd.matcher import NeRFMatcherCoarse, NeRFMatcherMS
from nerfmatch_amd.modules import init_backbone, init_backbone_8_2
from nerfmatch_amd.modules.convformer import ConvFormerStages

pytestmark = pytest.mark.gpu

TH, TW = _lib.NM_DWCONV_TILE_H, _lib.NM_DWCONV_TILE_W
F16, F32 = torch.float16, torch.float32


def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


@pytest.fixture
def native_only(monkeypatch):
    """The plain-torch path must not be what answers on the device."""
    def boom(self, img):
        raise AssertionError("the plain-torch path ran on a device tensor without autograd")
    monkeypatch.setattr(ConvFormerStages, "_forward_torch", boom)


# ------------------------------------------------------------------------------------------------------------------ nm_linear_f16
# (K, N, epilogue) of every GEMM of the walk: pwconv1 stores fp16, fc1 stores StarReLU(.) as fp16, pwconv2 / fc2 add the fp32 residual,
# the stem (147 patch columns in a row pitch of 152) and the downsample convolution add their bias and write fp32
LAYERS = [(128, 256, "f16"), (256, 128, "f32_res"), (128, 512, "f16_star"), (512, 128, "f32_res"),
          (256, 512, "f16"), (512, 256, "f32_res"), (256, 1024, "f16_star"), (1024, 256, "f32_res"),
          (152, 128, "f32_bias"), (1152, 256, "f32_bias")]
MS_ROWS = (1, 127, 128, 129, 257)
STAR = (0.83, -0.41)


def linear_case(K, N, epi, seed=0):
    """fp16 rows x (257, K), fp32 weight / bias / residual, and for the first 257 rows the float64 result of the fp16-rounded operands with
    its pointwise bound.
      accumulator (bias included)   v:  |v^ - v| <= Ev = (K + 8) 2^-24 (sum |a||w| + |bias|)        (fp32 accumulation of exact products)
      StarReLU f(v) = s relu(v)^2 + b, op for op in fp32 (r = relu(v), three roundings: r r, s t, t + b):
          relu is 1-Lipschitz, so |r^ - r| <= Ev and |r^2^ - r^2| <= (2 r + Ev) Ev;  each rounding adds at most 2^-24 of a value bounded by
          |s| (r + Ev)^2 + |b|: Ef = |s| (2 r + Ev) Ev + 4 2^-24 (|s| (r + Ev)^2 + |b|)            (4: the three roundings and second order)
      fp32 output with residual:        E = (K + 8) 2^-24 (sum |a||w| + |bias| + |res|)             (the residual add is one more rounding)
      fp16 output:                      E + 2^-11 |ref| + 2^-25                                      (one rounding; 2^-25: half a subnormal step)"""
    x16 = randn((257, K), 10 + seed).to(F16)
    w = randn((N, K), 20 + seed) / K ** 0.5
    bias = randn((N,), 30 + seed) if epi == "f32_bias" else None
    res = randn((257, N), 40 + seed) if epi == "f32_res" else None
    a, wd = x16.double(), w.to(F16).double()
    v = a @ wd.t()
    mag = a.abs() @ wd.abs().t()
    if bias is not None:
        v, mag = v + bias.double(), mag + bias.double().abs()
    if res is not None:
        mag = mag + res.double().abs()
    ev = (K + 8) * 2.0 ** -24 * mag
    if epi == "f16_star":
        s, b = STAR
        r = v.clamp_min(0)
        ref = s * r ** 2 + b
        bound = abs(s) * (2 * r + ev) * ev + 4 * 2.0 ** -24 * (abs(s) * (r + ev) ** 2 + abs(b))
    else:
        ref, bound = (v + res.double() if res is not None else v), ev
    if epi.startswith("f16"):
        bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    return x16, w, bias, res, ref, bound


def run_linear(gpu, x16, w, bias, res, epi, events=None):
    dev = lambda t: None if t is None else t.to(gpu)
    star = tuple(torch.tensor([v], device=gpu) for v in STAR) if epi == "f16_star" else None
    return ops.linear_f16(dev(x16), w, dev(bias), dev(res), star, F16 if epi.startswith("f16") else F32, events)


@pytest.mark.parametrize("K,N,epi", LAYERS)
def test_linear_f16_against_float64(gpu, built_lib, K, N, epi):
    x16, w, bias, res, ref, bound = linear_case(K, N, epi)
    wd = w.to(gpu)
    events = ops.f16_events(gpu)
    for M in MS_ROWS:
        got = run_linear(gpu, x16[:M], wd, bias, None if res is None else res[:M], epi, events)
        assert got.dtype == (F16 if epi.startswith("f16") else F32) and tuple(got.shape) == (M, N)
        err = (got.cpu().double() - ref[:M]).abs()
        worst = float((err / bound[:M]).max())
        print(f"linear_f16 K {K} N {N} {epi} M {M}: max err {float(err.max()):.2e}, worst err / bound {worst:.3f}")
        assert bool((err <= bound[:M]).all()), M
    assert int(events.item()) == 0


@pytest.mark.parametrize("K,N,epi", [(256, 1024, "f16_star"), (512, 128, "f32_res"), (1152, 256, "f32_bias"), (152, 128, "f32_bias"), (128, 256, "f16")])
def test_linear_f16_rows_do_not_depend_on_m(gpu, built_lib, K, N, epi):
    x16, w, bias, res, _, _ = linear_case(K, N, epi, seed=1)
    wd = w.to(gpu)
    cut = lambda t, a, b: None if t is None else t[a:b]
    whole = run_linear(gpu, x16, wd, bias, res, epi)
    for a, b in ((0, 129), (128, 257)):
        assert torch.equal(whole[a:b], run_linear(gpu, x16[a:b], wd, bias, cut(res, a, b), epi)), (a, b)
    for m in (0, 31, 127, 128, 200, 256):
        assert torch.equal(whole[m:m + 1], run_linear(gpu, x16[m:m + 1], wd, bias, cut(res, m, m + 1), epi)), m


def test_linear_f16_overflow_is_loud_and_counted(gpu, built_lib):
    """No saturation: a sum beyond the fp16 range is stored as infinity and counted; a large NEGATIVE pre-activation is StarReLU's `bias`."""
    x16 = torch.full((3, 128), 16.0, dtype=F16, device=gpu)
    w = torch.zeros(256, 128, device=gpu)
    w[0], w[1], w[2] = 64.0, -64.0, 1.0  # sums: 131072, -131072, 2048
    events = ops.f16_events(gpu)
    y = ops.linear_f16(x16, w, events=events).cpu()
    assert bool((y[:, 0] == float("inf")).all()) and bool((y[:, 1] == float("-inf")).all()) and bool((y[:, 2] == 2048).all())
    assert bool((y[:, 3:] == 0).all()) and int(events.item()) == 6
    star = (torch.tensor([1.0], device=gpu), torch.tensor([0.25], device=gpu))
    events.zero_()
    y = ops.linear_f16(x16, w, star=star, events=events).cpu()
    assert bool((y[:, 0] == float("inf")).all()) and bool((y[:, 1] == 0.25).all()) and bool((y[:, 3:] == 0.25).all())
    assert bool((y[:, 2] == float("inf")).all()) and int(events.item()) == 6  # 2048^2 is beyond the range too
    y32 = ops.linear_f16(x16, w, out_dtype=F32, events=events).cpu()  # fp32 rows hold the sums: nothing to count
    assert bool((y32[:, 0] == 131072).all()) and int(events.item()) == 6


def test_linear_f16_sees_a_changed_weight(gpu, built_lib):
    """The fp16 blob is cached on the weight's (data_ptr, _version), like the split-bf16 blobs: an in-place write and a replaced tensor are
    both seen.  (A write through `.data` changes neither key: the matcher's parameter fingerprint covers it, see
    test_stale_fp16_backbone_weights_are_noticed.)"""
    x16 = randn((40, 128), 1).to(F16).to(gpu)
    w = (randn((256, 128), 2) * 0.1).to(gpu)
    first = ops.linear_f16(x16, w)
    assert torch.equal(first, ops.linear_f16(x16, w))
    w.mul_(2.0)  # exact in fp16 and fp32: every sum doubles
    second = ops.linear_f16(x16, w)
    assert torch.equal(second.float(), (first.float() * 2).to(F16).float()) and not torch.equal(first, second)
    w2 = w.clone().neg_()
    assert torch.equal(ops.linear_f16(x16, w2), -second)
    with pytest.raises(_lib.NerfmatchAmdError):
        ops.linear_f16(x16, w, residual=torch.zeros(40, 256, device=gpu))  # a residual needs fp32 output
    with pytest.raises(_lib.NerfmatchAmdError):
        ops.linear_f16(x16.float(), w)  # fp16 rows in


# ------------------------------------------------------------------------------------------------------------------ nm_layernorm_f16
@pytest.mark.parametrize("rows,dim", [(1, 128), (5, 256), (1001, 128), (1001, 256), (7, 512)])
def test_layernorm_f16_is_layernorm_rounded(gpu, built_lib, rows, dim):
    x = (randn((rows, dim), rows) * 3 + 0.5).to(gpu)
    gamma, beta = (randn((dim,), 2) + 1).to(gpu), (randn((dim,), 3) * 0.1).to(gpu)
    events = ops.f16_events(gpu)
    got = ops.layernorm_f16(x, gamma, beta, 1e-6, events=events)
    assert got.dtype == F16 and torch.equal(got, ops.layernorm(x, gamma, beta, 1e-6).to(F16))
    assert int(events.item()) == 0
    gamma[1::3] *= 3e4  # beyond the fp16 range: infinities, the same ones, and counted
    got, want = ops.layernorm_f16(x, gamma, beta, 1e-6, events=events), ops.layernorm(x, gamma, beta, 1e-6)
    assert torch.equal(got, want.to(F16)) and bool(torch.isfinite(want).all())
    n_inf = int(torch.isinf(got).sum())
    assert n_inf > 0 and int(events.item()) == n_inf


# ------------------------------------------------------------------------------------------------------------------ nm_dwconv7_nhwc_f16
@pytest.mark.parametrize("shape", [(1, 1, 1, 64), (1, TH, TW, 64), (1, TH + 1, TW + 1, 64), (2, 7, 9, 256), (1, 13, 2 * TW + 3, 128)])
@pytest.mark.parametrize("act", [False, True])
def test_dwconv7_f16_is_dwconv7_rounded(gpu, built_lib, shape, act):
    x16 = (randn(shape, 3) * 2).to(F16).to(gpu)
    w = (randn((shape[3], 1, 7, 7), 4) * 0.3).to(gpu)
    sb = (torch.tensor([0.9], device=gpu), torch.tensor([-0.35], device=gpu)) if act else (None, None)
    events = ops.f16_events(gpu)
    got = ops.dwconv7_nhwc_f16(x16, w, *sb, events=events)
    assert got.dtype == F16 and torch.equal(got, ops.dwconv7_nhwc(x16.float(), w, *sb).to(F16))
    assert bool(torch.isfinite(got).all()) and int(events.item()) == 0


@pytest.mark.parametrize("act", [False, True])
def test_dwconv7_f16_no_bleed_between_images(gpu, built_lib, act):
    H, W, Cc = TH + 2, 5, 64
    w = randn((Cc, 1, 7, 7), 8).to(gpu)
    sb = (torch.tensor([0.9], device=gpu), torch.tensor([-0.35], device=gpu)) if act else (None, None)
    pair = torch.zeros(2, H, W, Cc, device=gpu, dtype=F16)
    pair[1] = 100.0
    both = ops.dwconv7_nhwc_f16(pair, w, *sb)
    assert torch.equal(both[:1], ops.dwconv7_nhwc_f16(pair[:1].contiguous(), w, *sb))
    assert torch.equal(both[1:], ops.dwconv7_nhwc_f16(pair[1:].contiguous(), w, *sb))
    assert torch.equal(both, ops.dwconv7_nhwc(pair.float(), w, *sb).to(F16))


def test_dwconv7_f16_overflow_is_counted(gpu, built_lib):
    x16 = torch.full((1, 3, 3, 64), 300.0, dtype=F16, device=gpu)
    w = torch.ones(64, 1, 7, 7, device=gpu)
    one = torch.ones(1, device=gpu)
    events = ops.f16_events(gpu)
    y = ops.dwconv7_nhwc_f16(x16, w, one, one, events=events)  # 9 taps x (300^2 + 1) = 810009
    assert bool(torch.isinf(y).all()) and int(events.item()) == y.numel()
    assert bool((ops.dwconv7_nhwc_f16(x16, w, events=events) == 2700).all()) and int(events.item()) == y.numel()


# ------------------------------------------------------------------------------------------------------------------ nm_conv_patches_f16
@pytest.mark.parametrize("layout,shape,k,s,p,ld", [(0, (2, 3, 30, 22), 7, 2, 3, 152), (0, (1, 3, 33, 37), 7, 4, 2, 152),
                                                   (1, (2, 12, 20, 128), 3, 4, 1, 1152), (1, (1, 5, 7, 128), 3, 2, 1, 1152)])
def test_conv_patches_f16_is_conv_patches_rounded(gpu, built_lib, layout, shape, k, s, p, ld):
    x = randn(shape, 5).to(gpu)
    if layout:
        x = x.to(F16)
    want, hw = ops.conv_patches(x.float(), k, s, p, ld, channel_last=bool(layout))
    events = ops.f16_events(gpu)
    got, hw16 = ops.conv_patches_f16(x, k, s, p, ld, channel_last=bool(layout), events=events)
    assert hw16 == hw and got.dtype == F16 and torch.equal(got, want.to(F16)) and int(events.item()) == 0
    # into a poisoned buffer: the pad columns are WRITTEN as zero
    rows = torch.full(tuple(got.shape), float("nan"), device=gpu, dtype=F16)
    B, Cc, H, W = (shape[0], shape[3], shape[1], shape[2]) if layout else shape
    _lib.check(_lib.lib().nm_conv_patches_f16(_lib.dptr(x, F16 if layout else F32), layout, B, Cc, H, W, k, s, p, ld, _lib.dptr(rows, F16), None,
                                              ops.stream()), "nm_conv_patches_f16")
    assert torch.equal(rows, want.to(F16))


def test_conv_patches_f16_nchw_slice_at_any_float(gpu, built_lib):
    """The NCHW gather reads single floats: image q of a batch of odd-sized images is taken as it is."""
    xd = randn((3, 3, 33, 37), 6).to(gpu)
    for q in (1, 2):
        assert xd[q:q + 1].data_ptr() % 16
        got = ops.conv_patches_f16(xd[q:q + 1], 7, 2, 3, 152)[0]
        assert torch.equal(got, ops.conv_patches(xd[q:q + 1], 7, 2, 3, 152)[0].to(F16))


# ------------------------------------------------------------------------------------------------------------------ whole backbone
def load_ms(state, gpu, precision="fp16"):
    m = init_backbone_8_2("convformer", precision=precision)
    m.model.load_state_dict(state, strict=True)
    return m.to(gpu).eval()


def load_mini(state, gpu, precision="fp16"):
    m = init_backbone("convformer", downsample=8, precision=precision)
    m.load_state_dict(state, strict=True)
    return m.to(gpu).eval()


@pytest.mark.parametrize("kind,shape", [("c2f", (2, 3, 32, 48)), ("c2f", (2, 3, 26, 38)), ("coarse", (2, 3, 64, 72))])
def test_backbone_fp16_against_float64_and_its_emulation(gpu, built_lib, native_only, kind, shape):
    """The yardstick is the emulation's own error against float64 on the same case: the kernels add fp32 accumulation order and the fp16
    roundings that flip with it, so 1.5 x that error bounds both the scaled maximum and the relative rms error of each map."""
    state, img, f_ref, c_ref = cu.case(kind, shape)
    f_em, c_em = fu.emulated(kind, shape)
    if kind == "c2f":
        m = load_ms(state, gpu)
        cfeat, ffeat = m(img.to(gpu))
        stages, maps = m.model, [("ffeat", ffeat, f_ref, f_em), ("cfeat", cfeat, c_ref, c_em)]
    else:
        m = load_mini(state, gpu)
        out = m(img.to(gpu))
        assert isinstance(out, list) and len(out) == 1
        stages, maps = m, [("cfeat", out[0], c_ref, c_em)]
    for name, got, ref, em in maps:
        assert tuple(got.shape) == tuple(ref.shape) and got.is_contiguous() and got.dtype == F32
        assert bool(torch.isfinite(got).all())
        e_max, e_rms = cu.scaled_err(got, ref), fu.rel_rms(got, ref)
        y_max, y_rms = cu.scaled_err(em, ref), fu.rel_rms(em, ref)
        print(f"backbone fp16 {kind} {shape} {name}: max of scale {e_max:.3e} (emulation {y_max:.3e}, ratio {e_max / y_max:.3f}), "
              f"rel. rms {e_rms:.3e} (emulation {y_rms:.3e}, ratio {e_rms / y_rms:.3f}); kernels against emulation: max of scale "
              f"{cu.scaled_err(got, em):.3e}")
        assert e_max <= 1.5 * y_max, name
        assert e_rms <= 1.5 * y_rms, name
    assert stages.overflow_events() == 0


def test_backbone_fp16_batch_invariance(gpu, built_lib, native_only):
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
    assert m.model.overflow_events() == 0


def test_backbone_same_is_the_untouched_walk(gpu, built_lib, native_only):
    """`inference_precision = "same"` -- the default, or set back from "fp16" -- gives the bits of a module that never heard of the switch,
    and "fp16" gives other bits (it is another arithmetic, not a relabelling)."""
    state, img, _, _ = cu.case("c2f", (2, 3, 32, 48))
    x = img.to(gpu)
    plain = init_backbone_8_2("convformer")
    plain.model.load_state_dict(state, strict=True)
    c0, f0 = plain.to(gpu).eval()(x)
    m = load_ms(state, gpu, "same")
    c1, f1 = m(x)
    assert torch.equal(c1, c0) and torch.equal(f1, f0)
    m.model.inference_precision = "fp16"
    c2, f2 = m(x)
    assert not torch.equal(c2, c0) and not torch.equal(f2, f0)
    m.model.inference_precision = "same"
    c3, f3 = m(x)
    assert torch.equal(c3, c0) and torch.equal(f3, f0)


def test_backbone_fp16_overflow_is_loud(gpu, built_lib, native_only):
    """One StarReLU scale times 1e7 drives fc1's activations out of the fp16 range: they are stored as infinity, the maps carry inf / NaN,
    and the counter says where it came from.  (A numerical check: nothing here faults.)"""
    state, img, _, _ = cu.case("c2f", (2, 3, 32, 48))
    m = load_ms(state, gpu)
    m(img.to(gpu))
    assert m.model.overflow_events() == 0
    m.model.stages_0.blocks[1].mlp.act.scale.mul_(1e7)
    cfeat, ffeat = m(img.to(gpu))
    assert not bool(torch.isfinite(ffeat).all()) and not bool(torch.isfinite(cfeat).all())
    assert m.model.overflow_events() > 0


# ------------------------------------------------------------------------------------------------------------------ wiring
def matcher_inputs(gpu, B, n, seed=31):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, 64, 64, generator=g)
    pt_feat = torch.relu(torch.randn(B, n, 256, generator=g))
    pt3d = torch.randn(B, n, 3, generator=g) * 2
    return img.to(gpu), pt_feat.to(gpu), pt3d.to(gpu)


def make_matcher(kind, gpu, precision="fp16"):
    cfg = synth.matcher_config(kind, backbone="convformer")
    if precision is not None:
        cfg.backbone_precision = precision
    m = (NeRFMatcherMS if kind == "c2f" else NeRFMatcherCoarse)(cfg)
    res = m.load_state_dict(synth.matcher_state_dict(kind), strict=False)
    assert not res.unexpected_keys
    m.backbone.load_state_dict(synth.backbone_state_dict(0, kind), strict=True)
    return m.to(gpu).eval()


@pytest.mark.parametrize("kind", ["c2f", "coarse"])
def test_matcher_runs_the_fp16_walk(gpu, built_lib, native_only, monkeypatch, kind):
    """A matcher built with `backbone_precision: fp16` sends its images through the fp16 walk -- every GEMM of the backbone is a call of
    ops.linear_f16 (stem, downsample, four per block) -- and one built without the key through none."""
    calls = []
    real = ops.linear_f16
    monkeypatch.setattr(ops, "linear_f16", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    img, pt_feat, pt3d = matcher_inputs(gpu, 1, 64)
    got = make_matcher(kind, gpu).forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)
    assert len(calls) == 2 + 4 * (3 + 12)
    assert bool(torch.isfinite(got["conf_matrix"]).all())
    del calls[:]
    want = make_matcher(kind, gpu, None).forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)
    assert not calls
    assert not torch.equal(got["im_cfeat"], want["im_cfeat"])


def test_stale_fp16_backbone_weights_are_noticed(gpu, built_lib, native_only):
    """A write through `.data` changes neither data_ptr nor _version, the keys of the cached fp16 blob; the matcher's parameter fingerprint
    covers the backbone, so the next pass repeats on fresh blobs -- exactly as for the split-bf16 blobs -- and does not return the old
    blob's result."""
    img, pt_feat, pt3d = matcher_inputs(gpu, 1, 64)
    m = make_matcher("c2f", gpu)
    first = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"].clone()
    assert torch.equal(first, m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"])
    m.backbone.model.stages_0.blocks[0].mlp.fc1.weight.data.mul_(1.5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        second = m.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"]
    assert not torch.equal(first, second)
    assert any("modified in place" in str(x.message) for x in w)
    fresh = make_matcher("c2f", gpu)
    fresh.backbone.model.stages_0.blocks[0].mlp.fc1.weight.data.mul_(1.5)
    assert torch.equal(second, fresh.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)["im_cfeat"])
