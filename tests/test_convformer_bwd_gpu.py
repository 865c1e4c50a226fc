"""GPU: the backward kernels of csrc/convformer_bwd.hip, the recording path of the ConvFormer stages built on them, and its wiring
into the matchers and the trainer.

References are float64 on the CPU (tests/convformer_bwd_util.py for the whole backbone); the torch device convolutions run only where a
test is about the plain-torch path itself (dispatch)."""
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convformer_bwd_util as bu
import convformer_util as cu
from nerfmatch_amd import _lib, autograd as ag, ops, synth
from nerfmatch_amd.matcher import NeRFMatcherCoarse, NeRFMatcherMS
from nerfmatch_amd.modules.convformer import ConvFormerStages

pytestmark = pytest.mark.gpu

TH, TW = _lib.NM_DWCONV_TILE_H, _lib.NM_DWCONV_TILE_W
U = 2.0 ** -24


def randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def randint(lo, hi, shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.fixture
def native_only(monkeypatch):
    """The plain-torch path must not be what answers."""
    def boom(self, img):
        raise AssertionError("the plain-torch path ran where the recording path on the kernels was expected")
    monkeypatch.setattr(ConvFormerStages, "_forward_torch", boom)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def dw_reference(x, w, dy, scale, bias):
    """float64 gradients of y = dwconv7(a(x)) against dy from fp32 inputs x, dy (B,H,W,C) and w (C,1,7,7), with the sums of absolute
    terms that the bounds need: dict(da, dx, g = 2 scale r, da_abs = sum_t |w||dy|, dw (49,C), dw_abs, ds, ds_abs, db, db_abs)."""
    xd, wd, dyd = nchw(x).double(), w.double(), nchw(dy).double()
    Cc = wd.shape[0]
    da = F.conv_transpose2d(dyd, wd, padding=3, groups=Cc)
    da_abs = F.conv_transpose2d(dyd.abs(), wd.abs(), padding=3, groups=Cc)
    r = torch.clamp(xd, min=0)
    if scale is None:
        a, g = xd, torch.ones_like(xd)
    else:
        a, g = float(scale) * r ** 2 + float(bias), 2 * float(scale) * r
    with torch.enable_grad():
        wl = wd.clone().requires_grad_(True)
        dw, = torch.autograd.grad((F.conv2d(a, wl, padding=3, groups=Cc) * dyd).sum(), wl)
        wl = wd.clone().requires_grad_(True)
        dw_abs, = torch.autograd.grad((F.conv2d(a.abs(), wl, padding=3, groups=Cc) * dyd.abs()).sum(), wl)
    t49 = lambda t: t.reshape(Cc, 49).t()
    return dict(da=nhwc(da), dx=nhwc(da * g), g=nhwc(g), da_abs=nhwc(da_abs), dw=t49(dw), dw_abs=t49(dw_abs), ds=(da * r ** 2).sum(),
                ds_abs=(da * r ** 2).abs().sum(), db=da.sum(), db_abs=da.abs().sum())


def dw_run(gpu, x, w, dy, scale, bias, need=(True, True, True)):
    sb = (None, None) if scale is None else (torch.tensor([scale]).to(gpu), torch.tensor([bias]).to(gpu))
    return ops.dwconv7_nhwc_bwd(dy.to(gpu), x.to(gpu), ops.dwconv_weight_taps(w.to(gpu)), *sb, need=need)


# ---------------------------------------------------------------------------------------------- 1. depthwise input gradient, float64
DW_SHAPES = [(1, 1, 1, 64), (2, 2, 3, 256), (2, 7, 9, 256), (1, 3, 40, 64), (1, TH, TW, 64), (1, TH + 1, TW + 1, 64),
             (2, 2 * TH + 3, TW - 1, 128)]


@pytest.mark.parametrize("shape", DW_SHAPES)
@pytest.mark.parametrize("act", [False, True])
def test_dwconv7_bwd_input_against_float64(gpu, built_lib, shape, act):
    """|err| <= 56 2^-24 (sum_t |w||dy|) |2 scale r(x)| (without the activation: the sum alone): the forward test's constant -- 49 fused
    steps, the epilogue's roundings, room for second-order terms."""
    x, w, dy = randn(shape, 3) * 2, randn((shape[3], 1, 7, 7), 4) * 0.3, randn(shape, 5)
    scale, bias = (0.9, -0.35) if act else (None, None)
    ref = dw_reference(x, w, dy, scale, bias)
    dx, _, _ = dw_run(gpu, x, w, dy, scale, bias, need=(True, False, False))
    err = (dx.cpu().double() - ref["dx"]).abs()
    bound = 56 * U * ref["da_abs"] * ref["g"].abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"dwconv7 bwd input {shape} act={act}: max err {float(err.max()):.2e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------- 2. exact integers
@pytest.mark.parametrize("shape", [(2, TH + 1, TW + 1, 64), (2, 2 * TH + 3, TW - 1, 128)])
def test_dwconv7_bwd_exact_integers(gpu, built_lib, shape):
    """x in {-1,0,1,2}, dy in {-1,0,1}, w in {-1,0,1,2}, scale = bias = 1: every sum is an integer below 2^24, so dx, dw49c, dscale and
    dbias equal the float64 values whatever the order of addition -- a lost term, a tile seam or a padded pixel counted with `bias`
    shows as a whole number."""
    x, dy, w = randint(-1, 2, shape, 1), randint(-1, 1, shape, 2), randint(-1, 2, (shape[3], 1, 7, 7), 3)
    ref = dw_reference(x, w, dy, 1.0, 1.0)
    assert max(float(ref["ds_abs"]), float(ref["db_abs"]), float(ref["dw_abs"].max())) < 2 ** 24
    dx, dw, dsb = dw_run(gpu, x, w, dy, 1.0, 1.0)
    assert torch.equal(dx.cpu().double(), ref["dx"])
    assert torch.equal(dw.cpu().double(), ref["dw"])
    assert float(dsb[0]) == float(ref["ds"]) and float(dsb[1]) == float(ref["db"])
    # without the activation: dx = da, and dw sums dy x with zeros outside
    ref = dw_reference(x, w, dy, None, None)
    dx, dw, dsb = dw_run(gpu, x, w, dy, None, None)
    assert dsb is None and torch.equal(dx.cpu().double(), ref["da"]) and torch.equal(dw.cpu().double(), ref["dw"])


@pytest.mark.parametrize("n", [1, 63, 257, 2 ** 20 + 3])
def test_star_relu_bwd_exact_integers(gpu, built_lib, n):
    x, dy = randint(-1, 2, (n,), n), randint(-1, 1, (n,), n + 1)
    r = torch.relu(x).double()
    dx, dsb = ops.star_relu_bwd(x.to(gpu), dy.to(gpu), torch.ones(1, device=gpu))
    assert torch.equal(dx.cpu().double(), dy.double() * 2 * r)
    assert float(dsb[0]) == float((dy.double() * r ** 2).sum()) and float(dsb[1]) == float(dy.double().sum())
    dx2, none = ops.star_relu_bwd(x.to(gpu), dy.to(gpu), torch.ones(1, device=gpu), need_params=False)
    assert none is None and torch.equal(dx2, dx)


# ---------------------------------------------------------------------------------------------- 3. random inputs: the reductions
@pytest.mark.parametrize("shape", [(2, 17, 33, 64), (1, 13, 17, 128)])
def test_dwconv7_bwd_reductions_against_float64(gpu, built_lib, shape):
    """|err| <= (n + 8) 2^-24 sum|terms| with n the number of terms of the sum: any order of fp32 addition stays inside.  For the two
    scalars n = B H W C and the bound is loose -- a check of magnitude; the exact-integer test counts their terms."""
    x, w, dy = randn(shape, 13) * 2, randn((shape[3], 1, 7, 7), 14) * 0.3, randn(shape, 15)
    ref = dw_reference(x, w, dy, 0.9, -0.35)
    _, dw, dsb = dw_run(gpu, x, w, dy, 0.9, -0.35)
    n = shape[0] * shape[1] * shape[2]
    assert n <= 1200
    err = (dw.cpu().double() - ref["dw"]).abs()
    bound = (n + 8) * U * ref["dw_abs"]
    print(f"dwconv7 bwd weight {shape}: max err {float(err.max()):.2e}, worst err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    for name, got, val, mag in (("dscale", dsb[0], ref["ds"], ref["ds_abs"]), ("dbias", dsb[1], ref["db"], ref["db_abs"])):
        e, b = abs(float(got) - float(val)), (n * shape[3] + 8) * U * float(mag)
        print(f"dwconv7 bwd {name} {shape}: {float(got):.6e} vs {float(val):.6e}, err {e:.2e}, bound {b:.2e}, err / sum|terms| {e / float(mag):.2e}")
        assert e <= b


# ---------------------------------------------------------------------------------------------- 4. run-to-run, per image
@pytest.mark.parametrize("act", [False, True])
def test_dwconv7_bwd_same_bits_every_run_and_per_image(gpu, built_lib, act):
    shape = (2, TH + 2, TW + 5, 128)
    x, w, dy = randn(shape, 23) * 2, randn((shape[3], 1, 7, 7), 24) * 0.3, randn(shape, 25)
    sb = (0.9, -0.35) if act else (None, None)
    first = dw_run(gpu, x, w, dy, *sb)
    for _ in range(2):
        again = dw_run(gpu, x, w, dy, *sb)
        for a, b in zip(first, again):
            assert (a is None and b is None) or torch.equal(a, b)
    for b in range(2):
        alone, _, _ = dw_run(gpu, x[b:b + 1], w, dy[b:b + 1], *sb, need=(True, False, False))
        assert torch.equal(first[0][b], alone[0]), b
        loud = dy.clone()
        loud[1 - b] = 1e3
        other, _, _ = dw_run(gpu, x, w, loud, *sb, need=(True, False, False))
        assert torch.equal(first[0][b], other[b]), b


def test_star_relu_bwd_same_bits_every_run(gpu, built_lib):
    n = 3 * 8192 + 5
    x, dy, s = (randn((n,), 31) * 2).to(gpu), randn((n,), 32).to(gpu), torch.tensor([0.83]).to(gpu)
    first = ops.star_relu_bwd(x, dy, s)
    for _ in range(2):
        again = ops.star_relu_bwd(x, dy, s)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    r = torch.relu(x.cpu().double())
    for got, terms in ((first[1][0], dy.cpu().double() * r ** 2), (first[1][1], dy.cpu().double())):
        assert abs(float(got) - float(terms.sum())) <= (n + 8) * U * float(terms.abs().sum())


# ---------------------------------------------------------------------------------------------- 5. nm_star_relu_bwd's dx
@pytest.mark.parametrize("n", [1, 2, 5, 63, 257, 2 * 8192 + 7])
def test_star_relu_bwd_dx_bits(gpu, built_lib, n):
    x, dy = randn((n,), n) * 3, randn((n,), n + 7)
    sp = torch.tensor([-0.0, float("nan"), 0.0, -2.5, 1e-20, float("inf")])
    x[:min(n, len(sp))] = sp[:n]
    if n > 2 * len(sp):
        x[-len(sp):] = sp  # (the scalar tail sees them too)
    scale = torch.tensor([0.83])
    want = dy * (2 * (scale * torch.relu(x)))
    dx, _ = ops.star_relu_bwd(x.to(gpu), dy.to(gpu), scale.to(gpu))
    got = dx.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and bool(nan.any()) == (n >= 2)
    assert torch.equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))


# ---------------------------------------------------------------------------------------------- 6. nm_conv_patches_bwd
def patches_cpu(x, k, s, p):
    """conv_patches of a channel-last x (B,H,W,C) restated with unfold: (B Ho Wo, k k C), columns in (ky, kx, c) order."""
    B, H, W, Cc = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    unf = F.unfold(nchw(x), k, padding=p, stride=s)
    return unf.view(B, Cc, k, k, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(B * Ho * Wo, k * k * Cc)


@pytest.mark.parametrize("shape,k,s,p", [((2, 13, 19, 128), 3, 4, 1), ((2, 13, 19, 128), 3, 2, 1), ((1, 4, 6, 128), 3, 4, 1)])
def test_conv_patches_bwd_is_the_exact_adjoint(gpu, built_lib, shape, k, s, p):
    kkc = k * k * shape[3]
    ld = kkc + 8
    with torch.enable_grad():
        xl = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        rows = patches_cpu(xl, k, s, p)
        drows = randint(-3, 3, (rows.shape[0], ld), 41)
        drows[:, kkc:] = 1e3  # the columns from k k C on are not read
        want, = torch.autograd.grad((rows * drows[:, :kkc].double()).sum(), xl)
    got = ops.conv_patches_bwd(drows.to(gpu), shape, k, s, p)
    assert torch.equal(got.cpu().double(), want)
    # <conv_patches(x), r> = <x, conv_patches_bwd(r)> on integers
    x = randint(-3, 3, shape, 42)
    fwd, _ = ops.conv_patches(x.to(gpu), k, s, p, ld, channel_last=True)
    assert float((fwd.cpu().double() * drows.double()).sum()) == float((x.double() * got.cpu().double()).sum())


# ---------------------------------------------------------------------------------------------- 7. whole backbone, float64
BACKBONE_CASES = [("c2f", (2, 3, 32, 48)), ("c2f", (2, 3, 26, 38)), ("coarse", (2, 3, 64, 72))]


def load_stages(kind, state, gpu):
    m = ConvFormerStages(**cu.MS, out_stages=(0, 1)) if kind == "c2f" else ConvFormerStages(**cu.MINI, out_stages=(1,))
    m.load_state_dict(state, strict=True)
    return m.to(gpu)


def train_pass(m, img, cots):
    """Forward inside autograd.training() and backward against the cotangents: (maps, name -> grad)."""
    m.zero_grad(set_to_none=True)
    with torch.enable_grad(), ag.training():
        maps = m(img)
        live = [(o, c.to(img.device)) for o, c in zip(maps, cots) if o.requires_grad]  # (a map below the first trainable tensor records nothing)
        torch.autograd.backward([o for o, _ in live], [c for _, c in live])
    return maps, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind,shape", BACKBONE_CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_backbone_gradients_against_float64(gpu, built_lib, native_only, monkeypatch, kind, shape, precision):
    """Every parameter gradient of the recording path against the float64 restatement: tensors by max|g - ref| / max(1, max|ref|), the
    1-element StarReLU parameters by |g - sum| / sum|contribution|; the bar is the forward backbone's (convformer_util.TOL = 1e-4)."""
    monkeypatch.setattr(ops, "LINEAR_PRECISION", precision)
    state, img, cots, ref = bu.case(kind, shape)
    m = load_stages(kind, state, gpu)
    _, grads = train_pass(m, img.to(gpu), cots)
    assert set(grads) == set(ref) == set(cu.expected_shapes())
    assert all(tuple(g.shape) == tuple(p.shape) for g, p in zip(grads.values(), m.parameters()))
    errs = bu.grad_errors(grads, ref)
    tens = {k: e for k, e in errs.items() if ref[k][1] is None}
    scal = {k: e for k, e in errs.items() if ref[k][1] is not None}
    wt, ws = max(tens, key=tens.get), max(scal, key=scal.get)
    print(f"backbone bwd {kind} {shape} {precision}: worst tensor {wt} {tens[wt]:.2e}, worst StarReLU scalar {ws} {scal[ws]:.2e}")
    assert tens[wt] <= cu.TOL and scal[ws] <= cu.TOL


# ---------------------------------------------------------------------------------------------- 8. forward bits
@pytest.mark.parametrize("kind,shape", BACKBONE_CASES[1:])
def test_recording_forward_returns_the_inference_bits(gpu, built_lib, native_only, kind, shape):
    state, img, cots, _ = bu.case(kind, shape)
    m = load_stages(kind, state, gpu)
    want = m(img.to(gpu))  # (the suite runs under no_grad)
    with torch.enable_grad(), ag.training():
        got = m(img.to(gpu))
    for a, b in zip(got, want):
        assert a.requires_grad and not b.requires_grad and a.is_contiguous() and torch.equal(a.detach(), b)


# ---------------------------------------------------------------------------------------------- 9. dispatch
def test_frozen_backbone_stays_on_the_inference_path(gpu, built_lib, native_only, monkeypatch):
    state, img, _, _ = bu.case("c2f", (2, 3, 26, 38))
    m = load_stages("c2f", state, gpu).requires_grad_(False)
    calls = []
    walk = ConvFormerStages._forward_kernels

    def spy(self, x, recording):
        calls.append(recording)
        return walk(self, x, recording)
    monkeypatch.setattr(ConvFormerStages, "_forward_kernels", spy)
    with torch.enable_grad(), ag.training():
        maps = m(img.to(gpu))
    # the kernel walk ran exactly once, in inference mode and not in recording mode (recorded with every parameter frozen otherwise)
    assert calls == [False] and not any(o.requires_grad for o in maps)


def test_partly_frozen_backbone(gpu, built_lib, native_only):
    """Only stages_1.* trainable: the frozen tensors keep grad None, the others match the float64 reference."""
    state, img, cots, ref = bu.case("c2f", (2, 3, 26, 38))
    m = load_stages("c2f", state, gpu)
    for k, p in m.named_parameters():
        p.requires_grad_(k.startswith("stages_1."))
    maps, grads = train_pass(m, img.to(gpu), cots)
    assert not maps[0].requires_grad and maps[1].requires_grad
    assert set(grads) == {k for k in ref if k.startswith("stages_1.")}
    errs = bu.grad_errors(grads, ref)
    assert max(errs.values()) <= cu.TOL


@pytest.mark.parametrize("how", ["train_native_off", "image_requires_grad", "outside_training"])
def test_everything_else_keeps_the_torch_path(gpu, built_lib, monkeypatch, how):
    """train_native = False, an image that requires grad, a direct call outside autograd.training(): each takes _forward_torch; its maps
    agree with the recording path's within TOL and its gradients with the float64 reference, in the measures of the float64 test."""
    state, img, cots, ref = bu.case("c2f", (2, 3, 26, 38))
    m = load_stages("c2f", state, gpu)
    want, _ = train_pass(m, img.to(gpu), cots)
    calls = []
    plain = ConvFormerStages._forward_torch
    monkeypatch.setattr(ConvFormerStages, "_forward_torch", lambda self, x: calls.append(1) or plain(self, x))
    x = img.to(gpu)
    m.zero_grad(set_to_none=True)
    with torch.enable_grad():
        if how == "train_native_off":
            m.train_native = False
            with ag.training():
                got = m(x)
        elif how == "image_requires_grad":
            with ag.training():
                got = m(x.requires_grad_())
        else:
            got = m(x)
        torch.autograd.backward(got, [c.to(gpu) for c in cots])
    assert calls == [1]
    for a, b in zip(got, want):
        assert cu.scaled_err(a, b.detach().cpu().double()) <= cu.TOL
    errs = bu.grad_errors({k: p.grad for k, p in m.named_parameters()}, ref)
    worst = max(errs, key=errs.get)
    print(f"plain-torch path ({how}): worst gradient {worst} {errs[worst]:.2e}")
    assert errs[worst] <= cu.TOL
    if how == "image_requires_grad":
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())


# ---------------------------------------------------------------------------------------------- 10. matcher and trainer
def train_batch(gpu, B=1, n=64, seed=31):
    """A 64 x 64 image (8 x 8 coarse cells), n points in front of an identity camera that project into it."""
    g = torch.Generator().manual_seed(seed)
    H = W = 64
    uv = torch.rand(B, n, 2, generator=g) * 56 + 4
    z = torch.rand(B, n, 1, generator=g) * 2 + 2
    f = 60.0
    pt3d = torch.cat([(uv - 32) / f * z, z], -1)
    K = torch.tensor([[f, 0, 32.0], [0, f, 32.0], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    ys, xs = torch.meshgrid(torch.arange(H // 8), torch.arange(W // 8), indexing="ij")
    M = (H // 8) * (W // 8)
    d = dict(image=torch.randn(B, 3, H, W, generator=g), im_mask=torch.ones(B, M, dtype=torch.bool), pt_mask=torch.ones(B, n, dtype=torch.bool),
             pt3d=pt3d, pt2d=(torch.stack([xs, ys], -1) * 8 + 4).float().reshape(1, M, 2).expand(B, M, 2).contiguous(),
             pt_feat=torch.relu(torch.randn(B, n, 256, generator=g)), K=K, c2w=torch.eye(4).expand(B, 4, 4).contiguous())
    return {k: v.to(gpu) for k, v in d.items()}


def make_matcher(kind, gpu):
    cls = NeRFMatcherMS if kind == "c2f" else NeRFMatcherCoarse
    m = cls(synth.matcher_config(kind, backbone="convformer"))
    res = m.load_state_dict(synth.matcher_state_dict(kind), strict=False)
    assert not res.unexpected_keys
    m.backbone.load_state_dict(synth.backbone_state_dict(0, kind), strict=True)
    return m.to(gpu)


@pytest.mark.parametrize("kind", ["c2f", "coarse"])
def test_matcher_trains_its_backbone_on_the_kernels(gpu, built_lib, native_only, kind):
    from nerfmatch_amd import supervision as sup

    m = make_matcher(kind, gpu)
    data = train_batch(gpu)
    np.random.seed(3)
    with torch.enable_grad():
        sup.supervise_batch(m, data)
        metrics = m.forward_with_metrics(data, training=True)
        assert bool(torch.isfinite(metrics["loss"]))
        metrics["loss"].backward()
    bb = dict(m.backbone.named_parameters())
    assert len(bb) == len(cu.expected_shapes())
    missing = [k for k, p in bb.items() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing
    stem = bb["model.stem.conv.weight" if kind == "c2f" else "stem.conv.weight"]
    assert float(stem.grad.abs().max()) > 0


def test_trainer_step_moves_the_stem(gpu, built_lib, native_only):
    from nerfmatch_amd.trainer import NeRFMatchMSTrainer

    optim = Namespace(lr=0.0004, coarse_only_epochs=0)
    tr = NeRFMatchMSTrainer(Namespace(model=synth.matcher_config("c2f", backbone="convformer"), optim=optim, gpu_num=1), device=gpu,
                            optimizer_factory=lambda params: torch.optim.Adam(params, lr=optim.lr))
    tr.model.load_state_dict(synth.matcher_state_dict("c2f"), strict=False)
    tr.model.backbone.load_state_dict(synth.backbone_state_dict(0, "c2f"), strict=True)
    w = tr.model.backbone.model.stem.conv.weight
    before = w.detach().clone()
    np.random.seed(3)
    with torch.enable_grad():
        m = tr.training_step(train_batch(gpu), 0)
    assert bool(torch.isfinite(m["loss"])) and not torch.equal(w.detach(), before)
