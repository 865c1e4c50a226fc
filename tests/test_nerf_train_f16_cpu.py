"""CPU: the host side of the fp16 mixed-precision NeRF training mode -- the float64 emulation of the walk's arithmetic
(tests/nerf_train_f16_util.py) pinned to nerf_train_util, the loss-scale state machine, and NerfRenderer.train_precision's values."""
import warnings

import pytest
import torch

import nerf_train_f16_util as f16u
import nerf_train_util as ntu
from nerfmatch_amd import synth
from test_nerf_train_gpu import draws_for, make_rays

R, S = 6, 8


def step_inputs(app):
    sd = synth.nerf_state_dict(seed=0, app_vocab=5 if app else 0, density_bias=3.0)
    g = torch.Generator().manual_seed(3)
    rays, gt = make_rays(R, 7), torch.rand(R, 3, generator=g)
    d = draws_for(R, S, 5)
    kw = dict(t_rand=d["t_rand"], jitter=d["jitter"], noise_coarse=d["noise_coarse"], noise_fine=d["noise_fine"], noise_std=1.0, white_bg=app,
              ray_id=torch.randint(0, 5, (R,), generator=g) if app else None, ray_reg_weight=0.01)
    return sd, rays, gt, kw


@pytest.mark.parametrize("app", [False, True])
def test_emulation_without_rounding_is_the_fp64_helper(app):
    """Every rounding site switched to the identity: the same preds, loss and gradients as nerf_train_util.train_step (1e-12: the emulation
    concatenates [dir | appearance] before the views layer's input, the helper all three at once -- the same sums)."""
    sd, rays, gt, kw = step_inputs(app)
    want = ntu.train_step(sd, rays, gt, **kw)
    got = f16u.train_step(sd, rays, gt, rounding=False, **kw)
    assert abs(float(got["loss"]) - float(want["loss"])) <= 1e-12 * abs(float(want["loss"]))
    for k, v in want["preds"].items():
        assert torch.allclose(got["preds"][k], v, rtol=1e-12, atol=1e-14), k
    assert set(got["grads"]) == set(want["grads"])
    for k, v in want["grads"].items():
        assert float(v.abs().max()) > 0 or k.endswith("embedding_a.weight"), k
        assert torch.allclose(got["grads"][k], v, rtol=1e-10, atol=1e-12 * float(v.abs().max())), k


def test_emulation_rounds():
    """With the sites on: a different step (the rounding is active), every parameter still takes a gradient, and a loss scale changes only
    what underflows: scale 1 loses gradient rows that scale 65536 keeps."""
    sd, rays, gt, kw = step_inputs(True)
    want = ntu.train_step(sd, rays, gt, **kw)
    got = f16u.train_step(sd, rays, gt, scale=65536.0, **kw)
    low = f16u.train_step(sd, rays, gt, scale=1.0, **kw)
    d = {n: ntu.net_l2(got["grads"], want["grads"], n) for n in ntu.NETS}
    d1 = {n: ntu.net_l2(low["grads"], want["grads"], n) for n in ntu.NETS}
    print("emulation against fp64:", d, " at scale 1:", d1)
    assert all(v > 0 for v in d.values())
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for k, g in got["grads"].items() if k.startswith(ntu.NETS))
    assert all(d1[n] > d[n] for n in ntu.NETS)
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0, 2.0 ** -26], dtype=torch.float64)
    assert f16u.r16(x).tolist() == [1.0, 1.0 + 2.0 ** -9, float("inf"), 0.0]  # ties to even, overflow to infinity, underflow to zero


def test_loss_scale_state_machine():
    from nerfmatch_amd.nerf_trainer import LossScale

    s = LossScale()
    assert s.scale == 65536.0 and s.skipped_steps == 0 and s.overflow_events == [0, 0]
    assert s.update(0, 0) is False and s.scale == 65536.0
    assert s.update(0, 3) is True and s.scale == 32768.0 and s.skipped_steps == 1 and s.overflow_events == [0, 3]  # backward event: skip, halve
    for i in range(1999):
        assert s.update(0, 0) is False
    assert s.scale == 32768.0  # 1999 clean steps: not yet
    assert s.update(0, 0) is False and s.scale == 65536.0  # the 2000th: doubled
    for i in range(1999):
        s.update(0, 0)
    assert s.update(0, 1) is True and s.scale == 32768.0  # an overflow resets the count of clean steps ...
    for i in range(1999):
        s.update(0, 0)
    assert s.scale == 32768.0
    s.update(0, 0)
    assert s.scale == 65536.0  # ... 2000 clean steps from there
    with pytest.warns(RuntimeWarning, match="forward"):
        assert s.update(2, 0) is True  # forward event: skipped, the scale is left alone
    assert s.scale == 65536.0 and s.skipped_steps == 3 and s.overflow_events == [2, 4]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # it warns once
        assert s.update(1, 1) is True
    assert s.scale == 32768.0 and s.skipped_steps == 4 and s.overflow_events == [3, 5]  # both: the backward rule
    import math

    for _ in range(40):
        s.update(0, 7)
    assert math.frexp(s.scale)[0] == 0.5 and s.scale == 2.0 ** (15 - 40)  # always a power of two


def test_train_precision_values():
    from nerfmatch_amd.nerf import train_render as tr
    from nerfmatch_amd.nerf.renderer import NerfRenderer

    cfg = synth.nerf_config("7scenes", num_pts=32, img_wh=(8, 8))
    ren = NerfRenderer(cfg)
    assert ren.train_precision == "same" and ren.train_loss_scale == 65536.0 and ren.train_overflow_events() == (0, 0)
    ren.train_precision = "f16"
    assert ren.train_precision == "f16"
    for bad in ("fp16", "bf16", None, 16):
        with pytest.raises(ValueError, match="train_precision"):
            ren.train_precision = bad
    assert ren.train_precision == "f16"
    cfg.train_precision = "f16"
    assert NerfRenderer(cfg).train_precision == "f16"
    cfg.train_precision = "half"
    with pytest.raises(ValueError, match="train_precision"):
        NerfRenderer(cfg)
    # an fp16 chunk holds twice the rays under the same byte limit
    assert tr.chunk_rays_for(128, 2 << 30, 2) == (2 << 30) // (128 * tr.SAVED_FLOATS * 2) >= 2 * tr.chunk_rays_for(128, 2 << 30)
    assert tr.chunk_rays_for(128, 2 << 30, 4) == tr.chunk_rays_for(128, 2 << 30)
