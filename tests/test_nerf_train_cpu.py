"""CPU: the NeRF training fixtures recorded from the reference against the fp64 helper, the plain-torch losses of utils/metrics.py,
init_pfeat_mask and the argument validation of the nerf_train entry points (nothing here enqueues a kernel)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nerf_train_util as ntu
from conftest import GOLDEN, load_golden
from nerfmatch_amd import synth

NAMES = ("nerf_train_7s", "nerf_train_cam")
_REF = {}


def helper_on(name):
    """The helper's fp64 step on a fixture's inputs and draws, computed once and shared."""
    if name not in _REF:
        fx = load_golden(name)
        app = bool(fx["app"])
        sd = synth.nerf_state_dict(seed=int(fx["weights_seed"]), app_vocab=5 if app else 0, density_bias=3.0)
        step = ntu.train_step(sd, fx["rays"], fx["rgbs"], t_rand=fx["t_rand"], jitter=fx["jitter"], noise_coarse=fx["noise_coarse"],
                              noise_fine=fx["noise_fine"], noise_std=float(fx["noise_std"]), white_bg=bool(fx["white_bg"]),
                              ray_id=fx["ray_id"] if app else None, mask=fx["mask"] if app else None, ray_reg_weight=float(fx["ray_reg_weight"]))
        _REF[name] = (fx, step)
    return _REF[name]


@pytest.mark.parametrize("name", NAMES)
def test_helper_reproduces_the_reference_step(name):
    """Loss within 1e-6 relative, preds within 1e-6 of scale, every gradient tensor within 1e-4 of its largest entry: per tensor is legitimate
    HERE because the fixture's seed was chosen flip-free (its recorded fp32-vs-fp64 distance is <= 1e-5)."""
    fx, step = helper_on(name)
    assert float(fx["ref_fp32_vs_fp64"]) <= 1e-5 and int(fx["S"]) == 32 and fx["rays"].shape == (37, 12)
    assert torch.allclose(fx["rays"][:, 3:6], 1.3 * fx["rays"][:, 8:11], rtol=1e-6)
    assert abs(float(step["loss"]) - float(fx["loss"])) < 1e-6 * float(fx["loss"])
    for k, v in step["preds"].items():
        e = float((v - fx[f"pred_{k}"].double()).abs().max() / v.abs().max())
        assert e < 1e-6, (k, e)
    for k in ("rgb_coarse_mse", "rgb_fine_mse", "rgb_coarse_psnr", "rgb_fine_psnr"):
        assert abs(float(step["metrics"][k]) - float(fx[f"metric_{k}"])) < 1e-5 * abs(float(fx[f"metric_{k}"])), k
    stride, worst = int(fx["sub_stride"]), 0.0
    for k, g in step["grads"].items():
        assert float(g.abs().max()) > 0, k
        if f"g_{k}" in fx:
            e = float((g - fx[f"g_{k}"].double()).abs().max() / g.abs().max())
        else:
            e = float((g.reshape(-1)[::stride] - fx[f"gsub_{k}"].double()).abs().max() / g.abs().max())
            assert abs(float(g.norm()) - float(fx[f"gnorm_{k}"])) < 1e-4 * float(g.norm()), k
        worst = max(worst, e)
        assert e < 1e-4, (k, e)
    print(f"{name}: helper fp64 against the reference's fp32 step: worst per-tensor gradient distance {worst:.2e}")
    if "embedding_a.weight" in step["grads"]:
        used = torch.bincount(fx["ray_id"], minlength=5) > 0
        assert torch.equal(step["grads"]["embedding_a.weight"].abs().amax(1) > 0, used)


def test_fixtures_regenerate_bit_for_bit(tmp_path):
    """With the reference tree present: the generator, run again, gives the committed arrays."""
    sys.path.insert(0, str(GOLDEN))
    try:
        import make_golden as mg
    finally:
        sys.path.remove(str(GOLDEN))
    if not mg.REF.exists():
        pytest.skip("the reference tree is not present")
    env = dict(os.environ, NM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, str(GOLDEN / "make_golden_nerf_train.py")], check=True, env=env, stdout=subprocess.DEVNULL)
    for name in NAMES:
        new, old = np.load(tmp_path / f"{name}.npz"), np.load(GOLDEN / f"{name}.npz")
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (name, k)
        assert (GOLDEN / f"{name}.npz").stat().st_size < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_metrics_on_cpu_tensors(name):
    """utils.metrics.compute_nerf_metrics / lossfun_distortion / distortion_loss / mse2psnr in plain torch against the fixture's numbers."""
    from nerfmatch_amd.utils import metrics as M

    fx, step = helper_on(name)
    app = bool(fx["app"])
    preds = {k[5:]: v for k, v in fx.items() if k.startswith("pred_")}
    loss_cfg = synth.nerf_config("cambridge" if app else "7scenes").loss
    got = M.compute_nerf_metrics(preds, fx["rgbs"], mask_loss=fx["mask"] if app else None, cnfg_loss=loss_cfg)
    assert abs(float(got["loss"]) - float(fx["loss"])) < 1e-6 * float(fx["loss"])
    for k in ("rgb_coarse_mse", "rgb_fine_mse", "rgb_coarse_psnr", "rgb_fine_psnr"):
        assert abs(float(got[k]) - float(fx[f"metric_{k}"])) < 1e-6 * abs(float(fx[f"metric_{k}"])), k
    want = ntu.lossfun_distortion(step["preds"]["s_fine"], step["preds"]["weights_fine"])
    per_ray = M.lossfun_distortion(preds["s_fine"], preds["weights_fine"])
    assert float((per_ray.double() - want).abs().max()) < 1e-5 * float(want.max())
    assert abs(float(M.distortion_loss(preds["s_fine"], preds["weights_fine"])) - float(want.mean())) < 1e-5 * float(want.mean())
    assert float(M.mse2psnr(torch.tensor(0.01))) == pytest.approx(20.0)
    # validation: no regulariser, the mask rounded; the loss is differentiable plain torch
    val = M.compute_nerf_metrics(preds, fx["rgbs"], mask_loss=fx["mask"] if app else None, validation_mode=True, cnfg_loss=loss_cfg)
    m = torch.round(fx["mask"]) if app else 1
    assert float(val["loss"]) == pytest.approx(float(0.5 * (m * (preds["rgb_coarse"] - fx["rgbs"]) ** 2).mean() + 0.5 * (m * (preds["rgb_fine"] - fx["rgbs"]) ** 2).mean()), rel=1e-6)
    with torch.enable_grad():
        w = preds["weights_fine"].clone().requires_grad_(True)
        M.compute_nerf_metrics(dict(preds, weights_fine=w), fx["rgbs"], cnfg_loss=loss_cfg)["loss"].backward()
    assert float(w.grad.abs().max()) > 0
    only_coarse = M.compute_nerf_metrics({"rgb_coarse": preds["rgb_coarse"]}, fx["rgbs"])
    assert float(only_coarse["rgb_fine_psnr"]) == float(only_coarse["rgb_coarse_psnr"])


def test_init_pfeat_mask():
    from nerfmatch_amd.nerf_trainer import init_pfeat_mask

    m = init_pfeat_mask([16, 24], ds=8, sample_num=2)
    assert m.shape == (2, 16, 24, 1) and m.dtype == torch.bool and int(m.sum()) == 2 * 2 * 3
    assert bool(m[1, 4, 12, 0]) and bool(m[0, 12, 20, 0]) and not bool(m[0, 0, 0, 0]) and not bool(m[0, 4, 5, 0])
    assert int(init_pfeat_mask([480, 480]).sum()) == 3600


def test_argument_validation_without_gpu(built_lib):
    """Bad arguments are refused before anything is enqueued: safe without a device."""
    from nerfmatch_amd import _lib

    h = _lib.lib()
    null = C.c_void_p(0)
    p = C.c_void_p(16)  # (never dereferenced: every call below fails its argument check first)
    assert h.nm_nerf_train_encode(null, null, 4, 32, null, null, null, 0, -1.0, null, null, null, null) == 1
    assert h.nm_nerf_train_encode(p, p, 0, 32, null, null, null, 0, -1.0, p, p, null, null) == 1
    assert h.nm_nerf_train_encode(p, p, 4, 32, null, null, p, 0, -1.0, p, p, null, null) == 1  # a table of zero rows
    ids = torch.tensor([0, 1, 5, 2])
    assert h.nm_nerf_train_encode(p, p, 4, 32, null, C.c_void_p(ids.data_ptr()), p, 5, -1.0, p, p, null, null) == 1  # host ids outside [0, V)
    assert h.nm_nerf_composite4(null, null, null, null, 0.0, 0, 4, 32, 32, null, null, null, null, null) == 1
    assert h.nm_nerf_composite4(p, p, p, null, 0.0, 0, 4, 2048, 2048, p, null, null, null, null) == _lib.NM_ERR_UNSUPPORTED
    assert h.nm_nerf_composite4_bwd(p, p, p, null, 0.0, 0, null, null, 4, 32, 32, p, null, null) == 1
    assert h.nm_nerf_composite4_bwd(p, p, p, null, 0.0, 0, p, null, 4, 2048, 2048, p, null, null) == _lib.NM_ERR_UNSUPPORTED
    for bad in (33, 0):  # S_act outside [1, S]
        assert h.nm_nerf_composite4(p, p, p, null, 0.0, 0, 4, 32, bad, p, null, null, null, null) == 1
        assert h.nm_nerf_composite4_bwd(p, p, p, null, 0.0, 0, p, null, 4, 32, bad, p, null, null) == 1
    assert h.nm_nerf_distortion_workspace_bytes() >= 8
    assert h.nm_nerf_distortion(p, 0, null, 4, 32, null, p, null, null, null) == 1  # t -> s needs the workspace
    assert h.nm_nerf_distortion(p, 1, p, 4, 32, null, null, null, null, null) == 1  # weights without a place for the loss
    assert h.nm_nerf_distortion_bwd(p, p, 4, 32, 1.0, null, null) == 1
    assert h.nm_nerf_photo_loss(p, p, p, null, 1.0, 0, p, null, null, null) == 1
    assert h.nm_nerf_app_grad(p, null, null, 4, 32, 0, p, p, null) == 1
