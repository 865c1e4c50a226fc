"""Shared by test_supervision_cpu.py / test_supervision_gpu.py: the cases of tests/golden/supervision.npz and how they are run."""
import torch

from conftest import load_golden
from nerfmatch_amd import supervision as sup

DS = 8
_FX = {}


def fixture():
    """The golden file, loaded once per process (the tests only read it)."""
    if not _FX:
        _FX.update(load_golden("supervision"))
    return _FX


def bar_px():
    """Tolerance of pt2d_proj in pixels: 4 x the largest |fp32 - fp64| of the REFERENCE's own projections over the fixture's cases A-D
    (1.038e-4 px, recorded by make_golden_supervision.py) = 4.154e-4 px.  The closed-form rigid inverse and the fixed operation order
    are a second, independent fp32 rounding of the same formula."""
    return 4.0 * float(fixture()["max_err_px"])


def run_case(tag, dev, fallback=None, dense=True):
    """supervision.coarse_supervision on the inputs of case `tag`, on device `dev` -> the filled batch dict."""
    fx = fixture()
    H, W = (int(v) for v in fx[f"{tag}_hw"])
    B = fx[f"{tag}_pt3d"].shape[0]
    data = dict(image=torch.zeros(B, 3, H, W, device=dev), K=fx[f"{tag}_K"].to(dev), c2w=fx[f"{tag}_c2w"].to(dev), pt3d=fx[f"{tag}_pt3d"].to(dev))
    if f"{tag}_pt_mask" in fx:
        data.update(pt_mask=fx[f"{tag}_pt_mask"].to(dev), im_mask=fx[f"{tag}_im_mask"].to(dev))
    return sup.coarse_supervision(data, ds=DS, fallback=fallback, dense=dense)


def check_case(tag, data, dense=True, pre=None):
    """Integers identical to the reference's, projections within the bar, dense matrix = the reference's and = a scatter of the triple."""
    fx = fixture()
    pre = pre or tag
    assert data["gt_cell"].dtype == torch.int32 and torch.equal(data["gt_cell"].cpu(), fx[f"{tag}_gt_cell"])
    for got, key in zip(data["gt_ids"], ("b_ids", "i_ids", "j_ids")):
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), fx[f"{pre}_{key}"]), (tag, key)
    got, ref = data["pt2d_proj"].cpu().double(), fx[f"{tag}_pt2d_proj64"].reshape(got_shape(data))
    err = (got - ref).abs().max().item()
    print(f"{tag}: max |pt2d_proj - fp64| = {err:.3e} px (bar {bar_px():.3e})")
    assert err <= bar_px()
    if dense:
        conf = data["conf_gt"]
        assert conf.dtype == torch.uint8
        if f"{pre}_conf_gt" in fx:
            assert torch.equal(conf.cpu(), fx[f"{pre}_conf_gt"])
        scat = torch.zeros_like(conf)
        scat[data["gt_ids"]] = 1
        assert torch.equal(conf, scat)
    else:
        assert "conf_gt" not in data


def got_shape(data):
    return tuple(data["pt2d_proj"].shape)
