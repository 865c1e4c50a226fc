"""Shared by test_ref_bank_cpu.py / test_ref_bank_gpu.py: banks over the cases of tests/golden/ref_bank.npz, synthetic banks of any shape
(small cameras of 64 x 48 px around the origin looking down +z at a slab of random points), and the comparison of a GPU bank with the
host path of the same bank."""
import numpy as np
import torch

from conftest import load_golden
from nerfmatch_amd import synth
from nerfmatch_amd.ref_bank import ReferencePointBank

W, H, FOCAL = 64, 48, 60.0
CASES = ("k1", "k3", "tie", "tie_m1", "k10", "scaled")
_FX = {}


def fixture():
    """The golden file, loaded once per process (the tests only read it)."""
    if not _FX:
        _FX.update(load_golden("ref_bank"))
    return _FX


def golden_bank(tag, device="cpu", **kw):
    fx = fixture()
    g = lambda key: fx[f"{tag}_{key}"]
    bank = ReferencePointBank(g("pt3d"), g("pt_feat"), g("c2w"), g("K"), g("frame_wh"), tuple(int(v) for v in fx["img_wh"]), unnorm_scene=g("unnorm_scene"),
                              device=device, **kw)
    return bank, g("ref_ids")[None]


def synth_args(F, n, D, seed=0, masks=True, spread=(2.8, 2.0), depth=(1.0, 5.0), max_angle=0.6):
    """Constructor arguments of a synthetic bank (host tensors: build a host bank and a GPU bank from the same ones).  Column 0 of the
    features is the row's id f n + r (exact in fp32 up to 2^24)."""
    g = np.random.default_rng(seed)
    c2w = torch.stack([synth.camera_pose(1000 * seed + f, max_t=0.6, max_angle=max_angle) for f in range(F)])
    pt3d = np.stack([g.uniform(-spread[0], spread[0], (F, n)), g.uniform(-spread[1], spread[1], (F, n)), g.uniform(depth[0], depth[1], (F, n))], -1)
    feat = g.standard_normal((F, n, D)).astype(np.float32)
    feat[..., 0] = np.arange(F * n).reshape(F, n)
    mask = torch.from_numpy(g.uniform(size=(F, n)) > 0.2) if masks else None
    return dict(pt3d=torch.from_numpy(pt3d.astype(np.float32)), pt_feat=torch.from_numpy(feat), c2w=c2w, K=synth.intrinsics(H, W, FOCAL), frame_wh=(W, H),
                img_wh=(W, H), pt_mask=mask, unnorm_scene=synth.unnorm_scene())


def source_ids(out):
    """the bank row f n + r every output row was copied from (column 0 of the features)"""
    return out["pt_feat"][..., 0].round().long()


def assert_rows_are_their_sources(bank, out):
    """every output row equals the bank row its id names, in all three tensors"""
    ids = source_ids(out).reshape(-1).to(bank.pt3d.device)
    assert torch.equal(out["pt3d"].reshape(-1, 3), bank.pt3d.reshape(-1, 3)[ids])
    assert torch.equal(out["pt_feat"].reshape(-1, bank.D), bank.pt_feat.reshape(-1, bank.D)[ids])
    assert torch.equal(out["pt_mask"].reshape(-1), bank.pt_mask.reshape(-1)[ids])


def words_u32(words):
    """visibility words as non-negative int64, from either path (the kernels' int32 tensors hold the uint32 bits)"""
    return words.cpu().to(torch.int64) & 0xFFFFFFFF


def assert_same_selection(dev_sel, host_sel):
    """words, decisions, n_visible and the whole list (list[:Nv] and its -1 tail) identical"""
    assert torch.equal(words_u32(dev_sel["words"]), words_u32(host_sel["words"]))
    for key in ("decisions", "n_visible", "list"):
        assert dev_sel[key].dtype == torch.int32 and torch.equal(dev_sel[key].cpu(), host_sel[key]), key


def same_bits(a, b):
    """equal dtype, shape and bytes (floats compared as their bit patterns: a NaN equals the same NaN)"""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def assert_same_sets(dev_out, host_out):
    for key in ("pt3d", "pt_feat", "pt_mask", "rc2w", "n_visible", "decisions"):
        assert same_bits(dev_out[key], host_out[key]), key
    assert (dev_out["unnorm_scene"] is None) == (host_out["unnorm_scene"] is None)
    if host_out["unnorm_scene"] is not None:
        assert torch.equal(dev_out["unnorm_scene"].cpu(), host_out["unnorm_scene"])
