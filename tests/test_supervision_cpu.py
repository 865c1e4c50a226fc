"""CPU: the torch path of nerfmatch_amd.supervision against the reference's numbers (tests/golden/supervision.npz, made by
tests/golden/make_golden_supervision.py), the fallback rule, the ground-truth id cache of the model, and the argument checks of
nm_gt_supervision (made before anything is enqueued: safe without a device).

Integers (cell ids, the triple and its order, the dense matrix) must be IDENTICAL: the generator asserts that every fixture point of
cases A-D projects >= 0.01 px away from every cell boundary and that the reference's fp32 and fp64 cells agree.  pt2d_proj: within
4 x the reference's own fp32-vs-fp64 error over the fixture = 4 x 1.038e-4 = 4.154e-4 px (supervision_util.bar_px)."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import supervision_util as su
from nerfmatch_amd import _lib
from nerfmatch_amd import supervision as sup

CPU = torch.device("cpu")
GOLDEN = Path(__file__).resolve().parent / "golden"


def test_bar_is_what_the_generator_measured():
    assert abs(su.bar_px() - 4.154e-4) < 1e-6


@pytest.mark.parametrize("tag", ["A", "B1", "B129", "C"])
def test_torch_path_vs_reference(tag):
    su.check_case(tag, su.run_case(tag, CPU))


def test_torch_path_multi_pair_full_size():
    """Case D: pt3d (1, 2, 2400, 3) flattened to N = 4800, M = 4800; ids only."""
    data = su.run_case("D", CPU, dense=False)
    assert data["pt2d_proj"].shape == (1, 4800, 2) and data["gt_cell"].shape == (1, 4800)
    su.check_case("D", data, dense=False)


def test_project_points3d_is_the_projection_of_the_supervision():
    fx = su.fixture()
    w2c = sup.w2c_from_c2w(fx["A_c2w"])
    pix = sup.project_points3d(fx["A_K"], w2c, fx["A_pt3d"])
    assert torch.equal(pix, su.run_case("A", CPU)["pt2d_proj"])
    assert torch.equal(sup.project_points3d(fx["A_K"][1], w2c[1], fx["A_pt3d"][1]), pix[1])  # unbatched
    assert (pix.double() - fx["A_pt2d_proj64"]).abs().max().item() <= su.bar_px()


def test_fixture_regenerates_bit_for_bit(tmp_path):
    """With the reference tree present: the generator, run again, gives the committed arrays."""
    sys.path.insert(0, str(GOLDEN))
    try:
        import make_golden as mg
    finally:
        sys.path.remove(str(GOLDEN))
    if not mg.REF.exists():
        pytest.skip("the reference tree is not present")
    env = dict(os.environ, NM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, str(GOLDEN / "make_golden_supervision.py")], check=True, env=env, stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / "supervision.npz"), np.load(GOLDEN / "supervision.npz")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k


def test_fallback_applies_iff_the_element_is_empty():
    fx = su.fixture()
    plain = su.run_case("C", CPU)
    assert not (plain["gt_ids"][0] == 0).any()  # element 0 sees nothing and, without a fallback, stays empty
    fb = su.run_case("C", CPU, fallback=fx["C_fallback"])
    su.check_case("C", fb, pre="C_fb")
    b, i, j = fb["gt_ids"]
    assert (b == 0).sum() == 1 and (i[0].item(), j[0].item()) == tuple(fx["C_fallback"][0].tolist())
    assert torch.equal(b[1:], plain["gt_ids"][0]) and torch.equal(i[1:], plain["gt_ids"][1]) and torch.equal(j[1:], plain["gt_ids"][2])
    assert torch.equal(fb["conf_gt"][1], plain["conf_gt"][1]) and fb["conf_gt"][0].sum() == 1 and plain["conf_gt"][0].sum() == 0
    assert torch.equal(fb["gt_cell"], plain["gt_cell"])  # geometry only
    # a fallback on a batch without an empty element changes nothing
    a0, a1 = su.run_case("A", CPU), su.run_case("A", CPU, fallback=[[1, 2], [3, 4]])
    assert torch.equal(a0["conf_gt"], a1["conf_gt"]) and all(torch.equal(x, y) for x, y in zip(a0["gt_ids"], a1["gt_ids"]))
    # a pair outside the matrix is ignored
    bad = su.run_case("C", CPU, fallback=[[48, 0], [0, 0]])
    assert torch.equal(bad["conf_gt"], plain["conf_gt"])


def test_seed_gt_ids_serves_the_cache():
    from nerfmatch_amd import synth
    from nerfmatch_amd.matcher import NeRFMatcherMS

    model = NeRFMatcherMS(synth.matcher_config("c2f"))
    data = su.run_case("A", CPU)
    conf, ids = data["conf_gt"], data["gt_ids"]
    model.seed_gt_ids(conf, ids)
    got = model._gt_ids(conf)
    assert all(g is s for g, s in zip(got, ids))  # the seeded objects, no scan
    other = conf.clone()
    again = model._gt_ids(other)  # a different tensor of the same shape: scanned
    assert all(g is not s for g, s in zip(again, ids)) and all(torch.equal(g, s) for g, s in zip(again, ids))
    model.seed_gt_ids(conf, ids)
    conf[0, 0, 0] = 1  # the same tensor in a new state (version bumped): scanned again
    assert model._gt_ids(conf)[0] is not ids[0]


def test_trainer_hook_leaves_a_supervised_batch_alone():
    sentinel = object()
    data = dict(conf_gt=sentinel, K=None, c2w=None, pt3d=None, image=None)
    assert sup.supervise_batch(None, data) is data and data["conf_gt"] is sentinel and "gt_ids" not in data
    assert "conf_gt" not in sup.supervise_batch(None, dict(image=torch.zeros(1, 3, 8, 8)))  # no geometry: untouched


def test_argument_validation_without_gpu(built_lib):
    """Null pointers -> NM_ERR_ARG (1); more than 6400 cells with the triple, or a size that is no multiple of ds -> NM_ERR_UNSUPPORTED (2);
    a missing workspace -> NM_ERR_WORKSPACE (4).  All returned before anything is enqueued (the pointers below are never dereferenced)."""
    h = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(pt3d=p, K=p, w2c=p, B=1, M=48, N=8, H=48, W=64, ds=8, proj=p, cell=p, conf=null, ids=p, ws=p, ws_bytes=1 << 20):
        return h.nm_gt_supervision(pt3d, K, w2c, null, null, null, B, M, N, H, W, ds, proj, cell, conf, ids, ids, ids, ids, ws, ws_bytes, null)

    assert h.nm_gt_supervision_workspace_bytes(2, 4800, 4800) == (2 * 4800 + 2) * 4
    assert call(pt3d=null) == 1 and call(K=null) == 1 and call(w2c=null) == 1 and call(proj=null) == 1
    assert call(B=0) == 1 and call(N=0) == 1 and call(ds=0) == 1
    assert call(cell=null) == 1  # projection only takes no id outputs
    assert h.nm_gt_supervision(p, p, p, null, null, null, 1, 48, 8, 48, 64, 8, p, p, null, p, null, p, p, p, 1 << 20, null) == 1  # a partial triple
    assert call(M=6401, H=8, W=8 * 6401) == 2
    assert call(W=60) == 2 and call(H=50) == 2
    assert call(ws=null) == 4 and call(ws_bytes=8) == 4
    assert _lib.NM_ERR_UNSUPPORTED == 2 and b"supported" in h.nm_error_string(2)
    with pytest.raises(ValueError):
        sup.supervision(torch.zeros(1, 4, 3), torch.eye(3)[None], torch.eye(4)[None], (48, 60))
