"""CPU: cosine mutual-NN matching and the NeRF two-view pose metrics against the reference's recorded numbers
(tests/golden/nerf_pose_metrics.npz, made by tests/golden/make_golden_nerf_pose.py), the float64 restatement the GPU tests measure
against, and the argument checks of nm_feature_mutual_nn (made before anything is enqueued: safe without a device).

Index lists must be IDENTICAL to the reference's, scores within 1e-6 (fp32 dot products of 64 terms of unit vectors, evaluated by the
same library call).  The four correspondence sets that compute_nerf_pose_metrics hands to its solver must equal the recorded ones
exactly: the points come out of the reference's own statement, and the generator asserts that no truncated pixel coordinate lies within
1e-3 px of an integer.  The returned dict: the rotation errors within 1e-3 degrees -- the reference multiplies the two rotations in fp32
(trace error <= 9 x 2^-24 = 5.4e-7, angle = acos((trace - 1) / 2) with d angle / d trace = 1 / (2 sin angle) <= 1 / (2 sin 6 deg) = 4.8 for
the fixture's poses: 2.6e-6 rad = 1.5e-4 deg), the translation errors within 1e-5 relative (an fp32 norm of three terms)."""
import ctypes as C
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import nerf_pose_util as pu
from nerfmatch_amd import _lib
from nerfmatch_amd.utils.geometry import mutual_nn_matching
from nerfmatch_amd.utils.metrics import compute_nerf_pose_metrics, pose_err

GOLDEN = Path(__file__).resolve().parent / "golden"


def test_torch_path_equals_the_reference():
    fx = pu.fixture()
    matches, scores = mutual_nn_matching(fx["nn_desc1"], fx["nn_desc2"])
    assert matches.dtype == torch.int64 and torch.equal(matches, fx["nn_matches"])
    assert float((scores - fx["nn_scores"]).abs().max()) <= 1e-6
    # planted: every match is a planted pair
    assert torch.equal(fx["nn_perm"][matches[:, 1]], matches[:, 0])


def test_f64_restatement_is_pinned_to_the_reference():
    fx = pu.fixture()
    ref = pu.mutual_nn_f64(fx["nn_desc1"], fx["nn_desc2"])
    assert torch.equal(ref["matches"], fx["nn_matches"])
    assert float((ref["scores"] - fx["nn_scores"].double()).abs().max()) <= 1e-6
    row_gap, col_gap = pu.gaps(ref["sim"])
    assert float(row_gap.min()) > pu.GAP and float(col_gap.min()) > pu.GAP  # no decision of the pinning case is a near tie


def test_threshold_and_empty_inputs():
    fx = pu.fixture()
    d1, d2 = fx["nn_desc1"], fx["nn_desc2"]
    full_m, full_s = mutual_nn_matching(d1, d2)
    thr = float(full_s.sort().values[len(full_s) // 2])  # a score of the list itself: strictly greater drops it
    m, s = mutual_nn_matching(d1, d2, threshold=thr)
    keep = full_s > thr
    assert 0 < len(m) < len(full_m) and torch.equal(m, full_m[keep]) and torch.equal(s, full_s[keep]) and float(s.min()) > thr
    for none in (None, 0, 0.0):
        m0, s0 = mutual_nn_matching(d1, d2, threshold=none)
        assert torch.equal(m0, full_m) and torch.equal(s0, full_s)
    for a, b in ((d1[:0], d2), (d1, d2[:0])):
        m, s = mutual_nn_matching(a, b)
        assert m.shape == (0, 2) and m.dtype == torch.int64 and s.shape == (0, 2) and s.dtype == torch.int64  # the reference's pair


def test_pose_metrics_reproduce_the_reference():
    fx = pu.fixture()
    rec = pu.Recorder()
    got = compute_nerf_pose_metrics(*pu.pose_inputs(), solver=rec)
    pu.check_sets(rec.calls)
    assert set(got) == set(pu.KEYS)
    assert got["num_matches"] == int(fx["pm_num_matches"]) == len(fx["pm_set2_pt2d"])
    assert abs(float(got["match_score"]) - fx["pm_match_score"]) <= 1e-6
    for k in ("R_err_depth", "R_err_match"):
        print(k, got[k], fx[f"pm_{k}"])
        assert abs(got[k] - fx[f"pm_{k}"]) <= 1e-3
    for k in ("t_err_depth", "t_err_match"):
        print(k, got[k], fx[f"pm_{k}"])
        assert abs(got[k] - fx[f"pm_{k}"]) <= 1e-5 * fx[f"pm_{k}"]
    # the four values are the means over the two images of pose_err of the recorder's poses, translations x 100
    c2w = fx["pm_c2w"].reshape(2, 4, 4)
    errs = []
    for q in range(4):
        w2c = torch.eye(4)
        w2c[:3, :3], w2c[:3, 3] = fx["pm_pose_R"][q], fx["pm_pose_t"][q]
        errs.append(pose_err(c2w[q % 2], w2c.inverse()))
    assert got["R_err_depth"] == 0.5 * (errs[0][0] + errs[1][0]) and got["t_err_match"] == 0.5 * (errs[2][1] + errs[3][1]) * 100


def test_pose_metrics_solver_failures_and_arguments():
    pts, mask, feat, data = pu.pose_inputs()
    rec = pu.Recorder(inner=lambda *a: None)
    got = compute_nerf_pose_metrics(pts, mask, feat, data, solver=rec)
    assert len(rec.calls) == 4 and all(math.isinf(got[k]) for k in ("R_err_depth", "t_err_depth", "R_err_match", "t_err_match"))
    one_fails = pu.Recorder()
    one_fails.inner = lambda p2, p3, K: None if len(one_fails.calls) == 3 else (np.eye(3), np.zeros(3), [])
    got = compute_nerf_pose_metrics(pts, mask, feat, data, solver=one_fails)
    assert math.isfinite(got["R_err_depth"]) and math.isinf(got["R_err_match"]) and math.isinf(got["t_err_match"])
    with pytest.raises(ValueError, match="two-view"):
        compute_nerf_pose_metrics(pts, mask, feat, dict(data, img_idx=[0]), solver=rec)
    with pytest.raises(ValueError, match="solver"):
        compute_nerf_pose_metrics(pts, mask, feat, data, solver="ransac")


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
    subprocess.run([sys.executable, str(GOLDEN / "make_golden_nerf_pose.py")], check=True, env=env, stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / "nerf_pose_metrics.npz"), np.load(GOLDEN / "nerf_pose_metrics.npz")
    assert sorted(new.files) == sorted(old.files) and (GOLDEN / "nerf_pose_metrics.npz").stat().st_size < 1_000_000
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k


def test_argument_validation_without_gpu(built_lib):
    """Non-positive sizes, null pointers, a negative / non-finite eps, a NaN threshold -> NM_ERR_ARG (1); C outside {64, 128, 256, 512} or a side
    above 2^20 rows -> NM_ERR_UNSUPPORTED (2); a workspace that is too small -> NM_ERR_WORKSPACE (4).  All returned before anything is
    enqueued (the pointers below are never dereferenced)."""
    h = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(d1=p, d2=p, n1=300, n2=200, c=64, eps=1e-9, thr=0.0, use=0, m=p, s=p, cnt=p, ws=p, ws_bytes=1 << 30):
        return h.nm_feature_mutual_nn(d1, d2, n1, n2, c, eps, thr, use, m, s, cnt, null, null, ws, ws_bytes, null)

    need = h.nm_feature_mutual_nn_workspace_bytes(300, 200, 64)
    assert 0 < need < 1 << 22 and h.nm_feature_mutual_nn_workspace_bytes(300, 200, 96) == 0 and h.nm_feature_mutual_nn_workspace_bytes(0, 200, 64) == 0
    assert call(d1=null) == 1 and call(d2=null) == 1 and call(m=null) == 1 and call(s=null) == 1 and call(cnt=null) == 1 and call(ws=null) == 1
    assert call(n1=0) == 1 and call(n2=-3) == 1 and call(eps=-1.0) == 1 and call(eps=float("inf")) == 1 and call(eps=float("nan")) == 1
    assert call(thr=float("nan"), use=1) == 1
    assert call(c=96) == 2 and call(c=32) == 2 and call(c=1024) == 2 and call(n1=(1 << 20) + 1) == 2
    assert call(ws_bytes=need - 1) == 4
    assert _lib.NM_ERR_UNSUPPORTED == 2
