"""CPU: the float64 restatement of the PnP-RANSAC solver (tests/pnp_util.py) on its own, the `solver="gpu"` dispatch, and the argument
checks / ABI of nm_pnp_ransac (made before anything is enqueued: safe without a device)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import pnp_util as pu
from nerfmatch_amd import _lib

ROOT = Path(__file__).resolve().parents[1]


def _exact_scene(n, outlier_frac, seed):
    """A scene whose inlier pixels are the float64 projections of its (float32) points: the true pose is the exact optimum."""
    sc = pu.make_scene(n, 0.0, outlier_frac, seed=seed)
    K, X = sc["K"].astype(np.float64), sc["pt3d"].astype(np.float64)
    pix, _ = pu.project(K, sc["R"], sc["t"], X)
    pt2d = sc["pt2d"].astype(np.float64)
    pt2d[sc["inlier"]] = pix[sc["inlier"]]
    return sc, pt2d, X, K


@pytest.mark.parametrize("outlier_frac", [0.0, 0.5])
def test_restatement_recovers_the_true_pose(outlier_frac):
    sc, pt2d, X, K = _exact_scene(200, outlier_frac, seed=3)
    out = pu.solve(pt2d, X, K, thr=1.0, n_hyps=64, refine_iters=10, seed=0)
    dR, dt = pu.pose_distance(sc["R"], sc["t"], out["R"], out["t"])
    print(f"outliers {outlier_frac}: rotation {dR:.3e} deg, translation {dt:.3e}, {out['n_inliers']} inliers")
    # float64 precision of the LM optimum: the normal equations of 100+ points at depth <= 10 with f = 500 have a condition number of
    # ~1e6, so the pose is determined to ~1e6 * 2e-16 relative; 1e-9 leaves a factor of a few
    assert dt < 1e-9 and np.abs(out["R"] - sc["R"]).max() < 1e-9
    assert np.array_equal(out["mask"], sc["inlier"]) and out["n_inliers"] == int(sc["inlier"].sum())
    again = pu.solve(pt2d, X, K, thr=1.0, n_hyps=64, refine_iters=10, seed=0)
    assert np.array_equal(again["R"], out["R"]) and np.array_equal(again["t"], out["t"]) and again["win"] == out["win"]
    assert [pu.sample_indices(1, h, 200) for h in range(64)] != [pu.sample_indices(0, h, 200) for h in range(64)]  # another seed: other samples


def test_p3p_roots_reproject_their_sample():
    """1000 random triangles, every fourth one near-collinear (the third point 1e-3 of the segment's length off the segment between the other
    two: sin of the angle at x1 between 1.25e-3 and 5e-3, an order above the AREA_FLOOR cut at 1e-4): every root reprojects the three points to
    < 1e-9 px, and the true pose is among the roots."""
    rng = np.random.default_rng(0)
    worst, roots, solved = 0.0, 0, 0
    for k in range(1000):
        sc = pu.make_scene(3, seed=1000 + k)
        x, K = sc["pt3d"].astype(np.float64), sc["K"].astype(np.float64)
        if k % 4 == 0:
            e = x[1] - x[0]
            perp = np.cross(e, rng.normal(size=3))
            x[2] = x[0] + e * rng.uniform(0.2, 0.8) + 1e-3 * np.linalg.norm(e) * perp / np.linalg.norm(perp)
        pix, z = pu.project(K, sc["R"], sc["t"], x)
        if not (z > 0.1).all():
            continue
        sols, _ = pu.p3p(pu.bearings(pix, K), x)
        solved += 1
        assert sols, f"triangle {k}: no root"
        for R, t in sols:
            p, zz = pu.project(K, R, t, x)
            assert (zz > 0).all()
            worst = max(worst, float(np.abs(p - pix).max()))
        roots += len(sols)
        assert min(np.abs(R - sc["R"]).max() for R, _ in sols) < 1e-5, f"triangle {k}: the true pose is not among the roots"
    print(f"{solved} triangles, {roots} roots, worst reprojection {worst:.3e} px")
    assert solved >= 900 and worst < 1e-9


def test_sampling_is_distinct_and_independent_of_everything_but_its_key():
    for n in (4, 5, 64, 1000):
        for h in range(50):
            idx = pu.sample_indices(7, h, n)
            assert len(set(idx)) == 4 and all(0 <= i < n for i in idx)
            assert idx == pu.sample_indices(7, h, n)
    assert pu.hash4(0, 0, 0, 0) == pu.mix32(pu.mix32(pu.mix32(pu.mix32(0x9E3779B9))))


def test_solve_pnp_dispatches_gpu(monkeypatch):
    from nerfmatch_amd import nerfmatch_evaluator as ne
    from nerfmatch_amd import pnp_gpu

    seen = []

    def fake(pt2d, pt3d, K, rthres=1, center_subpixel=False):
        seen.append((len(pt2d), rthres, center_subpixel))
        return np.eye(3), np.zeros(3), np.arange(len(pt2d))

    monkeypatch.setattr(pnp_gpu, "solve_pnp", fake)
    res = ne._solve_pnp("gpu", np.zeros((6, 2)), np.zeros((6, 3)), np.eye(3), 2, True)
    assert seen == [(6, 2, True)] and res[0].shape == (3, 3)
    assert ne._solve_pnp("gpu", np.zeros((3, 2)), np.zeros((3, 3)), np.eye(3), 2, True) is None and len(seen) == 1  # fewer than 4 matches
    with pytest.raises(ValueError):
        ne._solve_pnp("gpu2", np.zeros((6, 2)), np.zeros((6, 3)), np.eye(3), 1, False)


def test_argument_validation_without_gpu(built_lib):
    """Null buffers, a hypothesis count that is no multiple of 64 or above 4096, a bad threshold, decreasing host offsets -> NM_ERR_ARG (1);
    a missing or short workspace -> NM_ERR_WORKSPACE (4).  The pointers below are never dereferenced on the device."""
    h = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    Q, K = 2, 10

    def call(pt2d=p, pt3d=p, off=p, off_host=(0, 4, 10), Kmat=p, Q=Q, K=K, thr=1.0, n_hyps=64, iters=10, pose=p, n_inl=p, ws=p, ws_bytes=1 << 20):
        oh = None if off_host is None else (C.c_int * len(off_host))(*off_host)
        return h.nm_pnp_ransac(pt2d, pt3d, off, oh, Kmat, Q, K, thr, n_hyps, iters, 0, 0, pose, n_inl, null, null, null, ws, ws_bytes, null)

    assert h.nm_pnp_ransac_workspace_bytes(16, 1024) == 16 * 8 + 16 * 1024 * 52 and h.nm_pnp_ransac_workspace_bytes(0, 64) == 0
    assert call(pt2d=null) == 1 and call(pt3d=null) == 1 and call(off=null) == 1 and call(Kmat=null) == 1 and call(pose=null) == 1 and call(n_inl=null) == 1
    assert call(Q=0) == 1 and call(K=-1) == 1 and call(thr=0.0) == 1 and call(thr=float("nan")) == 1 and call(iters=-1) == 1
    assert call(n_hyps=0) == 1 and call(n_hyps=100) == 1 and call(n_hyps=32) == 1 and call(n_hyps=4160) == 1
    assert call(off_host=(0, 6, 5)) == 1 and call(off_host=(0, 4, 11)) == 1 and call(off_host=(-1, 4, 10)) == 1  # decreasing / outside [0, K]
    assert call(ws=null) == 4 and call(ws_bytes=64) == 4


def test_symbol_is_declared_exported_and_bound(built_lib):
    h = _lib.lib()
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "nerfmatch_amd.h").read_text(), flags=re.S)
    for name in ("nm_pnp_ransac", "nm_pnp_ransac_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", txt), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES and name not in h._nm_missing and getattr(h, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["nm_pnp_ransac"][1]) == 20
    assert h.nm_abi_version() == 3  # (these two were purely additive: no bump of their own; 3 = the merged per-ray compositing pair)


def test_recorded_bounds():
    """The two bounds of tests/test_pnp_gpu.py, re-measured from the restatement on that file's scenes: the float32 rounding of a hypothesis
    (exact arithmetic on fixed data: reproduces to the digits recorded) and the float32-against-float64 refinement (float32 sums and a
    float32 LAPACK Cholesky: within a factor of 2)."""
    import test_pnp_gpu as T

    worst, all_, total, flagged = pu.measure_hyp_rounding([(T.hyp_scene(n), nh) for counts, nh in T.HYP_RUNS for n in counts], T.SEED)
    print(f"{total} hypotheses, {len(all_)} finite, {flagged} flagged; own-sample residual after float32 rounding: max {worst:.3e} px, "
          f"median {np.median(all_):.2e}, 99th percentile {np.percentile(all_, 99):.2e}")
    assert abs(worst - pu.HYP_RESIDUAL_F32_PX) <= 0.005 * pu.HYP_RESIDUAL_F32_PX
    assert flagged <= 0.02 * total  # the scenes keep the restatement inside what test 1 allows to be excluded
    dR, dt = pu.measure_lm_f32_vs_f64(T.pose_scenes()[3], 256, T.SEED)
    print(f"refinement float32 against float64: {dR:.3e} deg, {dt:.3e}")
    assert pu.LM_F32_VS_F64[0] / 2 <= dR <= pu.LM_F32_VS_F64[0] * 2 and pu.LM_F32_VS_F64[1] / 2 <= dt <= pu.LM_F32_VS_F64[1] * 2
