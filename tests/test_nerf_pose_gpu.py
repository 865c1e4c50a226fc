"""GPU: nm_feature_mutual_nn (cosine mutual nearest neighbours on 128 x 128 register tiles) against the float64 restatement of
tests/nerf_pose_util.py, its tie / sign / padding rules asserted directly, and the two-view pose metrics built on it
(utils.metrics.compute_nerf_pose_metrics, NerfTrainer.validation_step).

Shapes: one entry, fewer rows than a wavefront, exactly one tile, ragged by one on both sides, several tiles each way, and nine row
tiles (two per XCD in the tile mapping).  The comparison rule (gap 2e-4, at most 1 % excused, scores within 1e-4) is in nerf_pose_util.
Exact ties do not go through that rule: equal descriptors give the kernel equal similarities (every entry is the same K-ordered chain on
the same operands, wherever it sits in a tile), so the LOWEST index is demanded."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import nerf_pose_util as pu

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

CASES = [(1, 1, 64), (5, 3, 64), (128, 128, 256), (129, 127, 128), (300, 520, 256), (1100, 260, 64)]


def run(d1, d2, gpu, **kw):
    from nerfmatch_amd import ops

    return ops.feature_mutual_nn(d1.to(gpu), d2.to(gpu), want_nn=True, **kw)


@pytest.mark.parametrize("n1,n2,C", CASES)
def test_parity_with_the_f64_restatement(gpu, built_lib, n1, n2, C):
    d1, d2 = pu.planted(n1, n2, C, 100 + CASES.index((n1, n2, C)))
    m, s, nn12, nn21 = run(d1, d2, gpu)
    assert nn12.dtype == torch.int32 and nn21.dtype == torch.int32 and s.dtype == torch.float32
    ref = pu.check_against_f64(d1, d2, m, s, nn12, nn21, what="planted")
    assert len(ref["matches"]) >= min(n1, n2) // 2  # the planted pairs are found


def _probe(v, g, noise=0.05):
    return v + noise * torch.randn(v.shape, generator=g)


# (first, second): same lane / neighbouring registers; the two lane halves (column bit 2); another 32-column block; another tile
TIE_PAIRS = [(16, 17), (3, 7), (50, 90), (5, 200)]


def test_exact_ties_go_to_the_lowest_column(gpu, built_lib):
    """identical rows in desc2, inside one tile and across a tile boundary: the rows of desc1 nearest to them report the first"""
    g = torch.Generator().manual_seed(11)
    d1, d2 = torch.randn(140, 64, generator=g), torch.randn(300, 64, generator=g)
    for k, (a, b) in enumerate(TIE_PAIRS):
        d2[b] = d2[a]
        d1[10 + 33 * k] = _probe(d2[a], g)
    _, _, nn12, _ = run(d1, d2, gpu)
    ref = pu.mutual_nn_f64(d1, d2)
    for k, (a, b) in enumerate(TIE_PAIRS):
        i = 10 + 33 * k
        assert int(ref["nn12"][i]) == a and float(ref["sim"][i, a]) == float(ref["sim"][i, b])
        assert int(nn12[i]) == a, (i, a, b, int(nn12[i]))


def test_exact_ties_go_to_the_lowest_row(gpu, built_lib):
    """the same in the column direction (rows are spread over lanes, wavefronts and tiles): pairs in one wavefront, in two wavefronts, in
    two tiles"""
    g = torch.Generator().manual_seed(12)
    d1, d2 = torch.randn(300, 64, generator=g), torch.randn(140, 64, generator=g)
    pairs = [(9, 12), (40, 100), (33, 65), (5, 200)]
    for k, (a, b) in enumerate(pairs):
        d1[b] = d1[a]
        d2[10 + 33 * k] = _probe(d1[a], g)
    m, _, nn12, nn21 = run(d1, d2, gpu)
    ref = pu.mutual_nn_f64(d1, d2)
    for k, (a, b) in enumerate(pairs):
        j = 10 + 33 * k
        assert int(ref["nn21"][j]) == a
        assert int(nn21[j]) == a, (j, a, b, int(nn21[j]))
        # both copies point to the probe, only the first is its mutual partner
        assert int(nn12[a]) == j and int(nn12[b]) == j
        rows = m[:, 0].tolist()
        assert a in rows and b not in rows


def test_all_zero_descriptors(gpu, built_lib):
    """an all-zero row normalises to zero: all its similarities are exactly 0, index 0 wins -- also over the zero-padded entries behind the
    matrix's last column / row, which must not take part"""
    g = torch.Generator().manual_seed(13)
    d1, d2 = torch.randn(150, 64, generator=g), torch.randn(300, 64, generator=g)
    d1[77] = 0
    d2[201] = 0
    _, _, nn12, nn21 = run(d1, d2, gpu)
    assert int(nn12[77]) == 0 and int(nn21[201]) == 0
    ref = pu.mutual_nn_f64(d1, d2)
    row_gap, col_gap = pu.gaps(ref["sim"])  # (0 for the two zero descriptors: asserted above instead)
    keep1, keep2 = row_gap >= pu.GAP, col_gap >= pu.GAP
    assert int((~keep1).sum() + (~keep2).sum()) <= 2 + pu.MAX_EXCUSED * 450 and not keep1[77] and not keep2[201]
    assert torch.equal(nn12.cpu().long()[keep1], ref["nn12"][keep1]) and torch.equal(nn21.cpu().long()[keep2], ref["nn21"][keep2])


def test_negative_maxima(gpu, built_lib):
    """(7, 1): desc2[0] = -sum(desc1), every similarity negative: one match with a negative score.  (130, 3): every similarity negative, two
    row tiles, ragged both ways.  An epilogue that compares bit patterns, starts a maximum from -1 or 0, or lets the zero similarities of the
    padded entries compete fails both."""
    g = torch.Generator().manual_seed(14)
    d1 = torch.randn(7, 64, generator=g)
    d2 = -d1.sum(0, keepdim=True)
    m, s, nn12, nn21 = run(d1, d2, gpu)
    ref = pu.check_against_f64(d1, d2, m, s, nn12, nn21, what="negative (7, 1)")
    assert float(ref["sim"].max()) < 0 and len(m) == 1 and float(s[0]) < 0 and m[0].tolist() == [int(ref["nn21"][0]), 0]
    # (all-positive against all-negative vectors have similar similarities: the seed is one for which the restatement's smallest gap,
    # 4.8e-4, is above the excuse threshold -- the 1 % cap allows a single excused row here)
    g = torch.Generator().manual_seed(19)
    d1, d2 = torch.randn(130, 64, generator=g).abs(), -torch.randn(3, 64, generator=g).abs()
    m, s, nn12, nn21 = run(d1, d2, gpu)
    ref = pu.check_against_f64(d1, d2, m, s, nn12, nn21, what="negative (130, 3)")
    assert float(ref["sim"].max()) < 0 and len(m) == len(ref["matches"]) > 0 and float(s.max()) < 0


def test_threshold_is_strict_and_determinism(gpu, built_lib):
    d1, d2 = pu.planted(300, 520, 256, 104)
    first = run(d1, d2, gpu)
    again = run(d1, d2, gpu)
    assert all(torch.equal(a, b) for a, b in zip(first, again))  # the same inputs give the same bytes
    m, s = first[:2]
    thr = float(s.sort().values[len(s) // 2])  # one of the kernel's own scores: `>` drops it, `>=` would keep it
    mt, st = run(d1, d2, gpu, threshold=thr)[:2]
    keep = s > thr
    assert 0 < int(keep.sum()) < len(s) and torch.equal(mt, m[keep]) and torch.equal(st, s[keep])
    for none in (None, 0, 0.0):
        m0, s0 = run(d1, d2, gpu, threshold=none)[:2]
        assert torch.equal(m0, m) and torch.equal(s0, s)
    neg = run(d1, d2, gpu, threshold=-0.5)[:2]  # a negative threshold is truthy and keeps every positive score
    assert torch.equal(neg[0], m)


def test_wrapper_and_empty_sides(gpu, built_lib):
    from nerfmatch_amd import _lib, ops
    from nerfmatch_amd.utils.geometry import mutual_nn_matching

    d1, d2 = pu.planted(129, 127, 128, 103)
    m, s = mutual_nn_matching(d1.to(gpu), d2.to(gpu))
    want = run(d1, d2, gpu)
    assert m.is_cuda and torch.equal(m, want[0]) and torch.equal(s, want[1])
    e = ops.feature_mutual_nn(d1[:0].to(gpu), d2.to(gpu), want_nn=True)
    assert e[0].shape == (0, 2) and e[1].shape == (0,) and e[2].shape == (0,) and e[3].shape == (127,)
    me, se = mutual_nn_matching(d1.to(gpu), d2[:0].to(gpu))
    assert me.shape == (0, 2) and se.shape == (0, 2)
    with pytest.raises(_lib.NerfmatchAmdError, match="supported"):
        ops.feature_mutual_nn(torch.zeros(4, 96, device=gpu), torch.zeros(4, 96, device=gpu))


def multi_tile_outputs():
    """one multi-tile case (C = 256: sixteen K-steps through the ring), for the comparison of the two libraries"""
    d1, d2 = pu.planted(300, 520, 256, 104)
    out = run(d1, d2, torch.device("cuda:0"))
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def test_counted_waits_agree_with_full_waits(gpu, built_lib, tmp_path):
    """the new tile kernel runs sim_tile's counted waits: the -DNM_SAFE_WAIT library, in a fresh process, gives the same bytes"""
    from nerfmatch_amd.build import SAFE_LIB, build

    build(safe=True)
    assert SAFE_LIB.exists()
    dump = tmp_path / "feature_nn_safewait.pt"
    code = (f"import sys, torch; sys.path.insert(0, {str(ROOT)!r}); sys.path.insert(0, {str(ROOT / 'tests')!r}); import test_nerf_pose_gpu as t; "
            f"from nerfmatch_amd import _lib; assert str(_lib.LIB_PATH) == {str(SAFE_LIB)!r}; torch.save(t.multi_tile_outputs(), {str(dump)!r})")
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NERFMATCH_AMD_LIB=str(SAFE_LIB)), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    safe, mine = torch.load(dump), multi_tile_outputs()
    assert len(safe) == len(mine) == 4 and len(mine[0]) > 100
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(mine, safe))


# ------------------------------------------------------------------------------------------------------------------- pose metrics
def test_pose_metrics_on_the_device(gpu, built_lib, monkeypatch):
    from nerfmatch_amd import pnp_gpu
    from nerfmatch_amd.utils.metrics import compute_nerf_pose_metrics, pose_err

    fx = pu.fixture()
    pts, mask, feat, data = pu.pose_inputs(gpu)
    # the sets handed to a solver are the reference's
    rec = pu.Recorder()
    got = compute_nerf_pose_metrics(pts, mask, feat, data, solver=rec)
    pu.check_sets(rec.calls)
    assert got["num_matches"] == int(fx["pm_num_matches"]) and abs(float(got["match_score"]) - fx["pm_match_score"]) <= pu.SCORE_TOL
    # solver="gpu": ONE call with Q = 4 whose poses equal four separate calls on the recorded sets
    calls = []
    inner = pnp_gpu.solve_pnp_batch

    def spy(*a, **kw):
        out = inner(*a, **kw)
        calls.append((a, kw, out))
        return out

    monkeypatch.setattr(pnp_gpu, "solve_pnp_batch", spy)
    got = compute_nerf_pose_metrics(pts, mask, feat, data, solver="gpu", seed=3)
    monkeypatch.undo()
    assert len(calls) == 1
    (p2, p3, counts, Ks), kw, (w2c, n_inl, _) = calls[0]
    assert w2c.shape == (4, 4, 4) and list(counts) == [len(c[0]) for c in rec.calls] and kw["seed"] == 3 and kw["rthres"] == 1
    errs = []
    for q, (s2, s3, K) in enumerate(rec.calls):
        one, n_one, _ = inner(s2.to(gpu), s3.to(gpu), [len(s2)], K[None], rthres=1, seed=3)
        assert torch.equal(one[0], w2c[q]) and int(n_one[0]) == int(n_inl[q]), q
        errs.append(pose_err(fx["pm_c2w"].reshape(2, 4, 4)[q % 2], w2c[q].cpu().inverse()) if int(n_inl[q]) >= 4 else (float("inf"), float("inf")))
    print("inliers of the four problems:", n_inl.tolist(), "errors:", errs)
    assert int(n_inl[0]) >= 4 and int(n_inl[1]) >= 4  # the depth problems are exact geometry truncated to whole pixels
    want = dict(R_err_depth=0.5 * (errs[0][0] + errs[1][0]), t_err_depth=0.5 * (errs[0][1] + errs[1][1]) * 100,
                R_err_match=0.5 * (errs[2][0] + errs[3][0]), t_err_match=0.5 * (errs[2][1] + errs[3][1]) * 100)
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    assert set(got) == set(pu.KEYS)


def _two_view_batch(gpu, w, h):
    from nerfmatch_amd import synth
    from test_nerf_train_gpu import make_rays

    n = 2 * w * h
    g = torch.Generator().manual_seed(51)
    c2w = torch.cat([synth.camera_pose(1), synth.camera_pose(2)])[None]
    K = torch.cat([synth.intrinsics(h, w, 30.0)] * 2)[None]
    batch = dict(rays=make_rays(n, 17, scale=1.0)[None].to(gpu), rgbs=torch.rand(1, n, 3, generator=g).to(gpu), seq_ind=[1, 2], img_idx=[0, 1],
                 img_wh=torch.tensor([[w, h]]), c2w=c2w, K=K, unnorm_scene=synth.unnorm_scene()[None])
    draws = dict(t_rand=torch.rand(n, 33, generator=g).to(gpu), jitter=synth.resample_jitter((n, 33), 53).to(gpu))
    return batch, draws


def test_validation_step_adds_the_pose_metrics(gpu, built_lib):
    from nerfmatch_amd import synth
    from nerfmatch_amd.nerf_trainer import NerfTrainer, init_pfeat_mask
    from nerfmatch_amd.utils.geometry import mutual_nn_matching

    w, h = 32, 24
    cfg = synth.nerf_config("7scenes", num_pts=32, img_wh=(w, h))
    cfg.data.train_pair_txt = "pairs.txt"
    tr = NerfTrainer(cfg, num_frames=5, device=gpu)
    tr.model.load_state_dict(synth.nerf_state_dict(seed=0, density_bias=3.0))
    batch, draws = _two_view_batch(gpu, w, h)
    assert tuple(tr.model.pfeat_mask.shape) == (2, w, h, 1)
    metrics = tr.validation_step(batch, **draws)
    assert set(pu.KEYS) < set(metrics) and "rgb_fine_psnr" in metrics and "loss" in metrics
    tr.model.ret_pfeat = True
    seq = torch.tensor([1, 2]).repeat_interleave(w * h)
    preds = tr.model.render_rays(batch["rays"][0], ray_id=seq, validation=True, **draws)
    kept = (w // 8) * (h // 8)
    assert preds["feat_fine"].shape == (2 * kept, 256)
    f1, f2 = preds["feat_fine"].reshape(2, kept, 256)
    m, s = mutual_nn_matching(f1, f2)
    assert metrics["num_matches"] == len(m) and (len(m) == 0 or float(metrics["match_score"]) == float(s.mean()))
    # one view: exactly the scalar metrics of the render
    one = {k: (v[:, : w * h] if k in ("rays", "rgbs") else v) for k, v in batch.items()}
    one.update(seq_ind=[1], img_idx=[0])
    tr.model.pfeat_mask = init_pfeat_mask((w, h), ds=8, sample_num=1)
    single = tr.validation_step(one, **{k: v[: w * h] for k, v in draws.items()})
    assert set(single) == {"rgb_coarse_mse", "rgb_coarse_psnr", "rgb_fine_mse", "rgb_fine_psnr", "loss"}
