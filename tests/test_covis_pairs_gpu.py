"""GPU: nm_covis_self_depth / nm_covis_scores / nm_covis_topk (csrc/covis_pairs.hip) through nerfmatch_amd.covis_pairs against the host
rule on the same tensors: torch.equal on scores, ids and n_pairs -- integers, no tolerance anywhere.

Shapes: F of 1, 2, T - 1, T, T + 1 and 2 T + 1 around the query tile T, row lists of length 1 and T + 1 out of order; n of 1, 63, 64, 65
(a wavefront and its neighbours), 255, 256, 257 (a workgroup) and 1025 (one point past the block of four points per thread); n = 4800 on
the 80 x 60 grid of a 640 x 480 frame with the depth test; k of 1, 20 and 64 with fewer than k candidates."""
import pytest
import torch

import covis_util as cu
import ref_bank_util as ru
from nerfmatch_amd import covis_pairs as cp
from nerfmatch_amd import synth
from nerfmatch_amd.ref_bank import ReferencePointBank

pytestmark = pytest.mark.gpu

T = cp.QUERY_TILE
TOL = 0.05


def bank_args(F, n, seed, **kw):
    """(pt3d, pt_mask, cams, img_wh) of a ref_bank_util.synth_args bank (random points in a slab in front of the cameras, random masks)"""
    a = ru.synth_args(F, n, 4, seed=seed, **kw)
    return a["pt3d"], a["pt_mask"], cp.camera_rows(a["c2w"], a["K"], a["frame_wh"], a["img_wh"]), a["img_wh"]


@pytest.mark.parametrize("F", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_frame_and_tile_edges(gpu, built_lib, F):
    sc = cu.scene(F, 3, flip=(5,) if F > 5 else ())
    args = cu.rule_args(sc)
    for kw in (dict(), dict(depth_tol=TOL, grid_wh=sc["grid_wh"])):
        s = cu.assert_kernels_equal_rule(args, gpu, ks=(1, 20), **kw)
        assert s.diagonal().tolist() == [0 if f == 5 else cu.N for f in range(F)]


@pytest.mark.parametrize("rows", [[T], [3, 2 * T, 0, 3] + list(range(T + 2, 5, -1))[: T - 3]])
def test_row_lists_out_of_order(gpu, built_lib, rows):
    assert len(rows) in (1, T + 1)
    sc = cu.scene(2 * T + 1, 3, flip=(5,))
    for kw in (dict(), dict(depth_tol=TOL, grid_wh=sc["grid_wh"])):
        s = cu.assert_kernels_equal_rule(cu.rule_args(sc), gpu, rows=rows, ks=(4,), **kw)
        assert s.shape == (len(rows), 2 * T + 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_point_counts(gpu, built_lib, n):
    s = cu.assert_kernels_equal_rule(bank_args(5, n, seed=n), gpu, ks=(3,))
    assert int(s.max()) > 0 or n == 1


def test_full_size_with_the_depth_test(gpu, built_lib):
    """n = 4800: the 80 x 60 cells of a 640 x 480 frame.  The bank's points are random, not a depth map, so the occlusion test rejects
    most of them; a last frame whose points ARE its depth map (one per cell centre, at depth 2) scores n on its own diagonal."""
    F, n, gw, gh = 17, 4800, 80, 60
    a = ru.synth_args(F, n, 4, seed=7)
    a["K"], a["frame_wh"], a["img_wh"] = synth.intrinsics(480, 640, 525.0), (640, 480), (640, 480)
    a["c2w"][-1] = torch.eye(4)
    c = torch.arange(n)
    a["pt3d"][-1] = torch.stack([((c % gw) * 8 + 4 - 320.0) / 525.0 * 2, ((c // gw) * 8 + 4 - 240.0) / 525.0 * 2, torch.full((n,), 2.0)], -1)
    a["pt_mask"][-1] = True
    args = (a["pt3d"], a["pt_mask"], cp.camera_rows(a["c2w"], a["K"], a["frame_wh"], a["img_wh"]), a["img_wh"])
    s = cu.assert_kernels_equal_rule(args, gpu, depth_tol=TOL, grid_wh=(gw, gh), ks=(20,))
    assert int(s[-1, -1]) == n and int(s[:-1].sum()) > 0
    cu.assert_kernels_equal_rule(args, gpu, rows=[16, 2], ks=(2,))


@pytest.mark.parametrize("depth_tol", [None, 0.0, 0.05])
def test_the_planted_scene(gpu, built_lib, depth_tol):
    sc = cu.scene(12, 3, flip=(5,))
    frames = list(range(12))
    frames[9] = 2  # a duplicated frame
    pt3d, pt_mask, cams, img_wh = cu.rule_args(sc, frames)
    pt_mask = pt_mask & (torch.arange(12 * cu.N).reshape(12, cu.N) % 7 != 3)  # masks: on the counted points and on the depth maps
    kw = dict() if depth_tol is None else dict(depth_tol=depth_tol, grid_wh=sc["grid_wh"])
    s = cu.assert_kernels_equal_rule((pt3d, pt_mask, cams, img_wh), gpu, ks=(3, 12), **kw)
    assert torch.equal(s[:, 2], s[:, 9]) and not s[5].any() and not s[:, 5].any()
    assert s.diagonal().tolist() == [0 if f == 5 else int(pt_mask[f].sum()) for f in range(12)]


def test_exact_boundaries(gpu, built_lib):
    pt3d, pt_mask, cams, img_wh, grid_wh, expect, expect_depth = cu.boundary_bank()
    args = (pt3d, pt_mask, cams, img_wh)
    s = cu.assert_kernels_equal_rule(args, gpu, ks=(2,))
    assert s[0, 1:].tolist() == [int(expect[0].sum()), int(expect[1].sum())] == [6, 0]
    s = cu.assert_kernels_equal_rule(args, gpu, depth_tol=0.25, grid_wh=grid_wh, ks=(2,))
    assert s[0, 1:].tolist() == [int(expect_depth[0].sum()), 0] == [3, 0]
    # one probe at a time: every boundary on its own
    dev = cu.to_gpu(args, gpu)
    for r in range(expect.numel()):
        only = torch.zeros_like(pt_mask)
        only[0] = pt_mask[0]
        only[1 + r // 8, r % 8] = True
        got = cp.covisibility_scores(dev[0], only.to(gpu), dev[2], img_wh, rows=[0]).cpu()
        assert got[0, 1:].sum().item() == int(expect.reshape(-1)[r]), r
        got = cp.covisibility_scores(dev[0], only.to(gpu), dev[2], img_wh, rows=[0], depth_tol=0.25, grid_wh=grid_wh).cpu()
        assert got[0, 1:].sum().item() == int(expect_depth.reshape(-1)[r]), r
    z = cu.to_gpu((cp.self_depth(pt3d, cams),), gpu)[0]
    from nerfmatch_amd import ops

    assert ru.same_bits(ops.covis_self_depth(dev[0], dev[2]), z)
    masked = ops.covis_self_depth(dev[0], dev[2], dev[1])  # the depth map the scores kernel gathers from: NaN where the mask is clear
    assert torch.equal(torch.isnan(masked), torch.isnan(z) | ~dev[1]) and ru.same_bits(torch.where(dev[1], masked, z), z)


@pytest.mark.parametrize("k", [1, 20, 64])
def test_topk_shapes(gpu, built_lib, k):
    sc = cu.scene(12, 3, flip=(5,))
    s = cu.assert_kernels_equal_rule(cu.rule_args(sc), gpu, ks=(k,))
    ids, n_pairs = cp.covisibility_pairs(*cu.to_gpu(cu.rule_args(sc), gpu), k=k)
    w_ids, w_n = cu.python_topk(s, range(12), k)
    assert torch.equal(ids.cpu(), w_ids) and torch.equal(n_pairs.cpu(), w_n)
    if k > 11:
        assert bool((ids[:, 11:] == -1).all()) and int(n_pairs.max()) <= 10
    for min_score in (0, 30, 49):
        cu.assert_kernels_equal_rule(cu.rule_args(sc), gpu, ks=(k,), min_score=min_score)


def test_two_calls_give_identical_bytes(gpu, built_lib):
    dev = cu.to_gpu(bank_args(T + 3, 1500, seed=11), gpu)
    sc = cu.scene(T + 1, 3, flip=(5,))
    dsc = cu.to_gpu(cu.rule_args(sc), gpu)
    for args, kw in ((dev, dict()), (dsc, dict(depth_tol=TOL, grid_wh=sc["grid_wh"]))):
        a, b = cp.covisibility_scores(*args, **kw), cp.covisibility_scores(*args, **kw)
        assert torch.equal(a, b)
        (ia, na), (ib, nb) = cp.covisibility_pairs(*args, k=20, **kw), cp.covisibility_pairs(*args, k=20, **kw)
        assert torch.equal(ia, ib) and torch.equal(na, nb)


def test_bank_method_end_to_end(gpu, built_lib):
    a = ru.synth_args(9, 48, 8, seed=5)
    dev, host = ReferencePointBank(**a, device=gpu), ReferencePointBank(**a, device="cpu")
    ref_ids = torch.tensor([[0, 3, 8], [4, 4, 1]])
    before = dev.reference_sets(ref_ids.to(gpu), sample_mode="rand", sample_pts=40)
    for kw in (dict(k=4), dict(k=4, depth_tol=0.3, ds=8), dict(k=2, rows=[8, 1], min_score=3)):
        ids, n_pairs = dev.covisibility_pairs(**kw)
        grid = dict(grid_wh=(ru.W // 8, ru.H // 8)) if "ds" in kw else {}
        mkw = {key: v for key, v in kw.items() if key != "ds"}
        m_ids, m_n = cp.covisibility_pairs(dev.pt3d, dev.pt_mask, dev.cams, dev.img_wh, **mkw, **grid)
        h_ids, h_n = host.covisibility_pairs(**kw)
        assert ids.is_cuda and torch.equal(ids, m_ids) and torch.equal(n_pairs, m_n)
        assert torch.equal(ids.cpu(), h_ids) and torch.equal(n_pairs.cpu(), h_n)
    assert int(dev.covisibility_pairs(k=4)[1].sum()) > 0
    pair_ids = cp.pairs_dict(None, dev.covisibility_pairs(k=4)[0])
    assert sorted(pair_ids) == list(range(9)) and all(q not in r for q, r in pair_ids.items())
    data = dev.fill({}, torch.tensor([dev.draw_ref_ids(pair_ids[0] or [1], 3, "train", rng=__import__("numpy").random.default_rng(0))]).to(gpu),
                    sample_mode="rand", sample_pts=40)
    assert data["pt3d"].shape == (1, 40, 3)
    after = dev.reference_sets(ref_ids.to(gpu), sample_mode="rand", sample_pts=40)
    ru.assert_same_sets(after, before)  # the bank's sets are unchanged by it
    ru.assert_same_sets(after, host.reference_sets(ref_ids, sample_mode="rand", sample_pts=40))
    assert dev.bad_ids == 0
