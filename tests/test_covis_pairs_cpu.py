"""CPU: the torch rule of nerfmatch_amd.covis_pairs (what the kernels of csrc/covis_pairs.hip are tested against) on a scene with planted
answers, the top-k against a Python sort, exact image-border and depth-tolerance boundaries, row subsets and sub-banks, the pair files,
the factored camera rows, and the C entry points' argument checks (no device needed: every check precedes the first HIP call).
Every comparison is exact equality of integers."""
import ctypes as C

import pytest
import torch

import covis_util as cu
import ref_bank_util as ru
from nerfmatch_amd import _lib, supervision, synth
from nerfmatch_amd import covis_pairs as cp
from nerfmatch_amd.ref_bank import ReferencePointBank

F, SEED, FLIP, TOL = 12, 3, (5,), 0.05


def _scores(sc, frames=None, **kw):
    return cp.covisibility_scores(*cu.rule_args(sc, frames), **kw)


def test_planted_answers():
    sc = cu.scene(F, SEED, FLIP)
    plain, depth = _scores(sc), _scores(sc, depth_tol=TOL, grid_wh=sc["grid_wh"])
    assert plain.dtype == torch.int32 and plain.shape == (F, F)
    want_diag = [0 if f in FLIP else cu.N for f in range(F)]
    assert plain.diagonal().tolist() == want_diag and depth.diagonal().tolist() == want_diag
    assert bool((depth <= plain).all()) and not torch.equal(depth, plain)
    off = plain[~torch.eye(F, dtype=torch.bool)]
    assert int(off.min()) == 0 and 0 < int(off.max()) <= cu.N and len(set(off.tolist())) > 10  # spread over 0 .. 48
    for s in (plain, depth):
        assert not s[5].any() and not s[:, 5].any()
    for kw in (dict(), dict(depth_tol=TOL, grid_wh=sc["grid_wh"])):
        ids, n_pairs = cp.covisibility_pairs(*cu.rule_args(sc), k=3, **kw)
        assert ids[5].tolist() == [-1, -1, -1] and int(n_pairs[5]) == 0 and not bool((ids == 5).any())
    a = cp.covisibility_pairs(*cu.rule_args(sc), k=3)[0]
    b = cp.covisibility_pairs(*cu.rule_args(sc), k=3, depth_tol=TOL, grid_wh=sc["grid_wh"])[0]
    assert int((a != b).any(1).sum()) == 4  # the occluder changes the top-3 of 4 of the 12 frames


def test_points_behind_a_camera_are_not_seen():
    """where ref_bank.visibility_words has no depth-sign test (a quirk of the reference it reproduces), this rule has one"""
    sc = cu.scene(F, SEED, FLIP)
    pt3d, pt_mask, cams, img_wh = cu.rule_args(sc)
    K, w2c = cams[:, :9].reshape(-1, 3, 3), cams[:, 9:].reshape(-1, 3, 4)
    pix, pz = supervision._project_torch(K[5:6], w2c[5:6], pt3d.reshape(1, -1, 3))
    inside = (pix[..., 0] >= 0) & (pix[..., 1] >= 0) & (pix[..., 0] < cu.W) & (pix[..., 1] < cu.H)
    assert int(inside.sum()) > 0 and bool((pz[inside] < 0).all())  # the flipped frame: mirrored projections inside the image
    assert not _scores(sc, rows=[5]).any()


def test_a_duplicated_frame():
    sc = cu.scene(F, SEED, FLIP)
    a, b = 2, 9
    frames = list(range(F))
    frames[b] = a
    for kw in (dict(), dict(depth_tol=TOL, grid_wh=sc["grid_wh"])):
        s = _scores(sc, frames, **kw)
        assert torch.equal(s[:, a], s[:, b]) and torch.equal(s[a], s[b])
        ids, _ = cp.covisibility_pairs(*cu.rule_args(sc, frames), k=F, **kw)
        both = 0
        for row in ids.tolist():
            if a in row and b in row:
                both += 1
                assert row.index(a) < row.index(b)  # equal scores: the lower index first
        assert both >= 3


@pytest.mark.parametrize("k,min_score", [(1, 1), (3, 1), (20, 1), (64, 1), (5, 30), (20, 49), (4, 0)])
def test_topk_is_the_python_sort(k, min_score):
    sc = cu.scene(F, SEED, FLIP)
    scores = _scores(sc)
    ids, n_pairs = cp.covisibility_pairs(*cu.rule_args(sc), k=k, min_score=min_score)
    w_ids, w_n = cu.python_topk(scores, range(F), k, min_score)
    assert ids.dtype == torch.int32 and n_pairs.dtype == torch.int32 and torch.equal(ids, w_ids) and torch.equal(n_pairs, w_n)
    assert all(q not in row for q, row in enumerate(ids.tolist()))  # self is never listed
    if k >= F:
        assert bool((ids[:, F - 1 :] == -1).all()) and int(n_pairs.max()) <= F - 2  # (frame 5 is nobody's candidate)
    if min_score == 49:
        assert not n_pairs.any() and bool((ids == -1).all())
    if min_score == 30:
        assert 0 < int(n_pairs.sum()) < 5 * F and int(n_pairs.min()) == 0  # the threshold cuts lists short
    t_ids, t_n = cp.topk_pairs(scores, None, k, min_score)
    assert torch.equal(t_ids, ids) and torch.equal(t_n, n_pairs)


def test_exact_boundaries():
    pt3d, pt_mask, cams, img_wh, grid_wh, expect, expect_depth = cu.boundary_bank()
    zself = cp.self_depth(pt3d, cams)
    assert zself[0].tolist() == [2.0] * 5 + [-1.0, 2.0, 2.0]
    rows = torch.tensor([0])
    seen = cp._seen_torch(pt3d, pt_mask, cams, rows, img_wh, None, None, None)[0]
    assert torch.equal(seen[1:], expect)
    seen_d = cp._seen_torch(pt3d, pt_mask, cams, rows, img_wh, zself, grid_wh, 0.25)[0]
    assert torch.equal(seen_d[1:], expect_depth)
    assert cp.covisibility_scores(pt3d, pt_mask, cams, img_wh, rows=[0])[0, 1:].tolist() == [6, 0]
    assert cp.covisibility_scores(pt3d, pt_mask, cams, img_wh, rows=[0], depth_tol=0.25, grid_wh=grid_wh)[0, 1:].tolist() == [3, 0]
    # the mask of the points themselves: a masked probe is not counted
    pt_mask[1, 0] = False
    assert cp.covisibility_scores(pt3d, pt_mask, cams, img_wh, rows=[0])[0, 1:].tolist() == [5, 0]


def test_rows_and_sub_banks():
    sc = cu.scene(F, SEED, FLIP)
    for kw in (dict(), dict(depth_tol=TOL, grid_wh=sc["grid_wh"])):
        full = _scores(sc, **kw)
        ids, n_pairs = cp.covisibility_pairs(*cu.rule_args(sc), k=4, **kw)
        for rows in ([7], [11, 0, 3, 3], list(range(F))[::-1]):
            assert torch.equal(_scores(sc, rows=rows, **kw), full[rows])
            r_ids, r_n = cp.covisibility_pairs(*cu.rule_args(sc), rows=rows, k=4, **kw)
            assert torch.equal(r_ids, ids[rows]) and torch.equal(r_n, n_pairs[rows])
        sub = [8, 1, 5, 10, 3]
        assert torch.equal(_scores(sc, sub, **kw), full[sub][:, sub])  # a pair's score depends on the two frames alone
    # the chunked passes of the host rule do not show
    args = cu.rule_args(sc)
    assert torch.equal(cp._scores_torch(*args[:3], torch.arange(F), args[3], None, None, chunk=1), _scores(sc))


def test_pair_files_round_trip(tmp_path):
    sc = cu.scene(F, SEED, FLIP)
    names = [f"seq-01/frame-{f:06d}.color.png" for f in range(F)]
    rows = [4, 0, 5, 9]
    ids, n_pairs = cp.covisibility_pairs(*cu.rule_args(sc), rows=rows, k=3)
    want = cp.pairs_dict(rows, ids)
    assert list(want) == rows and want[5] == [] and all(len(want[q]) == int(n) for q, n in zip(rows, n_pairs))
    path = tmp_path / "pairs-db-covis3.txt"
    assert cp.write_pairs_txt(path, names, rows, ids) == int(n_pairs.sum())
    lines = path.read_text().splitlines()
    assert len(lines) == int(n_pairs.sum()) and all(len(line.split()) == 2 for line in lines)
    assert [line.split()[0] for line in lines] == [names[q] for q in rows for _ in want[q]]  # the queries in row order
    got = cp.read_pairs_txt(path, names, names)
    assert got == {q: r for q, r in want.items() if r}  # (a query without pairs has no line)
    # unknown names are skipped: a reference list without frame want[4][0], a query list without frame 0
    gone = want[4][0]
    rnames = [n if f != gone else "elsewhere.png" for f, n in enumerate(names)]
    got = cp.read_pairs_txt(path, names[1:], rnames)  # (query ids shift by one)
    assert got == {q - 1: [r for r in rids if r != gone] for q, rids in want.items() if rids and q != 0}
    assert gone not in got[3] and len(got[3]) == len(want[4]) - 1
    with pytest.raises(ValueError, match="white space"):
        cp.write_pairs_txt(path, ["a b"] * F, rows, ids)
    assert cp.pairs_dict(None, ids[:2]) == {0: want[4], 1: want[0]}


def test_camera_rows_are_the_banks_rows():
    args = ru.synth_args(F=4, n=6, D=4, seed=2)
    Ks = torch.stack([synth.intrinsics(ru.H, ru.W, ru.FOCAL), synth.intrinsics(2 * ru.H, 2 * ru.W, 2 * ru.FOCAL), synth.intrinsics(ru.H, ru.W, 50.0),
                      synth.intrinsics(3 * ru.H, 3 * ru.W, 100.0)])
    whs = torch.tensor([(ru.W, ru.H), (2 * ru.W, 2 * ru.H), (ru.W, ru.H), (3 * ru.W, 3 * ru.H)])
    bank = ReferencePointBank(args["pt3d"], args["pt_feat"], args["c2w"], Ks, whs, (ru.W, ru.H), pt_mask=args["pt_mask"], device="cpu")
    cams = cp.camera_rows(args["c2w"], Ks, whs, (ru.W, ru.H))
    assert cams.shape == (4, 21) and cams.dtype == torch.float32 and torch.equal(bank.cams, cams)
    scale = torch.stack([ru.W / whs[:, 0].float(), ru.H / whs[:, 1].float(), torch.ones(4)], -1)
    assert torch.equal(cams[:, :9].reshape(4, 3, 3), scale[:, :, None] * Ks)
    assert torch.equal(cams[:, 9:].reshape(4, 3, 4), supervision.w2c_from_c2w(args["c2w"]))
    assert torch.equal(cp.camera_rows(args["c2w"], Ks[0], (ru.W, ru.H), (ru.W, ru.H))[:, :9], Ks[0].reshape(1, 9).expand(4, 9))
    # the bank's method hands its own tensors to the module function
    ids, n_pairs = bank.covisibility_pairs(k=2)
    w_ids, w_n = cp.covisibility_pairs(bank.pt3d, bank.pt_mask, bank.cams, bank.img_wh, k=2)
    assert torch.equal(ids, w_ids) and torch.equal(n_pairs, w_n)
    with pytest.raises(ValueError, match="both depth_tol and ds"):
        bank.covisibility_pairs(depth_tol=0.1)


def test_python_argument_checks():
    sc = cu.scene(F, SEED, FLIP)
    pt3d, pt_mask, cams, img_wh = cu.rule_args(sc)
    bad = [dict(rows=[F]), dict(rows=[-1]), dict(rows=[]), dict(depth_tol=0.1), dict(grid_wh=(8, 6)), dict(depth_tol=0.1, grid_wh=(8, 5)),
           dict(depth_tol=-0.1, grid_wh=(8, 6)), dict(depth_tol=float("nan"), grid_wh=(8, 6))]
    for kw in bad:
        with pytest.raises(ValueError):
            cp.covisibility_scores(pt3d, pt_mask, cams, img_wh, **kw)
    for k in (0, 65):
        with pytest.raises(ValueError, match="between 1 and 64"):
            cp.covisibility_pairs(pt3d, pt_mask, cams, img_wh, k=k)
    with pytest.raises(ValueError, match="pt_mask"):
        cp.covisibility_scores(pt3d, pt_mask[:, :5], cams, img_wh)
    with pytest.raises(ValueError, match="cams"):
        cp.covisibility_scores(pt3d, pt_mask, cams[:, :20], img_wh)
    with pytest.raises(ValueError, match="sides"):
        cp.covisibility_scores(pt3d, pt_mask, cams, (8193, 48))


def test_argument_validation_without_gpu(built_lib):
    """Null pointers, non-positive sizes, gw gh != n, a grid without a depth map, a negative or non-finite tolerance, k = 0 -> NM_ERR_ARG
    (1); k = 65, more than 2^20 frames, points or rows, Q F above 2^31, a side above 8192 -> NM_ERR_UNSUPPORTED (2).  All returned before
    anything is enqueued (the pointers below are never dereferenced)."""
    h = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    A, U = 1, _lib.NM_ERR_UNSUPPORTED

    def depth(pt3d=p, mask=null, cams=p, F=3, n=48, z=p):
        return h.nm_covis_self_depth(pt3d, mask, cams, F, n, z, null)

    assert depth(pt3d=null) == A and depth(cams=null) == A and depth(z=null) == A and depth(F=0) == A and depth(n=-4) == A
    assert depth(F=(1 << 20) + 1) == U and depth(n=(1 << 20) + 1) == U

    def scores(pt3d=p, mask=p, cams=p, rows=null, z=p, F=3, n=48, Q=3, w=64, hh=48, gw=8, gh=6, tol=0.05, out=p):
        return h.nm_covis_scores(pt3d, mask, cams, rows, z, F, n, Q, w, hh, gw, gh, tol, out, null)

    assert scores(pt3d=null) == A and scores(mask=null) == A and scores(cams=null) == A and scores(out=null) == A
    assert scores(F=0) == A and scores(n=0) == A and scores(Q=-1) == A and scores(w=0) == A and scores(hh=-48) == A
    assert scores(gw=8, gh=5) == A and scores(gw=0, gh=0) == A and scores(gw=-8, gh=-6) == A  # gw gh != n
    assert scores(tol=-0.01) == A and scores(tol=float("nan")) == A and scores(tol=float("inf")) == A
    assert scores(z=null) == A  # a grid without a depth map
    assert scores(F=(1 << 20) + 1) == U and scores(n=(1 << 20) + 1, gw=(1 << 20) + 1, gh=1) == U and scores(Q=(1 << 20) + 1) == U
    assert scores(F=1 << 20, Q=(1 << 11) + 1) == U  # Q F above 2^31
    assert scores(w=8193) == U and scores(hh=8193) == U and scores(n=8193, gw=8193, gh=1) == U

    def topk(s=p, rows=null, Q=3, F=3, k=20, ids=p, n_pairs=p):
        return h.nm_covis_topk(s, rows, Q, F, k, 1, ids, n_pairs, null)

    assert topk(s=null) == A and topk(ids=null) == A and topk(n_pairs=null) == A and topk(Q=0) == A and topk(F=-3) == A
    assert topk(k=0) == A and topk(k=-1) == A and topk(k=65) == U and topk(F=(1 << 20) + 1) == U and topk(Q=(1 << 11) + 1, F=1 << 20) == U
    assert h.nm_abi_version() == 3 and cp.QUERY_TILE == 32
