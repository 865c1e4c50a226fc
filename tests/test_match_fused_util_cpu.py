"""What test_match_fused_routes_gpu.py relies on (match_fused_util.py), checked without a GPU: the case table reaches the edges it names, every
decision of the float64 oracle outside a designed exact tie is 50 * TIE_REL from flipping, the designed ties are exact ties that the oracle
resolves to the lowest unmasked column, and the entry point's argument checks."""
import ctypes as C

import pytest
import torch

import match_fused_util as fu
from conftest import TIE_REL


def test_geometry_reports_the_edges_of_the_tile_cases():
    want = {(1, 1): (1, 1), (31, 33): (1, 1), (128, 128): (1, 1), (129, 127): (2, 1), (897, 130): (8, 1), (1025, 130): (9, 2), (2049, 70): (17, 3),
            (130, 641): (2, 1)}
    assert set(fu.TILE_SHAPES) == set(want)
    for (M, N), (tm, rpx) in want.items():
        g = fu.geometry(M, N)
        print(f"{M} x {N}: {g}")
        assert (g.tiles_m, g.rpx) == (tm, rpx) and g.grid == 8 * rpx * g.tiles_n and g.early == g.grid - tm * g.tiles_n
        assert all(f"tile-{M}x{N}-{m}" in fu.CASE for m in ("mutual", "rowmax"))
    # the neighbours of the rpx step: 8 row tiles fill the 8 XCDs, 9 leave XCDs 5..7 (row tiles 10..15) without work, 17 needs rpx = 3
    assert fu.geometry(897, 130).early == 0 and fu.geometry(1025, 130).early == 7 * 2 and fu.geometry(2049, 70).early == 7
    rpx = fu.geometry(1025, 130).rpx
    assert [x for x in range(8) if all(x * rpx + j >= 9 for j in range(rpx))] == [5, 6, 7]
    # one partly filled 32-row group: a single live wavefront; and M = 1
    assert fu.geometry(31, 33).live_waves_last == 1 and fu.geometry(1, 1).groups == 1 and fu.geometry(129, 127).live_waves_last == 1
    # tiles_n = 6: wavefronts 0 and 1 of match_select take two tiles each
    assert fu.geometry(130, 641).tiles_n == 6 and [len(range(w, 6, 4)) for w in range(4)] == [2, 2, 1, 1]
    # compaction: two sweeps of 1024 rows
    assert all(fu.CASE[n].M == 1153 and fu.CASE[n].N >= 1153 and not fu.CASE[n].mutual for n in ("compact-1153-all", "compact-1153-none", "compact-1153-second-sweep"))
    assert {c.C for c in fu.CASES} == {64, 128, 256, 512} and {c.P for c in fu.CASES} == {1, 3, 16}
    assert {c.group for c in fu.CASES} == set(fu.GROUPS)


def test_tie_layouts_reach_the_positions_they_name():
    lay = {name: (N, groups) for name, N, groups in fu.TIE_LAYOUTS}
    tile = lambda c: c // fu.FT
    for a, b in lay["same-half"][1]:
        assert tile(a) == tile(b) and fu.lane_half(a) == fu.lane_half(b) and fu.column_class(a) == fu.column_class(b)
    for a, b in lay["other-half"][1]:
        assert b == a + 4 and a // 8 == b // 8 and fu.lane_half(a) != fu.lane_half(b)
    sweep = lay["other-class"][1]
    assert [g for g in sweep[:8]] == [(c, c + 8) for c in range(8)] and all(fu.column_class(a) != fu.column_class(b) and tile(a) == tile(b) for a, b in sweep)
    assert {fu.column_class(a) for a, _ in sweep} == {0, 1}  # both directions: the lower copy in class 0 and in class 1
    assert all(tile(a) != tile(b) and fu.column_class(a) == fu.column_class(b) for a, b in lay["tiles-same-class"][1])
    assert all(tile(a) != tile(b) and fu.column_class(a) != fu.column_class(b) for a, b in lay["tiles-other-class"][1])
    assert [tile(c) for c in lay["three-tiles"][1][0]] == [0, 1, 5] and lay["three-tiles"][0] == 641
    for name, (N, groups) in lay.items():
        cols = [c for g in groups for c in g]
        assert len(set(cols)) == len(cols) and max(cols) < N, name
        for M in ((130, 1025) if name == "other-class" else (130,)):
            assert all(f"tie-{name}-M{M}-{m}{h}" in fu.CASE for m in ("mutual", "rowmax") for h in ("", "-hidden"))
    assert fu.column_class(7) == 0 and fu.column_class(15) == 1 and fu.column_class(100) == fu.column_class(101) == 0  # (the old tie test: one class)


@pytest.mark.parametrize("case", fu.CASES, ids=lambda c: c.name)
def test_every_row_is_decisive_or_a_designed_tie(case):
    """The condition the identical-index-lists comparison rests on, and what the designed ties are in the oracle."""
    assert fu.MARGIN == 50 * TIE_REL == 1e-3
    x, ref = fu.inputs_of(case), fu.oracle_of(case)
    for p, (conf, ii, jj, mconf) in enumerate(ref):
        assert fu.undecided_rows(conf, case.mutual, x["thr"]) == []
        assert torch.isfinite(conf).all() and torch.all(ii[1:] > ii[:-1])
        got = dict(zip(ii.tolist(), jj.tolist()))
        ties = fu.tie_rows(conf)
        kind = case.masks[p]
        ptm = x["pt_mask"][p] if x["pt_mask"] is not None else torch.ones(case.N, dtype=torch.uint8)
        imm = x["im_mask"][p] if x["im_mask"] is not None else torch.ones(case.M, dtype=torch.uint8)
        allowed = [set(g) for g in case.dups]
        for r, cols in ties.items():
            if kind in ("pt-all", "im-all"):  # one side entirely masked: conf = 1 / (M N) everywhere, the first column of every row
                assert cols == list(range(case.N)) and got[r] == 0
                continue
            if imm[r] == 0:  # a masked row meets the masked columns: two flat soft-maxes
                assert cols == torch.nonzero(ptm == 0)[:, 0].tolist()
                continue
            assert any(set(cols) <= g for g in allowed), (case.name, p, r, cols)
            assert all(ptm[c] for c in cols)  # a hidden copy has conf 0: it is no part of the tie
            if r in got:
                assert got[r] == min(cols)
        if kind in ("pt-all", "im-all"):
            assert len(ties) == case.M and len(ii) == case.M
        # the designed ties exist: the planted row of every duplicate group attains its maximum in all unmasked copies, first copy returned
        for k, g in enumerate(case.dups):
            live = [c for c in g if ptm[c]]
            assert torch.equal(x["pt"][p][list(g)], x["pt"][p][g[0]].expand(len(g), -1))
            assert (ties[k] == live if len(live) > 1 else k not in ties) and got[k] == live[0] and live[0] == (g[1] if case.hide else g[0])
            assert bool((conf[:, live] == conf[:, live[:1]]).all())  # equal bits in every row, not only the planted one
        for g in case.dup_rows:  # bit-identical image rows: equal rows of conf; under mutual matching all of them keep the planted column
            assert bool((conf[list(g)] == conf[g[0]]).all()) and len({got.get(r) for r in g}) == 1 and got.get(g[0]) == int(x["perm"][p][g[0]])
        if case.zero_row is not None:  # sim = 0 along the row and the column
            assert float(x["im"][p][case.zero_row].abs().max()) == 0 and float(x["pt"][p][case.zero_col].abs().max()) == 0
            assert case.zero_row not in ties
        if case.anti is not None:  # the anti-aligned entry: cosine -1 up to the 1e-6 of the normalisation
            a, b = x["im"][p][case.anti[0]].double(), x["pt"][p][case.anti[1]].double()
            assert abs(float(a @ b / (a.norm() * b.norm())) * (1.0 if case.scale > 0 else -1.0) + 1.0) < 1e-6
        planted = sum(got.get(i) == int(j) for i, j in enumerate(x["perm"][p]))
        print(f"{case.name} pair {p}: {len(ii)} matches ({planted} of {len(x['perm'][p])} planted), {len(ties)} tie rows, {x['reseeded'][p]} rows perturbed, "
              f"mconf {float(mconf.min()) if len(mconf) else 0:.3g} .. {float(mconf.max()) if len(mconf) else 0:.3g}")
    if case.group == "compact":
        want = {"compact-1153-all": 1153, "compact-1153-none": 0, "compact-1153-second-sweep": 1153 - 1024}[case.name]
        assert len(ref[0][1]) == want and (want == 0 or int(ref[0][1].min()) == case.M - want)


@pytest.mark.parametrize("name", ["thr-between-mutual", "thr-between-rowmax"])
def test_threshold_lies_between_two_oracle_confidences(name):
    case = fu.CASE[name]
    x = fu.inputs_of(case)
    thr = x["thr"]
    all_of = fu.oracle(x["im"][0], x["pt"][0], case.scale, None, None, case.mutual, 0.0)[3]
    kept = fu.oracle_of(case)[0][3]
    above, below = all_of[all_of > thr], all_of[all_of <= thr]
    print(f"{name}: thr {thr:.6g} keeps {len(kept)} of {len(all_of)}; nearest above {float(above.min()):.6g}, below {float(below.max()):.6g}")
    assert len(kept) == len(above) >= case.thr[1] and len(below) > 0
    assert float(above.min()) - thr >= fu.MARGIN * float(above.min()) and thr - float(below.max()) >= fu.MARGIN * float(below.max())


def test_scale_limit_is_the_entry_points():
    smax, over = fu.max_scale()
    f = lambda s: float(fu.np.float32(fu.np.float32(s) * fu.LOG2E_F32))
    assert f(smax) <= 60.0 < f(over) and 41.58 < smax < over < 41.59 and fu.np.float32(smax) == smax
    assert {c.scale for c in fu.CASES if c.group == "scale"} == {-10.0, smax, -smax}


def test_argument_validation_without_gpu(built_lib):
    """Null pointers and non-positive sizes -> NM_ERR_ARG; a feature width outside {64, 128, 256, 512}, |scale| log2 e above 60 (NaN included)
    or more than 65535 pairs -> NM_ERR_UNSUPPORTED; one byte less than nm_match_fused_workspace_bytes -> NM_ERR_WORKSPACE.  All returned before
    anything is enqueued (the pointers below are never dereferenced)."""
    from nerfmatch_amd import _lib
    h = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_char * 64)()
    q = C.cast(buf, C.c_void_p)
    smax, over = fu.max_scale()

    def call(im=q, pt=q, P=2, M=300, N=200, c=64, scale=10.0, oi=q, oj=q, oc=q, cnt=q, ws=q, ws_bytes=1 << 30):
        return h.nm_dual_softmax_match_fused(im, pt, P, M, N, c, scale, null, null, 0.0, 1, oi, oj, oc, cnt, ws, ws_bytes, null)

    need = h.nm_match_fused_workspace_bytes(2, 300, 200, 64)
    assert 0 < need < 1 << 22 and h.nm_match_fused_workspace_bytes(0, 300, 200, 64) == 0 and h.nm_match_fused_workspace_bytes(2, 300, -1, 64) == 0
    assert need % 256 == 0 and h.nm_match_fused_workspace_bytes(4, 300, 200, 64) > need
    A, U, W = fu.NM_ERR_ARG, fu.NM_ERR_UNSUPPORTED, fu.NM_ERR_WORKSPACE
    assert call(im=null) == A and call(pt=null) == A and call(oi=null) == A and call(oj=null) == A and call(oc=null) == A and call(cnt=null) == A
    assert call(ws=null) == A and call(P=0) == A and call(M=0) == A and call(N=-3) == A
    assert call(c=96) == U and call(c=32) == U and call(c=1024) == U and call(P=65536) == U
    assert call(scale=over) == U and call(scale=-over) == U and call(scale=50.0) == U and call(scale=float("nan")) == U and call(scale=float("inf")) == U
    assert call(ws_bytes=need - 1) == W and call(scale=smax, ws_bytes=need - 1) == W and call(scale=-smax, ws_bytes=0) == W  # (the limit itself passes the scale check)
    assert _lib.NM_ERR_UNSUPPORTED == U and (fu.NM_OK, A, W) == (0, 1, 4)
