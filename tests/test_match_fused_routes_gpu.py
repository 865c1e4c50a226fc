"""csrc/match_fused.hip at its tile, tie, mask, batch, threshold and scale edges: nm_dual_softmax_match_fused driven directly on buffers the
test fills (match_fused_util.run), against the float64 oracle of match_fused_util.py.  The case table, the edges it claims and the conditions
on its inputs (every decision of the oracle is 50 * TIE_REL from flipping, exact designed ties aside) are checked without a GPU in
test_match_fused_util_cpu.py; with them the index lists must be IDENTICAL to the oracle's, no row excused."""
import pytest
import torch

import match_fused_util as fu
from conftest import TIE_REL, compare_matches

pytestmark = pytest.mark.gpu

_WORST = {}  # group -> (largest |returned confidence - oracle|, case)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    """Two runs returned the same bytes: return code, indices, confidence bits, counts."""
    return a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(_bits(a[3]), _bits(b[3])) and torch.equal(a[4], b[4])


def _check_against_oracle(case, run, ref, what):
    """Index lists identical to the oracle's (zero rows excused), strictly increasing; confidence within TOL; index 0 / confidence 0 behind the
    count and no sentinel in front of it.  Returns the largest confidence error."""
    rc, oi, oj, oc, cnt = run
    assert rc == fu.NM_OK, (what, rc)
    worst = 0.0
    for p, (conf, ii, jj, mconf) in enumerate(ref):
        n = int(cnt[p])
        assert 0 <= n <= case.M, (what, p, n)
        gi, gj, gc = oi[p, :n], oj[p, :n], oc[p, :n]
        assert not (gi == fu.SENTINEL_ID).any() and not (gj == fu.SENTINEL_ID).any() and not (gc == fu.SENTINEL_CONF).any(), (what, p)
        assert bool((oi[p, n:] == 0).all()) and bool((oj[p, n:] == 0).all()) and bool((_bits(oc[p, n:]) == 0).all()), (what, p, "slots behind the count")
        assert bool((gi >= 0).all()) and bool((gi < case.M).all()) and bool((gj >= 0).all()) and bool((gj < case.N).all())
        assert torch.all(gi[1:] > gi[:-1]), (what, p)
        differing = compare_matches((ii, jj), (gi, gj), conf, case.mutual, f"{what} pair {p}", tol=TIE_REL, expect_zero=True)
        assert differing == 0 and n == len(ii)
        if n:
            worst = max(worst, (gc.double() - mconf).abs().max().item())
    assert worst < fu.TOL, (what, worst)
    return worst


@pytest.mark.parametrize("case", fu.CASES, ids=lambda c: c.name)
def test_case(gpu, built_lib, case):
    """Every case of match_fused_util.CASES: from a zero-filled workspace, from one filled with 0xFF bytes, and a third time; each run against
    the oracle, the three runs against each other bit for bit, and one byte of workspace less refused.
    Measured on the MI355X, largest |returned confidence - float64 oracle| per group (bar 1e-4): see test_worst_confidence_error_per_group."""
    x, ref = fu.inputs_of(case), fu.oracle_of(case)
    for p, r in enumerate(ref):
        assert fu.undecided_rows(r[0], case.mutual, x["thr"]) == []
    runs = [fu.run_fresh(x, case.scale, x["thr"], case.mutual, fill) for fill in (0, 0xFF, 0)]
    worst = max(_check_against_oracle(case, run, ref, f"{case.name} run {k}") for k, run in enumerate(runs))
    assert _same(runs[0], runs[1]), "a workspace of 0xFF bytes changes the result"
    assert _same(runs[0], runs[2]), "a third run differs"
    if worst >= _WORST.get(case.group, (-1.0, ""))[0]:
        _WORST[case.group] = (worst, case.name)
    print(f"{case.name}: counts {runs[0][4].tolist()[:4]}, confidence error {worst:.2e} ({fu.TOL:.0e})")
    # the workspace size the library reports is the size it needs: one byte less is refused and nothing is written
    dev = gpu
    need = fu.workspace_bytes(case.P, case.M, case.N, case.C)
    g = lambda t: None if t is None else t.to(dev)
    oi, oj = (torch.full((case.P, case.M), fu.SENTINEL_ID, device=dev, dtype=torch.int64) for _ in range(2))
    oc = torch.full((case.P, case.M), fu.SENTINEL_CONF, device=dev, dtype=torch.float32)
    cnt = torch.full((case.P,), fu.SENTINEL_ID, device=dev, dtype=torch.int32)
    ws = torch.zeros(need, device=dev, dtype=torch.uint8)
    rc, ri, rj, rcf, rn = fu.run(g(x["im"]), g(x["pt"]), case.scale, g(x["im_mask"]), g(x["pt_mask"]), x["thr"], case.mutual, ws, oi, oj, oc, cnt, ws_bytes=need - 1)
    assert rc == fu.NM_ERR_WORKSPACE
    assert bool((ri == fu.SENTINEL_ID).all()) and bool((rj == fu.SENTINEL_ID).all()) and bool((rcf == fu.SENTINEL_CONF).all()) and bool((rn == fu.SENTINEL_ID).all())


@pytest.mark.parametrize("name", [c.name for c in fu.CASES if c.P > 1])
def test_pair_of_a_batch_equals_the_pair_alone(gpu, built_lib, name):
    """Pair p of a batch (its own features and masks among P different ones) gives the bits of the same pair run as P = 1."""
    case = fu.CASE[name]
    x = fu.inputs_of(case)
    rc, oi, oj, oc, cnt = fu.run_fresh(x, case.scale, x["thr"], case.mutual)
    assert rc == fu.NM_OK
    for p in range(case.P):
        one = fu.run_fresh(x, case.scale, x["thr"], case.mutual, pairs=slice(p, p + 1))
        assert one[0] == fu.NM_OK and int(one[4][0]) == int(cnt[p]), (p, one[4].tolist(), cnt.tolist())
        assert torch.equal(one[1][0], oi[p]) and torch.equal(one[2][0], oj[p]) and torch.equal(_bits(one[3][0]), _bits(oc[p])), p


@pytest.mark.parametrize("name", ["thr-between-mutual", "thr-between-rowmax", "tile-130x641-rowmax"])
def test_threshold_on_the_bits_of_a_returned_confidence(gpu, built_lib, name):
    """`conf > threshold` is strict: with the bits of the k-th returned confidence as the threshold, exactly the rows whose confidence is
    strictly larger remain, with the columns and confidence bits they had."""
    case = fu.CASE[name]
    x = fu.inputs_of(case)
    rc, oi, oj, oc, cnt = fu.run_fresh(x, case.scale, 0.0, case.mutual)
    n = int(cnt[0])
    assert rc == fu.NM_OK and n > 20
    for k in (0, n // 2, int(oc[0, :n].argmax()), int(oc[0, :n].argmin())):
        thr = float(oc[0, k])
        keep = oc[0, :n] > thr
        assert not keep[k] and (k != int(oc[0, :n].argmax()) or not keep.any())
        rc2, pi, pj, pc, pn = fu.run_fresh(x, case.scale, thr, case.mutual)
        m = int(pn[0])
        print(f"{name}: threshold {thr:.9g} (slot {k}) keeps {m} of {n}")
        assert rc2 == fu.NM_OK and m == int(keep.sum())
        assert torch.equal(pi[0, :m], oi[0, :n][keep]) and torch.equal(pj[0, :m], oj[0, :n][keep]) and torch.equal(_bits(pc[0, :m]), _bits(oc[0, :n][keep]))
        assert bool((pi[0, m:] == 0).all()) and bool((pj[0, m:] == 0).all()) and bool((_bits(pc[0, m:]) == 0).all())


def test_scale_above_the_limit_is_refused_and_writes_nothing(gpu, built_lib):
    """The next float above the largest |scale| with |scale| log2 e <= 60, either sign: NM_ERR_UNSUPPORTED, outputs and counts untouched."""
    case = fu.CASE["scale-max-mutual"]
    x = fu.inputs_of(case)
    smax, over = fu.max_scale()
    assert case.scale == smax
    for s in (over, -over):
        rc, oi, oj, oc, cnt = fu.run_fresh(x, s, 0.0, True)
        assert rc == fu.NM_ERR_UNSUPPORTED
        assert bool((oi == fu.SENTINEL_ID).all()) and bool((oj == fu.SENTINEL_ID).all()) and bool((oc == fu.SENTINEL_CONF).all()) and bool((cnt == fu.SENTINEL_ID).all())


def test_worst_confidence_error_per_group(gpu, built_lib):
    """The figures test_case collected (run after it).  Measured on the MI355X against the float64 oracle, bar 1e-4 absolute:
      tile 1.24e-05, compact 1.25e-05, batch 1.20e-05, tie 1.29e-05, thr 1.02e-05, scale 2.60e-05 (scale-max-rowmax), C 5.01e-06."""
    for group in fu.GROUPS:
        if group in _WORST:
            print(f"{group}: {_WORST[group][0]:.2e} ({_WORST[group][1]})")
            assert _WORST[group][0] < fu.TOL
