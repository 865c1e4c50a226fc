"""CPU: the multi-iteration localisation loop (NeRFMatchEvaluator._localize_finish) against the reference's loop restated in
oracle/localize_oracle.py.  A duck-typed renderer whose points are a function of the pose, the ground-truth matches of
`match_oracle=True`, a scripted solver and a scripted iNeRF stand-in drive the loop through every start mode, solver outcome and
batch size; each query must get the oracle's trace -- the poses rendered from, the solver calls, the cache_iters traces and the
final pose, errors and match count -- whether it runs alone or in a batch."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from nerfmatch_amd import synth
from nerfmatch_amd.nerfmatch_evaluator import NeRFMatchEvaluator
from nerfmatch_amd.utils.metrics import pose_err
from oracle import localize_oracle as lo

H, W, N, C = 16, 24, 15, 8
M = (H // 8) * (W // 8)
INF = float("inf")


def _rot(axis, deg):
    a = torch.as_tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    th = torch.tensor(math.radians(deg), dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + torch.sin(th) * Kx + (1 - torch.cos(th)) * Kx @ Kx


def _gt(q):
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, :3] = _rot([1.0, 2.0, 0.5 + q], 10.0 + 7 * q)
    c2w[:3, 3] = torch.tensor([0.3 * q, -0.2, 1.0 + 0.1 * q])
    return c2w.float()


def _perturb(c2w, q, k, scale=1.0):
    """The ground truth moved by a seeded rotation of 2 deg / (k + 1) and 5 cm / (k + 1) (times `scale`)."""
    g = torch.Generator().manual_seed(1000 * q + k)
    P = c2w.double().clone()
    P[:3, :3] = _rot(torch.randn(3, generator=g, dtype=torch.float64), scale * 2.0 / (k + 1)) @ P[:3, :3]
    P[:3, 3] += torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0) * scale * 0.05 / (k + 1)
    return P.float()


def _as_solver_result(c2w):
    w2c = torch.linalg.inv(c2w.double())
    return w2c[:3, :3].numpy(), w2c[:3, 3].numpy(), np.ones(4, dtype=bool)


def _c2w_from_result(res):
    """The evaluator's conversion of a solver's (R, t) (nerfmatch_evaluator.py, _poses_from_matches): fp32 w2c, then its inverse."""
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.as_tensor(res[0], dtype=torch.float32)
    w2c[:3, 3] = torch.as_tensor(res[1], dtype=torch.float32).reshape(-1)
    return torch.linalg.inv(w2c)


_BASE = torch.randn(N, 3, generator=torch.Generator().manual_seed(5))
_FBASE = torch.randn(N, C, generator=torch.Generator().manual_seed(6))


def _points_of(pose):
    """What the fake renderer returns for one pose: points and features that depend on every entry of the pose."""
    pose = torch.as_tensor(pose).float()
    pt3d = _BASE @ pose[:3, :3].T + pose[:3, 3]
    pt_feat = torch.sin(_FBASE * (1.0 + pose.reshape(-1).sum()))
    return pt3d, pt_feat


class FakeRenderer:
    def __init__(self):
        self.calls = []

    def render_novel_views(self, img_hw, K, c2ws, unnorm, device, downsample=8, want_im_pred=False):
        c2ws = torch.as_tensor(c2ws).reshape(-1, 4, 4)
        self.calls.append(c2ws.clone())
        outs = [_points_of(p) for p in c2ws]
        return dict(pt3d=torch.stack([o[0] for o in outs]), pt_feat=torch.stack([o[1] for o in outs]))

    def render_novel_view(self, img_hw, K, c2w, unnorm, device, downsample=8, want_im_pred=False):
        out = self.render_novel_views(img_hw, K, torch.as_tensor(c2w)[None], unnorm, device)
        return dict(pt3d=out["pt3d"][0], pt_feat=out["pt_feat"][0])


def _query(q):
    """One query in the reference's batch schema (batch of one); `conf_gt` for match_oracle, cached points of the render shape."""
    g = torch.Generator().manual_seed(100 + q)
    conf_gt = torch.zeros(1, M, N, dtype=torch.bool)
    rows, cols = torch.randperm(M, generator=g)[:5], torch.randperm(N, generator=g)[:5 + q % 3]
    conf_gt[0, rows.repeat(3)[:len(cols)], cols] = True
    pt3d, pt_feat = _points_of(_perturb(_gt(q), q, 7, scale=3.0))
    return dict(image=torch.zeros(1, 3, H, W), K=synth.intrinsics(H, W, 20.0)[None], c2w=_gt(q)[None],
                rc2w=_perturb(_gt(q), q, 50, scale=4.0)[None], unnorm_scene=torch.eye(4)[None], pt2d=torch.rand(1, M, 2, generator=g) * 20,
                pt2d_proj=torch.rand(1, N, 2, generator=g) * 20 + q * 100, pt3d=pt3d[None], pt_feat=pt_feat[None], conf_gt=conf_gt,
                idx=torch.tensor([q]))


def _stack(qs):
    singles = [_query(q) for q in qs]
    return {k: torch.cat([b[k] for b in singles]) for k in singles[0]}


SCRIPTS = {  # solver outcome of (query, iteration): True = a pose, False = a failure
    "always": lambda q, k: True,
    "fail_it0": lambda q, k: k != 0,
    "fail_it1": lambda q, k: k != 1,
    "never": lambda q, k: False,
}


def _solution(q, k):
    return _perturb(_gt(q), q, k)


class Scripted:
    """Solver: which query a call is for follows from its pixels (the query's own `pt2d_proj`), the iteration from that query's
    call count.  Records every call's matches."""

    def __init__(self, script, qs, never=()):
        self.script, self.never = script, set(never)
        self.qbatches = {q: _query(q) for q in qs}
        self.calls = []
        self.count = {}

    def __call__(self, pt2d, pt3d, K, rthres):
        q = self._query_of(pt2d)
        k = self.count.get(q, 0)
        self.count[q] = k + 1
        self.calls.append((q, k, pt3d.clone()))
        if q in self.never or not self.script(q, k):
            return None
        return _as_solver_result(_solution(q, k))

    def _query_of(self, pt2d):
        for q, b in self.qbatches.items():
            i3d = torch.where(b["conf_gt"][0])[1]
            if torch.equal(pt2d, b["pt2d_proj"][0][i3d]):
                return q
        raise AssertionError("a solver call with pixels of no query")


def _make_solver(script, qs, never=()):
    return Scripted(script, qs, never)


class InerfStub:
    """Stands in for ev.inerf_refinement: records the pose it starts from, appends two inner entries to the traces when asked to
    (a refinement of num_optim = 4 steps, reference :491-493) and returns a scripted pose -- or inf errors (refinement failed)."""

    def __init__(self, fails=lambda q, k: False):
        self.fails, self.calls, self.count = fails, [], {}

    def result(self, q, k):
        pose = _perturb(_gt(q), q, 20 + k, scale=0.5)
        inner = [(0.1 * q + k + 0.5, 0.01 * (k + 1)), (0.1 * q + k + 0.25, 0.02 * (k + 1))]
        if self.fails(q, k):
            return pose, INF, INF, inner
        R, t = pose_err(_gt(q), pose)
        return pose, R, t, inner

    def __call__(self, batch, renderer, unnorm_scene, c2w_est, inerf_conf, cache_iters=False, iter_t_errs=None, iter_R_errs=None, **kw):
        q = int(batch["idx"][0])
        k = self.count.get(q, 0)
        self.count[q] = k + 1
        self.calls.append((q, torch.as_tensor(c2w_est).clone()))
        pose, R, t, inner = self.result(q, k)
        if cache_iters:
            for r, tt in inner:
                iter_t_errs.append(tt)
                iter_R_errs.append(r)
        return pose, torch.tensor(R) if R == INF else R, torch.tensor(t) if t == INF else t


@pytest.fixture(scope="module")
def ev():
    e = NeRFMatchEvaluator(Namespace(model=synth.matcher_config("c2f"), exp=Namespace(seed=0), data=Namespace()))
    e.model.forward = e.model.forward_begin = None  # match_oracle: the matcher must not be called at all
    return e


START = {"query2query": dict(query2query=True), "cached": dict(cached_pt=True), "rc2w": dict(cached_pt=False),
         "retrieval_only": dict(retrieval_only=True)}


def _oracle(q, iters, start, solver, cache_iters, inerf, never=False):
    """The loop oracle's trace of query q run on its own."""
    b = _query(q)
    i3d = torch.where(b["conf_gt"][0])[1]
    pose0 = lo.start_pose(b["c2w"][0], b["rc2w"][0], **START[start])
    cnt = {"s": 0, "r": 0}

    def solve(matches):
        k = cnt["s"]
        cnt["s"] += 1
        return None if never or not SCRIPTS[solver](q, k) else _c2w_from_result(_as_solver_result(_solution(q, k)))

    def refine(pose):
        k = cnt["r"]
        cnt["r"] += 1
        return inerf.result(q, k)

    return lo.localize(b["c2w"][0], pose0, b["pt3d"][0], iters, render=lambda p: _points_of(p)[0], match=lambda pts: pts[i3d],
                       solve=solve, refine=refine if inerf is not None else None, solver_none=solver == "none",
                       retrieval_only=start == "retrieval_only", cache_iters=cache_iters)


def _run(ev, qs, iters, start, solver, cache_iters, inerf, never=()):
    ren = FakeRenderer()
    sol = "none" if solver == "none" else _make_solver(SCRIPTS[solver], qs, never)
    stub = None
    if inerf is not None:
        stub = ev.inerf_refinement = inerf
    try:
        out = ev.eval_batch(_stack(qs), renderer=ren, inerf_conf=Namespace(num_optim=4) if inerf is not None else None, iters=iters,
                            solver=sol, match_oracle=True, cache_iters=cache_iters, **START[start])
    finally:
        ev.__dict__.pop("inerf_refinement", None)
    return out, ren, sol, stub


def _check_against_oracle(out, ren, sol, stub, qs, iters, start, solver, cache_iters, make_inerf, never=()):
    Q = len(qs)
    traces = {q: _oracle(q, iters, start, solver, cache_iters, make_inerf() if make_inerf else None, never=q in never) for q in qs}
    # renders: per iteration, the queries that have a pose, in query order, as ONE call each (no render for the others)
    want_calls = []
    for k in range(iters):
        poses = [p for q in qs for (kk, p) in traces[q]["renders"] if kk == k]
        if poses:
            want_calls.append(torch.stack([torch.as_tensor(p).float() for p in poses]))
    assert len(ren.calls) == len(want_calls), (len(ren.calls), len(want_calls))
    for got, want in zip(ren.calls, want_calls):
        assert torch.equal(got, want)
    for i, q in enumerate(qs):
        tr = traces[q]
        if solver != "none":
            mine = [(k, pt3d) for (qq, k, pt3d) in sol.calls if qq == q]
            assert len(mine) == len(tr["solves"]) == (0 if start == "retrieval_only" else iters)
            for (k, pt3d), (kk, matches, _) in zip(mine, tr["solves"]):
                assert k == kk and torch.equal(pt3d, matches), (q, k)
        if stub is not None:
            mine = [p for (qq, p) in stub.calls if qq == q]
            assert len(mine) == len(tr["refines"]) and all(torch.equal(a, torch.as_tensor(b)) for a, (_, b) in zip(mine, tr["refines"]))
        it_t = out["iter_t_errs"] if Q == 1 else out["iter_t_errs"][i]
        it_R = out["iter_R_errs"] if Q == 1 else out["iter_R_errs"][i]
        assert [float(v) for v in it_t] == pytest.approx(tr["iter_t_errs"], rel=1e-12, abs=1e-9)
        assert [float(v) for v in it_R] == pytest.approx(tr["iter_R_errs"], rel=1e-12, abs=1e-6)
        if not cache_iters:
            assert len(it_t) == len(it_R) == 0
        est = out["c2w_ests"][i]
        assert (est is None) == (tr["c2w_est"] is None)
        if est is not None:
            assert torch.equal(torch.as_tensor(est).float(), torch.as_tensor(tr["c2w_est"]).float())
        assert float(out["R_err"][i]) == pytest.approx(tr["R_err"], rel=1e-12, abs=1e-6)
        assert float(out["t_err"][i]) == pytest.approx(tr["t_err"], rel=1e-12, abs=1e-9)
        assert out["num_matches"][i] == tr["num_matches"]


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("start", list(START))
@pytest.mark.parametrize("solver", list(SCRIPTS) + ["none"])
@pytest.mark.parametrize("cache_iters", [False, True])
@pytest.mark.parametrize("inerf", ["off", "on", "failing"])
def test_loop_equals_the_oracle(ev, iters, start, solver, cache_iters, inerf):
    """Q = 1 per query, and a batch of three in which query 2 never gets a pose from the solver: every query's trace is the
    oracle's, and a query's results in the batch equal its results alone."""
    make = None if inerf == "off" else (lambda: InerfStub()) if inerf == "on" else (lambda: InerfStub(fails=lambda q, k: k % 2 == 0))
    singles = {}
    for q in range(3):
        never = (2,) if q == 2 else ()
        out, ren, sol, stub = _run(ev, [q], iters, start, solver, cache_iters, make() if make else None, never=never)
        _check_against_oracle(out, ren, sol, stub, [q], iters, start, solver, cache_iters, make, never=never)
        singles[q] = out
    out, ren, sol, stub = _run(ev, [0, 1, 2], iters, start, solver, cache_iters, make() if make else None, never=(2,))
    _check_against_oracle(out, ren, sol, stub, [0, 1, 2], iters, start, solver, cache_iters, make, never=(2,))
    for q in range(3):  # the batch rule, directly
        one = singles[q]
        assert out["num_matches"][q] == one["num_matches"][0]
        assert float(out["t_err"][q]) == float(one["t_err"][0]) and float(out["R_err"][q]) == float(one["R_err"][0])
        assert [float(v) for v in out["iter_t_errs"][q]] == [float(v) for v in one["iter_t_errs"]]
        a, b = out["c2w_ests"][q], one["c2w_est"]
        assert (a is None and b is None) or torch.equal(a, b)


def test_a_query_without_a_pose_does_not_stop_the_others_re_render(ev):
    """Cached points, Q = 2: query 0 is solved every iteration, query 1 never.  Query 0 is re-rendered from its solved pose in
    iterations 1 and 2 (alone in the render call); query 1 keeps its cached points, and its solver still runs every iteration."""
    out, ren, sol, _ = _run(ev, [0, 1], 3, "cached", "always", True, None, never=(1,))
    assert len(ren.calls) == 2 and all(c.shape == (1, 4, 4) for c in ren.calls)
    assert torch.equal(ren.calls[0][0], _c2w_from_result(_as_solver_result(_solution(0, 0))))
    assert torch.equal(ren.calls[1][0], _c2w_from_result(_as_solver_result(_solution(0, 1))))
    cached1 = _query(1)
    i3d = torch.where(cached1["conf_gt"][0])[1]
    assert [k for (q, k, _) in sol.calls if q == 1] == [0, 1, 2]
    assert all(torch.equal(p, cached1["pt3d"][0][i3d]) for (q, _, p) in sol.calls if q == 1)
    assert out["c2w_ests"][1] is None and len(out["iter_t_errs"]) == 2 and len(out["iter_t_errs"][1]) == 3


def test_a_failing_solver_is_called_every_iteration(ev):
    """reference :548-614: a failed solve does not end the loop; the same points are matched and solved again, and the trace has one
    entry per iteration."""
    out, ren, sol, _ = _run(ev, [0], 3, "cached", "never", True, None)
    assert len(sol.calls) == 3 and len(ren.calls) == 0
    assert len(out["iter_t_errs"]) == len(out["iter_R_errs"]) == 3 and all(float(v) == INF for v in out["iter_t_errs"])
    # a RANSAC-like solver that succeeds late: its pose is the result
    late = _make_solver(lambda q, k: k == 2, [0])
    o3 = ev.eval_batch(_stack([0]), renderer=FakeRenderer(), iters=3, solver=late, match_oracle=True, cache_iters=True)
    assert len(late.calls) == 3 and torch.equal(o3["c2w_est"], _c2w_from_result(_as_solver_result(_solution(0, 2))))
    assert float(o3["iter_t_errs"][-1]) < 0.1 and float(o3["iter_t_errs"][0]) == INF


def test_rows_of_another_shape_are_refused(ev):
    """A batch whose cached points have another shape than a render cannot be re-rendered query by query: refused, not mixed."""
    b = _stack([0, 1])
    b["pt3d"], b["pt_feat"] = b["pt3d"][:, :-1], b["pt_feat"][:, :-1]
    b["conf_gt"] = b["conf_gt"][:, :, :-1]
    sol = _make_solver(SCRIPTS["always"], [0, 1], never=(1,))
    with pytest.raises(ValueError, match="batches of one query"):
        ev.eval_batch(b, renderer=FakeRenderer(), iters=2, solver=sol, match_oracle=True)


def test_eval_data_loader_traces_are_one_row_per_query(ev):
    """eval_data_loader with iters = 2 and cache_iters over ragged batches (2, 2, 1): its records equal per-query eval_batch runs
    and its traces stack to (n_queries, L) in query order (reference :716-721)."""
    qs = list(range(5))
    kw = dict(iters=2, match_oracle=True, cached_pt=False, cache_iters=True)
    loader = [_stack([0, 1]), _stack([2, 3]), _stack([4])]
    sol = _make_solver(SCRIPTS["fail_it0"], qs, never=(3,))
    out = ev.eval_data_loader(renderer=FakeRenderer(), data_loader=loader, solver=sol, **kw)
    assert out["query_idx"].tolist() == qs
    t, R = np.stack(out["iter_t_errs"]), np.stack(out["iter_R_errs"])
    assert t.shape == R.shape == (5, 2)
    for q in qs:
        one = ev.eval_batch(_stack([q]), renderer=FakeRenderer(), solver=_make_solver(SCRIPTS["fail_it0"], [q], never=(3,) if q == 3 else ()), **kw)
        assert out["num_matches"][q] == one["num_matches"][0]
        assert out["R_err"][q] == np.float32(float(one["R_err"][0])) and out["t_err"][q] == np.float32(float(one["t_err"][0]))
        if one["c2w_est"] is not None:
            assert np.array_equal(out["c2w_est"][q], one["c2w_est"].numpy())
        assert t[q].tolist() == [float(v) for v in one["iter_t_errs"]] and R[q].tolist() == [float(v) for v in one["iter_R_errs"]]
    assert np.isinf(t[3]).all() and np.isfinite(t[0, 1])
