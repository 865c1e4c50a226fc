"""GPU: the multi-iteration localisation loop on the real renderer and matcher (small shapes).  A scripted solver hands back each
query's ground-truth pose moved by a seeded rotation / translation that shrink with the iteration (or fails where the script says
so); the renders, the matches the solver sees, the poses and the errors are pinned against direct kernel calls, the fp64 NeRF oracle,
fp64 pose errors, the loop oracle (oracle/localize_oracle.py) and -- for a batch -- each query's own batch-of-one run."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from nerfmatch_amd import synth
from oracle import localize_oracle as lo
from oracle import nerf_oracle as no
from test_evaluator_gpu import _c2f_evaluator, _renderer, _stack, make_batch

pytestmark = pytest.mark.gpu

H, W, S = 64, 96, 32
R = (H // 8) * (W // 8)
TOL = 1e-4  # the bars of tests/test_fullsize_gpu.py::test_render_novel_view_full_size_vs_oracle
MATCH_KEYS = ("mpt3d", "mconf", "mpt2d_f")


def _rot(axis, deg):
    a = torch.nn.functional.normalize(torch.as_tensor(axis, dtype=torch.float64), dim=0)
    Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    th = torch.tensor(np.radians(deg), dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + torch.sin(th) * Kx + (1 - torch.cos(th)) * Kx @ Kx


def _solution(c2w, q, k):
    """Query q's ground truth moved by 2 deg / (k + 1) and 5 cm / (k + 1) in seeded directions."""
    g = torch.Generator().manual_seed(1000 * q + k)
    P = torch.as_tensor(c2w).double().clone()
    P[:3, :3] = _rot(torch.randn(3, generator=g, dtype=torch.float64), 2.0 / (k + 1)) @ P[:3, :3]
    P[:3, 3] += torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0) * 0.05 / (k + 1)
    return P


def _c2w_of(res):
    """A solver result as the evaluator turns it into a pose (fp32 w2c, then its inverse)."""
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.as_tensor(res[0], dtype=torch.float32)
    w2c[:3, 3] = torch.as_tensor(res[1], dtype=torch.float32).reshape(-1)
    return torch.linalg.inv(w2c)


class Solver:
    """Call c of a batch of queries `qs` is query qs[c % Q] in iteration c // Q (the evaluator calls the solver once per query and
    iteration, in query order).  `fails(q, k)`: no pose."""

    def __init__(self, qs, fails=lambda q, k: False):
        self.qs, self.fails, self.calls = list(qs), fails, []

    def result(self, q, k):
        if self.fails(q, k):
            return None
        w2c = torch.linalg.inv(_solution(make_batch(H, W, q)["c2w"][0], q, k))
        return w2c[:3, :3].numpy(), w2c[:3, 3].numpy(), np.ones(4, dtype=bool)

    def __call__(self, pt2d, pt3d, K, rthres):
        c = len(self.calls)
        q, k = self.qs[c % len(self.qs)], c // len(self.qs)
        self.calls.append((q, k, pt2d.clone(), pt3d.clone()))
        return self.result(q, k)


def _setup(gpu):
    """Evaluator + renderer whose render_novel_views draws per-pose seeded random tensors and records every call (poses, random
    tensors, outputs); `matches` gets what the matcher left in the batch each time the solver is about to be called."""
    ev, ren = _c2f_evaluator(gpu, H, W), _renderer(gpu, H, W, S=S)
    raw, calls = ren.render_novel_views, []

    def rand_of(c2w):  # the samplers' random tensors belong to the pose rendered from, not to the call order
        s = int(round(float(torch.as_tensor(c2w)[0, 3]) * 1e6)) % (2**31 - 1)
        return torch.rand(R, S + 1, generator=torch.Generator().manual_seed(s)), synth.resample_jitter((R, S + 1), s + 1)

    def seeded(img_hw, K, c2ws, unnorm, device, **kw):
        c2ws = torch.as_tensor(c2ws).reshape(-1, 4, 4)
        rs = [rand_of(c) for c in c2ws]
        tr, jt = torch.cat([r[0] for r in rs]), torch.cat([r[1] for r in rs])
        out = raw(img_hw, K, c2ws, unnorm, device, t_rand=tr.to(gpu), jitter=jt.to(gpu), **kw)
        calls.append(dict(poses=c2ws.clone(), rand=rs, pt3d=out["pt3d"].clone(), pt_feat=out["pt_feat"].clone()))
        return out

    ren.render_novel_views = seeded
    matches = []
    pfm = ev._poses_from_matches

    def snap(batch, *a, **kw):  # what the matcher left in the batch, per iteration
        matches.append({**{k: batch[k].clone() for k in MATCH_KEYS}, "ids": torch.stack([t.clone() for t in batch["match_ids"]]),
                        "bids": batch["m_bids"].clone() if "m_bids" in batch else None})
        return pfm(batch, *a, **kw)

    ev._poses_from_matches = snap
    return ev, ren, calls, matches, rand_of


def test_three_iterations_from_the_retrieved_pose(gpu, built_lib):
    """Q = 1, iters = 3, start from rc2w: the poses rendered from are the ones the solver returned, each render is the kernel's render at
    that pose (bit for bit) and the fp64 oracle's (to the full-size bars), the solver sees the current iteration's matches, and the
    errors and traces are the fp64 / loop oracle's."""
    ev, ren, calls, matches, rand_of = _setup(gpu)
    b = make_batch(H, W, 0)
    c2w_gt, rc2w, K, unnorm = b["c2w"][0], b["rc2w"][0], b["K"][0], b["unnorm_scene"][0]
    sol = Solver([0])
    out = ev.eval_batch(b, renderer=ren, iters=3, solver=sol, cached_pt=False, cache_iters=True, mutual=True)
    assert len(calls) == 3 and len(sol.calls) == 3 and len(matches) == 3
    want = [rc2w.float()] + [_c2w_of(sol.result(0, k)) for k in range(2)]
    sd = synth.nerf_state_dict(seed=0, density_bias=3.0)
    for k, (c, pose) in enumerate(zip(calls, want)):
        assert torch.equal(c["poses"][0], pose), k
        tr, jt = c["rand"][0]
        direct = ren.render_novel_view((H, W), K, pose, unnorm, gpu, t_rand=tr.to(gpu), jitter=jt.to(gpu), want_im_pred=False)
        assert torch.equal(c["pt3d"][0], direct["pt3d"]) and torch.equal(c["pt_feat"][0], direct["pt_feat"]), k
        ref = no.render_novel_view(sd, (H, W), K, pose, unnorm, tr, jt, S, S, stop_layer=3)
        ef = (c["pt_feat"][0].cpu() - ref["pt_feat"].float()).abs().max().item()
        ep = (c["pt3d"][0].cpu() - ref["pt3d"].float()).abs().max().item()
        assert ef < TOL and ep < 3 * TOL, (k, ef, ep)
        # the solver got THIS iteration's matches: the matcher's on this iteration's rendered points
        d = dict(image=b["image"].to(gpu), im_mask=b["im_mask"].to(gpu), pt2d=b["pt2d"].to(gpu), pt3d=c["pt3d"], pt_feat=c["pt_feat"],
                 pt_mask=torch.ones_like(c["pt3d"][..., 0], dtype=torch.bool))
        ev.model.forward(d, mutual=True)
        assert torch.equal(torch.stack([t for t in d["match_ids"]]).cpu(), matches[k]["ids"].cpu()), k
        for key in MATCH_KEYS:
            assert torch.equal(d[key].cpu(), matches[k][key].cpu()), (k, key)
        assert torch.equal(sol.calls[k][3], d["mpt3d"].cpu()) and torch.equal(sol.calls[k][2], d["mpt2d_f"].detach().cpu())
    assert len(d["mpt3d"]) > 0
    est = _c2w_of(sol.result(0, 2))
    assert torch.equal(out["c2w_est"], est)
    R64, t64 = lo.pose_err(c2w_gt, est)
    assert float(out["R_err"][0]) == pytest.approx(R64, rel=1e-12, abs=1e-9) and float(out["t_err"][0]) == pytest.approx(t64, rel=1e-12, abs=1e-12)
    tr = lo.localize(c2w_gt, rc2w, None, 3, render=lambda p: p, match=lambda p: [0] * out["num_matches"][0],
                     solve=lambda m, it=iter(range(3)): _c2w_of(sol.result(0, next(it))), cache_iters=True)
    assert [k for k, _ in tr["renders"]] == [0, 1, 2] and all(torch.equal(c["poses"][0], p.float()) for c, (_, p) in zip(calls, tr["renders"]))
    assert [float(v) for v in out["iter_t_errs"]] == pytest.approx(tr["iter_t_errs"], rel=1e-12, abs=1e-12)
    assert [float(v) for v in out["iter_R_errs"]] == pytest.approx(tr["iter_R_errs"], rel=1e-12, abs=1e-9)
    assert tr["iter_t_errs"][2] < tr["iter_t_errs"][0]


def test_a_batch_gives_every_query_its_own_trace(gpu, built_lib):
    """Q = 4 from cached points (an earlier render), iters = 3; query 2's solve fails in iteration 1, query 3 is never solved.  Every
    query's renders, matches, poses and errors equal its own batch-of-one run bit for bit."""
    fails = lambda q, k: q == 3 or (q == 2 and k == 1)

    ev, ren, calls, matches, _ = _setup(gpu)
    base = []
    for q in range(4):  # the cached points: an earlier render from the retrieved pose
        b = make_batch(H, W, q)
        o = ren.render_novel_views((H, W), b["K"][0], b["rc2w"], b["unnorm_scene"][0], gpu, want_im_pred=False)
        b["pt3d"], b["pt_feat"], b["pt_mask"] = o["pt3d"].cpu(), o["pt_feat"].cpu(), torch.ones(1, R, dtype=torch.bool)
        base.append(b)
    runs = {}
    for q in range(4):
        calls.clear()
        matches.clear()
        sol = Solver([q], fails)
        out = ev.eval_batch({k: v.clone() for k, v in base[q].items()}, renderer=ren, iters=3, solver=sol, cached_pt=True, cache_iters=True)
        runs[q] = (out, list(calls), list(matches), sol)
    assert [len(runs[q][1]) for q in range(4)] == [2, 2, 1, 0]
    calls.clear()
    matches.clear()
    sol = Solver(range(4), fails)
    out = ev.eval_batch(_stack([{k: v.clone() for k, v in b.items()} for b in base]), renderer=ren, iters=3, solver=sol, cached_pt=True,
                        cache_iters=True)
    assert len(sol.calls) == 12 and len(matches) == 3
    # renders: iteration 1 of queries 0, 1, 2 (one launch sequence), iteration 2 of queries 0, 1; nothing for query 3
    assert [c["poses"].shape[0] for c in calls] == [3, 2]
    for i, (call, rows) in enumerate(zip(calls, ([0, 1, 2], [0, 1]))):
        for j, q in enumerate(rows):
            one = runs[q][1][i]
            for key in ("poses", "pt3d", "pt_feat"):
                assert torch.equal(call[key][j], one[key][0]), (q, key)
    for q in range(4):
        one, _, m1, s1 = runs[q]
        assert out["num_matches"][q] == one["num_matches"][0]
        assert float(out["R_err"][q]) == float(one["R_err"][0]) and float(out["t_err"][q]) == float(one["t_err"][0])
        assert (out["c2w_ests"][q] is None) == (one["c2w_est"] is None) and (q != 3) == (one["c2w_est"] is not None)
        if q != 3:
            assert torch.equal(out["c2w_ests"][q], one["c2w_est"])
        assert [float(v) for v in out["iter_t_errs"][q]] == [float(v) for v in one["iter_t_errs"]]
        assert [float(v) for v in out["iter_R_errs"][q]] == [float(v) for v in one["iter_R_errs"]]
        for k in range(3):
            sel = (matches[k]["bids"] == q).cpu()
            for key in MATCH_KEYS:
                assert torch.equal(matches[k][key].cpu()[sel], m1[k][key].cpu()), (q, k, key)
            ids = matches[k]["ids"].cpu()
            assert torch.equal(ids[1:, ids[0] == q], m1[k]["ids"].cpu()[1:]), (q, k)
            got = [c for c in sol.calls if c[0] == q and c[1] == k]
            assert len(got) == 1 and torch.equal(got[0][3], s1.calls[k][3]) and torch.equal(got[0][2], s1.calls[k][2])
    assert sum(out["num_matches"]) > 0


def test_retrieval_only(gpu, built_lib):
    """retrieval_only, iters = 2: nothing is rendered, the matcher is not called, the errors are those of the retrieved poses."""
    ev, ren, calls, matches, _ = _setup(gpu)
    spy = []
    for name in ("forward", "forward_begin"):
        f = getattr(ev.model, name)
        setattr(ev.model, name, lambda *a, _f=f, **kw: (spy.append(1), _f(*a, **kw))[1])
    sol = Solver([0, 1])
    bs = [make_batch(H, W, q) for q in range(2)]
    out = ev.eval_batch(_stack(bs), renderer=ren, iters=2, solver=sol, retrieval_only=True, cache_iters=True)
    assert len(calls) == 0 and len(spy) == 0 and len(sol.calls) == 0 and len(matches) == 0
    for q in range(2):
        R64, t64 = lo.pose_err(bs[q]["c2w"][0], bs[q]["rc2w"][0])
        assert float(out["R_err"][q]) == pytest.approx(R64, rel=1e-12) and float(out["t_err"][q]) == pytest.approx(t64, rel=1e-12)
        assert out["num_matches"][q] == 0 and len(out["iter_t_errs"][q]) == 2


def test_inerf_in_the_loop(gpu, built_lib):
    """iNeRF (num_optim = 2, eval_pose) inside a 2-iteration loop with cache_iters: the trace has the loop oracle's length and entries,
    and iteration 1 re-renders from the refined pose.  (The refinement's own values are pinned by tests/test_inerf_gpu.py.)"""
    ev, ren, calls, matches, _ = _setup(gpu)
    refined = []
    inerf = ev.inerf_refinement

    def rec(batch, renderer, unnorm, c2w_est, conf, **kw):
        res = inerf(batch, renderer, unnorm, c2w_est, conf, **kw)
        refined.append((torch.as_tensor(c2w_est).clone(), res))
        return res

    ev.inerf_refinement = rec
    b = make_batch(H, W, 1)
    sol = Solver([1])
    conf = Namespace(lrate=0.002, lrdecay=False, num_optim=2, eval_pose=True, ds=8)
    torch.manual_seed(3)
    out = ev.eval_batch(b, renderer=ren, inerf_conf=conf, iters=2, solver=sol, cached_pt=False, cache_iters=True)
    assert len(refined) == 2 and len(calls) == 2 and len(sol.calls) == 2
    it = iter(refined)
    tr = lo.localize(b["c2w"][0], b["rc2w"][0], None, 2, render=lambda p: p, match=lambda p: [0],
                     solve=lambda m, ks=iter(range(2)): _c2w_of(sol.result(1, next(ks))),
                     refine=lambda pose: (lambda r: (r[1][0], float(r[1][1]), float(r[1][2]), []))(next(it)), cache_iters=True)
    assert len(out["iter_t_errs"]) == len(tr["iter_t_errs"]) == 4
    assert [float(v) for v in out["iter_t_errs"]] == pytest.approx(tr["iter_t_errs"], rel=1e-12, abs=1e-12)
    assert [float(v) for v in out["iter_R_errs"]] == pytest.approx(tr["iter_R_errs"], rel=1e-12, abs=1e-9)
    for (k, pose), (start, _) in zip(tr["refines"], refined):
        assert torch.equal(start.float(), torch.as_tensor(pose).float())
    assert torch.equal(calls[1]["poses"][0], torch.as_tensor(refined[0][1][0]).float())
    assert torch.equal(torch.as_tensor(out["c2w_est"]), torch.as_tensor(refined[1][1][0]))
