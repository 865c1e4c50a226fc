"""Test helper (not product code): the fixture of the NeRF pose metrics, a float64 restatement of cosine mutual nearest-neighbour
matching (the yardstick of the GPU tests, pinned to the reference's recorded result by tests/test_nerf_pose_cpu.py), planted inputs and
the comparison rule.

Comparison rule for a kernel that forms the similarities in other arithmetic (split-bf16 matrix cores): a row (column) is excused only
if the restatement's own top-1 / top-2 gap in that row (column) is below GAP = 2e-4 -- twice the project's score tolerance of 1e-4, since
both candidates may move by it -- and at most 1 % of rows plus columns may be excused per case.  Every other nn12 / nn21 entry, and the
match list restricted to unexcused rows and columns, must be equal; every score within 1e-4 of the restatement's similarity."""
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
GAP = 2e-4
SCORE_TOL = 1e-4
MAX_EXCUSED = 0.01
KEYS = ("R_err_depth", "t_err_depth", "R_err_match", "t_err_match", "match_score", "num_matches")

_FX = None


def fixture():
    global _FX
    if _FX is None:
        z = np.load(GOLDEN / "nerf_pose_metrics.npz")
        _FX = {k: torch.from_numpy(np.asarray(z[k])) if z[k].ndim else z[k].item() for k in z.files}
    return _FX


def mutual_nn_f64(desc1, desc2, threshold=None, eps=1e-9):
    """d = desc / (|desc| + eps) per row, sim = d1 d2^T, nn12 / nn21 = first argmax per row / column, row i matches iff nn21[nn12[i]] == i;
    a truthy threshold keeps score > threshold.  Everything in float64 on the host."""
    d1, d2 = desc1.detach().cpu().double(), desc2.detach().cpu().double()
    d1 = d1 / (d1.norm(dim=1, keepdim=True) + eps)
    d2 = d2 / (d2.norm(dim=1, keepdim=True) + eps)
    sim = d1 @ d2.t()
    nn12, nn21 = torch.argmax(sim, dim=1), torch.argmax(sim, dim=0)  # (the first of several maxima)
    ids = torch.arange(sim.shape[0])
    keep = nn21[nn12] == ids
    matches, scores = torch.stack([ids[keep], nn12[keep]], dim=1), sim[ids, nn12][keep]
    if threshold:
        k = scores > threshold
        matches, scores = matches[k], scores[k]
    return dict(sim=sim, nn12=nn12, nn21=nn21, matches=matches, scores=scores)


def planted(n1, n2, C, seed, noise=0.7):
    """desc1 (n1, C) ~ N(0, 1); the first min(n1, n2) rows of desc2 are noisy copies of distinct rows of desc1, the others random; desc2's rows
    are then shuffled."""
    g = torch.Generator().manual_seed(seed)
    d1 = torch.randn(n1, C, generator=g)
    k = min(n1, n2)
    src = torch.randperm(n1, generator=g)[:k]
    d2 = torch.cat([d1[src] + noise * torch.randn(k, C, generator=g), torch.randn(n2 - k, C, generator=g)])
    return d1.contiguous(), d2[torch.randperm(n2, generator=g)].contiguous()


def gaps(sim):
    """top-1 minus top-2 of every row and of every column (inf where there is one candidate only)"""
    def gap(s):
        if s.shape[1] < 2:
            return torch.full((s.shape[0],), float("inf"), dtype=s.dtype)
        top = torch.topk(s, 2, dim=1).values
        return top[:, 0] - top[:, 1]

    return gap(sim), gap(sim.t())


def check_against_f64(desc1, desc2, matches, scores, nn12, nn21, what=""):
    """The comparison rule of the module docstring; prints the figures before it asserts.  Returns the restatement."""
    ref = mutual_nn_f64(desc1, desc2)
    matches, scores, nn12, nn21 = matches.cpu(), scores.cpu().double(), nn12.cpu().long(), nn21.cpu().long()
    n1, n2 = ref["sim"].shape
    row_gap, col_gap = gaps(ref["sim"])
    row_ok, col_ok = row_gap >= GAP, col_gap >= GAP
    excused = int((~row_ok).sum() + (~col_ok).sum())
    bad12, bad21 = int((nn12 != ref["nn12"])[row_ok].sum()), int((nn21 != ref["nn21"])[col_ok].sum())
    err = float((scores - ref["sim"][matches[:, 0], matches[:, 1]]).abs().max()) if len(matches) else 0.0
    restrict = lambda m: {(int(i), int(j)) for i, j in m.tolist() if row_ok[i] and col_ok[j]}
    print(f"{what} ({n1} x {n2}): {excused} of {n1 + n2} rows + columns excused (gap < {GAP:g}), {bad12} / {bad21} unexcused nn12 / nn21 entries differ, "
          f"{len(ref['matches'])} reference and {len(matches)} kernel matches, max score error {err:.3e}")
    assert excused <= MAX_EXCUSED * (n1 + n2), f"{what}: {excused} excused rows + columns, more than {MAX_EXCUSED:.0%} of {n1 + n2}"
    assert nn12.shape == (n1,) and nn21.shape == (n2,) and int(nn12.min()) >= 0 and int(nn12.max()) < n2 and int(nn21.min()) >= 0 and int(nn21.max()) < n1
    assert bad12 == 0 and bad21 == 0
    assert matches.dtype == torch.int64 and matches.shape == (len(scores), 2)
    assert bool((matches[1:, 0] > matches[:-1, 0]).all()), "matches are not in ascending row order"
    # the list is what the kernel's own nn12 / nn21 imply
    ids = torch.arange(n1)
    own = nn21[nn12] == ids
    assert torch.equal(matches, torch.stack([ids[own], nn12[own]], dim=1))
    assert restrict(matches) == restrict(ref["matches"])
    assert err <= SCORE_TOL
    return ref


def pose_inputs(device="cpu"):
    """(pts_fine, pt_mask, pts_feat, data) of fixture part (b)"""
    fx = fixture()
    data = dict(img_idx=[0, 1], img_wh=fx["pm_img_wh"], c2w=fx["pm_c2w"].to(device), K=fx["pm_K"].to(device), unnorm_scene=fx["pm_unnorm_scene"])
    return fx["pm_pts_fine"].to(device), fx["pm_pt_mask"], fx["pm_pts_feat"].to(device), data


class Recorder:
    """solver callable: records its (pt2d, pt3d, K) arguments, returns the fixture's pose of that call (or what `inner` returns)"""

    def __init__(self, inner=None):
        self.calls, self.inner = [], inner

    def __call__(self, pt2d, pt3d, K):
        self.calls.append((torch.as_tensor(pt2d).detach().cpu(), torch.as_tensor(pt3d).detach().cpu(), torch.as_tensor(K).detach().cpu()))
        if self.inner is not None:
            return self.inner(pt2d, pt3d, K)
        fx, q = fixture(), len(self.calls) - 1
        return fx["pm_pose_R"][q].numpy(), fx["pm_pose_t"][q].numpy(), np.arange(len(pt2d))


def check_sets(calls):
    """the four recorded correspondence sets against the fixture's: everything exactly"""
    fx = fixture()
    assert len(calls) == 4
    for q, (p2, p3, K) in enumerate(calls):
        assert torch.equal(p2.to(torch.int64), fx[f"pm_set{q}_pt2d"]), f"pixels of set {q}"
        assert p3.dtype == torch.float32 and torch.equal(p3, fx[f"pm_set{q}_pt3d"]), f"points of set {q}"
        assert torch.equal(K.float(), fx[f"pm_set{q}_K"]), f"intrinsics of set {q}"
