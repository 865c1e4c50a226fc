"""csrc/match.hip on every route of its dispatch: the C entry points nm_focal_count, nm_dual_softmax_match, nm_match_focal_loss and
nm_match_focal_loss_bwd, driven directly (match_loss_util.run_pair), against the float64 reference of match_loss_util.py.  The case table,
its routes and the conditions on its inputs are checked without a GPU in test_match_loss_util_cpu.py."""
import numpy as np
import pytest
import torch

import match_loss_util as mu
from conftest import compare_matches
from oracle import matcher_oracle as mo

pytestmark = pytest.mark.gpu

_RESULTS = {}


def _run(case, gpu):
    """Every selection of the case, twice, on fresh outputs: {selection: (first run, second run)}, a run being one run_pair dict per pair.
    Kept per case (d compares against the aligned run of the same data)."""
    if case.name in _RESULTS:
        return _RESULTS[case.name]
    x = mu.inputs_of(case)
    im, pt = x["im"].to(gpu), x["pt"].to(gpu)
    gt = mu.offset_view(x["gt"].to(gpu), case.gt_off)
    im_mask = None if x["im_mask"] is None else x["im_mask"].to(gpu)
    pt_mask = None if x["pt_mask"] is None else x["pt_mask"].to(gpu) if case.pm_off is None else mu.offset_view(x["pt_mask"].to(gpu), case.pm_off)
    assert gt.data_ptr() % 16 == case.gt_off and (case.pm_off is None or pt_mask.data_ptr() % 16 == case.pm_off)
    for b in range(case.B):
        got = mu.route(case.M, case.N, gt[b].data_ptr() % 4 == 0, pt_mask is None or pt_mask[b].data_ptr() % 4 == 0)
        assert got == case.expect, (case.name, b, got)
    grad_loss = 3.0 if case.masked else None
    out = {}
    for mutual, threshold in case.selections:
        runs = []
        for _ in range(2):
            acc = mu.focal_count(gt) if case.B > 1 else None  # a batch: counted once, one acc through all pairs (as autograd.py)
            runs.append([mu.run_pair(im[b], pt[b], case.scale, None if im_mask is None else im_mask[b], None if pt_mask is None else pt_mask[b],
                                     gt[b], case.alpha, case.gamma, case.clamp, mutual, threshold, case.flags, grad_loss, acc)
                         for b in range(case.B)])
        out[(mutual, threshold)] = tuple(runs)
    _RESULTS[case.name] = out
    return out


@pytest.mark.parametrize("case", mu.CASES, ids=lambda c: c.name)
def test_case(gpu, built_lib, case):
    """Bounds: match_loss_util.bound.  Measured on the MI355X, worst case of each route against float64 (bound):
      conf           stats:vec-cached 4.9e-07, stats:vec-uncached 1.2e-06, stats:scalar 3.3e-07 (1e-5); split-bf16 GEMM 7.1e-07 (1e-4)
      loss           loss:tile 9.8e-06, loss:two-kernel 6.3e-06, split-bf16 GEMM 7.4e-06 (1e-5 relative); the nine cases of
                     match_loss_util "measured bounds": 1.0e-05 .. 1.8e-05 (2.0e-05 .. 2.2e-05) and h 6.1e-04 (2.4e-03)
      row_t, col_t   loss:tile 2.4e-05, loss:two-kernel 6.1e-06 (1e-4); split-bf16 GEMM 7.5e-07 (5e-3)
      ddot           bwd:vec4 9.3e-06, bwd:vec1 1.8e-07 (1e-4); split-bf16 GEMM 3.1e-07 (5e-3)
      dscale         bwd:vec4 3.2e-06, bwd:vec1 7.9e-08 (1e-4); split-bf16 GEMM 6.6e-08 (5e-3)
    A second call gave the same bytes wherever asked; the misaligned runs of d the same conf bytes as the aligned one."""
    mu.check_input_conditions(case)
    x, ref = mu.inputs_of(case), mu.reference_of(case)
    g = 3.0 if case.masked else 1.0
    figures, same = [], []
    for (mutual, threshold), (first, again) in _run(case, gpu).items():
        sel = f"mutual={mutual} threshold={threshold}"
        ids, _ = mo.mutual_matches(ref["conf"], mutual=mutual, threshold=threshold)
        for b, (r, r2) in enumerate(zip(first, again)):
            # the same bytes from a second call: always for the confidence and the selection; for the sums where nothing is accumulated with
            # atomics (the tile form; dscale is one fp64 atomic per workgroup in either form)
            names = ("conf", "i_ids", "j_ids", "mconf") + (("acc", "row_t", "col_t", "ddot") if case.expect[1] == "loss:tile" else ("row_t",))
            same += [(f"pair {b} {sel} {n}", torch.equal(r[n], r2[n])) for n in names]
            for rr in (r, r2):
                figures.append((f"pair {b} conf", (rr["conf"].double() - ref["conf"][b]).abs().max().item(), mu.bound(case, "conf")))
                figures += [(f"pair {b} {n}", mu.rel(rr[n], g * ref[n][b] if n == "ddot" else ref[n][b]), mu.bound(case, n)) for n in ("row_t", "col_t", "ddot")]
                figures.append((f"pair {b} dscale", mu.rel_scalar(rr["dscale"], g * ref["dscale"][b], 1e-3), mu.bound(case, "dscale")))
                assert all(torch.isfinite(rr[n]).all() for n in ("conf", "row_t", "col_t", "ddot", "mconf"))
            pick = ids[0] == b
            gi, gj = r["i_ids"], r["j_ids"]
            compare_matches((ids[1][pick], ids[2][pick]), (gi, gj), ref["conf"][b], mutual, f"{case.name} pair {b} {sel}")
            assert torch.all(gi[1:] > gi[:-1])
            figures.append((f"pair {b} {sel} mconf", (r["mconf"].double() - ref["conf"][b][gi, gj]).abs().max().item() if len(gi) else 0.0, mu.bound(case, "conf")))
            if case.name.startswith("a-"):  # the planted indices exactly
                got = dict(zip(gi.tolist(), gj.tolist()))
                assert all(got.get(i) == int(x["perm"][b, i]) for i in range(case.k)), sel
        for run in (first, again):  # the loss of the batch: the acc behind the last pair
            acc = run[-1]["acc"]
            assert acc[2].item() == (x["gt"] == 1).sum().item() and acc[3].item() == (x["gt"] == 0).sum().item()
            figures.append(("loss", mu.rel_scalar(run[-1]["loss"], ref["loss"]), mu.bound(case, "loss")))
    if case.name.startswith("d-") and case.name != "d-aligned":
        # against the aligned run of the same data: the statistics and the confidence do not read conf_gt / pt_mask differently -- same bytes; the
        # sums are the same fp32 terms added in another order, which the gradient bound covers
        al, r = _run(mu.CASE["d-aligned"], gpu)[case.selections[0]][0][0], _run(case, gpu)[case.selections[0]][0][0]
        same += [(f"aligned run {n}", torch.equal(r[n], al[n])) for n in ("conf", "i_ids", "j_ids", "mconf")]
        figures += [(f"aligned run {n}", mu.rel(r[n], al[n]), mu.bound(case, n)) for n in ("row_t", "col_t", "ddot")]
        figures.append(("aligned run loss", mu.rel_scalar(r["loss"], al["loss"]), mu.bound(case, "loss")))
        figures.append(("aligned run dscale", mu.rel_scalar(r["dscale"], al["dscale"], 1e-3), mu.bound(case, "dscale")))
    worst = {}
    for what, err, bnd in figures:
        key = what.split(" ")[-1]
        if err >= worst.get(key, (-1.0, 0.0))[0]:
            worst[key] = (err, bnd)
    print(f"{case.name} {case.expect}: " + "  ".join(f"{k} {e:.2e} ({b:.1e})" for k, (e, b) in worst.items()))
    bad = [(what, err, bnd) for what, err, bnd in figures if not err < bnd]
    assert not bad, bad
    assert all(ok for _, ok in same), [n for n, ok in same if not ok]


@pytest.mark.parametrize("total", mu.COUNT_SIZES)
def test_focal_count_alone(gpu, built_lib, total):
    """nm_focal_count on unaligned bases, short buffers, ragged tails and past the grid cap: exact counts, accumulated over two calls."""
    for off in mu.COUNT_OFFSETS:
        data = mu.count_bytes(total, seed=off)
        buf = torch.zeros(total + 32, device=gpu, dtype=torch.uint8)
        view = buf[off:off + total]
        view.copy_(data)
        assert view.data_ptr() % 16 == off
        n_pos, n_neg = int(np.count_nonzero(data.numpy() == 1)), int(np.count_nonzero(data.numpy() == 0))
        acc = mu.focal_count(view)
        once = acc.cpu().tolist()
        mu.focal_count(view, acc)
        twice = acc.cpu().tolist()
        print(f"total {total} offset {off}: {once} then {twice}; numpy {n_pos} positives, {n_neg} negatives")
        assert once == [0.0, 0.0, float(n_pos), float(n_neg)] and twice == [0.0, 0.0, 2.0 * n_pos, 2.0 * n_neg]
