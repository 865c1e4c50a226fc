"""What test_match_routes_gpu.py relies on (match_loss_util.py), checked without a GPU: the generalised reference is the oracle's loss, the
case table reaches every kernel choice of csrc/match.hip, and no case has an entry next to a clamp bound."""
import math

import pytest
import torch

import match_loss_util as mu
from oracle import train_oracle as to


@pytest.mark.parametrize("name", ["c-90x70-B2", "d-aligned", "a-40x5124"])
def test_reference_loss_is_the_oracle_loss_bit_for_bit(name):
    case = mu.CASE[name]
    assert (case.alpha, case.gamma, case.clamp) == (0.25, 2.0, 1)
    x, r = mu.inputs_of(case), mu.reference_of(case)
    assert set(x["gt"].unique().tolist()) == {0, 1}
    assert torch.equal(r["conf"], r["conf_leaf"])  # the differentiated expression IS the oracle's coarse_matching
    want = to.matching_loss(r["conf"], x["gt"])
    assert r["loss"].dtype == torch.float64 and torch.equal(r["loss"], want)
    assert torch.equal(mu.focal_loss(r["conf"].float(), x["gt"].bool()), to.matching_loss(r["conf"].float(), x["gt"].bool()))


def test_reference_gradients_against_their_definitions():
    """ddot and dscale against central differences of the float64 loss; t, row_t, col_t against the closed form of the kernels' header."""
    case = mu.CASE["c-90x70-masked"]
    x, r = mu.inputs_of(case), mu.reference_of(case)
    gt, conf = x["gt"], r["conf"]
    wp, wn = 1.0 / (gt == 1).sum().item(), 1.0 / (gt == 0).sum().item()
    c = conf.clamp(1e-6, 1 - 1e-6)
    inside = (conf >= 1e-6) & (conf <= 1 - 1e-6)
    g_pos = -0.25 * wp * ((1 - c) ** 2 / c - 2 * (1 - c) * c.log())
    g_neg = -0.25 * wn * (2 * c * (1 - c).log() - c**2 / (1 - c))
    t = conf * torch.where(gt == 1, g_pos, g_neg) * inside
    assert mu.rel(r["t"], t, floor=0.0) < 1e-12 and mu.rel(r["row_t"], t.sum(2), floor=0.0) < 1e-12 and mu.rel(r["col_t"], t.sum(1), floor=0.0) < 1e-12
    assert mu.rel_scalar(r["dscale"].sum(), r["dscale_total"]) < 1e-12
    h = 1e-3  # (d loss / d scale is ~1e-6 of the loss here: the difference quotient carries 1e-16 / h of rounding)
    lp = mu.reference(x["im"], x["pt"], case.scale + h, x["im_mask"], x["pt_mask"], gt, 0.25, 2.0, 1)["loss"]
    lm = mu.reference(x["im"], x["pt"], case.scale - h, x["im_mask"], x["pt_mask"], gt, 0.25, 2.0, 1)["loss"]
    print(f"d loss / d scale: autograd {r['dscale_total'].item():.9e}, central difference {((lp - lm) / (2 * h)).item():.9e}")
    assert mu.rel_scalar((lp - lm) / (2 * h), r["dscale_total"]) < 1e-5
    # masked entries: no gradient (masked_fill), exactly; conf 0 but where a masked row meets a masked column (two flat soft-maxes: 1 / (M N))
    keep = x["im_mask"][:, :, None].bool() & x["pt_mask"][:, None].bool()
    assert (~keep).any() and bool((r["ddot"][~keep] == 0).all()) and r["conf"][~keep].max().item() <= 1.0001 / (case.M * case.N)
    # grad_loss scales ddot and dscale, nothing else
    r3 = mu.reference(x["im"], x["pt"], case.scale, x["im_mask"], x["pt_mask"], gt, 0.25, 2.0, 1, grad_loss=3.0)
    assert torch.equal(r3["ddot"], 3.0 * r["ddot"]) and torch.equal(r3["row_t"], r["row_t"]) and torch.equal(r3["loss"], r["loss"])


def test_route_restates_the_dispatch():
    assert mu.route(4800, 4800) == ("stats:vec-cached", "loss:tile", "bwd:vec4")
    assert mu.route(40, 5120)[0] == "stats:vec-cached" and mu.route(40, 5124)[0] == "stats:vec-uncached" and mu.route(40, 5121)[0] == "stats:scalar"
    # N = 8: 64 * 8 * 4 = 2048 bytes of scratch against align256(4 M) + 1024: the tile form up to M = 256
    assert mu.route(256, 8)[1] == "loss:tile" and mu.route(257, 8)[1] == "loss:two-kernel"
    assert mu.route(100, 72, gt_aligned=False) == ("stats:vec-cached", "loss:two-kernel", "bwd:vec1")
    assert mu.route(100, 72, pt_mask_aligned=False) == ("stats:vec-cached", "loss:tile", "bwd:vec1")
    assert mu.route(90, 70) == ("stats:scalar", "loss:two-kernel", "bwd:vec1")


def test_cases_cover_every_route_name():
    for c in mu.CASES:
        assert mu.route(c.M, c.N, (c.gt_off % 4 == 0) and (c.M * c.N % 4 == 0 or c.B == 1), c.pm_off is None or c.pm_off % 4 == 0) == c.expect, c.name
    for pos, names in enumerate(mu.ROUTE_NAMES):
        seen = {c.expect[pos] for c in mu.CASES}
        print(f"position {pos}: " + ", ".join(f"{n} ({sum(c.expect[pos] == n for c in mu.CASES)} cases)" for n in names))
        assert seen == set(names), (pos, seen)
    # the combinations the issue names: two-kernel loss in front of BOTH backward kernels, the uncached statistics in front of the tile loss
    combos = {c.expect for c in mu.CASES}
    assert ("stats:vec-cached", "loss:two-kernel", "bwd:vec4") in combos and ("stats:vec-cached", "loss:two-kernel", "bwd:vec1") in combos
    assert ("stats:vec-uncached", "loss:tile", "bwd:vec4") in combos and ("stats:vec-cached", "loss:tile", "bwd:vec1") in combos
    assert {c.C for c in mu.CASES} == {64, 128, 256, 512}
    assert {(c.alpha, c.gamma) for c in mu.CASES} >= {(0.25, 2.0), (0.4, 2.0), (0.25, 1.5), (0.25, 3.0), (1.0, 1.0)}


@pytest.mark.parametrize("case", mu.CASES, ids=lambda c: c.name)
def test_input_conditions(case):
    mu.check_input_conditions(case)
    x, r = mu.inputs_of(case), mu.reference_of(case)
    gt, conf = x["gt"], r["conf"]
    planted = conf[torch.arange(case.B)[:, None], torch.arange(case.k)[None], x["perm"]]
    print(f"{case.name}: n_pos {(gt == 1).sum().item()} n_neg {(gt == 0).sum().item()} ignored {(gt > 1).sum().item()}; planted conf "
          f"{planted.min().item():.3g} .. {planted.max().item():.3g}; positives {conf[gt == 1].min().item():.3g} .. {conf[gt == 1].max().item():.3g}; "
          f"negatives <= {conf[gt == 0].max().item():.3g}; loss {r['loss'].item():.6g}")
    assert torch.isfinite(r["ddot"]).all() and math.isfinite(r["loss"].item())


@pytest.mark.parametrize("name", ["g-100x72-clamp1", "g-90x70-clamp1", "h-64x64-peaked", "f-100x72", "f-90x70"])
def test_special_entries_in_the_reference(name):
    """What cases f, g, h are about holds in the reference the GPU results are compared with."""
    case = mu.CASE[name]
    x, r = mu.inputs_of(case), mu.reference_of(case)
    gt, m = x["gt"], x["marked"]
    b, i, j = m[:, 0], m[:, 1], m[:, 2]
    n_pos, n_neg = (gt == 1).sum().item(), (gt == 0).sum().item()
    plain = mu.reference(x["im"], x["pt"], case.scale, None, None, torch.where(gt > 1, torch.zeros_like(gt), gt), case.alpha, case.gamma, case.clamp)
    if case.special == "clamp-low":  # each labelled entry: -alpha (1 - 1e-6)^gamma log 1e-6 of the positive mean, t exactly 0
        assert bool((r["t"][b, i, j] == 0).all())
        others = gt.clone()
        others[b, i, j] = 2
        rest = mu.reference(x["im"], x["pt"], case.scale, None, None, others, case.alpha, case.gamma, case.clamp)
        term = -case.alpha * (1 - 1e-6) ** case.gamma * math.log(1e-6)
        pos_sum = lambda rr, g: (-case.alpha * (1 - rr["conf"].clamp(1e-6, 1 - 1e-6)[g == 1]) ** case.gamma * rr["conf"].clamp(1e-6, 1 - 1e-6)[g == 1].log()).sum().item()
        assert abs(pos_sum(r, gt) - pos_sum(rest, others) - 10 * term) < 1e-9 * 10 * term
    elif case.special == "peaked":  # the relabelled entries: -alpha c^gamma log(1 - c) at c = 1 - 1e-6 of the negative mean, t exactly 0
        assert bool((r["t"][b, i, j] == 0).all())
        sat = r["conf"] > 1 - 1e-6
        assert bool((r["t"][sat] == 0).all())
        term = -case.alpha * (1 - 1e-6) ** case.gamma * math.log(1e-6)
        c = r["conf"].clamp(1e-6, 1 - 1e-6)
        neg_terms = -case.alpha * c**case.gamma * (1 - c).log() * (gt == 0)
        assert mu.rel(neg_terms[b, i, j], torch.full((2,), term, dtype=torch.float64)) < 1e-9
        pos_terms = -case.alpha * (1 - c) ** case.gamma * c.log() * (gt == 1)
        assert pos_terms[sat].sum().item() < 1e-15  # the 30 saturated positives contribute ~0
        print(f"{name}: loss {r['loss'].item():.6g}, of which the two relabelled entries {2 * term / n_neg:.6g}")
    else:  # ignored: out of both means and counts, t exactly 0 there, the gradient there is the soft-max coupling alone
        assert bool((r["t"][b, i, j] == 0).all()) and (r["ddot"][b, i, j] != 0).any()
        rt, ct, conf = r["row_t"], r["col_t"], r["conf"]
        sim = case.scale * torch.einsum("bmd,bnd->bmn", *(f.double() / (f.double().norm(dim=-1, keepdim=True) + 1e-6) for f in (x["im"], x["pt"])))
        A, B = torch.softmax(sim, 1), torch.softmax(sim, 2)
        coupling = case.scale * (-A * ct[:, None, :] - B * rt[:, :, None])
        assert mu.rel(r["ddot"][b, i, j], coupling[b, i, j], floor=0.0) < 1e-10
        assert n_pos + n_neg + len(m) == gt.numel()
        assert abs(plain["loss"].item() - r["loss"].item()) > 1e-3 * r["loss"].item()  # labelling them negative instead is a different loss


@pytest.mark.parametrize("case", [c for c in mu.CASES if c.loose], ids=lambda c: c.name)
def test_recorded_fp32_errors(case):
    """The recorded float32 errors behind the loose bounds are float32 errors: a fresh evaluation lands within a factor 4 (the figure moves
    with the CPU's vector width and maths library, see "measured bounds" in match_loss_util.py)."""
    for what, recorded in case.loose:
        now = mu.fp32_error(case, what)
        print(f"{case.name} {what}: recorded {recorded:.3g}, here {now:.3g}; bound {mu.bound(case, what):.3g} against {mu.tolerances(case.flags)[what]:.3g}")
        assert recorded / 4 < now < recorded * 4 and mu.bound(case, what) == 4 * recorded
