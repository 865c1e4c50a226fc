"""GPU: nm_refbank_visibility / nm_refbank_select / nm_refbank_gather (csrc/ref_bank.hip) through ref_bank.ReferencePointBank against the
host path of the same bank -- torch.equal on the visibility words, decisions, n_visible, the list and every output tensor -- and against
the reference's visible sets (tests/golden/ref_bank.npz).

Shapes: n of 1, 63, 64, 65 (a wavefront and its neighbours), k n of 1025, 1026 and 1056 (just past the select kernel's 1024-candidate
chunk: a second chunk in the scan and a last partial wavefront), of 8193 (one candidate past the eight chunks it loads together), and
of 65536 and 65538 (a full scan group of 64 chunks, and two candidates past it: the carry between groups), k of 1, 2, 3, 10 and 32 (bit 31 of the words), D of 4, 128 and 256 (less than one,
half and exactly one 16-byte vector per lane), row counts of 1, Nv - 1, Nv, Nv + 1 and 2 Nv + 3, and Nv = 1."""
import pytest
import torch

import ref_bank_util as ru
from nerfmatch_amd.ref_bank import ReferencePointBank

pytestmark = pytest.mark.gpu


def banks(args, gpu, **kw):
    """the same bank on the GPU and on the host"""
    return ReferencePointBank(**args, device=gpu, **kw), ReferencePointBank(**args, device="cpu", **kw)


def check_against_host(dev, host, ref_ids, rows=None, **kw):
    """selection, stacked sets and sampled sets (row counts around the first query's Nv unless given) of `ref_ids`, kernels vs host path;
    -> the host selection"""
    ids_dev = ref_ids.to(dev.device)
    h_sel = host.select(ref_ids)
    ru.assert_same_selection(dev.select(ids_dev), h_sel)
    ru.assert_same_sets(dev.reference_sets(ids_dev), host.reference_sets(ref_ids))
    Nv = int(h_sel["n_visible"][0])
    for P in sorted({1, max(Nv - 1, 1), Nv, Nv + 1, 2 * Nv + 3}) if rows is None else rows:
        d_out = dev.reference_sets(ids_dev, sample_mode="rand", sample_pts=P, **kw)
        ru.assert_same_sets(d_out, host.reference_sets(ref_ids, sample_mode="rand", sample_pts=P, **kw))
        ru.assert_rows_are_their_sources(dev, d_out)
    assert dev.bad_ids == 0
    return h_sel


@pytest.mark.parametrize("n,k,D", [(1, 1, 4), (1, 32, 4), (63, 2, 128), (64, 3, 256), (65, 10, 4), (342, 3, 128), (33, 32, 4), (1025, 1, 4), (65, 32, 256), (2731, 3, 4),
                                   (16384, 4, 4), (21846, 3, 4)])
def test_shape_sweep(gpu, built_lib, n, k, D):
    F = 6
    dev, host = banks(ru.synth_args(F, n, D, seed=n + k), gpu, seed=n)
    g = torch.Generator().manual_seed(k)
    ref_ids = torch.randint(0, F, (2, k), generator=g)
    sel = check_against_host(dev, host, ref_ids)
    print(f"n = {n}, k = {k}, D = {D}: Nv = {sel['n_visible'].tolist()} of {k * n}, decisions = {[hex(d & 0xFFFFFFFF) for d in sel['decisions'].tolist()]}")
    assert int(sel["n_visible"].min()) >= 1


def test_both_decisions_occur_in_late_rounds(gpu, built_lib):
    """the sweep's banks are random: this one is checked to take unions and intersections after round 0, in one batch"""
    dev, host = banks(ru.synth_args(12, 65, 8, seed=1), gpu)
    g = torch.Generator().manual_seed(1)
    sel = check_against_host(dev, host, torch.randint(0, 12, (3, 3), generator=g), rows=(40,))
    dec = sel["decisions"].tolist()
    assert any(d >> 1 for d in dec) and any((~d & 0b110) for d in dec), dec


def test_a_single_visible_candidate(gpu, built_lib):
    args = ru.synth_args(2, 3, 4, seed=0)
    args["c2w"] = torch.eye(4)[None].repeat(2, 1, 1)
    args["pt3d"][0] = torch.tensor([[50.0, 0.0, 3.0], [0.1, 0.1, 3.0], [0.0, 50.0, 3.0]])
    dev, host = banks(args, gpu)
    sel = check_against_host(dev, host, torch.tensor([[0]]), rows=(1, 2, 5))
    assert sel["n_visible"].tolist() == [1] and sel["list"].tolist() == [[1, -1, -1]]
    out = dev.reference_sets(torch.tensor([[0]], device=gpu), sample_mode="rand", sample_pts=5)
    assert ru.source_ids(out).tolist() == [[1] * 5]


@pytest.mark.parametrize("tag", ru.CASES)
def test_the_references_visible_sets(gpu, built_lib, tag):
    """the kernels against the golden file directly (the ties 3 I == V and 3 I == V - 1 among the cases)"""
    fx = ru.fixture()
    dev, ref_ids = ru.golden_bank(tag, gpu)
    sel = dev.select(ref_ids.to(gpu))
    Nv = int(fx[f"{tag}_n_visible"])
    steps = fx[f"{tag}_steps"]
    assert sel["n_visible"].tolist() == [Nv]
    assert sel["decisions"].tolist() == [sum(int(u) << j for j, u in enumerate(steps[:, 2].tolist()))]
    assert torch.equal(sel["list"][0, :Nv].cpu().long(), torch.nonzero(fx[f"{tag}_visible"])[:, 0]) and bool((sel["list"][0, Nv:] == -1).all())
    check_against_host(dev, ru.golden_bank(tag)[0], ref_ids)
    rand = dev.reference_sets(ref_ids.to(gpu), sample_mode="rand", sample_pts=3)
    assert torch.equal(rand["rc2w"][0].cpu(), fx[f"{tag}_rc2w_rand"])
    assert torch.equal(dev.reference_sets(ref_ids.to(gpu))["rc2w"][0].cpu(), fx[f"{tag}_rc2w_none"])


def test_a_batch_of_three_with_different_nv(gpu, built_lib):
    dev, host = banks(ru.synth_args(F=7, n=40, D=8, seed=3), gpu, seed=5)
    rows = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 0, 3]])
    sel = check_against_host(dev, host, rows, sample_keys=[11, 12, 13], draw=2)
    assert len(set(sel["n_visible"].tolist())) == 3
    # a query alone is the query in the batch
    kw = dict(sample_mode="rand", sample_pts=60, draw=2)
    batch = dev.reference_sets(rows.to(gpu), sample_keys=[11, 12, 13], **kw)
    for b in range(3):
        alone = dev.reference_sets(rows[b : b + 1].to(gpu), sample_keys=[11 + b], **kw)
        assert all(torch.equal(alone[key][0], batch[key][b]) for key in ("pt3d", "pt_feat", "pt_mask", "rc2w", "n_visible", "decisions"))


def test_4096_points_without_a_border_margin(gpu, built_lib):
    """random points, projections anywhere (also on the borders' last bits): both paths are fixed-order fp32 and must agree bit for bit"""
    dev, host = banks(ru.synth_args(F=4, n=1024, D=4, seed=9), gpu)
    sel = check_against_host(dev, host, torch.tensor([[2, 0, 3, 1]]), rows=(500,))
    words = ru.words_u32(sel["words"])[0]
    assert 0 < int((words & 1).sum()) < 4096 and int(sel["n_visible"]) < 4096


def test_non_finite_points_and_depth_zero_set_no_bit(gpu, built_lib):
    args = ru.synth_args(F=3, n=70, D=4, seed=6)
    args["c2w"][0] = torch.eye(4)  # frame 0: p.z is the point's own z
    clean_dev, clean_host = banks(args, gpu)
    inf, nan = float("inf"), float("nan")
    bad_rows = torch.tensor([[nan, 0.0, 3.0], [0.0, nan, nan], [inf, 0.0, 3.0], [0.0, -inf, 3.0], [0.0, 0.0, inf], [-inf, inf, -inf], [0.3, 0.2, 0.0],
                             [0.0, 0.0, 0.0]])
    dirty = dict(args, pt3d=args["pt3d"].clone())
    dirty["pt3d"][1, 5 : 5 + len(bad_rows)] = bad_rows
    dev, host = banks(dirty, gpu)
    ref_ids = torch.tensor([[0, 1, 2], [1, 1, 0]])
    sel = check_against_host(dev, host, ref_ids, rows=(90,))
    words, clean = ru.words_u32(sel["words"]), ru.words_u32(clean_host.select(ref_ids)["words"])
    n = 70
    cand = torch.arange(5, 5 + len(bad_rows))
    for b, s in ((0, 1), (1, 0), (1, 1)):  # the appearances of frame 1: not finite -> no bit in any camera
        assert bool((words[b, s * n + cand[:6]] == 0).all())
    # depth 0 in frame 0's camera (slot 0 of query 0, slot 2 of query 1): that bit is clear
    assert bool((words[0, 1 * n + cand[6:]] & 1 == 0).all()) and bool((words[1, 0 * n + cand[6:]] & 4 == 0).all())
    # every other candidate's word is what it is without the bad rows
    keep = torch.ones(2, 3 * n, dtype=torch.bool)
    keep[0, 1 * n + cand] = keep[1, 0 * n + cand] = keep[1, 1 * n + cand] = False
    assert torch.equal(words[keep], clean[keep])
    ru.assert_same_selection(clean_dev.select(ref_ids.to(gpu)), clean_host.select(ref_ids))


def test_bad_frame_ids_are_clamped_and_counted(gpu, built_lib):
    F = 4
    dev, host = banks(ru.synth_args(F, 20, 8, seed=7), gpu)
    ids = torch.tensor([[F, -1, 1]], device=gpu)  # device ids are not read back: the kernels clamp
    clamped = torch.tensor([[F - 1, 0, 1]])
    ru.assert_same_sets(dev.reference_sets(ids), host.reference_sets(clamped))
    assert dev.bad_ids == 2
    ru.assert_same_sets(dev.reference_sets(ids, sample_mode="rand", sample_pts=33), host.reference_sets(clamped, sample_mode="rand", sample_pts=33))
    assert dev.bad_ids == 4  # (the counter is add-only: two more from the second gather)
    ru.assert_same_selection(dev.select(ids), host.select(clamped))
    with pytest.raises(ValueError, match="outside"):  # the same ids on the host raise
        dev.reference_sets(ids.cpu())


def test_two_calls_and_a_side_stream_give_the_same_bits(gpu, built_lib):
    dev, _ = banks(ru.synth_args(8, 200, 128, seed=8), gpu)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 8, (4, 10), generator=g).to(gpu)
    kw = dict(sample_mode="rand", sample_pts=777)
    first, second = dev.reference_sets(ids, **kw), dev.reference_sets(ids, **kw)
    sel1, sel2 = dev.select(ids), dev.select(ids)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third, sel3 = dev.reference_sets(ids, **kw), dev.select(ids)
        stacked3 = dev.reference_sets(ids)
    side.synchronize()
    stacked1 = dev.reference_sets(ids)
    for other, osel, ostack in ((second, sel2, stacked1), (third, sel3, stacked3)):
        ru.assert_same_sets(other, first)
        assert all(torch.equal(sel1[key], osel[key]) for key in sel1)
        assert all(ru.same_bits(stacked1[key], ostack[key]) for key in ("pt3d", "pt_feat", "pt_mask"))


def test_sets_are_made_without_a_host_read_back(gpu, built_lib):
    dev, _ = banks(ru.synth_args(4, 50, 8, seed=2), gpu)
    ids = torch.tensor([[0, 1, 2], [3, 2, 1]], device=gpu)
    dev.reference_sets(ids, sample_mode="rand", sample_pts=16)  # (library load, first launches)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = dev.reference_sets(ids, sample_mode="rand", sample_pts=40, draw=1)
        b = dev.reference_sets(ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert a["pt3d"].shape == (2, 40, 3) and b["pt3d"].shape == (2, 3, 50, 3)


@pytest.mark.parametrize("mode", [None, "rand"])
def test_the_gather_writes_only_its_own_tensors(gpu, built_lib, mode):
    """the three outputs sit inside larger poisoned buffers: the bytes around them are untouched"""
    dev, host = banks(ru.synth_args(5, 37, 12, seed=5), gpu)
    ids = torch.tensor([[4, 0, 2], [1, 1, 3]])
    B, k = ids.shape
    P = 29 if mode else k * dev.n
    pad = 256
    POISON_F, POISON_B = -123456.0, 0xAB
    bufs = [torch.full((2 * pad + B * P * w,), POISON_F, device=gpu) for w in (3, dev.D)] + [torch.full((2 * pad + B * P,), POISON_B, dtype=torch.uint8, device=gpu)]
    out = (bufs[0][pad:-pad].view(B, P, 3), bufs[1][pad:-pad].view(B, P, dev.D), bufs[2][pad:-pad].view(torch.bool).view(B, P))
    got = dev.reference_sets(ids.to(gpu), sample_mode=mode, sample_pts=P if mode else -1, out=out)
    want = host.reference_sets(ids, sample_mode=mode, sample_pts=P if mode else -1)
    ru.assert_same_sets(got, want)
    assert got["pt_feat"].data_ptr() == out[1].data_ptr()
    for buf, poison in zip(bufs, (POISON_F, POISON_F, POISON_B)):
        assert bool((buf[:pad] == poison).all()) and bool((buf[-pad:] == poison).all())
    assert not bool((bufs[1][pad:-pad] == POISON_F).any())
