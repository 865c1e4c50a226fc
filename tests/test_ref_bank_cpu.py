"""CPU: the host path of ref_bank.ReferencePointBank (the plain-torch statement of the rule the kernels of csrc/ref_bank.hip implement)
against the reference's own load_ref_pts (tests/golden/ref_bank.npz: visible sets, per-step counts, both rc2w quirks, the stacked rows),
the properties of the sampling, fill + coarse_supervision against the reference's match-matrix rule restated on the sampled set, the
limits, and from_scene_dir on files in the cache format."""
import numpy as np
import pytest
import torch

import ref_bank_util as ru
import supervision_util as su
from nerfmatch_amd import supervision, synth
from nerfmatch_amd.ref_bank import ReferencePointBank, covisible, sample_slots

ROWS = {"1": lambda Nv: 1, "Nv-1": lambda Nv: Nv - 1, "Nv": lambda Nv: Nv, "Nv+1": lambda Nv: Nv + 1, "2Nv+3": lambda Nv: 2 * Nv + 3}


@pytest.mark.parametrize("tag", ru.CASES)
def test_selection_is_the_references(tag):
    """identical visible set, Nv, decisions and per-step (I, V, union); no exceptions allowed: the fixture keeps every projection
    0.01 px from the borders"""
    fx = ru.fixture()
    bank, ref_ids = ru.golden_bank(tag)
    sel = bank.select(ref_ids)
    visible, steps = fx[f"{tag}_visible"], fx[f"{tag}_steps"]
    Nv = int(fx[f"{tag}_n_visible"])
    assert torch.equal(sel["visible"][0], visible)
    assert sel["n_visible"].tolist() == [Nv] and Nv >= 1
    assert torch.equal(sel["steps"][0], steps)
    assert sel["decisions"].tolist() == [sum(int(u) << j for j, u in enumerate(steps[:, 2].tolist()))]
    assert torch.equal(sel["list"][0, :Nv].long(), torch.nonzero(visible)[:, 0]) and bool((sel["list"][0, Nv:] == -1).all())
    out = bank.reference_sets(ref_ids, sample_mode="rand", sample_pts=Nv + 2)
    assert out["n_visible"].tolist() == [Nv] and torch.equal(out["decisions"], sel["decisions"])


def test_the_fixture_has_the_cases_it_claims():
    fx = ru.fixture()
    assert fx["k3_steps"][:, 2].tolist() == [0, 1, 0]
    I, V, u = fx["tie_steps"][0].tolist()
    assert 3 * I == V and u == 0
    I, V, u = fx["tie_m1_steps"][0].tolist()
    assert 3 * I == V - 1 and u == 1
    ids = fx["k10_ref_ids"].tolist()
    assert len(ids) == 10 and len(set(ids)) < 10
    assert fx["scaled_frame_wh"].tolist()[0] != [ru.W, ru.H]
    # k1: rows 28 .. 32 lie behind the camera and are visible
    bank, _ = ru.golden_bank("k1")
    depth = (bank.cams[0, 9:].reshape(3, 4)[2, :3] * bank.pt3d[0]).sum(-1) + bank.cams[0, 20]
    assert bool((depth[28:] < 0).all()) and bool(fx["k1_visible"][28:].all())


@pytest.mark.parametrize("tag", ru.CASES)
def test_stacked_layout_and_both_rc2w(tag):
    fx = ru.fixture()
    bank, ref_ids = ru.golden_bank(tag)
    k, n, D = ref_ids.shape[1], bank.n, bank.D
    out = bank.reference_sets(ref_ids)
    assert out["pt3d"].shape == (1, k, n, 3) and out["pt_feat"].shape == (1, k, n, D) and out["pt_mask"].shape == (1, k, n)
    assert torch.equal(out["pt3d"].reshape(-1, 3), fx[f"{tag}_stacked_pt3d"]) and torch.equal(out["pt_feat"].reshape(-1, D), fx[f"{tag}_stacked_pt_feat"])
    assert out["pt_mask"].dtype == torch.bool and torch.equal(out["pt_mask"].reshape(-1), fx[f"{tag}_stacked_pt_mask"])
    assert out["n_visible"].tolist() == [k * n] and out["decisions"].tolist() == [0]
    assert torch.equal(out["rc2w"][0], fx[f"{tag}_rc2w_none"]) and torch.equal(out["unnorm_scene"][0], fx[f"{tag}_unnorm_scene"])
    rand = bank.reference_sets(ref_ids, sample_mode="rand", sample_pts=5)
    assert torch.equal(rand["rc2w"][0], fx[f"{tag}_rc2w_rand"])  # the LAST frame's pose
    if k > 1 and ref_ids[0, 0] != ref_ids[0, -1]:
        assert not torch.equal(rand["rc2w"], out["rc2w"])


@pytest.mark.parametrize("tag", ru.CASES)
@pytest.mark.parametrize("rows", list(ROWS))
def test_sampling_properties(tag, rows):
    fx = ru.fixture()
    bank, ref_ids = ru.golden_bank(tag)
    Nv = int(fx[f"{tag}_n_visible"])
    P = max(ROWS[rows](Nv), 1)
    out = bank.reference_sets(ref_ids, sample_mode="rand", sample_pts=P)
    assert out["pt3d"].shape == (1, P, 3) and out["pt_feat"].shape == (1, P, bank.D) and out["pt_mask"].shape == (1, P)
    ru.assert_rows_are_their_sources(bank, out)
    # candidates behind the rows: the list position of every row (the duplicated frames of k10 make bank rows ambiguous, candidates not)
    sel = bank.select(ref_ids)
    cand = sel["list"][0].long()[sample_slots(Nv, P, bank.seed, 0, 0)]
    frames = ref_ids[0][cand // bank.n]
    assert torch.equal(ru.source_ids(out)[0], frames * bank.n + cand % bank.n)
    first = cand[: min(P, Nv)]
    assert len(set(first.tolist())) == len(first) and bool(fx[f"{tag}_visible"][first].all())  # distinct and visible
    if P > Nv:
        assert torch.equal(cand[Nv:], cand[: P - Nv])  # row q equals row q - Nv
        for key in ("pt3d", "pt_feat", "pt_mask"):
            assert torch.equal(out[key][0, Nv:], out[key][0, : P - Nv])
    counts = torch.bincount(cand, minlength=len(fx[f"{tag}_visible"]))
    assert bool((counts[~fx[f"{tag}_visible"]] == 0).all())
    vis_counts = counts[fx[f"{tag}_visible"]]
    assert int(vis_counts.min()) >= P // Nv and int(vis_counts.max()) <= -(-P // Nv)


def test_rows_without_duplicate_frames_are_distinct_bank_rows():
    """the same property read off the outputs alone (features' id column), where no frame occurs twice"""
    for tag in ("k3", "tie_m1", "scaled"):
        bank, ref_ids = ru.golden_bank(tag)
        fx = ru.fixture()
        Nv = int(fx[f"{tag}_n_visible"])
        ids = ru.source_ids(bank.reference_sets(ref_ids, sample_mode="rand", sample_pts=Nv))[0]
        stacked_ids = fx[f"{tag}_stacked_pt_feat"][:, 0].long()
        assert torch.equal(torch.sort(ids).values, torch.sort(stacked_ids[fx[f"{tag}_visible"]]).values)


def test_draw_and_sample_keys_give_other_orders_and_a_query_does_not_depend_on_its_batch():
    args = ru.synth_args(F=7, n=40, D=8, seed=3)
    bank = ReferencePointBank(**args, device="cpu", seed=5)
    rows = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 0, 3]])
    kw = dict(sample_mode="rand", sample_pts=150)
    batch = bank.reference_sets(rows, sample_keys=[11, 12, 13], **kw)
    assert len(set(batch["n_visible"].tolist())) == 3
    for b in range(3):
        alone = bank.reference_sets(rows[b : b + 1], sample_keys=[11 + b], **kw)
        for key in ("pt3d", "pt_feat", "pt_mask", "rc2w", "n_visible", "decisions"):
            assert torch.equal(alone[key][0], batch[key][b]), key
    base = ru.source_ids(batch)
    assert not torch.equal(ru.source_ids(bank.reference_sets(rows, sample_keys=[11, 12, 13], draw=1, **kw)), base)
    assert not torch.equal(ru.source_ids(bank.reference_sets(rows, sample_keys=[21, 22, 23], **kw)), base)
    other_seed = ReferencePointBank(**args, device="cpu", seed=6)
    assert not torch.equal(ru.source_ids(other_seed.reference_sets(rows, sample_keys=[11, 12, 13], **kw)), base)
    # the default keys are the positions in the batch
    assert torch.equal(ru.source_ids(bank.reference_sets(rows, **kw)), ru.source_ids(bank.reference_sets(rows, sample_keys=[0, 1, 2], **kw)))
    # the same sets of rows whatever the order: every draw samples the same visible candidates
    a, b = torch.sort(base[0, : int(batch["n_visible"][0])]).values, ru.source_ids(bank.reference_sets(rows, sample_keys=[11, 12, 13], draw=1, **kw))[0]
    assert torch.equal(a, torch.sort(b[: int(batch["n_visible"][0])]).values)


def test_covisible_keeps_at_least_one_candidate_and_handles_32_views():
    g = torch.Generator().manual_seed(0)
    words = torch.randint(0, 1 << 32, (64, 50), generator=g, dtype=torch.int64)
    words[:8] = 0  # never inside any image: every round takes the union of nothing
    words[8:16] &= 1 << 31
    out = covisible(words, 32)
    assert int(out["n_visible"].min()) >= 1 and out["n_visible"][:8].tolist() == [50] * 8
    assert out["decisions"][:8].tolist() == [-1] * 8  # 32 unions: all bits set, as int32
    assert out["decisions"].dtype == torch.int32 and out["steps"].shape == (64, 32, 3)


def _restated_match_matrix(K, c2w, pt3d, pt_mask, h, w, ds):
    """nerfmatch_dataset.py:553-577 for one sample in fp64 (no fallback draw) -> match_gt (M, N), the distance to the next cell border"""
    qw2c = np.linalg.inv(c2w.astype(np.float64))
    cam = pt3d.astype(np.float64) @ qw2c[:3, :3].T + qw2c[:3, 3]
    proj = ((cam / cam[:, 2:3]) @ K.astype(np.float64).T)[:, :2]
    cells = np.floor(proj / ds).astype(np.int64)
    visible = (cells.min(-1) > 0) & (cells[:, 0] < (w // ds)) & (cells[:, 1] < (h // ds))
    M = (w // ds) * (h // ds)
    ids = (cells[:, 0] + cells[:, 1] * (w // ds)).clip(0, M - 1)
    match = np.zeros((M, len(pt3d)), np.float32)
    match[ids, np.arange(len(pt3d))] = 1.0
    match = pt_mask[None, :] * visible[None, :] * match
    return match, np.abs(proj / ds - np.round(proj / ds)).min() * ds


@pytest.mark.parametrize("mode", [None, "rand"])
def test_fill_then_coarse_supervision(mode):
    bank = ReferencePointBank(**ru.synth_args(F=5, n=30, D=8, seed=4), device="cpu")
    B, k, P, ds = 2, 3, 70, 8
    ref_ids = torch.tensor([[0, 1, 2], [4, 2, 3]])
    qc2w = torch.stack([synth.camera_pose(77, max_t=0.3), synth.camera_pose(78, max_t=0.3)])
    data = dict(image=torch.zeros(B, 3, ru.H, ru.W), K=synth.intrinsics(ru.H, ru.W, ru.FOCAL)[None].repeat(B, 1, 1), c2w=qc2w)
    bank.fill(data, ref_ids, sample_mode=mode, sample_pts=P if mode else -1)
    N = P if mode else k * bank.n
    assert data["pt3d"].shape == ((B, P, 3) if mode else (B, k, bank.n, 3)) and data["rc2w"].shape == (B, 4, 4) and data["unnorm_scene"].shape == (B, 4, 4)
    supervision.coarse_supervision(data, ds=ds)
    assert data["conf_gt"].shape == (B, (ru.H // ds) * (ru.W // ds), N)
    for b in range(B):
        want, margin = _restated_match_matrix(data["K"][b].numpy(), qc2w[b].numpy(), data["pt3d"][b].reshape(N, 3).numpy(),
                                              data["pt_mask"][b].reshape(N).numpy(), ru.H, ru.W, ds)
        # no point of this fixture sits within the fp32 projection bar (4 x the reference's own fp32 error) of a cell border: the cells
        # are not a rounding question
        assert margin > su.bar_px()
        assert want.sum() > 5 and np.array_equal(data["conf_gt"][b].numpy(), want.astype(np.uint8))


def test_limits_and_bad_ids_raise():
    args = ru.synth_args(F=3, n=10, D=8, seed=1)
    bank = ReferencePointBank(**args, device="cpu")
    for D in (6, 1028):
        with pytest.raises(ValueError, match="feature dimension"):
            ReferencePointBank(**{**args, "pt_feat": torch.zeros(3, 10, D)}, device="cpu")
    with pytest.raises(ValueError, match="pt3d"):
        ReferencePointBank(**{**args, "pt_feat": torch.zeros(3, 9, 8)}, device="cpu")
    with pytest.raises(ValueError, match="pt_mask"):
        ReferencePointBank(**{**args, "pt_mask": torch.ones(3, 9, dtype=torch.bool)}, device="cpu")
    for ids in ([[0, 3]], [[-1, 0]]):
        with pytest.raises(ValueError, match="outside"):
            bank.reference_sets(torch.tensor(ids))
        with pytest.raises(ValueError, match="outside"):
            bank.select(ids)
    with pytest.raises(ValueError, match="at most 32 views"):
        bank.reference_sets(torch.zeros(1, 33, dtype=torch.int64))
    big = ReferencePointBank(torch.zeros(1, (1 << 16) + 1, 3), torch.zeros(1, (1 << 16) + 1, 4), torch.eye(4)[None], synth.intrinsics(ru.H, ru.W, ru.FOCAL),
                             (ru.W, ru.H), (ru.W, ru.H), device="cpu")
    with pytest.raises(ValueError, match="candidates"):  # 16 * (2^16 + 1) > 2^20
        big.reference_sets(torch.zeros(1, 16, dtype=torch.int64))
    for P in (0, -1):
        with pytest.raises(ValueError, match="sample_pts > 0"):
            bank.reference_sets([[0, 1]], sample_mode="rand", sample_pts=P)
    with pytest.raises(ValueError, match="above"):
        bank.reference_sets([[0, 1]], sample_mode="rand", sample_pts=(1 << 20) + 1)
    with pytest.raises(ValueError, match="sample_mode"):
        bank.reference_sets([[0, 1]], sample_mode="grid", sample_pts=4)
    with pytest.raises(ValueError, match="sample_keys"):
        bank.reference_sets([[0, 1]], sample_mode="rand", sample_pts=4, sample_keys=[1, 2])
    with pytest.raises(ValueError, match="ref_ids"):
        bank.reference_sets(torch.tensor([0, 1]))


def test_draw_ref_ids_is_the_references_choice():
    rids = [7, 3, 9, 4, 1]
    assert ReferencePointBank.draw_ref_ids(rids, 3, "test") == [7, 3, 9] and ReferencePointBank.draw_ref_ids(rids, 5, "val") == rids
    with pytest.raises(ValueError, match="are needed"):
        ReferencePointBank.draw_ref_ids(rids, 6, "test")
    # train: np.random.choice(rids, k) (nerfmatch_dataset.py:447): with replacement, the same numbers from the same state
    got = ReferencePointBank.draw_ref_ids(rids, 12, "train", rng=np.random.RandomState(3))
    assert got == np.random.RandomState(3).choice(rids, 12).tolist() and len(set(got)) < 12 and set(got) <= set(rids)
    np.random.seed(4)
    want = np.random.choice(rids, 4).tolist()
    np.random.seed(4)
    assert ReferencePointBank.draw_ref_ids(rids, 4, "train") == want
    with pytest.raises(ValueError, match="no reference frames"):
        ReferencePointBank.draw_ref_ids([], 2, "train")


def test_from_scene_dir_round_trips_cache_files(tmp_path):
    args = ru.synth_args(F=3, n=12, D=8, seed=2, masks=False)
    Ks = torch.stack([synth.intrinsics(ru.H, ru.W, ru.FOCAL), synth.intrinsics(2 * ru.H, 2 * ru.W, 2 * ru.FOCAL), synth.intrinsics(ru.H, ru.W, 50.0)])
    whs = [(ru.W, ru.H), (2 * ru.W, 2 * ru.H), (ru.W, ru.H)]
    frames = []
    for f in range(3):
        fp = f"seq-0{f}/frame-00000{f}.color.png"
        frames.append(dict(file_path=fp, transform_matrix=args["c2w"][f].tolist(), intrinsics=Ks[f].tolist(), width=whs[f][0], height=whs[f][1]))
        name = fp.replace("/", "_").replace(".color", "").replace(".png", "")  # the reference's rule (data_loading.py:40)
        np.save(tmp_path / f"{name}.npy", dict(pt3d=args["pt3d"][f].numpy(), unnorm_scene=args["unnorm_scene"].numpy(), pt_feat=args["pt_feat"][f].numpy(),
                                                pt_color=np.zeros((12, 3), np.float32)))
    bank = ReferencePointBank.from_scene_dir(tmp_path, frames, (ru.W, ru.H), device="cpu", seed=9)
    direct = ReferencePointBank(args["pt3d"], args["pt_feat"], args["c2w"], Ks, torch.tensor(whs), (ru.W, ru.H), unnorm_scene=args["unnorm_scene"], device="cpu", seed=9)
    for key in ("pt3d", "pt_feat", "pt_mask", "cams", "c2w", "unnorm_scene"):
        assert torch.equal(getattr(bank, key), getattr(direct, key)), key
    assert bool(bank.pt_mask.all()) and bank.seed == 9
    assert torch.allclose(bank.cams[1, :9], bank.cams[0, :9])  # the double-size frame scales back to the target resolution
    ids = torch.tensor([[2, 0, 1]])
    a, b = bank.reference_sets(ids, sample_mode="rand", sample_pts=9), direct.reference_sets(ids, sample_mode="rand", sample_pts=9)
    assert all(torch.equal(a[key], b[key]) for key in ("pt3d", "pt_feat", "pt_mask", "rc2w"))
    np.save(tmp_path / "seq-02_frame-000002.npy", dict(pt3d=np.zeros((11, 3), np.float32), unnorm_scene=np.eye(4, dtype=np.float32),
                                                       pt_feat=np.zeros((11, 8), np.float32)))
    with pytest.raises(ValueError, match="holds 11 points"):
        ReferencePointBank.from_scene_dir(tmp_path, frames, (ru.W, ru.H), device="cpu")
    with pytest.raises(ValueError, match="use_msk"):
        ReferencePointBank.from_scene_dir(tmp_path, frames[:2], (ru.W, ru.H), use_msk="sky", device="cpu")
