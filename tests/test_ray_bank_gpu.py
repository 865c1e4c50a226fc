"""GPU: nm_raybank_frame_flags / nm_raybank_gather (csrc/ray_bank.hip) through nerf.ray_bank.RayBank -- against the host path of the same
bank, the oracle, rows expanded by the reference's own functions (tests/golden/ray_bank.npz) and nm_raygen, whose rows the kernel shares
bit for bit; the in-kernel epoch permutation against `epoch_ids`; the validation dictionaries; NerfTrainer.fit on a bank.

Shapes: four frames of 24 x 32 px (3072 rays: twelve workgroups), ray counts below, at and across a wavefront (64) and a workgroup (256),
a 3 x 3 frame (the smallest legal H), index spaces of 3, 65, 1000 and 4097 entries (Feistel halves of 1, 4, 5 and 7 bits)."""
from argparse import Namespace

import pytest
import torch

import nerf_pose_util as pu
import ray_bank_util as rb
from conftest import load_golden
from nerfmatch_amd.nerf.ray_bank import RayBank, epoch_ids

pytestmark = pytest.mark.gpu
H, W = rb.H, rb.W
maxdiff = lambda a, b: float((a.double().cpu() - b.double().cpu()).abs().max())

_TABLES = {}


def table(gpu, norm=True):
    """(rays, rgbs, ts, mask) of every pixel of the four frames from ONE gather launch; computed once per norm_ray_dir, read-only"""
    if norm not in _TABLES:
        bank = rb.bank(gpu, with_masks=True, norm_ray_dir=norm)
        _TABLES[norm] = (bank, bank.batch(rb.all_ids().to(gpu)))
        assert bank.bad_ids == 0
    return _TABLES[norm]


@pytest.mark.parametrize("norm", [True, False])
def test_every_pixel_against_the_host_path_and_the_oracle(gpu, built_lib, norm):
    bank, (rays, rgbs, ts, mask) = table(gpu, norm)
    host = rb.bank("cpu", with_masks=True, norm_ray_dir=norm)
    h_rays, h_rgbs, h_ts, h_mask = host.batch(rb.all_ids())
    assert torch.equal(bank.flags.cpu(), host.flags) and host.flags.tolist() == [0, 0, 0, 1]
    assert torch.equal(rgbs.cpu(), h_rgbs) and torch.equal(ts.cpu(), h_ts) and torch.equal(mask.cpu(), h_mask)
    assert mask.shape == (4 * H * W, 1) and 0 < float(mask.sum()) < mask.numel()
    ref = rb.oracle_rows()
    cols = slice(0, 12) if norm else [0, 1, 2, 6, 7, 8, 9, 10]  # (the oracle states unit directions only)
    e_oracle, e_host = maxdiff(rays[:, cols], ref[:, cols]), maxdiff(rays, h_rays)
    print(f"norm_ray_dir={norm}: max |kernel - oracle| = {e_oracle:.3e}, max |kernel - host path| = {e_host:.3e}")
    assert e_oracle < rb.RAY_BAR and e_host < rb.RAY_BAR
    assert bool((rays[3 * H * W :, 7] == 1.0).all())  # the flagged frame
    if not norm:
        assert maxdiff(rays[:, 3:6], h_rays[:, 8:11]) > 1e-2  # columns 3:6 really are the unnormalised directions


@pytest.mark.parametrize("norm", [True, False])
def test_rows_expanded_by_the_reference(gpu, built_lib, norm):
    z = load_golden("ray_bank")
    bank = RayBank(z["images"], z["c2w"], z["K"], norm_ray_dir=norm, device=gpu)
    rays, rgbs, _, _ = bank.batch(torch.arange(2 * 7 * 9))
    err = maxdiff(rays, z["rays_norm" if norm else "rays_unnorm"])
    print(f"kernel vs reference rows (norm_ray_dir={norm}): max |diff| = {err:.3e}")
    assert err < rb.RAY_BAR and torch.equal(rgbs.cpu(), z["rgbs"]) and bank.flags.tolist() == z["flags"].tolist()


def test_rows_outside_the_last_image_row_are_nm_raygens_bit_for_bit(gpu, built_lib):
    from nerfmatch_amd import ops

    rays = table(gpu)[1][0].reshape(4, H, W, 12)
    ref, flags = ops.raygen_batch(rb.intrinsics(), rb.poses(), H, W, gpu, ds=1)
    ref = ref.reshape(4, H, W, 12)
    assert flags.tolist() == [0, 0, 0, 1]
    assert torch.equal(rays[:, : H - 1], ref[:, : H - 1])
    # the last row: everything but the radius is shared, the radius is the reference's (nm_raygen's is not)
    assert torch.equal(rays[:, H - 1, :, :11], ref[:, H - 1, :, :11])
    assert maxdiff(rays[:, H - 1, :, 11], rb.oracle_rows().reshape(4, H, W, 12)[:, H - 1, :, 11]) < rb.RAY_BAR
    assert maxdiff(rays[:, H - 1, :, 11], ref[:, H - 1, :, 11]) > 1e-4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ray_counts_and_id_orders(gpu, built_lib, n):
    bank, full = table(gpu)
    g = torch.Generator().manual_seed(n)
    total = 4 * H * W
    for ids in (torch.randint(0, total, (n,), generator=g),             # any order
                torch.randint(0, 5, (n,), generator=g) * 700,           # repeats
                torch.arange(total - 1, total - 1 - n, -1)):            # descending
        got = bank.batch(ids.to(gpu))
        for a, b in zip(got, full):
            assert a.shape[0] == n and torch.equal(a, b[ids.to(gpu)])
    assert bank.bad_ids == 0


def test_smallest_frame(gpu, built_lib):
    from nerfmatch_amd import synth

    K, pose = synth.intrinsics(3, 3, 4.0), synth.camera_pose(4)[None]
    img = rb.images(1, 3, 3)
    rays, rgbs, _, _ = RayBank(img, pose, K, device=gpu).batch(torch.arange(9))
    assert maxdiff(rays, rb.no.make_rays(3, 3, K, pose[0], ds=1)) < rb.RAY_BAR
    assert maxdiff(rays, RayBank(img, pose, K, device="cpu").batch(torch.arange(9))[0]) < rb.RAY_BAR
    assert torch.equal(rgbs.cpu(), img.reshape(-1, 3).float().div(255))
    assert torch.equal(rays[6:, 11], rays[:3, 11])  # H = 3: the last row's radius is row 0's


def test_ids_outside_the_table_are_clamped_and_counted(gpu, built_lib):
    full = table(gpu)[1]
    bank = rb.bank(gpu, with_masks=True)  # (its own counter)
    total = 4 * H * W
    ids = torch.tensor([5, -1, total, total - 1, 0], device=gpu)  # device ids are not read back: the kernel clamps
    got = bank.batch(ids)
    assert bank.bad_ids == 2
    clamped = torch.tensor([5, 0, total - 1, total - 1, 0], device=gpu)
    for a, b in zip(got, full):
        assert torch.equal(a, b[clamped])
    with pytest.raises(ValueError, match="outside"):  # the same ids on the host raise
        bank.batch(ids.cpu())


@pytest.mark.parametrize("shape", [(1, 3, 1), (1, 5, 13), (10, 10, 10), (1, 17, 241)])
def test_the_kernels_permutation_is_epoch_ids(gpu, built_lib, shape):
    N = shape[0] * shape[1] * shape[2]
    for R in (1, 7) if N > 3 else (1,):
        bank = rb.id_bank(*shape, gpu, batch_rays=R, seed=3)
        for epoch in (0, 2):
            bank.set_epoch(epoch)
            got = torch.cat([rb.ids_from_rgbs(b["rgbs"][0]) for b in bank])
            assert torch.equal(got, epoch_ids(N, 3, epoch, torch.arange(N // R * R)))
            assert bank.bad_ids == 0
    whole = rb.id_bank(*shape, gpu, batch_rays=N, seed=3)  # one launch over all positions: every pixel once
    assert len(whole) == 1
    assert torch.equal(torch.sort(rb.ids_from_rgbs(next(iter(whole))["rgbs"][0])).values, torch.arange(N))


def test_the_permutation_through_a_valid_table_and_two_ranks(gpu, built_lib):
    m = rb.masks(10, 10, 10)
    keep = torch.nonzero(m.reshape(-1) < 128).reshape(-1)
    NV = len(keep)
    assert 100 < NV < 900
    kw = dict(masks_u8=m, batch_rays=16, seed=1)
    pose = torch.stack([rb.synth.camera_pose(20 + f) for f in range(10)])
    mk = lambda **k: RayBank(rb.id_images(10, 10, 10), pose, rb.synth.intrinsics(10, 10, 30.0), device=gpu, **kw, **k)
    bank = mk()
    assert torch.equal(bank.valid.cpu(), keep) and len(bank) == NV // 16
    batches = list(bank)
    got = torch.cat([rb.ids_from_rgbs(b["rgbs"][0]) for b in batches])
    assert torch.equal(got, keep[epoch_ids(NV, 1, 0, torch.arange(NV // 16 * 16))])
    assert all(bool((b["mask"] == 1).all()) and b["mask"].shape == (16, 1) for b in batches)
    # two ranks: together the positions of the epoch, each once (the tail shorter than 2 x 16 is dropped)
    halves = [torch.cat([rb.ids_from_rgbs(b["rgbs"][0]) for b in mk(rank=r, world_size=2)]) for r in (0, 1)]
    n2 = NV // 32 * 32
    assert len(halves[0]) == len(halves[1]) == n2 // 2
    want = keep[epoch_ids(NV, 1, 0, torch.arange(n2))]
    assert torch.equal(torch.sort(torch.cat(halves)).values, torch.sort(want).values)
    assert torch.equal(halves[1][:16], want[16:32])  # rank 1's first batch = positions 16 .. 31
    # without exclude_masks every pixel is visited and the mask key carries 1 - round(m / 255)
    every = mk(exclude_masks=False)
    b = next(iter(every))
    ids = rb.ids_from_rgbs(b["rgbs"][0])
    assert every.valid is None and len(every) == 1000 // 16
    assert torch.equal(b["mask"][:, 0].cpu(), 1 - torch.round(m.reshape(-1)[ids].float() / 255))


def test_producing_a_training_batch_does_not_synchronise(gpu, built_lib):
    bank = rb.bank(gpu, with_masks=True)
    bank.train_batch(0)  # (library load, first launch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = bank.train_batch(1)
        it = iter(bank)
        b2 = next(it)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert b["rays"].shape == (1, 64, 12) and b2["rays"].shape == (1, 64, 12)
    with pytest.raises(RuntimeError):  # the mode does catch a synchronising call on this build
        torch.cuda.set_sync_debug_mode("error")
        try:
            b["rays"].sum().item()
        finally:
            torch.cuda.set_sync_debug_mode("default")


def test_frame_batch_is_nm_raygen(gpu, built_lib):
    from nerfmatch_amd import ops

    bank = rb.bank(gpu)
    for f in (0, 3):
        one = bank.frame_batch(f, ds=8)
        ref, flag = ops.raygen(rb.intrinsics(), rb.poses()[f], H, W, gpu, ds=8)
        assert one["rays"].shape == (1, 12, 12) and torch.equal(one["rays"][0], ref) and int(flag) == (f == 3)
        assert torch.equal(one["rgbs"][0].cpu(), rb.images()[f, 4::8, 4::8].reshape(-1, 3).float().div(255))
        assert one["img_wh"].tolist() == [[4, 3]] and one["seq_ind"] == [[3, 0, 2, 1][f]]


def test_pair_batch_feeds_validation_step(gpu, built_lib):
    from nerfmatch_amd import synth
    from nerfmatch_amd.nerf_trainer import NerfTrainer

    unnorm = synth.unnorm_scene()
    bank = rb.bank(gpu, unnorm_scene=unnorm)
    pair = bank.pair_batch(0, 1)
    n = H * W
    assert pair["rays"].shape == (1, 2 * n, 12) and pair["rgbs"].shape == (1, 2 * n, 3) and pair["ts"].shape == (1, 2 * n)
    assert pair["c2w"].shape == (1, 8, 4) and pair["K"].shape == (1, 6, 3) and pair["unnorm_scene"].shape == (1, 4, 4)
    assert pair["img_idx"] == [0, 1] and pair["seq_ind"] == [3, 0] and pair["img_wh"][0][:2].tolist() == [W, H]
    assert torch.equal(pair["c2w"][0], torch.cat([unnorm @ rb.poses()[0], unnorm @ rb.poses()[1]]))
    assert torch.equal(pair["rays"][0], table(gpu)[1][0][: 2 * n])
    cfg = synth.nerf_config("7scenes", num_pts=32, img_wh=(W, H))
    cfg.data.train_pair_txt = "pairs.txt"
    tr = NerfTrainer(cfg, num_frames=5, device=gpu)
    tr.model.load_state_dict(synth.nerf_state_dict(seed=0, density_bias=3.0))
    metrics = tr.validation_step(pair)
    assert set(pu.KEYS) < set(metrics) and "rgb_fine_psnr" in metrics


def test_fit_trains_on_a_bank(gpu, built_lib):
    from nerfmatch_amd import synth
    from nerfmatch_amd.nerf_trainer import NerfTrainer

    pose = torch.stack([synth.camera_pose(30 + f) for f in range(4)])
    bank = RayBank(rb.images(4, 16, 16), pose, synth.intrinsics(16, 16, 20.0), batch_rays=64, device=gpu)
    assert len(bank) == 16
    cfg = synth.nerf_config("7scenes", num_pts=32, img_wh=(16, 16))
    cfg.optim = Namespace(optimizer="adam", lr=5e-4, weight_decay=0.0, lr_scheduler=None)
    tr = NerfTrainer(cfg, num_frames=4, device=gpu)
    tr.model.load_state_dict(synth.nerf_state_dict(seed=0, density_bias=3.0))
    first = bank.train_batch(0)["rgbs"].clone()
    losses = []
    tr.fit(bank, max_epochs=1, log=lambda e, i, m: losses.append(m["loss"]))
    assert tr.global_step == 16 and tr.current_epoch == 1 and len(losses) == 16
    assert all(bool(torch.isfinite(l)) for l in losses)
    bank.set_epoch(tr.current_epoch)  # what fit does at the start of the next epoch
    assert not torch.equal(bank.train_batch(0)["rgbs"], first)
    assert bank.bad_ids == 0
