"""CPU: the host path of nerf.ray_bank.RayBank (the plain-torch statement of the rules the gather kernel implements) against the oracle
and against rows expanded by the reference's own functions (tests/golden/ray_bank.npz), and the epoch permutation `epoch_ids`."""
import math

import pytest
import torch

import ray_bank_util as rb
from conftest import load_golden
from nerfmatch_amd.nerf.ray_bank import RayBank, batch_positions, epoch_ids, perm_params

H, W = rb.H, rb.W
maxdiff = lambda a, b: float((a.double() - b.double()).abs().max())


# ----------------------------------------------------------------------------------------------------------------- ray rows
def test_host_rows_match_the_oracle_for_every_pixel():
    bank = rb.bank("cpu")
    rays, rgbs, ts, mask = bank.batch(rb.all_ids())
    ref = rb.oracle_rows()
    err = maxdiff(rays, ref)
    print(f"host path vs oracle, 4 x {H} x {W} pixels: max |diff| = {err:.3e}")
    assert rays.shape == ref.shape == (4 * H * W, 12) and err < rb.RAY_BAR
    assert mask is None and rgbs.shape == (4 * H * W, 3)
    assert torch.equal(rgbs, rb.images().reshape(-1, 3).float().div(255))
    assert torch.equal(ts, torch.tensor([3, 0, 2, 1]).repeat_interleave(H * W))


def test_fourth_frame_is_flagged_and_the_others_are_not_by_rounding():
    bank = rb.bank("cpu")
    assert bank.flags.tolist() == [0, 0, 0, 1]
    rays = bank.batch(rb.all_ids())[0].reshape(4, H * W, 12)
    assert bool((rays[3, :, 7] == 1.0).all()) and bool((rays[:3, :, 7] != 1.0).all())
    assert bool((rays[..., 6] == 0.01).all())
    # the unflagged frames' discriminants in fp64: far from the sign change
    o, v = rb.oracle_rows().double().reshape(4, H * W, 12)[:3, :, 0:3], rb.oracle_rows().double().reshape(4, H * W, 12)[:3, :, 8:11]
    disc = (o * v).sum(-1) ** 2 + (1 - (o * o).sum(-1)) * (v * v).sum(-1)
    print(f"smallest discriminant of the unflagged frames: {float(disc.min()):.3f}")
    assert float(disc.min()) > 0.9


def test_last_row_radius_is_that_of_row_h_minus_3():
    """render_utils.py:94-95: dx = cat([dx, dx[-2:-1]]) gives the last row |d(x, H-3) - d(x, H-2)|, not its own neighbour distance"""
    rays = rb.bank("cpu").batch(rb.all_ids())[0].reshape(4, H, W, 12)
    v = rb.oracle_rows().reshape(4, H, W, 12)[..., 8:11]
    dist = lambda a, b: torch.sqrt(((v[:, a] - v[:, b]) ** 2).sum(-1)) * 2 / math.sqrt(12)
    assert maxdiff(rays[:, H - 1, :, 11], dist(H - 3, H - 2)) < rb.RAY_BAR
    assert maxdiff(rays[:, H - 2, :, 11], dist(H - 2, H - 1)) < rb.RAY_BAR
    # ... and at this focal length that is not the same number as the last row's own neighbour distance
    assert float((dist(H - 3, H - 2) - dist(H - 2, H - 1)).abs().max()) > 1e-4


@pytest.mark.parametrize("norm", [True, False])
def test_host_rows_match_the_reference_fixture(norm):
    z = load_golden("ray_bank")
    bank = RayBank(z["images"], z["c2w"], z["K"], norm_ray_dir=norm, device="cpu")
    rays, rgbs, _, _ = bank.batch(torch.arange(2 * 7 * 9))
    ref = z["rays_norm" if norm else "rays_unnorm"]
    err = maxdiff(rays, ref)
    print(f"host path vs reference rows (norm_ray_dir={norm}): max |diff| = {err:.3e}")
    assert err < rb.RAY_BAR
    assert torch.equal(rgbs, z["rgbs"])
    assert bank.flags.tolist() == z["flags"].tolist()
    if not norm:  # the fixture tells the two direction columns apart
        assert float((ref[:, 3:6] - ref[:, 8:11]).abs().max()) > 1e-2


def test_h_below_3_and_ids_outside_the_table_raise():
    with pytest.raises(ValueError, match="H >= 3"):
        RayBank(torch.zeros(1, 2, 4, 3, dtype=torch.uint8), rb.poses()[:1], rb.intrinsics(), device="cpu")
    bank = rb.bank("cpu")
    for bad in (-1, 4 * H * W):
        with pytest.raises(ValueError, match="outside"):
            bank.batch(torch.tensor([0, bad]))


# ----------------------------------------------------------------------------------------------------------------- permutation
@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 1000, 4097])
def test_an_epoch_visits_every_index_once(N):
    pos = torch.arange(N)
    ids = epoch_ids(N, 0, 0, pos)
    assert ids.dtype == torch.int64 and torch.equal(torch.sort(ids).values, pos)
    if N >= 64:  # another epoch, another seed: another order
        assert not torch.equal(ids, epoch_ids(N, 0, 1, pos)) and not torch.equal(ids, epoch_ids(N, 1, 0, pos))
        assert torch.equal(torch.sort(epoch_ids(N, 7, 3, pos)).values, pos)


def test_large_n_stays_in_range_and_is_repeatable():
    N = (1 << 32) + 12345
    keys, half_bits = perm_params(N, 3, 1)
    assert half_bits == 17 and len(keys) == 4 and all(0 <= k < 1 << 32 for k in keys)
    pos = torch.cat([torch.arange(1000), torch.arange(N - 1000, N)])
    ids = epoch_ids(N, 3, 1, pos)
    assert int(ids.min()) >= 0 and int(ids.max()) < N and int(ids.max()) > 1 << 31
    assert torch.equal(ids, epoch_ids(N, 3, 1, pos)) and len(torch.unique(ids)) == len(ids)
    with pytest.raises(ValueError):
        epoch_ids(N, 3, 1, torch.tensor([N]))


def test_a_positions_index_depends_on_neither_batch_size_nor_world_size():
    N = 1000
    full = epoch_ids(N, 5, 2, torch.arange(N))
    for R, w in ((50, 2), (25, 4), (100, 1), (7, 3)):
        seen = []
        for k in range(N // (R * w)):
            for r in range(w):
                p0, n = batch_positions(k, R, r, w)
                ids = epoch_ids(N, 5, 2, p0 + torch.arange(n))
                assert torch.equal(ids, full[p0 : p0 + n])
                seen.append(p0 + torch.arange(n))
        seen = torch.cat(seen)
        # the ranks' positions partition the epoch (up to the dropped partial batch)
        assert torch.equal(torch.sort(seen).values, torch.arange(N // (R * w) * R * w))


# ----------------------------------------------------------------------------------------------------------------- epochs of a bank
def epoch_of(bank):
    out = list(bank)
    assert len(out) == len(bank)
    return out


def test_training_dictionaries_and_the_dropped_partial_batch():
    bank = rb.id_bank(1, 25, 40, "cpu", batch_rays=64)
    assert len(bank) == 1000 // 64
    batches = epoch_of(bank)
    b = batches[0]
    assert b["rays"].shape == (1, 64, 12) and b["rgbs"].shape == (1, 64, 3) and b["ts"].shape == (1, 64) and b["ts"].dtype == torch.int64
    assert b["img_wh"].tolist() == [[40, 25]] and "mask" not in b
    got = torch.cat([rb.ids_from_rgbs(x["rgbs"][0]) for x in batches])
    assert torch.equal(got, epoch_ids(1000, 0, 0, torch.arange(15 * 64)))
    bank.set_epoch(1)
    assert not torch.equal(rb.ids_from_rgbs(next(iter(bank))["rgbs"][0]), got[:64])


@pytest.mark.parametrize("exclude", [True, False])
def test_masks(exclude):
    m = rb.masks(2, 8, 8)
    bank = RayBank(rb.id_images(2, 8, 8), rb.poses()[:2], rb.intrinsics(), masks_u8=m, exclude_masks=exclude, batch_rays=1, device="cpu")
    keep = 1 - torch.round(m.reshape(-1).float() / 255)
    batches = epoch_of(bank)
    got = torch.cat([rb.ids_from_rgbs(b["rgbs"][0]) for b in batches])
    vals = torch.cat([b["mask"] for b in batches])
    assert vals.shape == (len(got), 1)
    want = torch.nonzero(keep).reshape(-1) if exclude else torch.arange(128)
    assert 0 < len(torch.nonzero(keep)) < 128
    assert torch.equal(torch.sort(got).values, want)  # exactly those pixels, once each
    assert torch.equal(vals[:, 0], keep[got])
    assert torch.equal(bank.batch(torch.arange(128))[3][:, 0], keep)  # explicit ids see every pixel either way


def test_frame_and_pair_dictionaries():
    bank = rb.bank("cpu", unnorm_scene=rb.synth.unnorm_scene(), img_idx=[10, 11, 12, 13])
    one = bank.frame_batch(2, ds=8)
    ref = rb.no.make_rays(H, W, rb.intrinsics(), rb.poses()[2], ds=8)
    assert one["rays"].shape == (1, 12, 12) and maxdiff(one["rays"][0], ref) < rb.RAY_BAR
    assert one["seq_ind"] == [2] and one["img_idx"] == [12] and one["img_wh"].tolist() == [[4, 3]]
    assert torch.equal(one["rgbs"][0], rb.images()[2, 4::8, 4::8].reshape(-1, 3).float().div(255))
    pair = bank.pair_batch(0, 1)
    n = H * W
    assert pair["rays"].shape == (1, 2 * n, 12) and pair["rgbs"].shape == (1, 2 * n, 3) and pair["K"].shape == (1, 6, 3)
    assert pair["c2w"].shape == (1, 8, 4) and pair["unnorm_scene"].shape == (1, 4, 4)
    assert pair["img_idx"] == [10, 11] and pair["seq_ind"] == [3, 0] and pair["img_wh"][0][:2].tolist() == [W, H]
    want = torch.cat([rb.synth.unnorm_scene() @ rb.poses()[0], rb.synth.unnorm_scene() @ rb.poses()[1]])
    assert torch.equal(pair["c2w"][0], want)
    assert maxdiff(pair["rays"][0], rb.oracle_rows()[: 2 * n]) < rb.RAY_BAR
