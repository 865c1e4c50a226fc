"""The split render kernels request their weight slots from running state (csrc/nerf_split_chain.h, ring_arm / ring_request): a 64-bit
source pointer that advances by two slots per request and a ring position that steps and wraps, both reset where a tile's stream starts
over (per chunk, per tile, leftover pass), with M0 set once per slot.  A wrong pointer or position reads another layer's weights or lands
them in the wrong ring slot, in every tile or only in a workgroup's later ones.  This file holds fp16x3 and bf16x3 to the fp32-MFMA kernel
on the same inputs where the stream has another length or starts over at another place -- colour heads on / off (it ends behind the views
layer or behind layer 7), appearance row present / absent (one slot more), a tap on layer 3, on layer 7 and none, every row length at which
a tile takes another form (32, 64, 128; 256: two chunks, the stream starts over inside a tile; 96: padded), 1 tile, CU count + 3 tiles (a
ragged second round) and 2.5 x CU count (a workgroup's third tile), zero_tail with its leftover pass -- and checks bit for bit that a
bundle's outputs do not depend on how many tiles its workgroups ran before.

The 1e-4-of-scale bar, networks and launches: tests/nerf_kernel_util.py (the networks of tests/test_nerf_gap_work_gpu.py)."""
import functools

import pytest
import torch

from nerf_kernel_util import KEYS, compare, fence_posts, launch, oracle_rays, styled_network, tol_for
from nerfmatch_amd import ops, synth

pytestmark = pytest.mark.gpu
ROWS = (32, 64, 128, 256, 96)
# (colour heads, appearance row, tap layer or None)
CONFIGS = ((True, True, 3), (True, False, 7), (True, False, None), (False, False, 3), (False, False, 7), (False, False, None))


@functools.lru_cache(maxsize=None)
def _bundle(S, R, first=0):
    rays = oracle_rays(256, 256, 200.0, 3, 2)[first:first + R].contiguous()  # (of 16384 rays)
    assert rays.shape[0] == R
    return rays, fence_posts(rays, S, 100 + S + 7 * first)


def _rays_for(S, tiles):
    """ray count that makes `tiles` tiles of 128 samples at row length S, the last one ragged where a tile holds several rays"""
    per_tile = max(1, 128 // S)
    return tiles * per_tile - (1 if per_tile > 1 and tiles > 1 else 0)


def _tile_counts():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(one=1, second_round=cus + 3, third_tile=(5 * cus) // 2)


def _launch(precision, app, rays, t, tap, rgb, **kw):
    ren, _, row = styled_network(None, app)
    return launch(ren, "coarse", precision, rays, t, row, tap_layer=-1 if tap is None else tap, need_rgb=rgb, need_feat=tap is not None, **kw)


@functools.lru_cache(maxsize=None)
def _fp32(app, S, R, tap, rgb):
    rays, t = _bundle(S, R)
    return _launch("fp32", app, rays, t, tap, rgb)


def _keys(rgb, tap):
    return tuple(k for k in KEYS if (rgb or k != "rgb") and (tap is not None or k != "feat"))


@pytest.mark.parametrize("tiles", ["one", "second_round", "third_tile"])
@pytest.mark.parametrize("S", ROWS)
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_stream_lengths_and_restarts_vs_fp32_kernel(gpu, built_lib, precision, S, tiles):
    R = _rays_for(S, _tile_counts()[tiles])
    rays, t = _bundle(S, R)
    tol = tol_for(precision, "default")
    for rgb, app, tap in CONFIGS:
        out = _launch(precision, app, rays, t, tap, rgb)
        ref = _fp32(app, S, R, tap, rgb)
        assert out["weights"].shape == (R, S) and (out["rgb"] is None) == (not rgb) and (out["feat"] is None) == (tap is None)
        assert float(ref["weights"].sum(-1).max()) > 0.3  # not vacuous
        compare(out, ref, tol, False, f"{precision} S {S} R {R} rgb {rgb} app {app} tap {tap} vs fp32 kernel", _keys(rgb, tap))


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_leftover_pass_vs_fp32_kernel(gpu, built_lib, precision, S):
    """zero_tail on a fine-style row over 2.5 x CU count tiles: every workgroup runs two or three regular tiles of S/2 samples per ray and
    then the leftover pass over the samples it queued, whose stream starts over like a tile's"""
    R = _rays_for(S // 2, _tile_counts()["third_tile"])
    rays, t_c = _bundle(S, R)
    w_c = _launch(precision, False, rays, t_c, None, False)["weights"]
    t_f, flag = ops.resample(t_c.to(w_c.device), w_c, synth.resample_jitter((R, S + 1), 200 + S).to(w_c.device), want_tail_flag=True)
    assert int(flag.item()) == 0  # the premise holds: the zero-tail path is taken
    out = _launch(precision, False, rays, t_f, 3, True, zero_tail=True, tail_flag=flag)
    ref = _launch("fp32", False, rays, t_f, 3, True, zero_tail=True, tail_flag=flag)
    assert float(ref["weights"].sum(-1).max()) > 0.3
    assert float(out["weights"][:, S // 2 + 1:].abs().max()) == 0.0
    compare(out, ref, tol_for(precision, "default"), False, f"{precision} zero tail S {S} R {R} vs fp32 kernel")


@pytest.mark.parametrize("rgb", [True, False])
@pytest.mark.parametrize("S", [64, 256])
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_outputs_do_not_depend_on_the_tiles_in_front(gpu, built_lib, precision, S, rgb):
    """A bundle rendered alone (its tiles are every workgroup's first) and behind a prefix of 128 k other rays -- whole tiles, so the
    bundle's own tiles hold the same rays, but run as workgroups' third tiles: the same bits in every output.  (No zero_tail: its leftover
    adds are atomics.  Precedent: test_batch_order_and_sharding_do_not_change_a_single_bit.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_tile = max(1, 128 // S)
    k = -(-2 * cus // (128 // per_tile))  # prefix of 128 k rays >= 2 x CU count tiles
    prefix, R = 128 * k, 5 * per_tile - (1 if per_tile > 1 else 0)
    rays, t = _bundle(S, prefix + R)
    own_rays, own_t = rays[prefix:].contiguous(), t[prefix:].contiguous()
    alone = _launch(precision, False, own_rays, own_t, 3, rgb, want_raw=True)
    behind = _launch(precision, False, rays, t, 3, rgb, want_raw=True)
    assert float(alone["weights"].sum(-1).max()) > 0.3
    for key in _keys(rgb, 3) + ("raw",):
        assert torch.equal(alone[key], behind[key][prefix:]), f"{precision} S {S} rgb {rgb}: {key} differs behind {prefix} rays"
