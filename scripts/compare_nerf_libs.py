"""Are two builds of the library the same arithmetic?  Every output of the split NeRF kernels from both, bit for bit.

  python scripts/compare_nerf_libs.py path/to/libA.so path/to/libB.so

A change of instruction PLACEMENT inside a K-step (csrc/nerf_split_chain.h) cannot change a bit, so anything but equality everywhere is a
bug.  Both builds are loaded by path with ctypes (the loader of scripts/ab_nerf_libs.py) next to the package's own library, which only
makes the inputs and packs the blobs: the blob layout must be the same in all three.  Seeded inputs, `synth` weights.
  nm_nerf_fwd_{fp16x3,bf16x3}: the four pass types of tests/test_nerf_ring_schedule_gpu.py and a tap on each of layers 0..6 with and
    without colour heads x with / without appearance row (Cambridge
    network) x S in {32, 64, 128, 256} x R giving 1, 5 and 2.5 x CU-count tiles of 128 samples, the last one ragged where a tile holds
    several rays
  nm_nerf_points_fwd_rays_bf16x3 / nm_nerf_points_bwd_tap_bf16x3: one, five and 2.5 x CU-count tiles
Prints one line per case and output, and a summary; exit status 1 unless everything is equal.  A script, not a test: it needs the parent's
build (git stash / git worktree, python -m nerfmatch_amd.build, copy the .so aside).
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from nerfmatch_amd import _lib, inerf, ops, synth
from nerfmatch_amd._lib import dptr
from nerfmatch_amd.nerf.renderer import NerfRenderer

PASSES = {  # tests/test_nerf_ring_schedule_gpu.py
    "rgb_tap7": dict(tap_layer=7, need_rgb=True, need_feat=True),
    "rgb_tap3": dict(tap_layer=3, need_rgb=True, need_feat=True),
    "norgb_tap3": dict(tap_layer=3, need_rgb=False, need_feat=True),
    "norgb_nofeat": dict(tap_layer=-1, need_rgb=False, need_feat=False),
}
for _tap in (0, 1, 2, 4, 5, 6):  # every other tap layer that goes through the workspace, with and without colour heads
    PASSES[f"rgb_tap{_tap}"] = dict(tap_layer=_tap, need_rgb=True, need_feat=True)
    PASSES[f"norgb_tap{_tap}"] = dict(tap_layer=_tap, need_rgb=False, need_feat=True)
ENTRIES = ("nm_nerf_fwd_fp16x3", "nm_nerf_fwd_bf16x3", "nm_nerf_points_fwd_rays_bf16x3", "nm_nerf_points_bwd_tap_bf16x3", "nm_nerf_points_gate_bytes")


def load(path):
    h = C.CDLL(str(Path(path).resolve()))
    fns = {}
    for e in ENTRIES:
        fn = getattr(h, e)
        fn.restype, fn.argtypes = _lib.SIGNATURES[e]
        fns[e] = fn
    return fns


def rays_for(tiles, S, dev):
    """rays that fill `tiles` tiles of 128 samples; where a tile holds several rays the count is made odd against it (ragged last tile)"""
    R = max(1, -(-tiles * 128 // S))
    nr = max(1, 128 // S)
    if nr > 1 and tiles > 1 and R % nr == 0:
        R += 1
    rays = torch.cat([ops.raygen(synth.intrinsics(), synth.camera_pose(q), 480, 640, dev)[0] for q in range(-(-R // 4800))])[:R].contiguous()
    return rays


def render(fn, precision, blob, rays, t, row, name, ws):
    R, S = t.shape[0], t.shape[1] - 1
    dev = rays.device
    p = PASSES[name]
    new = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
    out = dict(weights=new(R, S), pts=new(R, 3), depth=new(R), acc=new(R))
    out["feat"] = new(R, 256) if p["need_feat"] else None
    out["rgb"] = new(R, 3) if p["need_rgb"] else None
    flags = 0 if p["need_rgb"] else _lib.NM_NERF_SKIP_RGB
    status = (dptr(blob.nm_guard.status, torch.int32),) if precision == "fp16x3" else ()
    code = fn(dptr(blob, blob.dtype), dptr(rays), dptr(t), dptr(row), R, S, p["tap_layer"], 0, -1.0, flags, dptr(out["weights"]), dptr(out["feat"]),
              dptr(out["pts"]), dptr(out["rgb"]), dptr(out["depth"]), dptr(out["acc"]), None, None, dptr(ws if p["need_feat"] else None, torch.uint8),
              None, *status, _lib.stream())
    assert code == 0, code
    torch.cuda.synchronize()
    return {k: v for k, v in out.items() if v is not None}


def points_pair(fns, fused_blobs, rays, z, Sa, row, tap, grads):
    blob, blob_bwd = fused_blobs
    R, S, dev = z.shape[0], z.shape[1] - 1, rays.device
    n = R * Sa
    out4 = torch.full((n, 4), float("nan"), device=dev)
    gates = torch.zeros(fns["nm_nerf_points_gate_bytes"](n), dtype=torch.uint8, device=dev)
    feats = torch.full((n, 256), float("nan"), device=dev)
    code = fns["nm_nerf_points_fwd_rays_bf16x3"](dptr(blob, torch.uint8), dptr(rays), dptr(z), R, S, Sa, dptr(row), tap, dptr(out4), dptr(gates, torch.uint8),
                                               dptr(feats), _lib.stream())
    assert code == 0, code
    g4, w, g_pf = grads
    g0, g5 = torch.full((n, inerf.XI), float("nan"), device=dev), torch.full((n, inerf.XI), float("nan"), device=dev)  # (the shapes FusedField.backward allocates)
    gxd = torch.full((n, inerf.XD), float("nan"), device=dev)
    code = fns["nm_nerf_points_bwd_tap_bf16x3"](dptr(blob_bwd, torch.uint8), dptr(g4), dptr(gates, torch.uint8), R, Sa, tap, dptr(w), dptr(g_pf), dptr(g0),
                                              dptr(g5), dptr(gxd), _lib.stream())
    assert code == 0, code
    torch.cuda.synchronize()
    return dict(out4=out4, gates=gates, feats=feats, g_xi0=g0, g_xi5=g5, g_xd=gxd)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.uint8).reshape(-1), b.view(torch.uint8).reshape(-1))  # (bits: a NaN equals itself)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    a = ap.parse_args()
    A, B = load(a.lib_a), load(a.lib_b)
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ren = NerfRenderer(synth.nerf_config("cambridge", num_pts=64), num_frames=5, training=False, stop_layer=3)
    sd = synth.nerf_state_dict(seed=7, app_vocab=5, density_bias=3.0)
    ren.load_state_dict(sd, strict=True)
    ren.to(dev).eval()
    ren.calibrate(dev)
    row = sd["embedding_a.weight"][1].contiguous().to(dev)
    ws = ops._nerf_workspace(dev)
    n_cases = n_bad = 0
    for precision in ("fp16x3", "bf16x3"):
        blob = ren.nerf_fine.packed(dev, precision)
        for S in (32, 64, 128, 256):
            for tiles in (1, 5, int(2.5 * cus)):
                rays = rays_for(tiles, S, dev)
                R = rays.shape[0]
                t = ops.sample_coarse(rays, synth.uniform01((R, S + 1), 100 + S).to(dev), S)
                for app in (True, False):
                    for name in PASSES:
                        oa = render(A["nm_nerf_fwd_" + precision], precision, blob, rays, t, row if app else None, name, ws)
                        ob = render(B["nm_nerf_fwd_" + precision], precision, blob, rays, t, row if app else None, name, ws)
                        verdict = {k: same(oa[k], ob[k]) for k in oa}
                        finite = all(torch.isfinite(v).all().item() for v in oa.values())
                        n_cases += 1
                        n_bad += not all(verdict.values())
                        print(f"{precision} S {S:3d} R {R:5d} ({-(-R * S // 128)} tiles) {'row   ' if app else 'no row'} {name:12s} "
                              + " ".join(f"{k}:{'equal' if v else 'DIFFERENT'}" for k, v in verdict.items()) + ("" if finite else "  (non-finite values in A)"))
        if precision == "fp16x3":
            assert not blob.nm_guard.read()[0], "an fp16x3 operand saturated"
    # the pointwise pair of the iNeRF refinement
    fused = (ren.nerf_fine.packed(dev, "bf16x3"), ren.nerf_fine.packed(dev, "bwd_bf16x3"))
    Sa, S, tap = 65, 128, 3
    for tiles in (1, 5, int(2.5 * cus)):
        R = max(1, tiles * 128 // Sa)
        g = torch.Generator().manual_seed(5 + tiles)
        o = torch.randn(R, 3, generator=g) * 0.2
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        rays = torch.cat([o, d, torch.full((R, 1), 0.01), torch.ones(R, 1), d, torch.full((R, 1), 0.002)], -1).to(dev).contiguous()
        z = torch.sort(torch.rand(R, S + 1, generator=g) * 0.9 + 0.05, dim=-1).values.to(dev).contiguous()
        n = R * Sa
        g4 = (torch.randn(n, 4, generator=g) * 1e-4).to(dev).contiguous()
        w = (torch.rand(R, Sa, generator=g) * 0.1).to(dev).contiguous()
        g_pf = (torch.randn(R, 256, generator=g) * 1e-3).to(dev).contiguous()
        for app in (True, False):
            oa = points_pair(A, fused, rays, z, Sa, row if app else None, tap, (g4, w, g_pf))
            ob = points_pair(B, fused, rays, z, Sa, row if app else None, tap, (g4, w, g_pf))
            verdict = {k: same(oa[k], ob[k]) for k in oa}
            n_cases += 1
            n_bad += not all(verdict.values())
            print(f"points pair R {R:5d} x {Sa} ({-(-n // 128)} tiles) {'row   ' if app else 'no row'} " + " ".join(f"{k}:{'equal' if v else 'DIFFERENT'}" for k, v in verdict.items()))
    print(f"{n_cases} cases, {n_bad} with a difference: " + ("the two libraries agree bit for bit everywhere" if n_bad == 0 else "NOT the same arithmetic"))
    sys.exit(1 if n_bad else 0)


if __name__ == "__main__":
    main()
