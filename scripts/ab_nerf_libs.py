"""A/B of two builds of the library on the two launches of a render step, in ONE process with the arms alternating.

  python scripts/ab_nerf_libs.py NAME_A=path/to/libA.so NAME_B=path/to/libB.so [--rounds 9] [--reps 5] [--warmup 40] [--precision fp16x3]

Both builds are loaded by path with ctypes next to the package's own library (which only makes the inputs and packs the blobs: the blob
layout must be the same in all three).  Timed, HIP events around each launch of the split kernel alone (no guard pass, no allocation):
  coarse: colour heads + tap 7 (nerf_coarse, stratified samples)         16 x 4800 x 64
  fine:   colour heads + tap 3 (nerf_fine, samples resampled from the coarse weights)
Seeded random inputs, `synth` weights.  After a warm-up every round runs arm A then arm B (`reps` launches each, the round's time is their
median); per arm and launch type: median, minimum and spread (max - min) over the rounds.  A difference counts when the medians differ by
more than the FIRST arm's own spread (name the parent build first).
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from nerfmatch_amd import _lib, ops, synth
from nerfmatch_amd._lib import dptr
from nerfmatch_amd.nerf.renderer import NerfRenderer

ENTRY = {"fp16x3": "nm_nerf_fwd_fp16x3", "bf16x3": "nm_nerf_fwd_bf16x3", "fp16x1": "nm_nerf_fwd_fp16x1"}


def load(path, entry):
    h = C.CDLL(str(Path(path).resolve()))
    fn = getattr(h, entry)
    fn.restype, fn.argtypes = _lib.SIGNATURES[entry]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("arms", nargs=2, metavar="NAME=LIB")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=40, help="launches per arm and launch type before the rounds (clocks settle)")
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--precision", default="fp16x3", choices=sorted(ENTRY))
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds"
    entry = ENTRY[a.precision]
    arms = [(s.split("=", 1)[0], load(s.split("=", 1)[1], entry)) for s in a.arms]

    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    S = a.samples
    ren = NerfRenderer(synth.nerf_config("7scenes", num_pts=S), training=False, stop_layer=3)
    ren.load_state_dict(synth.nerf_state_dict(seed=0, density_bias=3.0))
    ren.to(dev).eval()
    rays = torch.cat([ops.raygen(synth.intrinsics(), synth.camera_pose(q), 480, 640, dev)[0] for q in range(a.queries)])
    R = rays.shape[0]
    t_c = ops.sample_coarse(rays, torch.rand(R, S + 1, device=dev), S)
    blob_c, blob_f = ren.nerf_coarse.packed(dev, a.precision), ren.nerf_fine.packed(dev, a.precision)
    w_c = ops.nerf_fwd(blob_c, rays, t_c, tap_layer=-1)["weights"]
    t_f = ops.resample(t_c, w_c, torch.rand(R, S + 1, device=dev))
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    out = dict(weights=new(R, S), feat=new(R, 256), pts=new(R, 3), rgb=new(R, 3), depth=new(R), acc=new(R))
    ws = ops._nerf_workspace(dev)
    status = (dptr(blob_c.nm_guard.status, torch.int32),) if a.precision == "fp16x3" else ()  # (only an fp16x3 blob carries a guard)

    def args(blob, t, tap):
        return (dptr(blob, blob.dtype), dptr(rays), dptr(t), None, R, S, tap, 0, -1.0, 0, dptr(out["weights"]), dptr(out["feat"]), dptr(out["pts"]),
                dptr(out["rgb"]), dptr(out["depth"]), dptr(out["acc"]), None, None, dptr(ws, torch.uint8), None, *status, _lib.stream())

    launches = {"coarse": args(blob_c, t_c, 7), "fine": args(blob_f, t_f, 3)}

    def once(fn, av):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        code = fn(*av)
        e1.record()
        assert code == 0, code
        e1.synchronize()
        return e0.elapsed_time(e1)

    print(f"{R} rays x {S} samples, {a.precision}; {a.rounds} rounds x {a.reps} launches per arm, arms alternate within a round; ms per launch")
    sums = {}
    for kind, av in launches.items():
        for _, fn in arms:
            for _ in range(a.warmup):
                once(fn, av)
        times = {name: [] for name, _ in arms}
        for rnd in range(a.rounds):
            for name, fn in (arms if rnd % 2 == 0 else arms[::-1]):  # (who goes first alternates too)
                times[name].append(statistics.median(once(fn, av) for _ in range(a.reps)))
        for name, _ in arms:
            v = times[name]
            sums[(kind, name)] = (statistics.median(v), min(v), max(v) - min(v))
            print(f"{kind:6s} {name:12s} median {sums[(kind, name)][0]:8.4f}  min {sums[(kind, name)][1]:8.4f}  spread {sums[(kind, name)][2]:7.4f}   rounds "
                  + " ".join(f"{x:.3f}" for x in v))
        (na, _), (nb, _) = arms
        d = sums[(kind, nb)][0] - sums[(kind, na)][0]
        print(f"{kind:6s} {nb} - {na}: {d:+.4f} ms ({100 * d / sums[(kind, na)][0]:+.2f} %), {na}'s spread {sums[(kind, na)][2]:.4f}: "
              + ("beyond it" if abs(d) > sums[(kind, na)][2] else "within it"))
    if a.precision == "fp16x3":
        assert not blob_c.nm_guard.read()[0], "an fp16x3 operand saturated"


if __name__ == "__main__":
    main()
