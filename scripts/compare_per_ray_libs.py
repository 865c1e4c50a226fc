"""Did merging the per-ray kernels change a bit or cost time?  The parent's four wavefront-per-ray compositing entry points and two encode
entry points against the branch's, bit for bit, then the four compositing launches timed with the arms alternating.

  python scripts/compare_per_ray_libs.py PARENT.so BRANCH.so [--rounds 9] [--reps 5] [--warmup 40]

PARENT exports nm_inerf_composite4(_bwd) and nm_nerf_train_composite(_bwd) (signatures kept below: the branch's binding no longer lists
them), BRANCH the one pair nm_nerf_composite4(_bwd); both export nm_inerf_encode and nm_nerf_train_encode.  Both are loaded by path with
ctypes (the loader of scripts/ab_nerf_libs.py); no package library is needed.  Seeded inputs; every output is compared as 32-bit patterns:
  compositing  the cases of test_wavefront_compositing_vs_per_ray_loops and test_composite_forward_backward_vs_fp64, and the workload shapes:
               refinement R = 4800, S = 128, S_act = 65 with g_weights; training R = 9216, S = 128 with noise, both backgrounds, g_weights
  encoding     R = 37, S in {32, 128}, with and without appearance (refinement: also S_act = S / 2 + 1; training: var_scale on, ids with one
               outside the table)
Timing, at the two workload shapes: HIP events around the launch alone, after a warm-up every round runs parent then branch (who goes first
alternates; `reps` launches each, the round's time is their median); per arm median, minimum and spread (max - min) over the rounds.  A
slowdown counts when the branch's median exceeds the parent's by more than the PARENT arm's own spread (the rule of ab_nerf_libs.py).
Exit status 1 on any unequal output.  A script, not a test: it needs the parent's build (git worktree, python -m nerfmatch_amd.build, copy
the .so aside).
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
ENCODE = {
    "nm_inerf_encode": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "nm_nerf_train_encode": (i32, [vp, vp, i32, i32, vp, vp, vp, i32, f32, vp, vp, vp, vp]),
}
PARENT = {
    "nm_inerf_composite4": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "nm_inerf_composite4_bwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "nm_nerf_train_composite": (i32, [vp, vp, vp, vp, f32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "nm_nerf_train_composite_bwd": (i32, [vp, vp, vp, vp, f32, i32, vp, vp, i32, i32, vp, vp]),
}
BRANCH = {
    "nm_nerf_composite4": (i32, [vp, vp, vp, vp, f32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "nm_nerf_composite4_bwd": (i32, [vp, vp, vp, vp, f32, i32, vp, vp, i32, i32, i32, vp, vp, vp]),
}


def load(path, sigs):
    h = C.CDLL(str(Path(path).resolve()))
    fns = {}
    for name, (res, args) in sigs.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
        fns[name] = fn
    return fns


def ptr(t):
    assert t is None or (t.is_cuda and t.is_contiguous())
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def inputs(R, S, Sa, noisy, with_gw, seed, dev):
    """out4 with ~40 % closed density gates, rays with |d| = 1.3, sorted fence posts, upstream gradients"""
    g = torch.Generator().manual_seed(seed)
    out4 = torch.randn(R * Sa, 4, generator=g)
    out4[:, 3] = out4[:, 3] * 40 + 10
    v = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    rays = torch.cat([(torch.rand(R, 3, generator=g) - 0.5) * 0.4, 1.3 * v, torch.full((R, 1), 0.05), torch.full((R, 1), 1.5), v,
                      torch.full((R, 1), 2e-3)], 1)
    t = 0.05 + 1.45 * torch.sort(torch.rand(R, S + 1, generator=g), dim=1).values
    d = dict(out4=out4, rays=rays, t=t, G=torch.randn(R, 3, generator=g), g_w=torch.randn(R, Sa, generator=g) if with_gw else None,
             noise=torch.randn(R, Sa, generator=g) if noisy else None)
    return {k: None if x is None else x.to(dev).contiguous() for k, x in d.items()}


def outputs(R, Sa, dev):
    new = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
    return dict(rgb=new(R, 3), depth=new(R), acc=new(R), w=new(R, Sa), g4=new(R * Sa, 4), g_d=new(R, 3))


def refine_calls(par, br, x, R, S, Sa):
    """(name, parent launch, branch launch, compared outputs) of the refinement's pair: white background, S_act, g_d"""
    fwd_p = lambda o: par["nm_inerf_composite4"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), R, S, Sa, ptr(o["rgb"]), ptr(o["w"]), stream())
    fwd_b = lambda o: br["nm_nerf_composite4"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), None, 0.0, 1, R, S, Sa, ptr(o["rgb"]), None, None,
                                               ptr(o["w"]), stream())
    bwd_p = lambda o: par["nm_inerf_composite4_bwd"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), ptr(x["G"]), ptr(x["g_w"]), R, S, Sa,
                                                     ptr(o["g4"]), ptr(o["g_d"]), stream())
    bwd_b = lambda o: br["nm_nerf_composite4_bwd"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), None, 0.0, 1, ptr(x["G"]), ptr(x["g_w"]), R, S, Sa,
                                                   ptr(o["g4"]), ptr(o["g_d"]), stream())
    return [("refine fwd", fwd_p, fwd_b, ("rgb", "w")), ("refine bwd", bwd_p, bwd_b, ("g4", "g_d"))]


def train_calls(par, br, x, R, S, std, white):
    """the training pair: density noise, either background, depth / acc, S_act = S, no g_d"""
    fwd_p = lambda o: par["nm_nerf_train_composite"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), ptr(x["noise"]), std, white, R, S, ptr(o["rgb"]),
                                                     ptr(o["depth"]), ptr(o["acc"]), ptr(o["w"]), stream())
    fwd_b = lambda o: br["nm_nerf_composite4"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), ptr(x["noise"]), std, white, R, S, S, ptr(o["rgb"]),
                                               ptr(o["depth"]), ptr(o["acc"]), ptr(o["w"]), stream())
    bwd_p = lambda o: par["nm_nerf_train_composite_bwd"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), ptr(x["noise"]), std, white, ptr(x["G"]),
                                                         ptr(x["g_w"]), R, S, ptr(o["g4"]), stream())
    bwd_b = lambda o: br["nm_nerf_composite4_bwd"](ptr(x["out4"]), ptr(x["t"]), ptr(x["rays"]), ptr(x["noise"]), std, white, ptr(x["G"]),
                                                   ptr(x["g_w"]), R, S, S, ptr(o["g4"]), None, stream())
    return [("train fwd", fwd_p, fwd_b, ("rgb", "depth", "acc", "w")), ("train bwd", bwd_p, bwd_b, ("g4",))]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=40, help="launches per arm and launch before the rounds (clocks settle)")
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds"
    par, br = load(a.parent, {**PARENT, **ENCODE}), load(a.branch, {**BRANCH, **ENCODE})
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    bad = []

    def compare(label, calls, R, Sa):
        for name, fp, fb, keys in calls:
            op, ob = outputs(R, Sa, dev), outputs(R, Sa, dev)
            assert fp(op) == 0 and fb(ob) == 0, (label, name)
            torch.cuda.synchronize()
            for k in keys:
                eq = same_bits(op[k], ob[k]) and not bool(torch.isnan(ob[k]).any())
                print(f"{'equal  ' if eq else 'DIFFERS'} {label:58s} {name:10s} {k}")
                if not eq:
                    bad.append((label, name, k))

    # ---- compositing: the two tests' cases, then the workload shapes
    for R, S, Sa, gw in [(50, 64, 33, False), (37, 128, 65, True), (9, 256, 129, True), (4801, 128, 128, False), (4800, 128, 65, True)]:
        x = inputs(R, S, Sa, False, gw, R + Sa, dev)
        compare(f"R={R} S={S} S_act={Sa} g_w={int(gw)}", refine_calls(par, br, x, R, S, Sa), R, Sa)
    train = [(37, 32, 0, 0, 0), (37, 32, 1, 1, 1), (37, 64, 1, 0, 1), (37, 64, 0, 1, 0), (37, 128, 1, 1, 0), (37, 128, 0, 0, 1), (9216, 128, 1, 1, 1),
             (9216, 128, 0, 1, 1)]
    for R, S, white, noisy, gw in train:
        x = inputs(R, S, S, bool(noisy), bool(gw), R + S + 2 * white + noisy, dev)
        compare(f"R={R} S={S} white={white} noise={noisy} g_w={gw}", train_calls(par, br, x, R, S, 1.0 if noisy else 0.0, white), R, S)

    # ---- encoding
    R = 37
    g = torch.Generator().manual_seed(7)
    table = torch.randn(5, 16, generator=g).to(dev)
    ids = torch.randint(0, 5, (R,), generator=g)
    ids[3] = 9  # (outside the table: clamped and counted)
    ids = ids.to(dev)
    for S in (32, 128):
        x = inputs(R, S, S, False, False, S, dev)
        for app in (False, True):
            for Sa in (S, S // 2 + 1):
                res = []
                for lib in (par, br):
                    xi, xd = torch.full((R * Sa, 96), float("nan"), device=dev), torch.full((R * Sa, 48), float("nan"), device=dev)
                    assert lib["nm_inerf_encode"](ptr(x["rays"]), ptr(x["t"]), R, S, Sa, ptr(table[1].contiguous()) if app else None, ptr(xi), ptr(xd),
                                                  stream()) == 0
                    res.append((xi, xd))
                torch.cuda.synchronize()
                for k, pa, pb in zip(("xi", "xd"), *res):
                    eq = same_bits(pa, pb) and not bool(torch.isnan(pb).any())
                    print(f"{'equal  ' if eq else 'DIFFERS'} {f'R={R} S={S} S_act={Sa} app={int(app)}':58s} {'inerf enc':10s} {k}")
                    if not eq:
                        bad.append((S, Sa, app, "nm_inerf_encode", k))
            res = []
            for lib in (par, br):
                xi, xd = torch.full((R * S, 96), float("nan"), device=dev), torch.full((R * S, 48), float("nan"), device=dev)
                status = torch.zeros(1, dtype=torch.int32, device=dev)
                assert lib["nm_nerf_train_encode"](ptr(x["rays"]), ptr(x["t"]), R, S, ptr(ids) if app else None, None, ptr(table) if app else None,
                                                   5 if app else 0, 0.5, ptr(xi), ptr(xd), ptr(status), stream()) == 0
                res.append((xi, xd, status.float()))
            torch.cuda.synchronize()
            for k, pa, pb in zip(("xi", "xd", "status"), *res):
                eq = same_bits(pa, pb) and not bool(torch.isnan(pb).any())
                print(f"{'equal  ' if eq else 'DIFFERS'} {f'R={R} S={S} app={int(app)} var_scale=0.5':58s} {'train enc':10s} {k}")
                if not eq:
                    bad.append((S, app, "nm_nerf_train_encode", k))

    # ---- timing at the workload shapes
    def once(fn, o):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        code = fn(o)
        e1.record()
        assert code == 0, code
        e1.synchronize()
        return e0.elapsed_time(e1)

    print(f"\n{a.rounds} rounds x {a.reps} launches per arm, arms alternate within a round; us per launch")
    xr, xt = inputs(4800, 128, 65, False, True, 1, dev), inputs(9216, 128, 128, True, True, 2, dev)
    timed = [(c, outputs(4800, 65, dev)) for c in refine_calls(par, br, xr, 4800, 128, 65)]
    timed += [(c, outputs(9216, 128, dev)) for c in train_calls(par, br, xt, 9216, 128, 1.0, 1)]
    slower = []
    for (name, fp, fb, _), o in timed:
        arms = [("parent", fp), ("branch", fb)]
        for _, fn in arms:
            for _ in range(a.warmup):
                once(fn, o)
        times = {"parent": [], "branch": []}
        for rnd in range(a.rounds):
            for arm, fn in (arms if rnd % 2 == 0 else arms[::-1]):
                times[arm].append(1e3 * statistics.median(once(fn, o) for _ in range(a.reps)))
        med = {arm: statistics.median(v) for arm, v in times.items()}
        for arm, v in times.items():
            print(f"{name:10s} {arm:6s} median {med[arm]:7.2f}  min {min(v):7.2f}  spread {max(v) - min(v):6.2f}   rounds " + " ".join(f"{t:.1f}" for t in v))
        d, spread = med["branch"] - med["parent"], max(times["parent"]) - min(times["parent"])
        verdict = "SLOWER beyond it" if d > spread else "within it" if abs(d) <= spread else "faster beyond it"
        print(f"{name:10s} branch - parent: {d:+.2f} us ({100 * d / med['parent']:+.2f} %), parent's spread {spread:.2f}: {verdict}")
        if d > spread:
            slower.append(name)
    print(f"\n{'every output equal bit for bit' if not bad else f'{len(bad)} outputs DIFFER: {bad}'}; "
          f"{'no launch slower beyond the parent arm own spread' if not slower else f'SLOWER: {slower}'}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
