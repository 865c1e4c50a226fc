"""Outputs of every entry point that inlines csrc/nerf_sample.h, on seeded inputs, for a bit-for-bit comparison of two builds.

  NERFMATCH_AMD_LIB=path/to/parent/libnerfmatch_amd.so python scripts/dump_nerf_sample_outputs.py parent.pt
  python scripts/dump_nerf_sample_outputs.py branch.pt
  python scripts/dump_nerf_sample_outputs.py --compare parent.pt branch.pt      (exit status 1 if any tensor differs)

Entry points and shapes:
  nm_nerf_fwd and the three split forwards (bf16x3, fp16x3, fp16x1): R = 5 rays, S in {32, 64, 128, 256}, tap 3 and tap 7, feat_comb max
    on and off, colour heads on; S in {64, 128, 256} again on resampled fence posts with the zero-tail skip (the leftover pass) and, at
    S = 64, a Cambridge-style network with its appearance row;
  nm_inerf_encode, nm_nerf_points_fwd_rays_bf16x3 / nm_nerf_points_bwd_tap_bf16x3: the cases of test_tapped_points_kernels_vs_gemm_chain;
  nm_inerf_encode_bwd / _bwd2: the shapes of test_encode_backward_vs_fp64_sums;
  nm_inerf_composite / nm_nerf_composite4 and their backwards: the shapes of test_wavefront_compositing_vs_per_ray_loops.
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from nerfmatch_amd import inerf, ops, synth
from nerfmatch_amd.nerf.renderer import NerfRenderer


def renderer(dev, app, S, seed):
    ren = NerfRenderer(synth.nerf_config("cambridge" if app else "7scenes", num_pts=S), num_frames=5 if app else None, training=False, stop_layer=3)
    sd = synth.nerf_state_dict(seed=seed, app_vocab=5 if app else 0, density_bias=3.0)
    ren.load_state_dict(sd)
    ren.to(dev).eval()
    return ren, (sd["embedding_a.weight"][1].contiguous().to(dev) if app else None)


def render_outputs(dev, out):
    R = 5
    all_rays = ops.raygen(synth.intrinsics(), synth.camera_pose(3), 480, 640, dev)[0]
    rays = all_rays[:: all_rays.shape[0] // R][:R].contiguous()
    for app in (False, True):
        ren, row = renderer(dev, app, 64, seed=7)
        for S in ((32, 64, 128, 256) if not app else (64,)):
            t = ops.sample_coarse(rays, synth.uniform01((R, S + 1), 100 + S).to(dev), S)
            w = ops.nerf_fwd(ren.nerf_coarse.packed(dev, "fp32"), rays, t, row, tap_layer=-1, need_feat=False)["weights"]
            t_tail, flag = ops.resample(t, w, synth.resample_jitter((R, S + 1), 200 + S).to(dev), randomized=True, want_tail_flag=True)
            for precision in ("fp32", "bf16x3", "fp16x3", "fp16x1"):
                blob = ren.nerf_fine.packed(dev, precision)
                for tap in (3, 7):
                    for fmax in (False, True):
                        o = ops.nerf_fwd(blob, rays, t, row, tap_layer=tap, feat_max=fmax, white_bg=app)
                        for k, v in o.items():
                            if v is not None:
                                out[f"render/app{int(app)}/S{S}/{precision}/tap{tap}/max{int(fmax)}/{k}"] = v.cpu()
                    if S >= 64:
                        o = ops.nerf_fwd(blob, rays, t_tail, row, tap_layer=tap, zero_tail=True, tail_flag=flag, white_bg=app)
                        for k, v in o.items():
                            if v is not None:
                                out[f"render/app{int(app)}/S{S}/{precision}/tap{tap}/tail/{k}"] = v.cpu()
                if precision == "fp16x3":
                    out[f"render/app{int(app)}/S{S}/fp16x3/saturated"] = torch.tensor(int(blob.nm_guard.read()[0]))


def points_outputs(dev, out):
    S = 128
    for app, R, Sa, tap in ((False, 61, 65, 3), (True, 37, 65, 7), (False, 19, 128, 0), (False, 300, 65, 5)):
        ren, row = renderer(dev, app, S, seed=21 + tap)
        g = torch.Generator().manual_seed(21 + tap)
        o = torch.randn(R, 3, generator=g) * 0.2
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        rays = torch.cat([o, d, torch.full((R, 1), 0.01), torch.ones(R, 1), d, torch.full((R, 1), 0.002)], -1).to(dev).contiguous()
        z = torch.sort(torch.rand(R, S + 1, generator=g) * 0.9 + 0.05, dim=-1).values.to(dev).contiguous()
        key, n = f"points/app{int(app)}_R{R}_Sa{Sa}_tap{tap}", R * Sa
        xi, xd = inerf._encode(rays, z, Sa, row)
        fused = inerf.FusedField(ren.nerf_fine, dev)
        out4, gates, feats = fused.forward_rays(rays, z, Sa, row, tap)
        g4 = (torch.randn(n, 4, generator=g) * 1e-4).to(dev)
        w = (torch.rand(R, Sa, generator=g) * 0.1).to(dev)
        g_pf = (torch.randn(R, 256, generator=g) * 1e-3).to(dev)
        (a0, a5), gxd = fused.backward(g4, gates, (tap, w, g_pf))
        for k, v in dict(xi=xi, xd=xd, out4=out4, gates=gates, feats=feats, g_xi0=a0, g_xi5=a5, g_xd=gxd).items():
            out[f"{key}/{k}"] = v.cpu()


def encode_bwd_outputs(dev, out):
    for R, S, Sa, two in ((37, 40, 33, False), (21, 128, 128, True), (9, 160, 129, True), (5, 64, 64, False)):
        g = torch.Generator().manual_seed(R * 1000 + Sa)
        o = torch.randn(R, 3, generator=g) * 0.2
        v = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        rays = torch.cat([o, v, torch.full((R, 1), 0.05), torch.full((R, 1), 1.5), v, torch.full((R, 1), 2e-3)], 1).to(dev).contiguous()
        z = (0.05 + 1.45 * torch.sort(torch.rand(R, S + 1, generator=g), dim=1).values).to(dev).contiguous()
        n = R * Sa
        ga, gb, gd = (torch.randn(n, c, generator=g).to(dev) for c in (96, 96, 48))
        g_o, g_v = inerf._encode_bwd(rays, z, Sa, (ga, gb) if two else ga, gd)
        out[f"encode_bwd/R{R}_S{S}_Sa{Sa}_two{int(two)}/g_o"], out[f"encode_bwd/R{R}_S{S}_Sa{Sa}_two{int(two)}/g_v"] = g_o.cpu(), g_v.cpu()


def composite_outputs(dev, out):
    for R, S, Sa, with_gw in ((50, 64, 33, False), (37, 128, 65, True), (9, 256, 129, True), (4801, 128, 128, False)):
        g = torch.Generator().manual_seed(R + Sa)
        n = R * Sa
        out4 = torch.randn(n, 4, generator=g)
        out4[:, 3] = out4[:, 3] * 40 + 10
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        rays = torch.cat([torch.zeros(R, 3), d, torch.full((R, 1), 0.05), torch.full((R, 1), 1.5), d, torch.full((R, 1), 2e-3)], 1).to(dev).contiguous()
        z = (0.05 + 1.45 * torch.sort(torch.rand(R, S + 1, generator=g), dim=1).values).to(dev).contiguous()
        G = torch.randn(R, 3, generator=g).to(dev)
        g_w = torch.randn(R, Sa, generator=g).to(dev) if with_gw else None
        out4 = out4.to(dev).contiguous()
        sig = torch.zeros_like(out4)
        sig[:, 0] = out4[:, 3]
        rgb4, _, _, w4 = inerf.composite(out4, z, rays, white_bg=True, S_act=Sa, depth_acc=False)
        g4, gd4 = inerf.composite_bwd(out4, z, rays, G, g_w, white_bg=True, S_act=Sa, want_g_d=True)
        rgb, w = inerf._composite(out4, sig, z, rays, Sa, want_weights=True)
        g_logit, g_sig, gd = inerf._composite_bwd(out4, sig, z, rays, Sa, G, g_w)
        for k, v in dict(rgb4=rgb4, w4=w4, g4=g4, gd4=gd4, rgb=rgb, w=w, g_logit=g_logit, g_sig=g_sig, gd=gd).items():
            out[f"composite/R{R}_S{S}_Sa{Sa}/{k}"] = v.cpu()


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    assert sorted(a) == sorted(b), "the two files hold different tensors"
    bad = [k for k in sorted(a) if a[k][:2] != b[k][:2]]
    numel = lambda shape: int(torch.tensor(shape).prod()) if shape else 1
    for grp in sorted({k.split("/")[0] for k in a}):
        ks = [k for k in a if k.startswith(grp + "/")]
        print(f"{grp}: {len(ks)} tensors, {sum(numel(a[k][1]) for k in ks)} values, {sum(k in bad for k in ks)} tensors differ")
    for k in bad:
        va, vb = a[k][2], b[k][2]
        print(f"DIFFERS {k} {a[k][1]}" + (f": {int((va != vb).sum())} of {va.numel()} values" if va is not None and vb is not None and va.shape == vb.shape else ""))
    print("every tensor bit-equal (digest of the bytes; implies torch.equal): " + ("yes" if not bad else "NO"))
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    out = {}
    render_outputs(dev, out)
    points_outputs(dev, out)
    encode_bwd_outputs(dev, out)
    composite_outputs(dev, out)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in out.values() if v.is_floating_point()), "a non-finite output"
    # a digest of every tensor's bytes (bit equality, stricter than torch.equal: it tells -0 from 0); the values themselves only of
    # the small ones, so that a difference can be counted
    import hashlib
    rec = {k: (hashlib.sha256(v.reshape(-1).contiguous().view(torch.uint8).numpy().tobytes()).hexdigest(), tuple(v.shape), v if v.numel() <= 8192 else None)
           for k, v in out.items()}
    torch.save(rec, sys.argv[1])
    print(f"{len(rec)} tensors -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
