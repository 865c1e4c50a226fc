#!/usr/bin/env python3
"""What the native ConvFormer backbone (nerfmatch_amd/modules/convformer.py) costs per query batch, and where the time goes.

For every image size in --sizes and batch in --batches (defaults: 480x480 and 480x640, Q = 1 and 16), multi-scale strides:

  backbone_us      HIP-event time of ConvFormerMS.forward for the three arithmetics -- ops.LINEAR_PRECISION fp32 / bf16x3 and the opt-in fp16
                   walk (`inference_precision = "fp16"`) -- measured side by side in this process, their windows taken in turn
  fp16             the fp16 walk's launches timed alone like `kernels` below (bytes, bytes/s, share of the copy rate), the GEMMs' share, the
                   walk's overflow events; and at the end, once: the share of a synthetic matcher's mutual matches that stay identical
                   between the bf16x3 and the fp16 backbone (recorded, not judged)
  kernels          each kernel of csrc/convformer.hip alone at the shapes the forward gives it (one chunk of images), with its compulsory
                   bytes (one read of the input, one write of the output), bytes/s and that as a fraction of the 6.29 TB/s float4-copy rate,
                   and `per_forward_us` = time x launches per forward
  gemm_us, layernorm_us   the ops.linear / ops.layernorm calls of one forward, timed alone the same way, and their share of backbone_us
  torch_us         the same architecture through torch's device convolutions (the module's plain-torch path), measured in a CHILD process
                   with a time limit of its own (--torch-timeout seconds; 0 skips it): MIOpen's solver search on a fresh process can be
                   long -- when the child does not finish, the field says so and the rest is reported without it

Kernels timed alone re-read operands that the previous call left in the 256 MiB Infinity Cache whenever they fit (every Q = 1 shape):
that is also what they meet inside the forward, where the producer has just written them.  Times are HIP events over windows of --calls
calls, --reps windows: median / min / max.  No pass / fail: prints one JSON line.

    python scripts/perf_backbone.py [--sizes 480x480,480x640] [--batches 1,16] [--calls 5] [--reps 5] [--torch-timeout 240] [--out FILE]"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nerfmatch_amd import ops, synth  # noqa: E402
from nerfmatch_amd.modules import init_backbone_8_2  # noqa: E402

COPY_BYTES_PER_US = 6.29e6  # float4 copy, MI355X


def spread(vals):
    v = sorted(vals)
    return dict(median=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2))


def event_windows(fn, calls, reps, warmup=2):
    """microseconds per call of fn(): `reps` windows of `calls` calls between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return spread(out)


def interleaved_windows(fns, calls, reps, warmup=2):
    """name -> microseconds per call for several fn() measured side by side: every round times one window of each, in turn, so that clock and
    co-tenant drift falls on all of them alike"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {k: spread(v) for k, v in out.items()}


def breakdown_fp16(m, Q, H, W, dev, calls, reps):
    """Every launch of one fp16 forward (`inference_precision = "fp16"`), timed alone on one chunk of n images: compulsory bytes (one read of
    every operand row, one write of the output; weights not counted), bytes/s, share of the copy rate, and the GEMMs' share of the sum."""
    st = m.model
    h0, w0 = (ops.conv_out_size(v, 7, st.stem_stride, st.stem_pad) for v in (H, W))
    h1, w1 = (ops.conv_out_size(v, 3, st.down_stride, 1) for v in (h0, w0))
    n = min(Q, max(1, st.chunk_bytes // (max(h0 * w0 * 512, h1 * w1 * 1024) * 2)))
    chunks = Q / n
    f16 = torch.float16
    rnd = lambda *s: torch.randn(*s, device=dev)
    one = (torch.ones(1, device=dev), torch.zeros(1, device=dev))
    kern = {}
    img = rnd(n, 3, H, W)
    M0, M1 = n * h0 * w0, n * h1 * w1
    kern["conv_patches_f16_stem"] = kernel_item(lambda: ops.conv_patches_f16(img, 7, st.stem_stride, st.stem_pad, 152), img.numel() * 4 + M0 * 152 * 2,
                                                chunks, calls, reps)
    x0h = rnd(n, h0, w0, 128).to(f16)
    kern["conv_patches_f16_downsample"] = kernel_item(lambda: ops.conv_patches_f16(x0h, 3, st.down_stride, 1, 1152, channel_last=True),
                                                      (x0h.numel() + M1 * 1152) * 2, chunks, calls, reps)
    for name, hh, ww, d in (("fine", h0, w0, 128), ("coarse", h1, w1, 256)):
        xm = rnd(n, hh, ww, d)
        kern[f"nhwc_to_nchw_{name}"] = kernel_item(lambda: ops.nhwc_to_nchw(xm), 2 * xm.numel() * 4, chunks, calls, reps)
    for s, (d, depth, hh, ww, M) in enumerate(((128, 3, h0, w0, M0), (256, 12, h1, w1, M1))):
        u = rnd(n, hh, ww, 2 * d).to(f16)
        wdw = rnd(2 * d, 1, 7, 7)
        kern[f"dwconv7_f16_stage{s}"] = kernel_item(lambda: ops.dwconv7_nhwc_f16(u, wdw, *one), 2 * u.numel() * 2, depth * chunks, calls, reps)
        xr, g, z = rnd(M, d), torch.ones(d, device=dev), torch.zeros(d, device=dev)
        # (stage 0's rows also pass the downsample's norm; the stem's norm makes the fp32 stream)
        kern[f"layernorm_f16_stage{s}"] = kernel_item(lambda: ops.layernorm_f16(xr, g, z, 1e-6), xr.numel() * 6, (2 * depth + (s == 0)) * chunks, calls, reps)
        if s == 0:
            kern["layernorm_stem"] = kernel_item(lambda: ops.layernorm(xr, g, z, 1e-6), xr.numel() * 8, chunks, calls, reps)
        # (N, K, residual, StarReLU): pwconv1, pwconv2, fc1, fc2
        for label, N, K, res, star in (("pwconv1", 2 * d, d, False, False), ("pwconv2", d, 2 * d, True, False), ("fc1", 4 * d, d, False, True),
                                       ("fc2", d, 4 * d, True, False)):
            a, wt = rnd(M, K).to(f16), rnd(N, K) * K ** -0.5
            nbytes = M * K * 2 + (M * N * 8 if res else M * N * 2)  # fp32 residual in + fp32 rows out, or fp16 rows out
            fn = (lambda: ops.linear_f16(a, wt, residual=xr, out_dtype=torch.float32)) if res else \
                 (lambda: ops.linear_f16(a, wt, star=one if star else None))
            kern[f"linear_f16_{label}_stage{s}"] = kernel_item(fn, nbytes, depth * chunks, calls, reps)
            del a, wt
        del u
    for label, M, N, K in (("stem", M0, 128, 152), ("downsample", M1, 256, 1152)):
        a, wt, b = rnd(M, K).to(f16), rnd(N, K) * K ** -0.5, rnd(N)
        kern[f"linear_f16_{label}"] = kernel_item(lambda: ops.linear_f16(a, wt, b, out_dtype=torch.float32), M * K * 2 + M * N * 4, chunks, calls, reps)
    total = sum(k["per_forward_us"] for k in kern.values())
    gemm = sum(k["per_forward_us"] for name, k in kern.items() if name.startswith("linear_f16"))
    return dict(images_per_chunk=n, kernels=kern, kernels_us=round(total, 1), gemm_us=round(gemm, 1), gemm_share_of_kernels=round(gemm / total, 3),
                bytes_per_forward=int(sum(k["bytes"] * k["launches_per_forward"] for k in kern.values())))


def match_agreement(dev, H, W, n_pts=1024, seed=5):
    """Share of the mutual coarse matches of a synthetic c2f matcher that stay identical when its backbone goes from bf16x3 to the fp16 walk
    (same weights, one random image, random point features), and the fp16 walk's overflow events on that image.  Recorded, not asserted."""
    from nerfmatch_amd.matcher import NeRFMatcherMS

    ops.LINEAR_PRECISION = "bf16x3"  # (the matcher's own linears, in both runs)
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(1, 3, H, W, generator=g).to(dev)
    pt_feat, pt3d = torch.relu(torch.randn(1, n_pts, 256, generator=g)).to(dev), (torch.randn(1, n_pts, 3, generator=g) * 2).to(dev)
    ids = {}
    for prec in ("same", "fp16"):
        cfg = synth.matcher_config("c2f", backbone="convformer")
        cfg.backbone_precision = prec
        mm = NeRFMatcherMS(cfg)
        mm.load_state_dict(synth.matcher_state_dict("c2f"), strict=False)
        mm.backbone.load_state_dict(synth.backbone_state_dict(0, "c2f"), strict=True)
        mm = mm.to(dev).eval()
        out = mm.forward_match(img, pt_feat, pt3d, mutual=True, ret_feats=True)
        i_ids, j_ids = out["match_ids"][-2].cpu().tolist(), out["match_ids"][-1].cpu().tolist()
        ids[prec] = dict(zip(i_ids, j_ids))
        events = mm.backbone.model.overflow_events()
    same = sum(1 for i, j in ids["same"].items() if ids["fp16"].get(i) == j)
    return dict(matches_bf16x3=len(ids["same"]), matches_fp16=len(ids["fp16"]), identical=same,
                identical_share=round(same / max(1, len(ids["same"])), 4), fp16_overflow_events=events)


def backbone(dev, seed=0):
    m = init_backbone_8_2("convformer")
    m.load_state_dict(synth.backbone_state_dict(seed, "c2f"), strict=True)
    return m.to(dev).eval()


def kernel_item(fn, nbytes, launches, calls, reps):
    t = event_windows(fn, calls, reps)
    rate = nbytes / t["median"]
    return dict(us=t, bytes=nbytes, bytes_per_us=round(rate), of_copy_rate=round(rate / COPY_BYTES_PER_US, 3), launches_per_forward=launches,
                per_forward_us=round(t["median"] * launches, 1))


def breakdown(m, Q, H, W, dev, calls, reps):
    """Every launch of one forward, timed alone on one chunk of n images and scaled to the forward's chunks."""
    st = m.model
    h0, w0 = (ops.conv_out_size(v, 7, st.stem_stride, st.stem_pad) for v in (H, W))
    h1, w1 = (ops.conv_out_size(v, 3, st.down_stride, 1) for v in (h0, w0))
    n = min(Q, max(1, st.chunk_bytes // (max(h0 * w0 * 512, h1 * w1 * 1024) * 4)))
    chunks = Q / n
    rnd = lambda *s: torch.randn(*s, device=dev)
    one = (torch.ones(1, device=dev), torch.zeros(1, device=dev))
    kern, gemm_us, ln_us = {}, 0.0, 0.0
    img = rnd(n, 3, H, W)
    M0, M1 = n * h0 * w0, n * h1 * w1
    kern["conv_patches_stem"] = kernel_item(lambda: ops.conv_patches(img, 7, st.stem_stride, st.stem_pad, 152), (img.numel() + M0 * 152) * 4,
                                            chunks, calls, reps)
    x0 = rnd(n, h0, w0, 128)
    kern["conv_patches_downsample"] = kernel_item(lambda: ops.conv_patches(x0, 3, st.down_stride, 1, 1152, channel_last=True),
                                                  (x0.numel() + M1 * 1152) * 4, chunks, calls, reps)
    kern["nhwc_to_nchw_fine"] = kernel_item(lambda: ops.nhwc_to_nchw(x0), 2 * x0.numel() * 4, chunks, calls, reps)
    x1 = rnd(n, h1, w1, 256)
    kern["nhwc_to_nchw_coarse"] = kernel_item(lambda: ops.nhwc_to_nchw(x1), 2 * x1.numel() * 4, chunks, calls, reps)
    for s, (d, depth, hh, ww, M) in enumerate(((128, 3, h0, w0, M0), (256, 12, h1, w1, M1))):
        u = rnd(n, hh, ww, 2 * d)
        wdw = rnd(2 * d, 1, 7, 7)
        kern[f"dwconv7_stage{s}"] = kernel_item(lambda: ops.dwconv7_nhwc(u, wdw, *one), 2 * u.numel() * 4, depth * chunks, calls, reps)
        hbuf = rnd(M, 4 * d)
        kern[f"star_relu_stage{s}"] = kernel_item(lambda: ops.star_relu(hbuf, *one, inplace=True), 2 * hbuf.numel() * 4, depth * chunks, calls, reps)
        xr, g, z = rnd(M, d), torch.ones(d, device=dev), torch.zeros(d, device=dev)
        ln_us += event_windows(lambda: ops.layernorm(xr, g, z, 1e-6), calls, reps)["median"] * (2 * depth + 1) * chunks
        for (N, K, res) in ((2 * d, d, False), (d, 2 * d, True), (4 * d, d, False), (d, 4 * d, True)):
            a, wt = rnd(M, K), rnd(N, K) * K ** -0.5
            r = xr if res else None
            gemm_us += event_windows(lambda: ops.linear(a, wt, residual=r), calls, reps)["median"] * depth * chunks
            del a, wt
        del u, hbuf
    for (M, N, K) in ((M0, 128, 152), (M1, 256, 1152)):
        a, wt, b = rnd(M, K), rnd(N, K) * K ** -0.5, rnd(N)
        gemm_us += event_windows(lambda: ops.linear(a, wt, b), calls, reps)["median"] * chunks
    new_us = sum(k["per_forward_us"] for k in kern.values())
    return dict(images_per_chunk=n, kernels=kern, new_kernels_us=round(new_us, 1), gemm_us=round(gemm_us, 1), layernorm_us=round(ln_us, 1))


def torch_child(H, W, Q, calls, reps):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    m = backbone(dev)
    img = torch.randn(Q, 3, H, W, device=dev)
    with torch.no_grad():
        t = event_windows(lambda: m.model._forward_torch(img), calls, reps, warmup=1)
    print(json.dumps(t), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x480,480x640")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-timeout", type=float, default=240.0)
    ap.add_argument("--torch-child", nargs=3, type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_backbone.py needs a GPU: there is no CPU timing to report")
    if a.torch_child:
        return torch_child(*a.torch_child, max(a.calls // 2, 1), min(a.reps, 3))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_grad_enabled(False)
    m = backbone(dev)
    res = dict(copy_bytes_per_us=COPY_BYTES_PER_US, calls_per_window=a.calls, windows=a.reps, chunk_bytes=m.model.chunk_bytes, items=[])
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        for Q in (int(v) for v in a.batches.split(",")):
            item = dict(img_hw=[H, W], Q=Q)
            img = torch.randn(Q, 3, H, W, device=dev)
            def forward(linear, walk):
                ops.LINEAR_PRECISION, m.model.inference_precision = linear, walk
                return m(img)
            # the three arithmetics side by side in this process: windows taken in turn (fp16: the opt-in walk, ops.LINEAR_PRECISION unused)
            walks = dict(fp32=lambda: forward("fp32", "same"), bf16x3=lambda: forward("bf16x3", "same"), fp16=lambda: forward("fp32", "fp16"))
            for prec, t in interleaved_windows(walks, a.calls, a.reps).items():
                item[f"backbone_us_{prec}"] = t
                item[f"us_per_image_{prec}"] = round(t["median"] / Q, 1)
            item["fp16_speedup_over_bf16x3"] = round(item["backbone_us_bf16x3"]["median"] / item["backbone_us_fp16"]["median"], 3)
            item["fp16_overflow_events"] = m.model.overflow_events()
            m.model.inference_precision = "same"
            item["fp16"] = breakdown_fp16(m, Q, H, W, dev, a.calls, a.reps)
            ops.LINEAR_PRECISION = "bf16x3"
            item.update(breakdown(m, Q, H, W, dev, a.calls, a.reps))  # (the GEMMs alone: bf16x3)
            item["gemm_share_bf16x3"] = round(item["gemm_us"] / item["backbone_us_bf16x3"]["median"], 3)
            item["new_kernels_share_bf16x3"] = round(item["new_kernels_us"] / item["backbone_us_bf16x3"]["median"], 3)
            ops.LINEAR_PRECISION = "fp32"
            if a.torch_timeout > 0:
                cmd = [sys.executable, str(Path(__file__).resolve()), "--torch-child", str(H), str(W), str(Q), "--calls", str(a.calls), "--reps", str(a.reps)]
                try:
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.torch_timeout)
                    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
                    item["torch_us"] = json.loads(lines[-1]) if out.returncode == 0 and lines else f"child failed (exit {out.returncode})"
                except subprocess.TimeoutExpired:
                    item["torch_us"] = f"not finished within {a.torch_timeout:.0f} s (solver search of torch's convolution library)"
            res["items"].append(item)
            print(json.dumps(item), file=sys.stderr, flush=True)
    H, W = (int(v) for v in a.sizes.split(",")[0].split("x"))
    res["match_agreement_bf16x3_vs_fp16"] = match_agreement(dev, H, W)
    ops.LINEAR_PRECISION = "fp32"
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
