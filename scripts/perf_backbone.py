#!/usr/bin/env python3
"""What the native ConvFormer backbone (nerfmatch_amd/modules/convformer.py) costs per query batch, and where the time goes.

For every image size in --sizes and batch in --batches (defaults: 480x480 and 480x640, Q = 1 and 16), multi-scale strides:

  backbone_us      HIP-event time of ConvFormerMS.forward, for both GEMM arithmetics (ops.LINEAR_PRECISION fp32 / bf16x3)
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
            for prec in ("fp32", "bf16x3"):
                ops.LINEAR_PRECISION = prec
                item[f"backbone_us_{prec}"] = event_windows(lambda: m(img), a.calls, a.reps)
                item[f"us_per_image_{prec}"] = round(item[f"backbone_us_{prec}"]["median"] / Q, 1)
            item.update(breakdown(m, Q, H, W, dev, a.calls, a.reps))  # (the GEMMs alone: in the arithmetic set last, bf16x3)
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
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
