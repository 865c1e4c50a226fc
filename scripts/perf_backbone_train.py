#!/usr/bin/env python3
"""What a training step of the ConvFormer backbone alone costs: forward + backward of ConvFormerMS against fixed cotangents on the two
returned maps, on the recording path of the HIP kernels (ConvFormerStages.train_native, the default) and on the plain-torch path
(train_native = False: torch's device convolutions, what the backbone trained on before the backward kernels existed), in ONE process on
the same GPU.

For every batch in --batches of --size images, under both GEMM arithmetics (ops.LINEAR_PRECISION fp32 / bf16x3; the torch path has no
such switch and is measured once):

  native_us, torch_us     HIP-event time of zero_grad + forward + backward; median / min / max over --reps windows of --calls steps
  *_peak_bytes            torch.cuda.max_memory_allocated over one step, minus what was allocated before it
  kernels                 every kernel of csrc/convformer.hip and csrc/convformer_bwd.hip alone at the shapes the step gives it, times its
                          launches per step, and the share of native_us (bf16x3) that they sum to; the rest is the GEMM and LayerNorm
                          forward / backward kernels and autograd's own adds
  bounds                  the two depthwise backward kernels against their byte bound (compulsory traffic at the 6.29 TB/s float4-copy
                          rate) and their FMA bound (49 per element at 39.3 T unpacked fp32 FMAs/s)

All native cells are measured first and written to --out as they finish; the torch cells follow (their first step pays the solver search
of torch's convolution library, outside the timed windows).  No pass / fail: prints one JSON line.

    python scripts/perf_backbone_train.py [--size 480x480] [--batches 2,8] [--calls 2] [--reps 5] [--out FILE] [--no-torch]"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nerfmatch_amd import autograd as ag, ops, synth  # noqa: E402
from nerfmatch_amd.modules import init_backbone_8_2  # noqa: E402

COPY_BYTES_PER_US = 6.29e6  # float4 copy, MI355X
FMA_PER_US = 39.3e6         # unpacked fp32 FMAs


def spread(vals):
    v = sorted(vals)
    return dict(median=round(v[len(v) // 2], 1), min=round(v[0], 1), max=round(v[-1], 1))


def event_windows(fn, calls, reps, warmup=1):
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


def make_step(m, img, cots):
    def step():
        m.zero_grad(set_to_none=True)
        with torch.enable_grad(), ag.training():
            torch.autograd.backward(m(img), cots)
    return step


def measure(m, img, cots, calls, reps):
    step = make_step(m, img, cots)
    step()  # (allocator warm, derived weight copies made, solver search done)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return event_windows(step, calls, reps, warmup=0), peak


def kernels_alone(st, B, H, W, dev, calls, reps):
    h0, w0 = (ops.conv_out_size(v, 7, st.stem_stride, st.stem_pad) for v in (H, W))
    h1, w1 = (ops.conv_out_size(v, 3, st.down_stride, 1) for v in (h0, w0))
    rnd = lambda *s: torch.randn(*s, device=dev)
    one = (torch.ones(1, device=dev), torch.zeros(1, device=dev))
    t = lambda fn: event_windows(fn, calls, reps)["median"]
    kern, bounds = {}, {}
    img, x0, x1 = rnd(B, 3, H, W), rnd(B, h0, w0, 128), rnd(B, h1, w1, 256)
    drows = rnd(B * h1 * w1, 1152)
    kern["conv_patches (stem + downsample)"] = t(lambda: ops.conv_patches(img, 7, st.stem_stride, st.stem_pad, 152)) + \
        t(lambda: ops.conv_patches(x0, 3, st.down_stride, 1, 1152, channel_last=True))
    kern["conv_patches_bwd"] = t(lambda: ops.conv_patches_bwd(drows, tuple(x0.shape), 3, st.down_stride, 1))
    kern["nhwc_to_nchw + its backward"] = sum(t(lambda: ops.nhwc_to_nchw(x)) + t(lambda: ops.nchw_to_tokens(x.view(B, x.shape[3], x.shape[1], x.shape[2])))
                                             for x in (x0, x1))
    del drows
    for s, (d, depth, hh, ww) in enumerate(((128, 3, h0, w0), (256, 12, h1, w1))):
        u, du, wdw = rnd(B, hh, ww, 2 * d), rnd(B, hh, ww, 2 * d), rnd(2 * d, 1, 7, 7)
        taps = ops.dwconv_weight_taps(wdw)
        n = u.numel()
        kern[f"dwconv7 stage {s}"] = t(lambda: ops.dwconv7_nhwc(u, wdw, *one)) * depth
        ti = t(lambda: ops.dwconv7_nhwc_bwd(du, u, taps, *one, need=(True, False, True)))
        tw = t(lambda: ops.dwconv7_nhwc_bwd(du, u, taps, *one, need=(False, True, False)))
        kern[f"dwconv7_bwd_input stage {s}"], kern[f"dwconv7_bwd_weight stage {s}"] = ti * depth, tw * depth
        for name, us, nbytes in ((f"dwconv7_bwd_input stage {s}", ti, 3 * n * 4), (f"dwconv7_bwd_weight stage {s}", tw, 2 * n * 4)):
            bounds[name] = dict(us=round(us, 1), bytes=nbytes, byte_bound_us=round(nbytes / COPY_BYTES_PER_US, 1), fma=49 * n,
                                fma_bound_us=round(49 * n / FMA_PER_US, 1), of_copy_rate=round(nbytes / us / COPY_BYTES_PER_US, 3))
        del u, du
        hbuf, dh = rnd(B * hh * ww, 4 * d), rnd(B * hh * ww, 4 * d)
        kern[f"star_relu stage {s}"] = t(lambda: ops.star_relu(hbuf, *one)) * depth
        kern[f"star_relu_bwd stage {s}"] = t(lambda: ops.star_relu_bwd(hbuf, dh, one[0])) * depth
        del hbuf, dh
    return {k: round(v, 1) for k, v in kern.items()}, bounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="480x480")
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_backbone_train.py needs a GPU: there is no CPU timing to report")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_grad_enabled(False)
    H, W = (int(v) for v in a.size.split("x"))
    m = init_backbone_8_2("convformer")
    m.load_state_dict(synth.backbone_state_dict(0, "c2f"), strict=True)
    m = m.to(dev)
    res = dict(img_hw=[H, W], calls_per_window=a.calls, windows=a.reps, copy_bytes_per_us=COPY_BYTES_PER_US, fma_per_us=FMA_PER_US, items=[])

    def flush():
        line = json.dumps(res)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(line + "\n")
        return line

    g = torch.Generator().manual_seed(1)
    cells = []
    for B in (int(v) for v in a.batches.split(",")):
        img = torch.randn(B, 3, H, W, generator=g).to(dev)
        cots = [torch.randn(*o.shape, generator=g).to(dev) for o in m(img[:1])]
        cots = [c.expand(B, *c.shape[1:]).contiguous() for c in cots]
        item = dict(B=B)
        m.model.train_native = True
        for prec in ("fp32", "bf16x3"):
            ops.LINEAR_PRECISION = prec
            item[f"native_us_{prec}"], item[f"native_peak_bytes_{prec}"] = measure(m, img, cots, a.calls, a.reps)
        item["kernels_us_per_step"], item["bounds"] = kernels_alone(m.model, B, H, W, dev, max(a.calls, 3), a.reps)
        item["new_kernels_us"] = round(sum(item["kernels_us_per_step"].values()), 1)
        item["new_kernels_share_bf16x3"] = round(item["new_kernels_us"] / item["native_us_bf16x3"]["median"], 3)
        ops.LINEAR_PRECISION = "fp32"
        res["items"].append(item)
        cells.append((item, img, cots))
        print(json.dumps(item), file=sys.stderr, flush=True)
        flush()
    if not a.no_torch:
        m.model.train_native = False
        for item, img, cots in cells:
            item["torch_us"], item["torch_peak_bytes"] = measure(m, img, cots, a.calls, a.reps)
            for prec in ("fp32", "bf16x3"):
                item[f"torch_over_native_{prec}"] = round(item["torch_us"]["median"] / item[f"native_us_{prec}"]["median"], 2)
            print(json.dumps({k: v for k, v in item.items() if k.startswith("torch") or k == "B"}), file=sys.stderr, flush=True)
            flush()
        m.model.train_native = True
    print(flush(), flush=True)


if __name__ == "__main__":
    main()
