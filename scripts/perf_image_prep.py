#!/usr/bin/env python3
"""What preparing images costs with nerfmatch_amd.image_prep (nm_image_resize_u8), beside the reference's host form and the byte floor:

  query_1080p   --batch frames of 1080 x 1920 x 3 -> 480 x 480 through query_images (the Cambridge configs: 4 x and 2.25 x)
  query_480p    --batch frames of 480 x 640 x 3 -> 480 x 480 through query_images (7-Scenes: the horizontal pass only)
  nerf_frames   --frames frames of 1080 x 1920 x 3 with a background and a transient mask through nerf_frames (three launches)
  pillow_*      the same work as the reference does it: PIL.Image.resize(..., Image.LANCZOS) on ONE host core, the `/ 255` (or the
                blend) in numpy as process_img writes it, then the copy of the result to the device; per frame, from --host-frames frames
                (file decoding is NOT counted); only when Pillow is importable
  floor_us      (source bytes + output bytes) / 6.3 TB/s, the streaming rate measured on this chip (8 TB/s is its specification)

The device items read decoded uint8 frames that are already on the device.  Every timed call takes another of several input sets whose
total size exceeds the 256 MiB Infinity Cache, so the source really comes from HBM.  Times are HIP events over windows of --calls calls
(a host clock ending in a synchronise for pillow_*), --reps windows each: median / min / max over the windows.  No pass / fail: prints
one JSON line.

    python scripts/perf_image_prep.py [--batch 16] [--frames 200] [--calls 20] [--reps 7] [--host-frames 8] [--no-host] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nerfmatch_amd import image_prep  # noqa: E402

WH = (480, 480)
HBM_BYTES_PER_US = 6.3e6  # 6.3 TB/s
CACHE_BYTES = 256 << 20


def spread(vals):
    v = sorted(vals)
    return dict(median=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2))


def event_windows(fn, calls, reps, warmup=3):
    """microseconds per call of fn(i): `reps` windows of `calls` calls between two events"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for r in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(r * calls + i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return spread(out)


def frames_on_device(n, H, W, C, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    shape = (n, H, W, C) if C else (n, H, W)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)


def query_item(B, H, W, dev, calls, reps):
    src_bytes, out_bytes = B * H * W * 3, B * 3 * WH[0] * WH[1] * 4
    sets = [frames_on_device(B, H, W, 3, dev, s) for s in range(max(2, -(-2 * CACHE_BYTES // src_bytes)))]
    t = event_windows(lambda i: image_prep.query_images(sets[i % len(sets)], WH), calls, reps)
    floor = (src_bytes + out_bytes) / HBM_BYTES_PER_US
    return dict(frames=B, source=[H, W, 3], input_sets=len(sets), us_per_call=t, us_per_frame=round(t["median"] / B, 2), floor_us=round(floor, 2),
                times_floor=round(t["median"] / floor, 2), source_bytes=src_bytes, output_bytes=out_bytes)


def pillow_query(H, W, n, dev, reps):
    from PIL import Image

    g = np.random.default_rng(0)
    frames = [Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8), "RGB") for _ in range(n)]
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for im in frames:
            x = np.array(im.resize(WH, Image.LANCZOS)) / 255.0
            torch.tensor(x).permute(2, 0, 1).float().to(dev)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / n)
    return spread(out)


def pillow_nerf(H, W, n, dev, reps):
    from PIL import Image

    g = np.random.default_rng(1)
    frames = [(Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8), "RGB"), Image.fromarray(g.integers(0, 2, (H, W), dtype=np.uint8) * 255, "L"),
               Image.fromarray(g.integers(0, 2, (H, W), dtype=np.uint8) * 255, "L")) for _ in range(n)]
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for im, bg, tr in frames:
            x = torch.from_numpy(np.array(im.resize(WH, Image.LANCZOS))).float().div(255)
            m = torch.round(torch.from_numpy(np.array(bg.resize(WH, Image.LANCZOS))).float().div(255))[..., None]
            x = x * (1 - m) + m * torch.tensor([1.0, 1.0, 1.0])
            t = torch.from_numpy(np.array(tr.resize(WH, Image.LANCZOS))).float().div(255)
            x.to(dev), t.to(dev)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / n)
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-frames", type=int, default=8)
    ap.add_argument("--no-host", action="store_true", help="skip the Pillow items")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_image_prep.py needs a GPU: there is no CPU timing to report")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_num_threads(1)  # the host items: one core, as a DataLoader worker has
    res = dict(img_wh=list(WH), calls_per_window=a.calls, windows=a.reps, hbm_bytes_per_us=HBM_BYTES_PER_US, tile_wh=list(image_prep.TILE_WH))
    res["query_1080p"] = query_item(a.batch, 1080, 1920, dev, a.calls, a.reps)
    res["query_480p"] = query_item(a.batch, 480, 640, dev, a.calls, a.reps)
    # a scene's frames with both masks: 1.2 GB of frames and 0.8 GB of masks, far beyond the cache
    F, H, W = a.frames, 1080, 1920
    images, bg, tr = frames_on_device(F, H, W, 3, dev, 7), frames_on_device(F, H, W, 0, dev, 8), frames_on_device(F, H, W, 0, dev, 9)
    t = event_windows(lambda i: image_prep.nerf_frames(images, WH, bg_masks_u8=bg, trnz_masks_u8=tr), max(a.calls // 5, 2), a.reps, warmup=1)
    src_bytes, out_bytes = F * H * W * 5, F * WH[0] * WH[1] * (5 + 1)  # (+ 1: the resized background mask is read back by the image launch)
    floor = (src_bytes + out_bytes) / HBM_BYTES_PER_US
    res["nerf_frames"] = dict(frames=F, source=[H, W, 3], masks=2, us_per_call=t, us_per_frame=round(t["median"] / F, 2), floor_us=round(floor, 2),
                              times_floor=round(t["median"] / floor, 2), source_bytes=src_bytes, output_bytes=out_bytes)
    del images, bg, tr
    # the device path returns the host path's bytes at these sizes (one frame each; the tests hold the full comparison)
    one = frames_on_device(1, 1080, 1920, 3, dev, 3)
    res["equals_host_path_1080p"] = bool(torch.equal(image_prep.resize_lanczos_u8(one, WH).cpu(), image_prep.resize_lanczos_u8(one.cpu(), WH)))
    try:
        import PIL  # noqa: F401
    except ImportError:
        PIL = None
    if PIL is not None and not a.no_host:
        res["pillow_version"] = PIL.__version__
        res["pillow_query_1080p_us_per_frame"] = pillow_query(1080, 1920, a.host_frames, dev, min(a.reps, 3))
        res["pillow_query_480p_us_per_frame"] = pillow_query(480, 640, a.host_frames, dev, min(a.reps, 3))
        res["pillow_nerf_frame_us_per_frame"] = pillow_nerf(1080, 1920, a.host_frames, dev, min(a.reps, 3))
    elif not a.no_host:
        res["pillow_version"] = None  # not importable: the host items are not measured
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
