"""Command-line benchmark of the localisation loop with the reference's flag set (model_eval/benchmark_nerfmatch.py:209-250).

    python -m nerfmatch_amd.benchmark_nerfmatch --ckpts <matcher.ckpt> --nerf_path <nerf.ckpt> --mutual --solver colmap ...
    python -m nerfmatch_amd.benchmark_nerfmatch --synthetic 8 --solver none --query2query --mutual        # no data, no checkpoints

Same flags, defaults and control flow as the reference's script: checkpoint search (`--ckpt_dir` / `--model_name` / `--feats` /
`--scene`), one evaluation per seed (`--seeds`) into `<ckpt dir>/<cache_tag>run<i>` or `.../results`, `eval_ckpt` building
`data_conf` / `inerf_conf` from the arguments and making the keyword call of :126-151 against `NeRFMatchEvaluator.eval_multi_scenes`.
What differs is underneath (HIP kernels) and at the edges the reference delegates to out-of-scope code:

  * datasets (NeRFMatchPair / NeRFMatchMultiPair) are not part of this package: real data needs
    `NeRFMatchEvaluator.dataset_factory`; without one the call raises and says so;
  * `--synthetic N` (extension) runs the same code path on N synthetic 640x480 queries per scene (`--synthetic_scenes`), synthetic
    NeRF and matcher weights (nerfmatch_amd.synth), the stub backbone, and -- unless `--ckpts` is given -- a synthetic matcher
    checkpoint written in the reference's Lightning layout next to the results; `--image_hw HxW` changes the query size;
  * `collect_results` (reference :22-94) reads the result files written by the runs and prints the per-scene table.
"""
import argparse
import tempfile
from argparse import Namespace
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from . import synth
from .nerfmatch_evaluator import load_nerfmatch_from_ckpt
from .utils.metrics import average_pose_metrics, summarize_pose_statis


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # the reference's flags, names and defaults (benchmark_nerfmatch.py:209-250)
    p.add_argument("--split", type=str, default="test")
    p.add_argument("--ckpt_dir", type=str, default=None)
    p.add_argument("--scene_anno_path", type=str, default=None)
    p.add_argument("--ckpts", type=str, nargs="*", default=[])
    p.add_argument("--model_name", type=str, default="best_tmed")
    p.add_argument("--coarse_only", action="store_true")
    p.add_argument("--mutual", action="store_true")
    p.add_argument("--query2query", action="store_true")
    p.add_argument("--match_thres", type=float, default=0.0)
    p.add_argument("--ow_cache", action="store_true")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--solver", type=str, default="colmap")
    p.add_argument("--rthres", type=float, default=10)
    p.add_argument("--center_subpixel", action="store_true")
    p.add_argument("--iters", type=int, default=1)
    p.add_argument("--nerf_path", type=str, default=None)
    p.add_argument("--test_pair_txt", type=str, default=None)
    p.add_argument("--scene_dir", type=str, default=None)
    p.add_argument("--dataset", type=str, default=None)
    p.add_argument("--scene", type=str, default=None)
    p.add_argument("--pair_topk", type=int, default=1)
    p.add_argument("--sample_pts", type=int, default=-1)
    p.add_argument("--sample_mode", type=str, default=None)
    p.add_argument("--mask", type=str, default="default")
    p.add_argument("--cache_tag", type=str, default=None)
    p.add_argument("--inerf", action="store_true")
    p.add_argument("--inerf_optim", type=int, default=5)
    p.add_argument("--inerf_lr", type=float, default=0.001)
    p.add_argument("--inerf_lrd", action="store_true")
    p.add_argument("--inerf_ds", type=int, default=8)
    p.add_argument("--inerf_pose", action="store_true")
    p.add_argument("--inerf_match_loss", action="store_true")
    p.add_argument("--cache_iters", action="store_true")
    p.add_argument("--no_cache_pt", action="store_true")
    p.add_argument("--retrieval_only", action="store_true")
    p.add_argument("--match_oracle", action="store_true")
    p.add_argument("--visualize", action="store_true")
    p.add_argument("--seeds", type=int, nargs="*", default=[])
    p.add_argument("--feats", type=str, nargs="*", default=[])
    # extensions (synthetic run without datasets / checkpoints)
    p.add_argument("--synthetic", type=int, default=0, help="N > 0: N synthetic queries per scene instead of the (out-of-scope) dataset classes")
    p.add_argument("--synthetic_scenes", type=str, nargs="*", default=["chess"])
    p.add_argument("--image_hw", type=str, default="480x640")
    p.add_argument("--samples", type=int, default=64, help="samples per ray of the synthetic NeRF (coarse = fine)")
    p.add_argument("--batch_size", type=int, default=1, help="queries per launch sequence (the reference's loop takes 1)")
    # (no default: absent from the parsed arguments unless given, so that the checkpoint's own `backbone_precision` holds)
    p.add_argument("--backbone_precision", type=str, default=argparse.SUPPRESS, choices=["same", "fp16"],
                   help="inference arithmetic of the native ConvFormer backbone (modules/convformer.py); default: what the checkpoint's config says")
    return p


# ----------------------------------------------------------------------------------------------- synthetic scenes
class SyntheticScene(torch.utils.data.Dataset):
    """Stand-in for one scene of NeRFMatchPair (datasets/nerfmatch_dataset.py:311-325): `.scene`, `.scene_dir` and per-query dicts
    without the batch dimension (image, im_mask, K, c2w, rc2w, pt2d, unnorm_scene)."""

    def __init__(self, scene, n, H, W, seed=0):
        self.scene, self.scene_dir = scene, f"synthetic/{scene}/inter_layer3/ds8lin"
        unnorm = synth.unnorm_scene()
        M = (H // 8) * (W // 8)
        ys, xs = torch.meshgrid(torch.arange(H // 8), torch.arange(W // 8), indexing="ij")
        pt2d = (torch.stack([xs, ys], -1) * 8 + 4).float().reshape(M, 2)
        self.samples = []
        for q in range(n):
            g = torch.Generator().manual_seed(1000 * seed + q)
            self.samples.append(dict(image=torch.randn(3, H, W, generator=g), im_mask=torch.ones(M, dtype=torch.bool), K=synth.intrinsics(H, W),
                                     c2w=unnorm @ synth.camera_pose(q), rc2w=unnorm @ synth.camera_pose(q + 100), pt2d=pt2d, unnorm_scene=unnorm))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return self.samples[i]


def synthetic_factories(args, device):
    from .nerf.renderer import NerfRenderer

    H, W = (int(v) for v in args.image_hw.lower().split("x"))

    def dataset_factory(data_conf, split):
        return [SyntheticScene(s, args.synthetic, H, W, seed=i) for i, s in enumerate(args.synthetic_scenes)]

    def renderer_factory(scene, scene_dir, stop_layer):
        ren = NerfRenderer(synth.nerf_config("7scenes", num_pts=args.samples, img_wh=(W, H)), training=False, stop_layer=stop_layer)
        ren.load_state_dict(synth.nerf_state_dict(seed=sum(map(ord, scene)) % 97, density_bias=3.0))
        ren.to(device).eval()
        ren.unnorm_scene = synth.unnorm_scene()
        return ren

    return dataset_factory, renderer_factory


def write_synthetic_ckpt(path, coarse_only=False):
    kind = "coarse" if coarse_only else "c2f"
    cfg = Namespace(model=synth.matcher_config(kind), exp=Namespace(seed=0), data=Namespace())
    sd = {f"model.{k}": v for k, v in synth.matcher_state_dict(kind).items()}
    torch.save(dict(state_dict=sd, hyper_parameters=vars(cfg), epoch=0, global_step=0), path)
    return path


# ----------------------------------------------------------------------------------------------- the reference's functions
def eval_ckpt(args):
    """reference :97-151."""
    ev = load_nerfmatch_from_ckpt(args.ckpt, args, arg_mask=args.mask)
    if not ev.coarse_only:
        ev.coarse_only = args.coarse_only
    data_conf = Namespace()
    if args.pair_topk > 1:
        data_conf = Namespace(dataset="NeRFMatchMultiPair", sample_mode=args.sample_mode, sample_pts=args.sample_pts, pair_topk=args.pair_topk)
    if args.scene and "allscenes" in args.ckpt:
        print("### Set scene to : ", args.scene)
        data_conf.scenes = [args.scene]
    if args.scene_anno_path:
        print("### Set scene annotation to : ", args.scene_anno_path)
        data_conf.scene_anno_path = args.scene_anno_path
    inerf_conf = None
    if args.inerf:
        inerf_conf = Namespace(num_optim=args.inerf_optim, lrate=args.inerf_lr, lrdecay=args.inerf_lrd, eval_pose=args.inerf_pose, ds=args.inerf_ds,
                               use_match_loss=args.inerf_match_loss)
    extra = {}
    if args.synthetic > 0:
        ev.dataset_factory, ev.renderer_factory = synthetic_factories(args, ev.device)
        extra["batch_size"] = args.batch_size
    return ev.eval_multi_scenes(
        rthres=args.rthres, center_subpixel=args.center_subpixel, solver=args.solver, split=args.split, mutual=args.mutual,
        match_thres=args.match_thres, iters=args.iters, nerf_path=args.nerf_path, test_pair_txt=args.test_pair_txt, scene_dir=args.scene_dir,
        data_conf=data_conf, query2query=args.query2query, ow_cache=args.ow_cache, inerf_conf=inerf_conf, debug=args.debug,
        cached_pt=not args.no_cache_pt, cache_dir=args.cache_dir, cache_iters=args.cache_iters, retrieval_only=args.retrieval_only,
        match_oracle=args.match_oracle, visualize=args.visualize, seed=args.seed, **extra)


def benchmark(args):
    """reference :154-206: find the checkpoints, run every seed into its own result directory."""
    if args.ckpts:
        ckpts = [Path(c) for c in args.ckpts]
    elif args.ckpt_dir:
        ckpt_dir = Path(args.ckpt_dir)
        pattern = f"{args.model_name}.ckpt" if "allscenes" in str(ckpt_dir) else f"*_{args.model_name}.ckpt"
        if args.feats:
            ckpts = [c for k in args.feats for c in ckpt_dir.glob(f"{k}/{pattern}")]
        else:
            ckpts = list(ckpt_dir.glob(f"*/{pattern}"))
        if args.scene:
            ckpts = [c for c in ckpts if args.scene in str(c)]
    elif args.synthetic > 0:
        root = Path(tempfile.mkdtemp(prefix="nerfmatch_amd_bench_")) / "synthetic"
        root.mkdir(parents=True)
        ckpts = [write_synthetic_ckpt(root / f"synthetic_{args.model_name}.ckpt", args.coarse_only)]
    else:
        raise SystemExit("give --ckpts or --ckpt_dir (or --synthetic N for a run without checkpoints)")
    print(f"Found the following {len(ckpts)} ckpts:\n" + "\n".join(str(c) for c in ckpts) + ".")
    cache_tag = f"{args.cache_tag}_" if args.cache_tag else ""
    if args.model_name != "best":
        cache_tag += f"{args.model_name}_"
    out = {}
    for ckpt in ckpts:
        runs = [(i, s) for i, s in enumerate(args.seeds)] or [(None, None)]
        for i, seed in runs:
            print(f"\n>>> Benchmark {ckpt}" + (f" - Run {i} - Seed {seed}." if i is not None else "."))
            args.ckpt, args.seed = str(ckpt), seed
            args.cache_dir = ckpt.parent / (f"{cache_tag}run{i}" if i is not None else f"{cache_tag}results")
            out[(str(ckpt), seed)] = eval_ckpt(args)
    return out


def collect_results(cache_dirs, scenes, conf, pose_thres, print_out=True):
    """reference :22-94 in brief: per-scene result files -> summarize_pose_statis -> averages over scenes and runs."""
    scores = defaultdict(list)
    for cache_dir in cache_dirs:
        metr_all = []
        for scene in scenes:
            path = Path(cache_dir) / f"{scene}_{conf}.npy"
            if not path.exists():
                print(f"{path} doesn't exist!")
                continue
            metr_all.append(summarize_pose_statis(np.load(path, allow_pickle=True).item(), pose_thres=pose_thres[scene], t_unit="cm", t_scale=1e2,
                                                  print_out=print_out))
        if metr_all:
            print(["/".join(f"{x:.1f}" for x in (f["t_med"], f["r_med"], f["recall"])) for f in metr_all])
            for k, v in average_pose_metrics(metr_all).items():
                scores[k].append(v)
    return scores


def main(argv=None):
    return benchmark(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
