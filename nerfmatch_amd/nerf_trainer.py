"""Training of a NeRF scene model without pytorch-lightning (reference: NerfTrainer, nerfmatch/nerf_trainer.py:28-188, launched by
train() :307-397).  Host-side plumbing: the training render and the losses are the kernels of nerf/train_render.py under
torch.autograd.Function, the optimiser and schedule table is trainer._TrainerBase's (the NeRF yamls set `optim.lr`), data parallelism
is one process per GPU with dist.GradBuckets as in the matcher trainers.

Batches carry the reference's keys: `rays` (1,R,12), `rgbs` (1,R,3), `ts` (1,R) appearance ids, `mask` (R,1) (read when
loss.use_sem_mask), `seq_ind`, `img_idx`, `img_wh`; a two-view validation batch (the pair dataset's) also `c2w` (1,8,4), `K` (1,6,3) and
`unnorm_scene` (1,4,4).  validation_step returns the scalar metrics and, for a two-view batch, the pose metrics of log_step
(utils.metrics.compute_nerf_pose_metrics, :125-133): cosine mutual-NN matching of the two views' point features and four PnP problems, on
the GPU.  nerf.ray_bank.RayBank produces all three kinds of batch from frames held on the GPU: `fit(bank)` trains a scene.  Not built: image
logging."""
import torch

from . import dist as nmdist
from .nerf.renderer import NerfRenderer
from .nerf.train_render import training_metrics
from .nerf_evaluator import save_nerf_ckpt
from .trainer import _TrainerBase
from .utils.metrics import compute_nerf_metrics, compute_nerf_pose_metrics


def init_pfeat_mask(img_wh, ds=8, sample_num=1):
    """Boolean mask (sample_num, img_wh[0], img_wh[1], 1) of the rays whose point features a validation render keeps: every ds-th pixel
    from ds // 2 (reference :28-32)."""
    pfeat_mask = torch.zeros(sample_num, *img_wh, 1).bool()
    pfeat_mask[:, ds // 2 :: ds, ds // 2 :: ds] = 1
    return pfeat_mask


class LossScale:
    """Loss-scale state of the "f16" training mode with torch.cuda.amp.GradScaler's rule and defaults: initial scale 65536; a step that counted
    a BACKWARD overflow event is skipped and the scale halved; after 2000 consecutive clean steps the scale doubles.  The scale stays a
    power of two, so multiplying by it and by its inverse is exact.  A FORWARD event (an activation stored as non-finite fp16 from a finite
    accumulator) skips the step as well but leaves the scale alone -- no scale cures it -- and warns once."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.scale, self.growth_factor, self.backoff_factor, self.growth_interval = float(init_scale), growth_factor, backoff_factor, growth_interval
        self.clean_steps = self.skipped_steps = 0
        self.overflow_events = [0, 0]  # forward, backward
        self._warned = False

    def update(self, forward_events, backward_events):
        """The step's event counts -> True when the optimiser step must be skipped."""
        self.overflow_events[0] += int(forward_events)
        self.overflow_events[1] += int(backward_events)
        if forward_events and not self._warned:
            self._warned = True
            import warnings

            warnings.warn(f"NeRF training (train_precision='f16'): {int(forward_events)} activations left fp16's range in the forward pass; the step "
                          "is skipped and the loss scale kept (it does not act on the forward pass).  If this repeats, train this scene with "
                          "train_precision='same'.", RuntimeWarning, stacklevel=3)
        if not (forward_events or backward_events):
            self.clean_steps += 1
            if self.clean_steps >= self.growth_interval:
                self.scale *= self.growth_factor
                self.clean_steps = 0
            return False
        if backward_events:
            self.scale *= self.backoff_factor
        self.clean_steps = 0
        self.skipped_steps += 1
        return True


class NerfTrainer(_TrainerBase):
    def __init__(self, config, num_frames=300, device="cuda", bucket_mb=64, optimizer_factory=None, scheduler_factory=None, closest_ind=None):
        self.config = config
        self.closest_ind = closest_ind
        sample_num = 2 if getattr(config.data, "train_pair_txt", None) else 1
        self.model = NerfRenderer(config, num_frames).to(device)
        self.model.pfeat_mask = init_pfeat_mask(config.data.img_wh, ds=8, sample_num=sample_num)
        self.cnfg_loss = getattr(config, "loss", None)
        self.mask_loss = bool(getattr(self.cnfg_loss, "use_sem_mask", False)) if self.cnfg_loss else False
        self.gpu_num = getattr(config, "gpu_num", None) or nmdist.world()[1]
        self.current_epoch = self.global_step = 0
        self.optimizer = self.scheduler = None
        self._opt_factory, self._sched_factory = optimizer_factory, scheduler_factory
        nmdist.broadcast_module(self.model, src=0)
        self.buckets = nmdist.GradBuckets(self.model.parameters(), bucket_mb=bucket_mb)
        self.scaler = LossScale()  # (read only under model.train_precision == "f16")

    # the loss-scale state of the "f16" mode (LossScale): master parameters, .grad, the optimiser and checkpoints stay fp32
    loss_scale = property(lambda self: self.scaler.scale, lambda self, v: setattr(self.scaler, "scale", float(v)))
    skipped_steps = property(lambda self: self.scaler.skipped_steps)
    overflow_events = property(lambda self: tuple(self.scaler.overflow_events))

    @staticmethod
    def _rows(x, cols):
        return x.reshape(-1, cols)

    def training_step(self, data, batch_idx=0, **render_kw):
        """forward + backward + gradient all-reduce + optimiser step (reference :140-158); returns the step's metrics (detached).
        render_kw: explicit random draws for the render (t_rand, jitter, noise_coarse, noise_fine).
        Under model.train_precision == "f16" the backward pass runs on loss_scale times the loss (the gradients that reach .grad are
        unscaled fp32) and a step that counted an fp16 overflow is skipped: no optimiser step, see LossScale."""
        if self.optimizer is None:
            self.configure_optimizers()
        m = self.model
        m.ret_pfeat = False
        m.set_training_mode(True)
        rays = self._rows(data["rays"], data["rays"].shape[-1])
        dev = next(m.parameters()).device
        f16 = m.train_precision == "f16"
        if f16:
            m.train_loss_scale = self.scaler.scale
            m._train_events(dev).zero_()
        with torch.enable_grad():
            preds = m.forward(rays.to(dev), step=self.global_step, ray_id=data["ts"].reshape(-1) if "ts" in data else None, **render_kw)
            mask = data["mask"].to(dev) if self.mask_loss else None
            metrics = training_metrics(preds, self._rows(data["rgbs"], 3).to(dev), mask, self.cnfg_loss)
            self.optimizer.zero_grad(set_to_none=True)
            self.buckets.start()
            metrics["loss"].backward()
        self.buckets.finish()
        skip = False
        if f16:  # one read of the two counters per step (what torch's GradScaler does with its found-inf flag)
            ev = m._train_events(dev)
            if nmdist.world()[1] > 1:
                torch.distributed.all_reduce(ev)  # every rank takes the same decision
            skip = self.scaler.update(*ev.tolist())
        if not skip:
            self.optimizer.step()  # (in-place updates bump the parameters' versions: the inference blobs are re-packed on their next use)
        self.global_step += 1
        return {k: v.detach() for k, v in metrics.items()}

    def validation_step(self, data, batch_idx=0, **render_kw):
        """Validation render (ret_pfeat=True, pfeat_mask honoured) and its scalar metrics (reference :160-180); a batch of more than one
        view (len(data["img_idx"]) > 1) adds R_err_depth, t_err_depth, R_err_match, t_err_match, match_score and num_matches (:125-133)."""
        m = self.model
        m.ret_pfeat = True
        m.set_training_mode(False)
        rays = self._rows(data["rays"], data["rays"].shape[-1])
        dev = next(m.parameters()).device
        seq = torch.as_tensor(data["seq_ind"]).reshape(-1).long()
        ray_id = seq.repeat_interleave(rays.shape[0] // len(seq))
        with torch.no_grad():
            preds = m.forward(rays.to(dev), ray_id=ray_id, validation=True, **render_kw)
            mask = data["mask"].to(dev) if self.mask_loss else None
            metrics = compute_nerf_metrics(preds, self._rows(data["rgbs"], 3).to(dev), mask_loss=mask, validation_mode=True, cnfg_loss=self.cnfg_loss)
            if len(data["img_idx"]) > 1:
                metrics.update(compute_nerf_pose_metrics(preds["pts_fine"], m.pfeat_mask[0, ..., 0], preds["feat_fine"], data))
        return metrics

    def fit(self, loader, max_epochs=1, log=None):
        from ._lib import steady_gc

        for _ in range(max_epochs):
            if hasattr(loader, "set_epoch"):  # (nerf.ray_bank.RayBank: the epoch keys its permutation, like DistributedSampler.set_epoch)
                loader.set_epoch(self.current_epoch)
            with steady_gc():
                for i, batch in enumerate(loader):
                    metrics = self.training_step(batch, i)
                    if log is not None:
                        log(self.current_epoch, i, metrics)
            self.on_epoch_end()

    def save_checkpoint(self, path):
        """A checkpoint in the reference's Lightning layout, as load_nerf_render_from_ckpt reads it."""
        sd = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        save_nerf_ckpt(path, self.config, sd, unnorm_scene=self.model.unnorm_scene, epoch=self.current_epoch, global_step=self.global_step)
