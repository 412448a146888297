"""Minimal training loop with the reference's step semantics (vidgen/engine/trainer.py:56-128,
train_loop.py:112-133, defaults.py:273-310), minus its per-step host synchronisations:

  * `run_step`: next batch -> `model(data, mode='supervised')` -> sum of the loss dict -> backward ->
    every ACCUMULATION_STEPS: all optimizers step, then all zero_grad; schedulers step once per iteration.
  * losses are kept on the device; they are fetched (one D2H copy) only every `log_period` iterations, where the
    finiteness check of `_detect_anomaly` is also applied.  The reference does `.item()` + a gloo gather of a
    pickled dict every step, which serialises the ranks.
  * SOLVER.CLIP_GRADIENTS (solver/clip.py): on an iteration that steps, the data-parallel reduction is joined and ONE clipper over
    all optimizers prepares the step (global norm / skip flag on the device, or the clamp); the accumulated gradient is
    clipped once.  No host synchronisation: `grad_norm` and `skipped_steps` ride in the D2H copy of the losses at `log_period`.
    Disabled (the default), the trainer holds no clipper and the sequence above is unchanged.
  * MODEL.CODEBOOK.RESTART: `codebook_perplexity`, `codebook_dead` and `codebook_restarts` (device scalars of the quantiser's
    health record) ride in the same copy.  Off (the default), nothing changes.
  * SOLVER.MODEL_EMA (solver/ema.py): the fused optimizers keep a Polyak average of every parameter they step, inside the step
    launch, so it advances exactly on the iterations that step (ACCUMULATION_STEPS is respected) and costs no host
    synchronisation.  Every checkpoint gets an averaged twin `model_*_ema.pth` with the module's own keys (sub-networks with an
    optimizer only); `last_checkpoint` keeps naming the live file.  Resuming restores the shadows from the twin of the resumed
    file, or starts them from the loaded weights.  Off (the default), the trainer holds no ModelEma and nothing changes.
  * checkpoints: one Checkpointer per sub-network, `model_{iter:07d}.pth` / `model_final.pth`, rank 0 only.
"""
import logging
import os
import time

import torch

from ..solver.build import build_grad_clipper, build_model_ema
from ..solver.ema import ema_twin
from ..utils import comm
from ..utils.checkpoint import PeriodicCheckpointer
from ..utils.events import EventStorage


class Trainer:
    def __init__(self, cfg, model, data_iter, log_period=20):
        self.cfg, self.model, self.data_iter, self.log_period = cfg, model, data_iter, log_period
        self.optimizers, self.checkpointers = model.configure_optimizers_and_checkpointers()
        if comm.get_world_size() > 1:
            model.wrap_parallel(device_ids=[comm.get_local_rank()], broadcast_buffers=False)
        self.clipper = build_grad_clipper(cfg, self.optimizers)       # None unless SOLVER.CLIP_GRADIENTS.ENABLED
        self.model_ema = build_model_ema(cfg, self.optimizers)        # None unless SOLVER.MODEL_EMA.ENABLED
        model.train()
        self.start_iter, self.max_iter = 0, cfg.SOLVER.MAX_ITER
        self.accumulation_steps = cfg.SOLVER.ACCUMULATION_STEPS
        self.periodic = [PeriodicCheckpointer(c["checkpointer"], cfg.SOLVER.CHECKPOINT_PERIOD, self.max_iter)
                         for c in self.checkpointers] if comm.is_main_process() else []
        self.logger = logging.getLogger("lvt_amd")
        self.iter = 0

    def resume_or_load(self, resume=True):
        for item in self.checkpointers:
            ck = item["checkpointer"]
            resumed = ck.get_checkpoint_file() if resume and ck.has_checkpoint() else ""
            ck.resume_or_load(item["pretrained"], resume=resume)
            if self.model_ema is None or not self.model_ema.owns(ck.model):
                continue
            twin = ema_twin(resumed) if resumed else ""
            if twin and os.path.isfile(twin):           # the averaged weights that went with the resumed checkpoint
                data = torch.load(twin, map_location="cpu")
                self.model_ema.load_shadows(ck.model, data["model"], data.get("ema_updates"))
                self.logger.info("averaged weights of %s restored from %s", os.path.basename(ck.save_dir), twin)
            else:                                       # none on disk: the average restarts from the loaded weights
                self.model_ema.reset_shadows(ck.model)

    def _save_twins(self):
        """`model_*_ema.pth` next to every checkpoint written at this iteration: the state dict of each sub-network that has
        an optimizer, taken while the parameters hold the averaged weights (buffers are the live ones)."""
        if self.model_ema is None or not self.periodic or not self.periodic[0].due(self.iter):
            return
        with self.model_ema.averaged():
            for pc in self.periodic:
                if self.model_ema.owns(pc.checkpointer.model):
                    pc.step_twin(self.iter, ema_updates=self.model_ema.updates)

    def run_step(self):
        assert self.model.training, "model was changed to eval mode!"
        data = next(self.data_iter)
        loss_dict = self.model(data, mode="supervised")
        losses = sum(loss_dict.values())
        losses.backward()
        if (self.iter + 1) % self.accumulation_steps == 0:
            if self.clipper is not None:
                self.model.finish_gradient_sync()          # the norm is taken over the REDUCED gradients: the same on every rank
                self.clipper.prepare()
            for item in self.optimizers:
                item["optimizer"].step()
            for item in self.optimizers:
                item["optimizer"].zero_grad()
        for item in self.optimizers:
            item["scheduler"].step()
        return loss_dict

    def train(self, max_iter=None):
        max_iter = self.max_iter if max_iter is None else max_iter
        t0, last = time.perf_counter(), None
        with EventStorage(self.start_iter) as storage:
            for self.iter in range(self.start_iter, max_iter):
                last = self.run_step()
                if (self.iter + 1) % self.log_period == 0 or self.iter == max_iter - 1:
                    clip = {}
                    clipping = self.clipper is not None and self.clipper.norm is not None
                    health = getattr(self.model, "codebook_health", None)
                    health = health() if health is not None else None
                    if not clipping and health is None:
                        vals = {k: float(v.detach()) for k, v in last.items()}          # the only D2H sync
                    else:       # losses, gradient norm and skip counter in ONE copy (a skipped step's norm is inf / nan: not an anomaly)
                        names, extra = [], []
                        if health is not None:      # (always finite; logged like the clipper's pair, outside the losses)
                            names += ["codebook_perplexity", "codebook_dead", "codebook_restarts"]
                            extra += list(health)
                        if clipping:
                            names += ["grad_norm", "skipped_steps"]
                            extra += [self.clipper.norm, self.clipper.skipped]
                        host = torch.stack([v.detach().reshape(()).double() for v in list(last.values()) + extra]).tolist()
                        vals = dict(zip(last, host))
                        clip = dict(zip(names, host[len(last):]))
                    if not all(torch.isfinite(torch.tensor(list(vals.values())))):
                        raise FloatingPointError("Loss became infinite or NaN at iteration={}! {}".format(self.iter, vals))
                    storage.put_scalars(**vals)
                    storage.put_scalars(smoothing_hint=False, **clip)
                    vals.update(clip)
                    if comm.is_main_process():
                        dt = (time.perf_counter() - t0) / (self.iter + 1 - self.start_iter)
                        self.logger.info("iter %d  %s  %.4f s/it", self.iter,
                                         "  ".join("%s: %.5f" % kv for kv in vals.items()), dt)
                for pc in self.periodic:
                    pc.step(self.iter)
                self._save_twins()
                storage.step()
        return last
