"""Optimizer, learning-rate-schedule, gradient-clipper and averaged-weights factories (fused multi-tensor Adam / RMSprop on the device)."""
from . import build as _build

build_optimizer, build_lr_scheduler = _build.build_optimizer, _build.build_lr_scheduler
build_grad_clipper = _build.build_grad_clipper
build_model_ema = _build.build_model_ema

__all__ = ("build_optimizer", "build_lr_scheduler", "build_grad_clipper", "build_model_ema")
