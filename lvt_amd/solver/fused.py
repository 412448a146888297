"""torch.optim-compatible optimizers whose `step()` is a fused multi-tensor HIP launch.

Same constructor arguments, param_groups / state layout (state keys `step`, `exp_avg`, `exp_avg_sq`
for Adam; `step`, `square_avg`, `momentum_buffer` for RMSprop) and update rule as torch.optim.Adam /
torch.optim.RMSprop, so checkpoints and LR schedulers are interchangeable.  Parameters that are not on a
GPU fall back to raising: there is no CPU path in this package.

Gradient clipping (solver/clip.py) happens inside the step kernels: `set_grad_clip` hands the NEXT `step()` a device record
with the clip coefficient and the skip flag of the global gradient norm, and / or an elementwise clamp.  `step()` consumes it:
a step that was handed nothing calls the unclipped entry points.  `p.grad` is never rewritten.

Polyak-averaged weights (solver/ema.py) happen inside the step kernels too: after `enable_ema(decay)` every parameter carries a
shadow `state[p]["ema"]`, and `step()` calls the `_ema` entry points, which move the shadow towards the new parameter value
while the launch still holds it in a register.  Off (the default), `step()` calls what it always called.
"""
import ctypes as C
import math

import torch
from torch.optim import Optimizer

from ..hip import binding as L


def _entries(items):
    arr = (L.OptEntry * len(items))()
    for i, (p, g, s0, s1, lr, wd) in enumerate(items):
        e = arr[i]
        e.p, e.g, e.s0 = p.data_ptr(), g.data_ptr(), s0.data_ptr()
        e.s1 = s1.data_ptr() if s1 is not None else None
        e.n, e.lr, e.wd = p.numel(), lr, wd
    return arr


def ema_decay_at(t, decay, warmup=True):
    """Decay of update number `t` (0 for the first update an optimizer launches): `decay`, or with `warmup`
    min(decay, (1 + t) / (10 + t)), which starts at 0.1 so that the average forgets its initial value quickly."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def check_ema_decay(decay):
    if not isinstance(decay, (int, float)) or isinstance(decay, bool) or not math.isfinite(decay) or not 0.0 <= decay < 1.0:
        raise ValueError("the decay of the averaged weights must be finite and lie in [0, 1) (got {!r})".format(decay))


def _shadows(tensors, ents):
    """Host array of the shadows' device pointers for lvt_*_step_ema: one per entry, as long as the entry's parameter."""
    if len(tensors) != len(ents):
        raise L.LvtError("fused optimizers: %d shadows for %d parameters" % (len(tensors), len(ents)))
    arr = (C.c_void_p * len(tensors))()
    for i, (e, ent) in enumerate(zip(tensors, ents)):
        p = ent[0]
        if e is None or not e.is_cuda or e.dtype != p.dtype or e.numel() != p.numel() or not e.is_contiguous():
            raise L.LvtError("fused optimizers: the shadow of parameter %d is missing or does not match it" % i)
        arr[i] = e.data_ptr()
    return arr


class _FusedBase(Optimizer):
    _clip = None            # (record tensor or None, clamp) for the next step(): set_grad_clip
    _ema = None             # (decay, warmup) once enable_ema was called
    ema_updates = 0         # updates launched since enable_ema (a skipped step counts: the count lives on the host)

    def enable_ema(self, decay, warmup=True):
        """From now on every `step()` also moves `state[p]["ema"]` (a clone of `p`, made with the parameter's state, or here
        for state that exists already) towards the new `p`: e += (1 - d_t) (p - e), d_t = ema_decay_at(t, decay, warmup), t
        counting the updates launched since this call.  The shadow is part of `state_dict()` like `exp_avg`."""
        check_ema_decay(decay)
        self._ema = (float(decay), bool(warmup))
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st is not None and len(st) and "ema" not in st:
                    st["ema"] = self._new_shadow(p)

    def disable_ema(self):
        """`step()` calls the entry points without averaging again; the shadows stay where they are, and in `state_dict()`."""
        self._ema = None

    def _new_shadow(self, p):
        init = getattr(self, "_ema_init", {}).pop(p, None)            # ModelEma.load_shadows: a shadow waiting for its state
        return p.detach().clone(memory_format=torch.preserve_format) if init is None else init

    def _ema_weight(self):
        """w = 1 - decay of the update about to be launched (double on the host, float in the kernel), or None when off."""
        if self._ema is None:
            return None
        return 1.0 - ema_decay_at(self.ema_updates, *self._ema)

    def set_grad_clip(self, record=None, clamp=0.0):
        """The next `step()` (and only that one) updates with clamp(g * coef) in the place of every gradient g: `record` is the
        device lvt_clip_record GradClipper filled (coef, and skip: a set flag makes the step store nothing), `clamp` = c > 0
        limits every element to [-c, c], 0 is off."""
        if record is None and not clamp > 0:
            raise ValueError("set_grad_clip needs a record, a clamp > 0, or both")
        self._clip = (record, float(clamp))

    def _take_clip(self):
        clip, self._clip = self._clip, None
        return clip

    def zero_grad(self, set_to_none=True):
        """torch semantics; gradients living in a data-parallel bucket (engine/grad_reducer.py) are always DROPPED
        (`.grad = None`: `set_to_none=False` is not honoured for them -- a zeroed view that stays attached would make autograd
        add every new gradient into it with a kernel of its own; the reducer moves fresh gradients into the bucket instead)."""
        bucketed, plain = {}, []
        for group in self.param_groups:
            for p in group["params"]:
                ref = getattr(p, "_lvt_reducer", None)
                red = ref() if ref is not None else None
                if red is not None and red.active:
                    bucketed.setdefault(id(red), (red, set()))[1].add(p)
                else:
                    plain.append(p)
        for red, ps in bucketed.values():
            red.zero_grad(only=ps)
        for p in plain:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    def _collect(self, make_state):
        """-> dict step_count -> list of (p, grad, s0, s1, lr, wd)."""
        by_step = {}
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise L.LvtError("fused optimizers need parameters on a MI355X; there is no CPU path")
                g = p.grad
                if g.is_sparse or not g.is_contiguous() or not p.is_contiguous():
                    raise L.LvtError("fused optimizers need dense contiguous parameters and gradients")
                st = self.state[p]
                if len(st) == 0:
                    make_state(st, p, group)
                if self._ema is not None and "ema" not in st:
                    st["ema"] = self._new_shadow(p)
                st["step"] += 1
                by_step.setdefault(int(st["step"]), []).append((p, g, st, group))
        return by_step


class FusedAdam(_FusedBase):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None

        def make(st, p, group):
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        clip, w, launched = self._take_clip(), self._ema_weight(), False
        for step, items in self._collect(make).items():
            # groups may differ in betas/eps in principle; batch by (betas, eps)
            batches, shadows = {}, {}
            for p, g, st, group in items:
                key = (group["betas"], group["eps"])
                batches.setdefault(key, []).append((p, g, st["exp_avg"], st["exp_avg_sq"], group["lr"],
                                                    group["weight_decay"]))
                if w is not None:
                    shadows.setdefault(key, []).append(st.get("ema"))
            for (betas, eps), ents in batches.items():
                arr = _entries(ents)
                launched = True
                if w is not None:
                    record, clamp = clip if clip is not None else (None, 0.0)
                    L.check(L.lib().lvt_adam_step_ema(arr, _shadows(shadows[(betas, eps)], ents), len(ents), betas[0], betas[1],
                                                      eps, step, w, L.ptr(record), clamp, L.stream_ptr()), "lvt_adam_step_ema")
                elif clip is None:
                    L.check(L.lib().lvt_adam_step(arr, len(ents), betas[0], betas[1], eps, step, L.stream_ptr()),
                            "lvt_adam_step")
                else:
                    L.check(L.lib().lvt_adam_step_scaled(arr, len(ents), betas[0], betas[1], eps, step, L.ptr(clip[0]),
                                                         clip[1], L.stream_ptr()), "lvt_adam_step_scaled")
        if w is not None and launched:
            self.ema_updates += 1
        L.bump_epoch()          # parameters were rewritten through raw pointers: cached max |.| records are stale
        return loss


class FusedRMSprop(_FusedBase):
    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum,
                                      centered=False))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None

        def make(st, p, group):
            st["step"] = 0
            st["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if group["momentum"] > 0:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        clip, w, launched = self._take_clip(), self._ema_weight(), False
        for step, items in self._collect(make).items():
            batches, shadows = {}, {}
            for p, g, st, group in items:
                key = (group["alpha"], group["eps"], group["momentum"])
                batches.setdefault(key, []).append((p, g, st["square_avg"], st.get("momentum_buffer"), group["lr"],
                                                    group["weight_decay"]))
                if w is not None:
                    shadows.setdefault(key, []).append(st.get("ema"))
            for (alpha, eps, mom), ents in batches.items():
                arr = _entries(ents)
                launched = True
                if w is not None:
                    record, clamp = clip if clip is not None else (None, 0.0)
                    L.check(L.lib().lvt_rmsprop_step_ema(arr, _shadows(shadows[(alpha, eps, mom)], ents), len(ents), alpha, eps,
                                                         mom, w, L.ptr(record), clamp, L.stream_ptr()), "lvt_rmsprop_step_ema")
                elif clip is None:
                    L.check(L.lib().lvt_rmsprop_step(arr, len(ents), alpha, eps, mom, L.stream_ptr()), "lvt_rmsprop_step")
                else:
                    L.check(L.lib().lvt_rmsprop_step_scaled(arr, len(ents), alpha, eps, mom, L.ptr(clip[0]), clip[1],
                                                            L.stream_ptr()), "lvt_rmsprop_step_scaled")
        if w is not None and launched:
            self.ema_updates += 1
        L.bump_epoch()
        return loss
