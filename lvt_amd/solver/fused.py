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
    """`step()` and everything around it.  An optimizer supplies `_entry` (the name of its plain C entry point; `_scaled` and
    `_ema` are appended), `_make_state(st, p, group)`, `_batch_item(st, group)` -> (hyper-parameter key, s0, s1) -- the one
    call `step()` makes per parameter -- and `_hyper(key, step)` -> the arguments between the table and the clip."""
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

    def _collect(self):
        """-> {step count: {hyper-parameter key: ([(p, grad, s0, s1, lr, wd)], [shadow])}}: the launches of a `step()`, both
        levels in first-seen order; the shadows only while averaging is on.  This loop is the host cost of a step (269 tensors
        for DSFVT): one hook call per parameter, no second pass."""
        by_step, state, averaging, batch_item = {}, self.state, self._ema is not None, self._batch_item
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda:
                    raise L.LvtError("fused optimizers need parameters on a MI355X; there is no CPU path")
                if g.is_sparse or not g.is_contiguous() or not p.is_contiguous():
                    raise L.LvtError("fused optimizers need dense contiguous parameters and gradients")
                st = state[p]
                if len(st) == 0:
                    st["step"] = 0
                    self._make_state(st, p, group)
                if averaging and "ema" not in st:
                    st["ema"] = self._new_shadow(p)
                st["step"] += 1
                key, s0, s1 = batch_item(st, group)
                step = int(st["step"])
                batches = by_step.get(step)
                if batches is None:
                    batches = by_step[step] = {}
                batch = batches.get(key)
                if batch is None:
                    batch = batches[key] = ([], [])
                batch[0].append((p, g, s0, s1, group["lr"], group["weight_decay"]))
                if averaging:
                    batch[1].append(st["ema"])
        return by_step

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        clip, w, launched = self._take_clip(), self._ema_weight(), False
        for step, batches in self._collect().items():
            for key, (ents, shadows) in batches.items():
                arr, n, hyper = _entries(ents), len(ents), self._hyper(key, step)
                launched = True
                if w is not None:
                    record, clamp = clip if clip is not None else (None, 0.0)
                    name, args = self._entry + "_ema", (arr, _shadows(shadows, ents), n) + hyper + (w, L.ptr(record), clamp)
                elif clip is None:
                    name, args = self._entry, (arr, n) + hyper
                else:
                    name, args = self._entry + "_scaled", (arr, n) + hyper + (L.ptr(clip[0]), clip[1])
                L.check(getattr(L.lib(), name)(*args, L.stream_ptr()), name)
        if w is not None and launched:
            self.ema_updates += 1
        L.bump_epoch()          # parameters were rewritten through raw pointers: cached max |.| records are stale
        return loss


def walk_parameters(optimizers):
    """(optimizer, group, parameter) in optimizer, group and parameter order; a parameter that appears twice is yielded once."""
    seen = set()
    for opt in optimizers:
        for group in opt.param_groups:
            for p in group["params"]:
                if id(p) not in seen:
                    seen.add(id(p))
                    yield opt, group, p


def require_fused(optimizers, message):
    """What lives in the step kernels has no other home: `message` (with one %s for the class name) for any other optimizer."""
    for opt in optimizers:
        if not isinstance(opt, _FusedBase):
            raise L.LvtError(message % type(opt).__name__)


class FusedAdam(_FusedBase):
    _entry = "lvt_adam_step"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _make_state(self, st, p, group):
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _batch_item(self, st, group):
        # groups may differ in betas/eps in principle; batch by (betas, eps)
        return (group["betas"], group["eps"]), st["exp_avg"], st["exp_avg_sq"]

    def _hyper(self, key, step):
        (beta1, beta2), eps = key
        return beta1, beta2, eps, step


class FusedRMSprop(_FusedBase):
    _entry = "lvt_rmsprop_step"

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum,
                                      centered=False))

    def _make_state(self, st, p, group):
        st["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if group["momentum"] > 0:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _batch_item(self, st, group):
        return (group["alpha"], group["eps"], group["momentum"]), st["square_avg"], st.get("momentum_buffer")

    def _hyper(self, key, step):
        return key                          # (alpha, eps, momentum): RMSprop does not read the step count
