"""Polyak-averaged weights (SOLVER.MODEL_EMA): an exponential moving average of every parameter the fused optimizers step.

The average costs no pass of its own.  `FusedAdam / FusedRMSprop.enable_ema(decay, warmup)` gives every parameter a shadow
`state[p]["ema"]`, and the step kernels (lvt_adam_step_ema / lvt_rmsprop_step_ema) apply e += (1 - d_t) (p_new - e) while they
hold the new parameter value in a register: the `lerp_` form of torch.optim.swa_utils.get_ema_multi_avg_fn, with
d_t = ema_decay_at(t, decay, warmup).  A step that the gradient clipper skips leaves the shadows alone as well, but still
counts as an update on the host (the wart Adam's bias correction has after a skipped step).

`ModelEma(optimizers).averaged()` is how the average is USED: inside the context the parameters hold the averaged values
and the shadows hold the live ones (lvt_ema_swap exchanges the contents; no pointer moves, so captured sampling graphs and
the max-|.| prefetch plan stay valid), and leaving it restores every bit.

What is averaged: the parameters the given fused optimizers step, and nothing else.  Buffers are used as they are -- BN
running statistics, EMA codebooks (which are averages already) and the restart counters; a sub-network without an optimizer
has no averaged twin.  One decay for all sub-networks.  Under data parallelism the shadows are a pure function of the reduced
gradients, so every rank holds the same bits without a collective.
"""
import contextlib
import ctypes as C
import os

import torch

from ..hip import binding as L
from .fused import check_ema_decay, ema_decay_at  # noqa: F401  (ema_decay_at: part of this module's interface)
from .fused import require_fused, walk_parameters


def ema_twin(path):
    """`.../model_0000099.pth` -> `.../model_0000099_ema.pth`: the file with the averaged weights written next to a checkpoint."""
    root, ext = os.path.splitext(path)
    return root + "_ema" + ext


class ModelEma:
    def __init__(self, optimizers, decay=0.9999, warmup=True):
        check_ema_decay(decay)
        self.optimizers = [o["optimizer"] if isinstance(o, dict) else o for o in optimizers]
        require_fused(self.optimizers,
                      "averaged weights live in the fused optimizers' step kernels; got %s (there is no CPU path)")
        self.decay, self.warmup = float(decay), bool(warmup)
        for opt in self.optimizers:
            opt.enable_ema(self.decay, self.warmup)
        self._inside = False

    @property
    def updates(self):
        return max([opt.ema_updates for opt in self.optimizers] or [0])

    def _pairs(self):
        """(parameter, shadow) of every parameter of every optimizer, shared parameters once.  A parameter that has not been
        stepped yet has no state: its average is the parameter itself, and the shadow it will start from is made here."""
        pairs = []
        for opt, _, p in walk_parameters(self.optimizers):
            st = opt.state.get(p)
            if st is not None and "ema" in st:
                e = st["ema"]
            else:
                init = opt.__dict__.setdefault("_ema_init", {})
                if p not in init:
                    init[p] = p.detach().clone(memory_format=torch.preserve_format)
                e = init[p]
            pairs.append((p, e))
        return pairs

    def shadows(self, module=None):
        """name -> shadow for the parameters of `module` that are averaged (all of them, by position, without a module)."""
        by_id = {id(p): e for p, e in self._pairs()}
        if module is None:
            return {i: e for i, e in enumerate(by_id.values())}
        return {name: by_id[id(p)] for name, p in module.named_parameters() if id(p) in by_id}

    def owns(self, module):
        """Whether any parameter of `module` is averaged (a sub-network without an optimizer has no averaged twin)."""
        return len(self.shadows(module)) > 0

    @torch.no_grad()
    def load_shadows(self, module, state_dict, updates=None):
        """Shadows of `module`'s averaged parameters <- the entries of `state_dict` (an `_ema` twin).  Returns the names that
        were restored.  `updates` restores the position in the decay schedule."""
        done = []
        for name, e in self.shadows(module).items():
            if name in state_dict:
                e.copy_(state_dict[name].to(e.device, e.dtype).reshape(e.shape))
                done.append(name)
        if updates is not None:
            for opt in self.optimizers:
                opt.ema_updates = max(opt.ema_updates, int(updates))
        return done

    @torch.no_grad()
    def reset_shadows(self, module):
        """Shadows of `module`'s averaged parameters <- the parameters (after weights were loaded into the module)."""
        by_id = {id(p): e for p, e in self._pairs()}
        for p in module.parameters():
            if id(p) in by_id:
                by_id[id(p)].copy_(p.detach())

    def _swap(self):
        pairs = self._pairs()
        if not pairs:
            return
        n = len(pairs)
        a, b, counts = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_longlong * n)()
        for i, (p, e) in enumerate(pairs):
            L.require(p, e)
            if p.dtype != torch.float32 or e.dtype != torch.float32 or e.numel() != p.numel():
                raise L.LvtError("ModelEma: parameter %d and its shadow must be float32 tensors of one size" % i)
            a[i], b[i], counts[i] = p.data_ptr(), e.data_ptr(), p.numel()
        L.check(L.lib().lvt_ema_swap(a, b, counts, n, L.stream_ptr()), "lvt_ema_swap")
        L.bump_epoch()          # parameters were rewritten through raw pointers: cached max |.| records are stale

    @contextlib.contextmanager
    def averaged(self):
        """Inside, the parameters hold the averaged weights (buffers are untouched); on the way out every bit is restored.
        Do not step an optimizer inside."""
        if self._inside:
            raise L.LvtError("ModelEma.averaged() is not re-entrant")
        self._swap()
        self._inside = True
        try:
            yield self
        finally:
            self._inside = False
            self._swap()
