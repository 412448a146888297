"""Gradient clipping for the fused optimizers (detectron2's SOLVER.CLIP_GRADIENTS, which the reference dropped).

`GradClipper.prepare()` runs between the backward and the optimizers' `step()`:

  * "norm": the 2-norm over the gradients of EVERY parameter of EVERY optimizer it was given (lvt_grad_sqnorm: fp64 partials
    per 16K-element chunk; lvt_grad_clip_coef: one workgroup that adds them in a fixed order) becomes a 16-byte device record
    (norm, coef = min(1, max_norm / (norm + 1e-6)), skip).  The step kernels multiply every gradient by `coef` on the way in,
    the rule of torch.nn.utils.clip_grad_norm_; a norm that is not finite sets `skip`, and the step then stores nothing.
  * "value": no norm pass; the step kernels clamp every gradient element to [-c, c] (torch.nn.utils.clip_grad_value_).
    Non-finite gradients are not detected in this mode.

Nothing is read back: `norm`, `coef`, `skip` and `skipped` (steps skipped so far) are device tensors.  `p.grad` keeps the
unclipped gradient.  The step count of a skipped step still advances (`state["step"]` lives on the host).
"""
import torch

from ..hip import binding as L
from .fused import require_fused, walk_parameters

CLIP_TYPES = ("norm", "value")


def check_clip_args(clip_type, clip_value, norm_type):
    if clip_type not in CLIP_TYPES:
        raise ValueError("Unknown gradient clip type: {} (one of {})".format(clip_type, CLIP_TYPES))
    if float(norm_type) != 2.0:
        raise ValueError("gradient clipping is built for NORM_TYPE 2.0 only (got {})".format(norm_type))
    if not 0.0 < float(clip_value) < float("inf"):
        raise ValueError("CLIP_VALUE must be positive and finite (got {})".format(clip_value))


class GradClipper:
    def __init__(self, optimizers, clip_type="norm", clip_value=1.0, norm_type=2.0):
        check_clip_args(clip_type, clip_value, norm_type)
        self.optimizers = list(optimizers)
        require_fused(self.optimizers,
                      "gradient clipping lives in the fused optimizers' step kernels; got %s (there is no CPU path)")
        self.clip_type, self.clip_value = clip_type, float(clip_value)
        self.record = self.norm = self.coef = self.skip = self.skipped = None        # device tensors, made by the first prepare()

    def _gradients(self):
        """Gradients of all parameters in optimizer, group and parameter order; shared parameters once, absent gradients left out."""
        grads = []
        for _, _, p in walk_parameters(self.optimizers):
            g = p.grad
            if g is None:
                continue
            if not g.is_cuda:
                raise L.LvtError("gradient clipping needs gradients on a MI355X; there is no CPU path")
            if g.is_sparse or not g.is_contiguous() or g.dtype != torch.float32:
                raise L.LvtError("gradient clipping needs dense contiguous float32 gradients")
            grads.append(g)
        return grads

    def _state(self, device):
        if self.record is None or self.record.device != device:
            self.record = torch.zeros(4, dtype=torch.float32, device=device)          # lvt_clip_record
            self.norm, self.coef = self.record[0], self.record[1]
            self.skip = self.record.view(torch.int32)[2]
            self.skipped = torch.zeros((), dtype=torch.int64, device=device)

    @torch.no_grad()
    def prepare(self):
        """Hand the next `step()` of every optimizer its clip.  Call after the backward (and after the data-parallel join:
        every rank then holds the same reduced gradients and computes the same record, no collective of its own)."""
        if self.clip_type == "value":
            for opt in self.optimizers:
                opt.set_grad_clip(None, self.clip_value)
            return
        grads = self._gradients()
        if not grads:
            return                                  # nothing will step
        self._state(grads[0].device)
        arr = (L.GradEntry * len(grads))()
        for e, g in zip(arr, grads):
            e.g, e.n = g.data_ptr(), g.numel()
        lib = L.lib()
        chunks = lib.lvt_grad_sqnorm_partials(arr, len(grads))
        if chunks <= 0:
            raise L.LvtError("lvt_grad_sqnorm_partials: bad gradient entry")
        partials = L.workspace(8 * chunks, self.record.device, "clip")
        stream = L.stream_ptr()
        L.check(lib.lvt_grad_sqnorm(arr, len(grads), L.ptr(partials), chunks, stream), "lvt_grad_sqnorm")
        L.check(lib.lvt_grad_clip_coef(L.ptr(partials), chunks, self.clip_value, L.ptr(self.record), L.ptr(self.skipped),
                                       stream), "lvt_grad_clip_coef")
        for opt in self.optimizers:
            opt.set_grad_clip(self.record, 0.0)
