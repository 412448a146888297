"""Pixel loss = lambda * (mse | l1) (reference: vidgen/modeling/loss/loss.py:5-20; the shipped configs use "l2")."""
import torch
from torch import nn

from ...hip import ew


class _MseFn(torch.autograd.Function):
    """scale * mean((a - b)^2) over `denom` real elements (pads contribute exact zeros), fixed-order
    reduction; backward w.r.t. `a` only (targets are data / detached in every call site)."""

    @staticmethod
    def forward(ctx, a, b, denom, scale, l1=False):
        ctx.save_for_backward(a, b)
        ctx.denom, ctx.scale, ctx.l1 = denom, scale, l1
        return ew.mse_fwd(a, b, denom, scale, l1=l1)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return ew.mse_bwd(a, b, ctx.denom, ctx.scale, gout=g.contiguous().view(1), l1=ctx.l1), None, None, None, None


def mse(a, b, denom=None, scale=1.0):
    return _MseFn.apply(a.contiguous(), b.contiguous(), float(denom if denom is not None else a.numel()), scale)


def l1(a, b, denom=None, scale=1.0):
    """scale * mean |a - b| (F.l1_loss, loss.py:11-12)."""
    return _MseFn.apply(a.contiguous(), b.contiguous(), float(denom if denom is not None else a.numel()), scale, True)


class PixelLoss(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        mode = cfg.LOSS.PIXEL.MODE
        if mode not in ("l1", "l2"):
            raise NotImplementedError                      # (loss.py:15-16)
        self._fn = l1 if mode == "l1" else mse
        self._lambda = cfg.LOSS.PIXEL.LAMBDA

    def forward(self, input, target, denom=None):
        return self._fn(input, target, denom, self._lambda)


class _PixelSsimFn(torch.autograd.Function):
    """(scale * mean((a - b)^2 | |a - b|), lam * (1 - mean SSIM(u(a), u(b)))) of channels-last frames (N, 1, H, W, Cp): the pixel
    loss of `_MseFn` and the SSIM term (csrc/ssim_loss.hip) as two scalar outputs of one node, so that the gradient
    w.r.t. `a` leaves as ONE tensor written by one launch (lvt_mse_bwd_plus) with a valid max-|.| record.  The SSIM kernel
    writes its gradient in the forward launch, and only when a backward will follow (`want_grad`)."""

    @staticmethod
    def forward(ctx, a, b, denom, scale, l1_mode, mean, std, data_range, lam, want_grad):
        pix = ew.mse_fwd(a, b, denom, scale, l1=l1_mode)
        ssim, G = ew.ssim_loss_fwd(a, b, mean, std, data_range, lam, want_grad=want_grad)
        if want_grad:
            ctx.save_for_backward(a, b, G)
        ctx.denom, ctx.scale, ctx.l1 = denom, scale, l1_mode
        return pix, ssim

    @staticmethod
    def backward(ctx, g_pix, g_ssim):
        a, b, G = ctx.saved_tensors
        out = ew.mse_bwd(a, b, ctx.denom, ctx.scale, gout=g_pix.contiguous().view(1), l1=ctx.l1,
                         g_plus=g_ssim.contiguous().view(1), plus=G)
        return (out,) + (None,) * 9


class ReconstructionLoss(nn.Module):
    """The reconstruction loss of the auto-encoders as a dict: the pixel loss (PixelLoss's choice for the VQ-VAE, `pixel=True`; the
    plain mse of AutoEncoderModel otherwise) under `key`, and with LOSS.SSIM.LAMBDA > 0 also `loss_ssim` = LAMBDA * (1 - mean
    SSIM) of the de-normalised frames.  With LAMBDA == 0 it calls exactly what was called before the term
    existed."""

    def __init__(self, cfg, pixel=True):
        super().__init__()
        lam = cfg.LOSS.SSIM.LAMBDA
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= float(lam) < float("inf"):
            raise ValueError("LOSS.SSIM.LAMBDA must be a non-negative finite number (0.0: off), got %r" % (lam,))
        self.ssim_lambda = float(lam)
        self.pixel_loss = PixelLoss(cfg) if pixel else None
        self.data_range = 1.0 if cfg.INPUT.SCALE_TO_ZEROONE else 255.0
        self._mean_std = (tuple(cfg.MODEL.PIXEL_MEAN), tuple(cfg.MODEL.PIXEL_STD))
        self._dev = {}             # device -> (mean, std) float32 tensors; plain attributes: the checkpoint layout does not change

    def _tables(self, device):
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(torch.tensor(v, dtype=torch.float32, device=device) for v in self._mean_std)
        return t

    def forward(self, input, target, denom=None, key="loss_reconstruction"):
        if self.ssim_lambda == 0.0:
            if self.pixel_loss is not None:
                return {key: self.pixel_loss(input, target, denom=denom)}
            return {key: mse(input, target, denom=denom)}
        if self.pixel_loss is not None:
            scale, l1_mode = self.pixel_loss._lambda, self.pixel_loss._fn is l1
        else:
            scale, l1_mode = 1.0, False
        mean, std = self._tables(input.device)
        want = torch.is_grad_enabled() and input.requires_grad
        pix, ssim = _PixelSsimFn.apply(input.contiguous(), target.contiguous(), float(denom if denom is not None else input.numel()),
                                       scale, l1_mode, mean, std, self.data_range, self.ssim_lambda, want)
        return {key: pix, "loss_ssim": ssim}
