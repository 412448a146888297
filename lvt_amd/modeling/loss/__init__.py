"""Training losses of the auto-encoders (`PixelLoss`: L1 / L2 reconstruction term; `ReconstructionLoss`: that term plus the
optional SSIM term, LOSS.SSIM.LAMBDA)."""
from . import loss as _impl

PixelLoss = _impl.PixelLoss
ReconstructionLoss = _impl.ReconstructionLoss

__all__ = ("PixelLoss", "ReconstructionLoss")
