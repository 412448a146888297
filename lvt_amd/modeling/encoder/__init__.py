"""Encoders: the registry / factory pair, the abstract base, the residual conv encoder of the VQ-VAE and the plain
conv encoder (3x3 convolutions, LeakyReLU, average pools)."""
from . import build as _build
from . import encoder as _base
from . import convencoder as _conv
from . import resencoder as _res

ENCODER_REGISTRY, build_encoder = _build.ENCODER_REGISTRY, _build.build_encoder
Encoder = _base.Encoder
ResEncoder = _res.ResEncoder
ConvEncoder = _conv.ConvEncoder

__all__ = ("ENCODER_REGISTRY", "build_encoder", "Encoder", "ResEncoder", "ConvEncoder")
