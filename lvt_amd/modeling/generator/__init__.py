"""Generators (decoder networks): registry / factory, abstract base, residual ConvTranspose decoder of the VQ-VAE, its sub-pixel
variant (3x3 convolutions + PixelShuffle), plain conv decoder (3x3 convolutions, LeakyReLU, nearest upsamples)."""
from . import build as _build
from . import generator as _base
from . import convdecoder as _conv
from . import resdecoder as _res

GENERATOR_REGISTRY, build_generator = _build.GENERATOR_REGISTRY, _build.build_generator
Generator = _base.Generator
ResDecoder = _res.ResDecoder
ResShuffleDecoder = _res.ResShuffleDecoder
ConvDecoder = _conv.ConvDecoder

__all__ = ("GENERATOR_REGISTRY", "build_generator", "Generator", "ResDecoder", "ResShuffleDecoder", "ConvDecoder")
