"""Vector quantisation: one codebook (`VQEmbedding`) and the product quantiser over channel groups
(`DVQEmbedding`), both backed by the HIP nearest / gather / EMA kernels; and the finite scalar quantiser (`FSQEmbedding`),
whose codebook is implicit."""
from . import vq_embedding as _impl
from .fsq_embedding import FSQEmbedding

VQEmbedding = _impl.VQEmbedding
DVQEmbedding = _impl.DVQEmbedding
SingleVQEmbedding = _impl.SingleVQEmbedding

__all__ = ("VQEmbedding", "DVQEmbedding", "SingleVQEmbedding", "FSQEmbedding")
