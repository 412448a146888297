"""Vector quantisation: one wide codebook (`SingleVQEmbedding`) and the product quantiser over channel groups
(`DVQEmbedding`), both `CodebookQuantiser`s over `VQEmbedding` containers and backed by the HIP nearest / gather / EMA kernels; and
the finite scalar quantiser (`FSQEmbedding`), whose codebook is implicit."""
from .fsq_embedding import FSQEmbedding
from .vq_embedding import DVQEmbedding, SingleVQEmbedding, VQEmbedding

__all__ = ("VQEmbedding", "DVQEmbedding", "SingleVQEmbedding", "FSQEmbedding")
