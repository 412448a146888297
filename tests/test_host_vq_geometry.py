"""Codebook geometry accepted by the quantiser modules (no GPU needed): every supported (NUM, SIZE, DIM) constructs with the
reference's state_dict keys and shapes, everything else is refused at construction with a message naming the supported set."""
import pytest

from lvt_amd.modeling.vq import DVQEmbedding, SingleVQEmbedding


@pytest.mark.parametrize("num,K,D", [(8, 1024, 256), (2, 256, 256), (4, 2048, 256), (16, 64, 256), (1, 256, 256), (1, 64, 48)])
def test_dvq_supported_geometries_construct(num, K, D):
    m = DVQEmbedding(num, K, D, True)
    sd = m.state_dict()
    assert sorted(sd) == sorted("ve.%d.%s" % (i, k) for i in range(num) for k in ("embedding.weight", "running_size", "running_sum"))
    assert tuple(sd["ve.0.embedding.weight"].shape) == (K, D // num)
    assert tuple(sd["ve.%d.running_size" % (num - 1)].shape) == (K,)


@pytest.mark.parametrize("K", [64, 1024, 2048])
def test_single_supported_sizes_construct(K):
    m = SingleVQEmbedding(K, 256, True)
    assert sorted(m.state_dict()) == ["embedding.weight", "running_size", "running_sum"]
    assert tuple(m.embedding.weight.shape) == (K, 256)


@pytest.mark.parametrize("ctor", [
    lambda: DVQEmbedding(8, 512, 192, True),          # Dg = 24
    lambda: DVQEmbedding(1, 512, 320, True),          # Dg = 320 > 256 (a multiple of 64: NUM == 1 here is still a product
    lambda: DVQEmbedding(1, 256, 512, True),          # quantiser, its kernels see DIM-wide sub-vectors)
    lambda: DVQEmbedding(2, 512, 640, True),          # Dg = 320
    lambda: DVQEmbedding(4, 100, 256, True),          # K = 100
    lambda: DVQEmbedding(4, 4096, 256, True),         # K = 4096
    lambda: SingleVQEmbedding(100, 256, True),
    lambda: SingleVQEmbedding(4096, 256, True),
    lambda: SingleVQEmbedding(512, 96, True),         # NUM == 1 keeps its 64-d group route
])
def test_unsupported_geometries_refused(ctor):
    with pytest.raises(NotImplementedError, match="multiple of 64 from 64 to 2048"):
        ctor()
