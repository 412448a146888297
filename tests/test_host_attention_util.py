"""CPU checks of tests/util_attention.py: the bf16x3 split the plane-kernel tests build their operands with is exact for the
draws they use (so the fp64 reference may take the fp32 operands as they are), and it is the split they claim it is."""
import pytest
import torch

from util_attention import DA, S, bf16x3_split, rand, reference, split_restores


@pytest.mark.parametrize("scale", [1.0, 3.0, 0.5, 0.25, 8.0, 16.0])
def test_bf16x3_split_restores_the_operand(scale):
    x = rand(2 * S, 4 * DA, seed=7) * scale
    x[5] = 0                                                      # the zero rows of the zero-row tests
    p = bf16x3_split(x)
    assert p.dtype == torch.bfloat16 and p.shape == (3,) + x.shape
    assert split_restores(x, p)
    p1 = x.to(torch.bfloat16)
    p2 = (x - p1.float()).to(torch.bfloat16)
    assert torch.equal(p[0], p1) and torch.equal(p[1], p2)
    assert torch.equal(p[2].float(), x - p1.float() - p2.float())  # the third plane is the remainder itself, not a rounding of it


def test_split_restores_notices_a_lossy_split():
    x = torch.tensor([1.0 + 2.0 ** -9 + 2.0 ** -23])               # one bit in each plane
    p = bf16x3_split(x)
    assert split_restores(x, p) and bool((p != 0).all())
    for pl in range(3):
        bad = p.clone()
        bad[pl, 0] = 0
        assert not split_restores(x, bad)


def test_reference_returns_the_attention_matrix():
    B, H, blk = 1, 2, (4, 8, 8)
    q, k, v, go = (rand(B * S, H * DA, seed=s) for s in (1, 2, 3, 4))
    banks = [rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    out = reference(q, k, v, go, banks, blk, True)
    assert len(out) == 10
    o, P = out[0], out[9]
    assert P.shape == (B, H, S, S) and float(P.triu(1).abs().max()) == 0.0
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    vh = v.double().view(B, S, H, DA).permute(0, 2, 1, 3)
    assert torch.allclose((P @ vh).permute(0, 2, 1, 3).reshape(B * S, H * DA), o, rtol=0, atol=1e-12)
