"""The m-contiguous loaders of the wide (256 x 128) f16x2 GEMM against its k-contiguous (NT) form.

lvt_gemm_wide_kernel<1,1> (TN: every weight gradient) and <0,1> (NN: every data gradient) keep an operand that is contiguous
along its non-reduction index in LDS in memory order and fetch the MFMA fragments with transposing reads; <0,0> (NT) stages
k-contiguous rows and reads them with ds_read_b128.  Handed the same numbers under the same max |.| records, all three forms
build the same fp16 planes, run the same MFMAs in the same k order and reduce split-K partials in the same order: the
results must be torch.equal.  Every shape has M > 128 and K % 32 == 0, which is what sends a product to the wide kernel.
Column sums (a_colsum, TN only) are a fixed-order fp32 sum: equal from run to run, and within TOL of fp64."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5          # tests/test_gpu_engine.py


@pytest.fixture(autouse=True)
def f16x2_mode():
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    yield
    L.set_math_mode(before)


def _dev():
    return torch.device("cuda:0")


VALUES = ("uniform", "heavy_tail", "zero_tile")


def _operand(k, cols, values, seed):
    """(k, cols) fp32, cols contiguous.  heavy_tail: a few entries 2^20 times the rest (the scale comes from the max, the
    bulk lives in the low plane's range); zero_tile: the first 32 k of the first 128 columns, one staged tile, are zero
    (half of them where that tile is the whole operand); zero_all: the whole operand is zero, its max |.| record is 0
    (test_zero_operand_equals_nt only)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * k + cols)
    t = torch.rand(k, cols, generator=g) * 2 - 1
    if values == "heavy_tail":
        n = max(3, t.numel() // 4096)
        idx = torch.randint(0, t.numel(), (n,), generator=g)
        t.view(-1)[idx] *= 2.0 ** 20
    elif values == "zero_tile":
        t[:32, :128 if t.numel() > 32 * 128 else 64] = 0
    elif values == "zero_all":
        t.zero_()
    return t


def _transposed_like(t, src):
    """t^T as a k-contiguous operand that carries the SAME max |.| record as `src` (same scale, same planes)."""
    from lvt_amd.hip import binding as L
    tt = t.transpose(-1, -2).contiguous()
    return L.set_amax(tt, L.amax_of(src))


# (M, N, K, splits): one, two and three k-tiles = the three exits of the pipelined loop; ragged M and N edges alone and with
# one k-tile per split
SHAPES = [(256, 128, 32, 1), (256, 128, 64, 1), (256, 128, 96, 1), (260, 132, 96, 1), (260, 132, 96, 3)]


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("M,N,K,splits", SHAPES)
def test_tn_equals_nt(M, N, K, splits, values):
    from lvt_amd.hip import gemm as G
    d = _dev()
    x, y = _operand(K, M, values, 1).to(d), _operand(K, N, values, 2).to(d)
    got = torch.full((M, N), float("nan"), device=d)
    G.gemm(x, y, got, M, N, K, ta=1, tb=1, splits=splits)
    want = torch.full((M, N), float("nan"), device=d)
    G.gemm(_transposed_like(x, x), _transposed_like(y, y), want, M, N, K, ta=0, tb=0, splits=splits)
    assert torch.equal(got, want)


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("M,N,K,splits", SHAPES)
def test_nn_equals_nt(M, N, K, splits, values):
    from lvt_amd.hip import gemm as G
    d = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.rand(M, K, generator=g) * 2 - 1).to(d)
    y = _operand(K, N, values, 3).to(d)
    got = torch.full((M, N), float("nan"), device=d)
    G.gemm(a, y, got, M, N, K, ta=0, tb=1, splits=splits)
    want = torch.full((M, N), float("nan"), device=d)
    G.gemm(a, _transposed_like(y, y), want, M, N, K, ta=0, tb=0, splits=splits)
    assert torch.equal(got, want)


@pytest.mark.parametrize("values", VALUES)
def test_tn_splitk_with_column_sums(values):
    """Weight-gradient form: 2 x 3 output tiles, 8 k-tiles per split, the bias gradient from the same launch."""
    from lvt_amd.hip import gemm as G
    M, N, K, splits = 512, 384, 1024, 4
    d = _dev()
    xc, yc = _operand(K, M, values, 4), _operand(K, N, values, 5)
    x, y = xc.to(d), yc.to(d)
    got, cs = torch.full((M, N), float("nan"), device=d), torch.full((M,), float("nan"), device=d)
    G.gemm(x, y, got, M, N, K, ta=1, tb=1, splits=splits, a_colsum=cs)
    want = torch.full((M, N), float("nan"), device=d)
    G.gemm(_transposed_like(x, x), _transposed_like(y, y), want, M, N, K, ta=0, tb=0, splits=splits)
    assert torch.equal(got, want)
    got2, cs2 = torch.full((M, N), float("nan"), device=d), torch.full((M,), float("nan"), device=d)
    G.gemm(x, y, got2, M, N, K, ta=1, tb=1, splits=splits, a_colsum=cs2)
    assert torch.equal(got, got2) and torch.equal(cs, cs2)
    assert rel_err(cs, xc.double().sum(0)) < TOL
    assert rel_err(got, xc.double().t() @ yc.double()) < TOL


@pytest.mark.parametrize("values", VALUES)
def test_nn_packed_b_with_column_offset(values):
    """q/k/v data-gradient style: B is one (K, N) column block of a packed (K, 3 N) buffer, ldb = 3 N."""
    from lvt_amd.hip import gemm as G
    M, N, K = 384, 128, 128
    d = _dev()
    g = torch.Generator().manual_seed(9)
    a = (torch.rand(M, K, generator=g) * 2 - 1).to(d)
    packed = _operand(K, 3 * N, values, 6).to(d)
    b = packed.view(-1)[N:]                     # the wrappers take contiguous tensors: the block starts at element N, ldb = 3 N
    got = torch.full((M, N), float("nan"), device=d)
    G.gemm(a, b, got, M, N, K, ta=0, tb=1, ldb=3 * N)
    want = torch.full((M, N), float("nan"), device=d)
    G.gemm(a, _transposed_like(packed[:, N:2 * N], b), want, M, N, K, ta=0, tb=0)
    assert torch.equal(got, want)


@pytest.mark.parametrize("ta", [0, 1])
def test_batched_equals_nt(ta):
    """batch_inner = 2 with ragged edges: per-batch operand bases and output offsets."""
    from lvt_amd.hip import gemm as G
    M, N, K = 260, 132, 64
    d = _dev()
    xs = torch.stack([_operand(K, M, "uniform", 10 + i) for i in range(2)]).to(d)        # (2, K, M)
    ys = torch.stack([_operand(K, N, "heavy_tail", 20 + i) for i in range(2)]).to(d)     # (2, K, N)
    xt, yt = _transposed_like(xs, xs), _transposed_like(ys, ys)                         # (2, M, K), (2, N, K)
    a = xs if ta else xt
    got = torch.full((2, M, N), float("nan"), device=d)
    G.gemm(a, ys, got, M, N, K, ta=ta, tb=1, batch_inner=2, sA=(0, M * K), sB=(0, K * N), sC=(0, M * N))
    want = torch.full((2, M, N), float("nan"), device=d)
    G.gemm(xt, yt, want, M, N, K, ta=0, tb=0, batch_inner=2, sA=(0, M * K), sB=(0, K * N), sC=(0, M * N))
    assert torch.equal(got, want)


@pytest.mark.parametrize("zero", ["x", "y"])
@pytest.mark.parametrize("M,N,K,splits", [(256, 128, 32, 1), (260, 132, 96, 3)])
def test_zero_operand_equals_nt(M, N, K, splits, zero):
    """values = zero_all: a WHOLE operand is zero (max |.| record 0: the scale's exponent sits at its clamp, and s * 2048 of the
    split must stay finite).  TN and NN equal NT bit for bit, and the product is +0 everywhere -- not 0 * inf = NaN."""
    from lvt_amd.hip import gemm as G
    d = _dev()
    x = _operand(K, M, "zero_all" if zero == "x" else "uniform", 1).to(d)
    y = _operand(K, N, "zero_all" if zero == "y" else "uniform", 2).to(d)
    xt, yt = _transposed_like(x, x), _transposed_like(y, y)
    want = torch.full((M, N), float("nan"), device=d)
    G.gemm(xt, yt, want, M, N, K, ta=0, tb=0, splits=splits)
    tn = torch.full((M, N), float("nan"), device=d)
    G.gemm(x, y, tn, M, N, K, ta=1, tb=1, splits=splits)
    nn = torch.full((M, N), float("nan"), device=d)
    G.gemm(xt, y, nn, M, N, K, ta=0, tb=1, splits=splits)
    assert not bool(want.view(torch.int32).any())
    assert torch.equal(tn.view(torch.int32), want.view(torch.int32)) and torch.equal(nn.view(torch.int32), want.view(torch.int32))
