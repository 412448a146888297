"""The reference of tests/test_gpu_conv_matrix.py checked on the CPU: `util_conv.conv_ref` against torch's own padded convolutions,
its fp32 evaluation against the tolerance the GPU kernels are held to (so the bound is known to be met by a plain fp32 convolution),
and the bookkeeping of the cell table."""
import pytest
import torch
import torch.nn.functional as F

import util_conv as U


@pytest.fixture(scope="module")
def cell_bounds():
    cache = {}

    def get(c):
        if c.name not in cache:
            x, w, dy = U.operands(c)
            cache[c.name] = (x, w, dy, U.bounds(c, x, w, dy))
        return cache[c.name]
    return get


@pytest.mark.parametrize("c", U.CELLS, ids=repr)
def test_conv_ref_equals_torch_padding(c):
    """Where the geometry is symmetric, conv_ref in fp64 is F.conv3d with padding= (and F.conv2d for the T = 1 cells)."""
    if not c.symmetric:
        assert c.name == "v3x5x6_causal_12to132"            # the one cell whose pads only torch's F.pad can express
        return
    x, w, _ = U.operands(c)
    y = U.conv_ref(x, w, c.kernel, c.stride, c.pad, c.out)
    y3 = F.conv3d(x.double(), w.double(), stride=c.stride, padding=c.pad)
    assert y.shape == y3.shape
    assert float((y - y3).abs().max()) <= 1e-13 * float(y3.abs().max())
    if c.ins[0] == 1 and c.kernel[0] == 1:
        y2 = F.conv2d(x.double()[:, :, 0], w.double()[:, :, 0], stride=c.stride[1:], padding=c.pad[1:])
        assert float((y[:, :, 0] - y2).abs().max()) <= 1e-13 * float(y2.abs().max())


def test_causal_cell_is_a_front_padded_convolution():
    """The asymmetric cell against an explicit construction: zeros in front of t and h, one column on either side of w."""
    c = U.CELL["v3x5x6_causal_12to132"]
    assert U.back_pads(c.ins, c.kernel, c.stride, c.pad, c.out) == (0, 0, 1)
    x, w, _ = U.operands(c)
    xp = torch.zeros(c.N, c.ci_real, 3 + 2, 5 + 2, 6 + 2, dtype=torch.float64)
    xp[:, :, 2:, 2:, 1:7] = x.double()
    assert torch.equal(U.conv_ref(x, w, c.kernel, c.stride, c.pad, c.out), F.conv3d(xp, w.double()))


def test_negative_back_pad_crops():
    """out= smaller than the input allows: the rows no window reaches are cropped, and get a zero gradient."""
    g = torch.Generator().manual_seed(3)
    x, w = U.rand((1, 2, 1, 7, 7), g), U.rand((3, 2, 1, 4, 4), g)
    out = (1, 2, 2)                                          # k4 s2 p0 on 7x7: (2 - 1) 2 + 4 - 7 = -1
    assert U.back_pads((1, 7, 7), (1, 4, 4), (1, 2, 2), (0, 0, 0), out) == (0, -1, -1)
    y = U.conv_ref(x, w, (1, 4, 4), (1, 2, 2), (0, 0, 0), out)
    assert torch.equal(y, F.conv3d(x.double(), w.double(), stride=(1, 2, 2)))
    xr = x.double().requires_grad_(True)
    U.conv_ref(xr, w, (1, 4, 4), (1, 2, 2), (0, 0, 0), out).sum().backward()
    assert not bool(xr.grad[..., 6, :].any()) and not bool(xr.grad[..., :, 6].any()) and bool(xr.grad[..., :6, :6].all())


@pytest.mark.parametrize("c", U.CELLS, ids=repr)
def test_fp32_reference_meets_the_bound(c, cell_bounds):
    """An fp32 evaluation of conv_ref stays inside |.| <= 1e-5 mag + 2^-21 |ref| for y, dx, dw (and db inside 1e-5 sum |dy|): the
    bound of the GPU matrix is met by a plain fp32 convolution with room to spare (a draft cell list measured a worst ratio of
    0.031)."""
    x, w, dy, b = cell_bounds(c)
    y, dx, dw, db = U.passes(c, x, w, dy, torch.float32)
    worst = 0.0
    for name, got in (("y", y), ("dx", dx), ("dw", dw)):
        ratio = float(((got.double() - b[name]).abs() / U.tol(b["mag_" + name], b[name]).clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    ratio = float(((db.double() - b["db"]).abs() / (U.EPS_ACC * b["mag_db"])).max())
    assert ratio <= 1.0, ("db", ratio)
    print("%s: worst error / bound of the fp32 reference %.3f" % (c.name, max(worst, ratio)))


@pytest.mark.parametrize("c", U.CELLS, ids=repr)
def test_magnitudes_bound_the_results(c, cell_bounds):
    """|y| <= sum |x||w| and so on, element by element, and the magnitudes have the shapes of the results."""
    _, _, _, b = cell_bounds(c)
    for name in ("y", "dx", "dw", "db"):
        assert b[name].shape == b["mag_" + name].shape
        assert bool((b[name].abs() <= b["mag_" + name] * (1 + 1e-12)).all()), name
    assert b["y"].shape == (c.N, c.co_real) + c.out and b["dx"].shape == (c.N, c.ci_real) + c.ins
    assert b["dw"].shape == (c.co_real, c.ci_real) + c.kernel and b["db"].shape == (c.co_real,)


def test_cell_table_bookkeeping():
    """Positive output extents, device channel counts that are multiples of 4 and hold the real ones, no cell above 2048 output
    positions, and the recorded preconditions of lvt_conv3d_bwd_data (K % s == 0, in % s == 0): every cell of the table meets them
    (the geometries that do not are the refusals of the GPU file)."""
    for c in U.CELLS:
        assert all(o > 0 for o in c.out), c
        assert c.ci % 4 == 0 and c.co % 4 == 0 and c.ci - 4 < c.ci_real <= c.ci and c.co - 4 < c.co_real <= c.co, c
        assert c.pix <= U.MAX_PIX, c
        assert c.bwd_data_ok == all(k % s == 0 and i % s == 0 for k, s, i in zip(c.kernel, c.stride, c.ins))
        assert c.bwd_data_ok, c
    assert not U.ConvCell("k3s2", (1, 1, 8, 8), 12, 12, (1, 3, 3), (1, 2, 2), (0, 1, 1)).bwd_data_ok
    assert not U.ConvCell("h7s2", (1, 1, 7, 8), 12, 12, (1, 4, 4), (1, 2, 2), (0, 1, 1)).bwd_data_ok
    assert sum(c.near_miss for c in U.CELLS) == 7
    assert sum(not c.symmetric for c in U.CELLS) == 1


def test_layout_helpers_round_trip():
    g = torch.Generator().manual_seed(5)
    x = U.rand((2, 3, 2, 5, 7), g)
    cl = U.to_cl(x)
    assert cl.shape == (2, 2, 5, 7, 4) and not bool(cl[..., 3].any())
    assert torch.equal(U.from_cl(cl, 3), x)
    fill = torch.full((2, 2, 5, 7, 8), 9.0)
    cl8 = U.to_cl(x, 8, fill=fill)
    assert bool((cl8[..., 3:] == 9.0).all()) and torch.equal(U.from_cl(cl8, 3), x)


def test_epilogue64_order():
    v = torch.tensor([[-2.0, -1.0, 1.0, 3.0]], dtype=torch.float64)
    bias = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    res = torch.tensor([[0.0, 0.5, 0.0, 0.0]], dtype=torch.float64)
    mask = torch.tensor([[1.0, 1.0, 0.0, -1.0]], dtype=torch.float64)
    e = U.epilogue64
    assert e(v, U.EPI_BIAS | U.EPI_RESIDUAL | U.EPI_RELU | U.EPI_MASK, bias, res, mask).tolist() == [[0.0, 0.0, 0.0, 0.0]]
    assert e(v, U.EPI_BIAS | U.EPI_RESIDUAL | U.EPI_MASK, bias, res, mask).tolist() == [[-1.0, -0.5, 0.0, 0.0]]
    assert e(v, U.EPI_LEAKY).tolist() == [[-0.4, -0.2, 1.0, 3.0]]
    assert e(v, U.EPI_MASK | U.EPI_LEAKY_MASK, mask=mask)[0, 2:].tolist() == pytest.approx([0.2, 0.6])
    s = e(v, U.EPI_SIGMOID, npad=3)
    assert s[0, 1:].tolist() == [0.0, 0.0, 0.0] and float(s[0, 0]) == pytest.approx(1 / (1 + 2.718281828459045 ** 2))
