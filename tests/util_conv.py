"""fp64 reference of the convolution entry points (lvt_conv3d_fwd / _bwd_data / _bwd_weight, lvt_amd/csrc/gemm_engine.hip) and the
cell table shared by tests/test_host_conv_reference.py (CPU) and tests/test_gpu_conv_matrix.py (GPU).  No GPU needed to import.

`conv_ref` gives `pad` and `out=` the meaning `gemm.conv_geom` gives them: `pad` is the FRONT padding per dimension and the output
extents are whatever the caller says, so the back padding follows as (out - 1) s + k - in - front -- zero rows where it is
positive, input rows that no window reaches (cropped) where it is negative.  Everything else is one plain F.conv3d.

`bounds` returns, per element, the fp64 results of the three passes and the magnitudes the tolerance of the matrix is made of:
the same function on absolute values (sum |x||w| for y) and autograd on absolute operands (sum |dy||w| for dx, sum |x||dy| for dw).

The tolerance (`tol`), per element: |got - ref64| <= EPS_ACC mag + EPS_EPI (|bias| + |res| + |ref64|), EPS_ACC = 1e-5 and
EPS_EPI = 2^-21 as in tests/test_gpu_gemm_matrix.py; 1e-5 sum |a||b| is also the ceiling tests/test_gpu_envelope.py::_judge
holds the convolution kernels to in f16x2."""
import torch
import torch.nn.functional as F

EPS_ACC, EPS_EPI = 1e-5, 2.0 ** -21
LEAKY_SLOPE = 0.2


def pad4(c):
    return (c + 3) // 4 * 4


def out_extents(ins, kernel, stride, pad):
    """Output extents of a symmetric-padded convolution (the default of gemm.conv_geom)."""
    return tuple((i + 2 * p - k) // s + 1 for i, p, k, s in zip(ins, pad, kernel, stride))


def back_pads(ins, kernel, stride, front_pad, out):
    return tuple((o - 1) * s + k - i - f for i, k, s, f, o in zip(ins, kernel, stride, front_pad, out))


def conv_ref(x, w, kernel, stride, front_pad, out, dtype=torch.float64):
    """y (N, Co, To, Ho, Wo) of x (N, Ci, Ti, Hi, Wi) and w (Co, Ci, Kt, Kh, Kw) in `dtype`."""
    x, w = x.to(dtype), w.to(dtype)
    assert tuple(w.shape[2:]) == tuple(kernel) and x.shape[1] == w.shape[1]
    back = back_pads(x.shape[2:], kernel, stride, front_pad, out)
    # F.pad takes (W front, W back, H front, H back, T front, T back); a negative amount crops
    xp = F.pad(x, (front_pad[2], back[2], front_pad[1], back[1], front_pad[0], back[0]))
    y = F.conv3d(xp, w, stride=tuple(stride))
    assert tuple(y.shape[2:]) == tuple(out), (tuple(y.shape), out)
    return y


# ---- layouts ---------------------------------------------------------------------------------------------------------
def to_cl(x, cpad=None, fill=None):
    """(N, C, T, H, W) -> channels-last (N, T, H, W, Cpad); the pad channels are 0, or `fill` (a tensor of the padded shape)."""
    n, c, t, h, w = x.shape
    cpad = cpad or pad4(c)
    out = torch.zeros(n, t, h, w, cpad, dtype=x.dtype) if fill is None else fill.clone().to(x.dtype)
    assert tuple(out.shape) == (n, t, h, w, cpad)
    out[..., :c] = x.permute(0, 2, 3, 4, 1)
    return out


def from_cl(y, c):
    """Channels-last (N, T, H, W, Cpad) -> (N, C, T, H, W) of the first c channels."""
    return y[..., :c].permute(0, 4, 1, 2, 3).contiguous()


# ---- cells -----------------------------------------------------------------------------------------------------------
class ConvCell:
    """One geometry.  ci / co: the channel counts of the device buffers (multiples of 4); ci_real / co_real: those of the torch
    weight.  pad: front pads; out: output extents (None: the symmetric-padding default)."""

    def __init__(self, name, nthw, ci, co, kernel, stride, pad, out=None, ci_real=None, co_real=None, near_miss=False):
        self.name, self.N = name, nthw[0]
        self.ins = tuple(nthw[1:])
        self.ci, self.co = ci, co
        self.ci_real, self.co_real = ci_real or ci, co_real or co
        self.kernel, self.stride, self.pad = tuple(kernel), tuple(stride), tuple(pad)
        self.out = tuple(out) if out is not None else out_extents(self.ins, kernel, stride, pad)
        self.near_miss = near_miss

    def __repr__(self):
        return self.name

    @property
    def symmetric(self):
        """The geometry is F.conv3d's `padding=`: equal pads on both sides, or only unreached rows behind."""
        return self.out == out_extents(self.ins, self.kernel, self.stride, self.pad)

    @property
    def bwd_data_ok(self):
        """Preconditions of lvt_conv3d_bwd_data: K % s == 0 and in % s == 0 in every dimension."""
        return all(k % s == 0 and i % s == 0 for k, s, i in zip(self.kernel, self.stride, self.ins))

    @property
    def pix(self):
        return self.N * self.out[0] * self.out[1] * self.out[2]

    def with_real(self, ci_real=None, co_real=None):
        return ConvCell(self.name, (self.N,) + self.ins, self.ci, self.co, self.kernel, self.stride, self.pad, self.out,
                        ci_real or self.ci_real, co_real or self.co_real, self.near_miss)


def _cells():
    k133, k144, s1, s122, p011, p0 = (1, 3, 3), (1, 4, 4), (1, 1, 1), (1, 2, 2), (0, 1, 1), (0, 0, 0)
    c = []
    # ragged 2-D: K = taps Ci = 36 (K % 32 != 0), odd non-square extents, M = 105 output positions
    c.append(ConvCell("r7x5_3to128", (3, 1, 7, 5), 4, 128, k133, s1, p011, ci_real=3))
    # Ci % 32 != 0: quads straddle taps inside a k-tile; Co = 36 one quad past the 32-wide tile bound; the generic unpack with
    # real < padded channel counts on both sides
    c.append(ConvCell("r7x5_34to33", (3, 1, 7, 5), 36, 36, k133, s1, p011, ci_real=34, co_real=33))
    # extent < kernel; the 128x32 tile (Co <= 32); 5 output positions: the second split-K range of the weight gradient is empty
    c.append(ConvCell("r1x1_12to28", (5, 1, 1, 1), 12, 28, k133, s1, p011))
    # three column tiles, the last one a single quad
    c.append(ConvCell("r2x9_12to260", (2, 1, 2, 9), 12, 260, k133, s1, p011))
    c.append(ConvCell("r9x11_36to132_p0", (1, 1, 9, 11), 36, 132, k133, s1, p0))
    c.append(ConvCell("r6x10_k5_12to32", (2, 1, 6, 10), 12, 32, (1, 5, 5), s1, (0, 2, 2)))
    # 1x1: the wide-kernel shortcut of the forward pass (f16x2, Ci % 32 == 0, M > 128) and of the data gradient (Co % 32 == 0) on
    # and off at M = 127 / 129 / 1000
    for nthw in ((1, 1, 1, 127), (1, 1, 3, 43), (1, 1, 25, 40)):
        for ci, co in ((36, 132), (32, 128), (36, 128), (64, 132)):
            c.append(ConvCell("p%dx%d_%dto%d" % (nthw[2], nthw[3], ci, co), nthw, ci, co, (1, 1, 1), s1, p0))
    # strided: four phases of unequal halo; both data-gradient tiles (Ci <= 32 / > 32, the latter with the roles swapped)
    for ci, co in ((12, 128), (12, 28)):
        c.append(ConvCell("s10x6_%dto%d_p1" % (ci, co), (3, 1, 10, 6), ci, co, k144, s122, p011))
        c.append(ConvCell("s10x6_%dto%d_p0" % (ci, co), (3, 1, 10, 6), ci, co, k144, s122, p0))
    c.append(ConvCell("s10x6_128to12_p1", (3, 1, 10, 6), 128, 12, k144, s122, p011))
    c.append(ConvCell("s6x14_k2_36to36", (2, 1, 6, 14), 36, 36, (1, 2, 2), s122, p0))                # one tap per phase
    c.append(ConvCell("s8x7_k43_12to36", (2, 1, 8, 7), 12, 36, (1, 4, 3), (1, 2, 1), p011))          # stride in one dim: two classes
    # image side: Wo = 24 (generic kernels; the 64-row tile of the weight gradient, M = 16 taps x 4) against Wo = 32 (f16x2: the
    # thin kernel of thin_conv.hip)
    c.append(ConvCell("i12x48_3to128", (2, 1, 12, 48), 4, 128, k144, s122, p011, ci_real=3))
    c.append(ConvCell("i6x64_3to128", (2, 1, 6, 64), 4, 128, k144, s122, p011, ci_real=3))
    # 3-D: the transformer's causal geometry (front-only pads in t and h, out=) with T > 2; 27 taps, K = 972; temporal stride;
    # eight stride classes with 64 taps (the tiled unpack refuses: Co % 64 / the 64 KB of LDS)
    c.append(ConvCell("v3x5x6_causal_12to132", (2, 3, 5, 6), 12, 132, (3, 3, 3), s1, (2, 2, 1), out=(3, 5, 6)))
    c.append(ConvCell("v4x4x5_k333_36to28", (1, 4, 4, 5), 36, 28, (3, 3, 3), s1, (1, 1, 1)))
    c.append(ConvCell("v4x3x5_k211_12to36", (2, 4, 3, 5), 12, 36, (2, 1, 1), (2, 1, 1), p0))
    c.append(ConvCell("v4x6x4_k444_12to36", (1, 4, 6, 4), 12, 36, (4, 4, 4), (2, 2, 2), (1, 1, 1)))
    c.append(ConvCell("v4x6x4_k444_12to64", (1, 4, 6, 4), 12, 64, (4, 4, 4), (2, 2, 2), (1, 1, 1)))
    # near misses: one field off patch_conv_eligible / wg_role (extent, pad, T), the channel field off, and one field off the
    # parity / phase / stride-2 weight-gradient kernels
    c.append(ConvCell("n32x32_k3_32to128", (2, 1, 32, 32), 32, 128, k133, s1, p011, near_miss=True))
    c.append(ConvCell("n18x18_k3p0_32to128", (2, 1, 18, 18), 32, 128, k133, s1, p0, near_miss=True))
    c.append(ConvCell("n2x16x16_k3_32to128", (1, 2, 16, 16), 32, 128, k133, s1, p011, near_miss=True))
    c.append(ConvCell("n16x16_k3_36to128", (2, 1, 16, 16), 36, 128, k133, s1, p011, near_miss=True))
    c.append(ConvCell("n16x16_k3_32to132", (2, 1, 16, 16), 32, 132, k133, s1, p011, near_miss=True))
    c.append(ConvCell("n32x16_k4s2_32to128", (2, 1, 32, 16), 32, 128, k144, s122, p011, near_miss=True))
    c.append(ConvCell("n32x32_k4s2_32to132", (2, 1, 32, 32), 32, 132, k144, s122, p011, near_miss=True))
    return c


CELLS = _cells()
CELL = {c.name: c for c in CELLS}
assert len(CELL) == len(CELLS)
MAX_PIX = 2048                                  # no cell is larger than this many output positions


# ---- operands and bounds -------------------------------------------------------------------------------------------------
def rand(shape, g, lo=-1.0, hi=1.0):
    """Uniform fp32 values (drawn in fp64, rounded once)."""
    return torch.rand(*shape, generator=g, dtype=torch.float64).float() * (hi - lo) + lo


def operands(c, seed=0):
    """x (N, ci_real, T, H, W), w (co_real, ci_real, Kt, Kh, Kw), dy (N, co_real, To, Ho, Wo): fp32, uniform in (-1, 1)."""
    g = torch.Generator().manual_seed(7000 + seed + 31 * CELLS_INDEX.get(c.name, 0))
    x = rand((c.N, c.ci_real) + c.ins, g)
    w = rand((c.co_real, c.ci_real) + c.kernel, g)
    dy = rand((c.N, c.co_real) + c.out, g)
    return x, w, dy


CELLS_INDEX = {c.name: i for i, c in enumerate(CELLS)}


def passes(c, x, w, dy, dtype=torch.float64):
    """(y, dx, dw, db) of the cell in `dtype`, by autograd through conv_ref."""
    xr = x.to(dtype).clone().requires_grad_(True)
    wr = w.to(dtype).clone().requires_grad_(True)
    y = conv_ref(xr, wr, c.kernel, c.stride, c.pad, c.out, dtype)
    dx, dw = torch.autograd.grad(y, (xr, wr), dy.to(dtype))
    return y.detach(), dx, dw, dy.to(dtype).sum((0, 2, 3, 4))


def bounds(c, x, w, dy):
    """-> dict: fp64 `y`, `dx`, `dw`, `db` and the magnitudes `mag_y` = sum |x||w|, `mag_dx` = sum |dy||w|, `mag_dw` = sum |x||dy|,
    `mag_db` = sum |dy| per element: the same function on absolute values."""
    y, dx, dw, db = passes(c, x, w, dy)
    my, mdx, mdw, mdb = passes(c, x.abs(), w.abs(), dy.abs())
    return dict(y=y, dx=dx, dw=dw, db=db, mag_y=my, mag_dx=mdx, mag_dw=mdw, mag_db=mdb)


def tol(mag, ref, bias=None, res=None):
    """The per-element bound of the matrix."""
    extra = ref.abs()
    if bias is not None:
        extra = extra + bias.abs()
    if res is not None:
        extra = extra + res.abs()
    return EPS_ACC * mag + EPS_EPI * extra


# ---- the epilogue in fp64, in the engine's order (lvt_epilogue: bias, residual, relu / leaky, tanh, sigmoid, mask) ----------------
EPI_BIAS, EPI_RESIDUAL, EPI_RELU, EPI_TANH, EPI_MASK, EPI_SIGMOID, EPI_LEAKY, EPI_LEAKY_MASK = 1, 2, 4, 8, 16, 128, 1 << 11, 1 << 12


def epilogue64(v, flags, bias=None, res=None, mask=None, npad=0):
    """v, res, mask: channels-last (..., C) fp64 over the PADDED channel count; bias (C).  SIGMOID stores the last `npad`
    channels as 0."""
    if flags & EPI_BIAS:
        v = v + bias
    if flags & EPI_RESIDUAL:
        v = v + res
    if flags & EPI_RELU:
        v = v.clamp_min(0.0)
    if flags & EPI_LEAKY:
        v = torch.where(v > 0, v, LEAKY_SLOPE * v)
    if flags & EPI_TANH:
        v = torch.tanh(v)
    if flags & EPI_SIGMOID:
        v = torch.sigmoid(v)
        if npad:
            v = v.clone()
            v[..., v.shape[-1] - npad:] = 0.0
    if flags & EPI_MASK:
        v = torch.where(mask > 0, v, LEAKY_SLOPE * v if flags & EPI_LEAKY_MASK else torch.zeros_like(v))
    return v
