"""Every route that scales an f16x2 operand from its max |.|, on operands at the ends of the scale's range.

The f16x2 arithmetic scales each operand by a power of two s taken from a device scalar >= max |operand| (lvt_f16_scale,
lvt_amd/csrc/lvt_common.h) and splits a s into hi + lo / 2048.  The low term is formed as a * (s * 2048): with the scale's
exponent clamped at 252 that product was +inf for every operand with max |a| < 2^-102, so an all-zero operand (a dead layer, a
zeroed weight, a branch with loss weight 0) gave 0 * inf = NaN in every output of the launch, and a tiny one gave inf.  These
tests pin the behaviour on every route: all-zero operands, operands on both sides of 2^-102, fp32-subnormal ones and huge
ones, each as the A and as the B operand, against an fp64 evaluation on the CPU.

Per launch: every output is finite; the element-wise bound of tests/test_gpu_gemm_matrix.py holds unchanged,
|C - C64| <= 1e-5 (|A||B|)_mn + 2^-21 (|bias_n| + |res_mn| + |C_old,mn| + |C64_mn|); for the class of fp32-subnormal
operands (t126) plus K 2^-126 max |partner|, the most that flushing every subnormal input element to zero can move an output
(K: the length of the reduction); a zero operand therefore leaves exactly the epilogue terms, and exactly +0 without an
epilogue; the launch's record of max |C| equals torch's; a second launch gives the same bits.

The flash attention kernels and the quantiser derive their own scales (per row, with their own clamps: FA_EMIN in
attention_flash.hip, vqf_pow2 in vq.hip) and are held to their own files' rules on whole-zero operands."""
import pytest
import torch
import torch.nn.functional as F

from lvt_amd.hip import binding as L, gemm as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS_ACC, EPS_EPI = 1e-5, 2.0 ** -21            # tests/test_gpu_gemm_matrix.py
FLUSH = 2.0 ** -126                            # an fp32-subnormal element is smaller than this
B_, R_, A_ = L.EPI_BIAS, L.EPI_RESIDUAL, L.EPI_ACCUM

# class -> (binary exponent of the operand X, of its partner); None: all zeros.  The partners keep the exact product an
# ordinary fp32 number.
CLASSES = {"zero": (None, 0), "zero_x_zero": (None, None), "zero_x_huge": (None, 100), "t126": (-126, 100), "t110": (-110, 100),
           "t103": (-103, 100), "t101": (-101, 100), "huge": (126, -120)}
CLS = list(CLASSES)
SIDES = ["A", "B"]


@pytest.fixture(autouse=True)
def f16x2_mode():
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    yield
    L.set_math_mode(before)


# ---- operands and the bound -------------------------------------------------------------------------------------------
def _uniform(shape, e, g):
    """uniform [-1, 1) times 2^e, exactly (None: zeros); built on the CPU, so that no device pass flushes it first."""
    u = torch.rand(*shape, generator=g) * 2 - 1
    return torch.zeros(*shape) if e is None else torch.ldexp(u, torch.tensor(e))


def _pair(cls, side, shape_a, shape_b, seed):
    """-> A, B (CPU fp32; the class on `side`, its partner on the other) and the flush allowance per reduction term."""
    g = torch.Generator().manual_seed(seed)
    ex, ep = CLASSES[cls]
    a = _uniform(shape_a, ex if side == "A" else ep, g)
    b = _uniform(shape_b, ep if side == "A" else ex, g)
    partner = b if side == "A" else a
    return a, b, (FLUSH * float(partner.abs().max()) if cls == "t126" else 0.0)


def _check(got, acc, mag, epi=(), flush=0.0, post=None, what=""):
    """`got` against C64 = post(acc + sum(epi)) under the gemm-matrix bound (+ `flush`, the t126 allowance, already times K).
    A zero operand has mag == 0: C must then equal the epilogue terms within the 2^-21 term, and be +0 bit for bit without one."""
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite outputs of %d (%d NaN)" % (
        what, int((~torch.isfinite(got)).sum()), got.numel(), int(torch.isnan(got).sum()))
    v, extra = acc.clone(), torch.zeros_like(acc)
    for e in epi:
        v = v + e.double()
        extra = extra + e.double().abs()
    if post is not None:
        v = post(v)
    tol = EPS_ACC * mag + EPS_EPI * (extra + v.abs()) + flush
    err = (got.double() - v).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), "%s: %d elements out of bound (worst: err %g, tol %g)" % (
        what, int(bad.sum()), float(err[bad].max()), float(tol[bad][err[bad].argmax()]))
    if not epi and float(mag.max()) == 0.0:
        assert not bool(got.view(torch.int32).any()), "%s: a zero product is not +0 bit for bit" % what


def _record_is_max(t, what=""):
    """The launch's OWN record of max |t| (amax_of would scan the tensor afresh where a route stopped reporting one)."""
    slot = L._valid_amax(t)
    assert slot is not None, "%s: the launch left no record of max |C|" % what
    rec = float(slot)
    assert rec == rec and rec == float(t.abs().max()), "%s: record %r, max %r" % (what, rec, float(t.abs().max()))


def _same_bits(a, b, what=""):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: a second launch gave other bits" % what


# ---- lvt_gemm_f32: lvt_gemm_kernel<.., MATH 2> and the wide kernel ------------------------------------------------------
def _gemm_route(M, N, K, ta, tb, cls, side, splits=1, colsum=False):
    A, Bm, fl = _pair(cls, side, (M, K), (K, N), 7 * M + 13 * N + 17 * K + 2 * ta + tb)
    g = torch.Generator().manual_seed(M + N + K)
    bias, res, cold = _uniform((N,), 0, g), _uniform((M, N), 0, g), _uniform((M, N), 0, g)
    acc, mag = A.double() @ Bm.double(), A.double().abs() @ Bm.double().abs()
    a_src, b_src = (A.t() if ta else A).contiguous(), (Bm if tb else Bm.t()).contiguous()

    def launch(flags):
        a, b = a_src.to(DEV), b_src.to(DEV)
        c = cold.to(DEV) if flags & A_ else torch.full((M, N), float("nan"), device=DEV)
        cs = torch.full((M,), float("nan"), device=DEV) if colsum else None
        kw = {}
        if flags & B_:
            kw["bias"] = bias.to(DEV)
        if flags & R_:
            kw["res"] = res.to(DEV)
        G.gemm(a, b, c, M, N, K, ta=ta, tb=tb, flags=flags, splits=splits, a_colsum=cs, **kw)
        return c, cs

    for flags, epi in ((0, ()), (B_ | R_, (bias.expand(M, N), res)), (A_, (cold,))):
        if splits > 1 and flags & (B_ | R_):
            continue                                            # (a split-K launch takes ACCUM only)
        what = "gemm M%d N%d K%d t%d%d splits %d flags %x %s on %s" % (M, N, K, ta, tb, splits, flags, cls, side)
        c1, cs1 = launch(flags)
        c2, cs2 = launch(flags)
        _check(c1, acc, mag, epi, K * fl, what=what)
        _same_bits(c1, c2, what)
        if splits <= 1:
            _record_is_max(c1, what)
        if colsum and not (cls == "huge" and side == "A"):       # (68 terms of 2^126: the sums themselves leave the fp32 range)
            ad = A.double()
            _check(cs1, ad.sum(1), ad.abs().sum(1), (), K * FLUSH if (cls == "t126" and side == "A") else 0.0, what=what + " a_colsum")
            _same_bits(cs1, cs2, what + " a_colsum")


# K % 32 != 0 keeps every shape on lvt_gemm_kernel (the wide kernel needs M > 128 and K % 32 == 0); ragged M and N, K = 40 and
# 68 in each of the three instantiated forms NT, NN, TN (ta = 1 with tb = 0 is not instantiated); N = 98: the scalar epilogue
SMALL = [(129, 132, 68, 0, 0), (97, 98, 40, 0, 0), (129, 132, 40, 0, 1), (97, 100, 68, 0, 1), (128, 132, 68, 1, 1), (100, 96, 40, 1, 1)]


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("M,N,K,ta,tb", SMALL)
def test_gemm_kernel(M, N, K, ta, tb, cls, side):
    _gemm_route(M, N, K, ta, tb, cls, side)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
def test_gemm_kernel_tn_splitk_colsum(cls, side):
    """Weight-gradient form: two k ranges and the column sums of A from the same launch (those of a zero A are exactly 0)."""
    _gemm_route(128, 132, 68, 1, 1, cls, side, splits=2, colsum=True)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(256, 128, 32), (260, 132, 96)])
def test_wide_gemm(M, N, K, ta, tb, cls, side):
    """lvt_gemm_wide_kernel<ta, tb> (f16x2, M > 128, K % 32 == 0): the k-contiguous loaders and the two transposing ones."""
    _gemm_route(M, N, K, ta, tb, cls, side)


# ---- lvt_gemm_p2_f32 -----------------------------------------------------------------------------------------------------
def _p2_image(x):
    dst = torch.empty_like(x)
    amax = L.amax_of(x)
    G.p2_pack([(x, False, dst, amax)])
    return G.P2Image(dst, amax)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("a_image", [False, True])
def test_gemm_p2(a_image, cls, side):
    M, N, K = 256, 128, 64
    A, Bm, fl = _pair(cls, side, (M, K), (K, N), 31 + int(a_image))
    g = torch.Generator().manual_seed(5)
    bias, res = _uniform((N,), 0, g), _uniform((M, N), 0, g)
    acc, mag = A.double() @ Bm.double(), A.double().abs() @ Bm.double().abs()
    what = "gemm_p2 a_image %d %s on %s" % (a_image, cls, side)

    def launch(flags, **kw):
        a, w = A.to(DEV), Bm.t().contiguous().to(DEV)
        out = torch.full((M, N), float("nan"), device=DEV)
        G.gemm_p2(_p2_image(a) if a_image else a, _p2_image(w), out, M, N, K, flags=flags, **kw)
        return out

    for flags, kw, epi in ((0, {}, ()), (B_ | R_, dict(bias=bias.to(DEV), res=res.to(DEV)), (bias.expand(M, N), res))):
        c1, c2 = launch(flags, **kw), launch(flags, **kw)
        _check(c1, acc, mag, epi, K * fl, what=what)
        _same_bits(c1, c2, what)
        _record_is_max(c1, what)


# ---- convolutions -------------------------------------------------------------------------------------------------------
def _nhwc(x):   # (N, C, H, W) -> (N, 1, H, W, C) contiguous, on the device
    return x.permute(0, 2, 3, 1).contiguous().unsqueeze(1).to(DEV)


def _nchw(y):   # (N, 1, H, W, C) -> (N, C, H, W)
    return y.squeeze(1).permute(0, 3, 1, 2).contiguous()


def _geom(N, H, W, Ci, Co, k, s, p):
    return G.conv_geom(N, 1, H, W, Ci, Co, (1, k, k), (1, s, s), (0, p, p))


# route -> N, H, W, Ci, Co, k, s, p, real input channels.  Where lvt_conv3d_fwd sends each one in f16x2 mode:
#   implicit_3x3_8x8, implicit_3x3_co32, implicit_1x1_8x8: the implicit-GEMM tile kernel lvt_gemm_kernel<A_CONV_K, B_NPLAIN, ..>
#     (128 x 128 tiles; 128 x 32 for Co <= 32) -- 8x8 frames are not served by the frame-resident kernels (16x16 only), and the
#     1x1 layer has M = N Ho Wo = 64 <= 128 output positions, too few for the wide kernel;
#   wide_1x1: a 1x1 / stride 1 / unpadded layer with Ci % 32 == 0 and M = 256 > 128 IS a plain product: lvt_gemm_wide_kernel<0, 1>;
#   patch_3x3, parity_k4s2: the frame-resident kernel (asserted by its predicates); image_side: the 4 -> 128 channel kernel.
FWD = {"implicit_3x3_8x8": (1, 8, 8, 32, 128, 3, 1, 1, 32), "implicit_3x3_co32": (1, 8, 8, 32, 32, 3, 1, 1, 32),
       "implicit_1x1_8x8": (1, 8, 8, 128, 256, 1, 1, 0, 128), "wide_1x1": (1, 16, 16, 128, 256, 1, 1, 0, 128),
       "patch_3x3": (1, 16, 16, 32, 128, 3, 1, 1, 32), "parity_k4s2": (1, 32, 32, 32, 128, 4, 2, 1, 32),
       "image_side": (2, 16, 128, 4, 128, 4, 2, 1, 3)}


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("route", list(FWD))
def test_conv_forward(route, cls, side):
    """Forward convolution with bias + residual, the class on x (A) and on w (B): the implicit-GEMM tile kernel (both tile
    shapes), the wide kernel that a large 1x1 layer runs on, the frame-resident patch kernel, its parity-class form and the
    image-side kernel (the table above says why each geometry lands where it does)."""
    N, H, W, Ci, Co, k, s, p, real = FWD[route]
    x, w, fl = _pair(cls, side, (N, Ci, H, W), (Co, Ci, k, k), 100 + Ci + Co + k)
    x[:, real:] = 0
    w[:, real:] = 0
    g = _geom(N, H, W, Ci, Co, k, s, p)
    assert G.uses_patch_kernel(g) == (route == "patch_3x3") and G.fwd_by_parity(g) == (route == "parity_k4s2")
    gen = torch.Generator().manual_seed(3)
    b, res = _uniform((Co,), 0, gen), _uniform((N, Co, g.Ho, g.Wo), 0, gen)
    acc = F.conv2d(x.double(), w.double(), None, stride=s, padding=p)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride=s, padding=p)
    what = "conv_fwd %s %s on %s" % (route, cls, side)

    def launch():
        wd = w.unsqueeze(2).to(DEV)
        if route == "parity_k4s2":
            return G.conv_fwd(g, _nhwc(x), None, bias=b.to(DEV), res=_nhwc(res), wq=G.pack_weight_parity(g, wd, Ci, Co))
        return G.conv_fwd(g, _nhwc(x), G.pack_weight(g, wd, Ci, Co), bias=b.to(DEV), res=_nhwc(res))

    y1, y2 = launch(), launch()
    _check(_nchw(y1), acc, mag, (b.view(1, -1, 1, 1).expand_as(acc), res), real * k * k * fl, what=what)
    _same_bits(y1, y2, what)
    _record_is_max(y1, what)


# route -> geometry of the FORWARD convolution whose data gradient is taken (dy has Co channels, dx has Ci)
BWD_DATA = {"implicit": (1, 16, 16, 128, 32, 3, 1, 1), "as_conv": (1, 16, 16, 128, 32, 3, 1, 1), "by_phases": (1, 32, 32, 128, 32, 4, 2, 1)}


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("route", list(BWD_DATA))
def test_conv_backward_data(route, cls, side):
    """dx with residual + mask, the class on dy (A) and on w (B): the implicit-GEMM route, the forward convolution over
    transposed weights (frame-resident kernel) and the phase-by-phase form of the stride-2 layers."""
    N, H, W, Ci, Co, k, s, p = BWD_DATA[route]
    g = _geom(N, H, W, Ci, Co, k, s, p)
    assert G.bwd_data_as_conv(g) == (s == 1) and G.bwd_data_by_phases(g) == (s == 2)
    dy, w, fl = _pair(cls, side, (N, Co, g.Ho, g.Wo), (Co, Ci, k, k), 200 + k)
    gen = torch.Generator().manual_seed(4)
    res, msrc = _uniform((N, Ci, H, W), 0, gen), _uniform((N, Ci, H, W), 0, gen)
    acc = F.conv_transpose2d(dy.double(), w.double(), stride=s, padding=p)
    mag = F.conv_transpose2d(dy.double().abs(), w.double().abs(), stride=s, padding=p)
    what = "conv_bwd_data %s %s on %s" % (route, cls, side)

    def launch():
        wd = w.unsqueeze(2).to(DEV)
        kw = dict(res=_nhwc(res), mask=_nhwc(msrc))
        if route == "as_conv":
            return G.conv_bwd_data(g, _nhwc(dy), None, wt=G.pack_weight_t(g, wd, Ci, Co), **kw)
        if route == "by_phases":
            return G.conv_bwd_data(g, _nhwc(dy), None, wph=G.pack_weight_phases(g, wd, Ci, Co), **kw)
        return G.conv_bwd_data(g, _nhwc(dy), G.pack_weight(g, wd, Ci, Co), **kw)

    d1, d2 = launch(), launch()
    terms = Co * (k // s) ** 2                                 # reduction length of one dx element
    _check(_nchw(d1), acc, mag, (res,), terms * fl, post=lambda v: torch.where(msrc > 0, v, torch.zeros_like(v)), what=what)
    assert bool((_nchw(d1).cpu()[msrc <= 0] == 0).all()), what + ": masked elements are not 0"
    _same_bits(d1, d2, what)
    _record_is_max(d1, what)


BWD_WEIGHT = {"frames_s1": (2, 16, 256, 32, 3, 1, 1), "frames_s2": (3, 32, 32, 256, 4, 2, 1), "implicit_1x1": (1, 16, 128, 256, 1, 1, 0)}


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("route", list(BWD_WEIGHT))
def test_conv_backward_weight(route, cls, side):
    """dw and the fused bias gradient, the class on x (A) and on dy (B): the frame-resident kernels (stride 1, stride 2) and the
    implicit-GEMM route.  A zero dy gives dw == 0 and db == 0 exactly; db is a plain fp32 sum of dy (bound: 1e-5 sum |dy|; not
    judged for dy = uniform 2^126, whose channel sums are no fp32 numbers)."""
    import ctypes
    N, H, Ci, Co, k, s, p = BWD_WEIGHT[route]
    g = _geom(N, H, H, Ci, Co, k, s, p)
    assert L.lib().lvt_conv3d_bwd_weight_fuses_bias(ctypes.byref(g), L.math_flag()) == 1
    x, dy, fl = _pair(cls, side, (N, Ci, H, H), (N, Co, g.Ho, g.Wo), 300 + k)
    acc = torch.nn.grad.conv2d_weight(x.double(), (Co, Ci, k, k), dy.double(), stride=s, padding=p)
    mag = torch.nn.grad.conv2d_weight(x.double().abs(), (Co, Ci, k, k), dy.double().abs(), stride=s, padding=p)
    what = "conv_bwd_weight %s %s on %s" % (route, cls, side)

    def launch():
        return G.conv_bwd_weight(g, _nhwc(x), _nhwc(dy), Ci, Co, want_bias=True)

    (w1, b1), (w2, b2) = launch(), launch()
    terms = N * g.Ho * g.Wo
    _check(w1.squeeze(2), acc, mag, (), terms * fl, what=what)
    _same_bits(w1, w2, what)
    assert b1 is not None
    _same_bits(b1, b2, what + " db")
    if cls == "huge" and side == "B":
        return                                                  # (sums of >= 256 terms of 2^126 leave the fp32 range)
    dyd = dy.double()
    _check(b1, dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3)), (), terms * FLUSH if (cls == "t126" and side == "B") else 0.0, what=what + " db")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("cls", CLS)
@pytest.mark.parametrize("act", [False, True], ids=["plain", "tanh"])
@pytest.mark.parametrize("N,Ci,Cr,Hi,Wi", [(1, 128, 3, 8, 32), (3, 32, 3, 5, 7)], ids=["mfma", "fma"])
def test_thin_conv_transpose(N, Ci, Cr, Hi, Wi, act, cls, side):
    """ConvTranspose2d(Ci -> 3, k4 s2 p1) on the image-side kernels (matrix cores: 128 channels on 8 x 32 bands; fp32 FMA
    otherwise), the class on x (A) and on w (B): act(bias) is what a zero operand leaves; the carried 4th channel is 0."""
    x, w, fl = _pair(cls, side, (N, Ci, Hi, Wi), (Ci, Cr, 4, 4), 400 + Ci)
    b = _uniform((Cr,), 0, torch.Generator().manual_seed(6))
    acc = F.conv_transpose2d(x.double(), w.double(), None, stride=2, padding=1)
    mag = F.conv_transpose2d(x.double().abs(), w.double().abs(), None, stride=2, padding=1)
    what = "convT4 Ci %d act %d %s on %s" % (Ci, act, cls, side)

    def launch():
        return G.convT4_fwd(_nhwc(x), w.to(DEV), b.to(DEV), act)

    y1, y2 = launch(), launch()
    assert y1.shape == (N, 1, 2 * Hi, 2 * Wi, 4)
    got = _nchw(y1)
    _check(got[:, :Cr], acc, mag, (b.view(1, -1, 1, 1).expand_as(acc),), Ci * 4 * fl, post=torch.tanh if act else None, what=what)
    assert bool((got[:, Cr:] == 0).all()), what + ": the carried channel is not 0"
    _same_bits(y1, y2, what)


@pytest.mark.parametrize("form", ["plain", "t", "parity", "phases"])
def test_weight_images_of_a_zero_weight(form):
    """lvt_conv3d_weight_images of an all-zero weight (scale from a max of 0), read by one consumer launch of each pack layout:
    the result is the epilogue terms alone."""
    gen = torch.Generator().manual_seed(8)
    if form in ("plain", "t"):
        N, H, Ci, Co, k, s, p = (1, 16, 32, 128, 3, 1, 1) if form == "plain" else (1, 16, 128, 32, 3, 1, 1)
    else:
        N, H, Ci, Co, k, s, p = (1, 32, 32, 128, 4, 2, 1) if form == "parity" else (1, 32, 128, 32, 4, 2, 1)
    g = _geom(N, H, H, Ci, Co, k, s, p)
    w = torch.zeros(Co, Ci, 1, k, k, device=DEV)
    fwd = form in ("plain", "parity")
    a = _uniform((N, Ci, H, H) if fwd else (N, Co, g.Ho, g.Wo), 0, gen)
    res = _uniform((N, Co, g.Ho, g.Wo) if fwd else (N, Ci, H, H), 0, gen)
    bias = _uniform((Co if fwd else Ci,), 0, gen)
    pb = G.PackBatch()
    wp = getattr(pb, form)(g, w, Ci, Co)
    pb.launch()
    assert getattr(wp, "_lvt_wimg", False), "no image was made for this pack"
    if form == "plain":
        y = G.conv_fwd(g, _nhwc(a), wp, bias=bias.to(DEV), res=_nhwc(res))
    elif form == "parity":
        y = G.conv_fwd(g, _nhwc(a), None, bias=bias.to(DEV), res=_nhwc(res), wq=wp)
    elif form == "t":
        y = G.conv_bwd_data(g, _nhwc(a), None, bias=bias.to(DEV), res=_nhwc(res), wt=wp)
    else:
        y = G.conv_bwd_data(g, _nhwc(a), None, bias=bias.to(DEV), res=_nhwc(res), wph=wp)
    zero = torch.zeros_like(res, dtype=torch.float64)
    _check(_nchw(y), zero, zero, (bias.view(1, -1, 1, 1).expand_as(res), res), what="weight image " + form)
    _record_is_max(y, "weight image " + form)


@pytest.mark.parametrize("cls", ["zero", "t110"])
def test_onehot_tn_gemm_dense(cls):
    """The one-hot weight-gradient GEMM (dense=True: always on the matrix cores; the one-hot operand is exact and unscaled, dout
    is scaled from its max): dout all zero and dout times 2^-110."""
    from lvt_amd.hip import tx
    N, ns, nv, b, P = 64, 1, 512, 5, 300
    g = torch.Generator().manual_seed(N + ns)
    idx = torch.randint(0, nv, (b, ns, P), generator=g)
    dout = _uniform((b * P, N), CLASSES[cls][0], g)
    ref = torch.zeros(nv, N, dtype=torch.float64).index_add_(0, idx.reshape(-1), dout.double())
    mag = torch.zeros(nv, N, dtype=torch.float64).index_add_(0, idx.reshape(-1), dout.double().abs())

    def launch():
        return tx.onehot_tn_gemm(idx.to(DEV), nv, [0], ns * P, 1, P, b * P, dout.to(DEV), N, ldb=N, dense=True)

    g1, g2 = launch(), launch()
    _check(g1, ref, mag, what="onehot dense " + cls)
    _same_bits(g1, g2, "onehot dense " + cls)


# ---- flash attention and the quantiser: scales of their own, with their own clamps ----------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("onepass", [True, False], ids=["onepass", "twopass"])
@pytest.mark.parametrize("which", ["q", "k", "v", "dO", "v_dO_t110"])
def test_flash_attention_whole_zero_and_tiny_operands(which, onepass, masked):
    """Each of q, k, v, dO zero as a whole tensor, and v and dO times 2^-110 together, at B 1, H 8, S 256: finite everywhere and
    within 2e-5 of each output's fp64 maximum (bank gradients: of the largest bank gradient), the rule of
    tests/test_gpu_flash_attention.py -- an output whose fp64 reference is all zero must be exactly 0.  With v and dO at 2^-110
    the outputs that are linear in them (o, dv) are ordinary numbers of that size; dq, dk and the bank gradients are bilinear in
    (v, dO), about 2^-220, far below the smallest fp32 subnormal 2^-149: what fp32 can hold of them is 0 or one unit of 2^-149,
    and that is what is asserted."""
    from test_gpu_flash_attention import DA, NAMES, S, _flash, _reference
    B, H, blk = 1, 8, (1, 16, 16)
    g = torch.Generator().manual_seed(21)
    q, k, v, go = (_uniform((B * S, H * DA), 0, g) for _ in range(4))
    if which == "q":
        q = torch.zeros_like(q)
    elif which == "k":
        k = torch.zeros_like(k)
    elif which == "v":
        v = torch.zeros_like(v)
    elif which == "dO":
        go = torch.zeros_like(go)
    else:
        v, go = torch.ldexp(v, torch.tensor(-110)), torch.ldexp(go, torch.tensor(-110))
    banks = [_uniform((H, 2 * n - 1), -1, g) for n in blk]
    ref = _reference(q, k, v, go, banks, blk, masked)
    got = _flash(q, k, v, go, banks, blk, masked, onepass)
    bank_scale = max(float(ref[i].abs().max()) for i in (6, 7, 8))
    for n, a, r in zip(NAMES, got, ref):
        assert bool(torch.isfinite(a).all()), (which, n)
        if which == "v_dO_t110" and n in ("dq", "dk", "ddt", "ddh", "ddw"):
            assert float(r.abs().max()) < 2.0 ** -200 and float(a.abs().max()) <= 2.0 ** -149, (which, n, float(a.abs().max()))
            continue
        scale = bank_scale if n.startswith("dd") else float(r.abs().max())
        err = float((a.double().cpu() - r).abs().max())
        assert err <= 2e-5 * scale, (which, n, err, scale)


@pytest.mark.parametrize("which", ["z", "codebook"])
@pytest.mark.parametrize("Dg,K", [(64, 512), (32, 512)], ids=["specialised", "generic"])
def test_quantiser_whole_zero_operands(Dg, K, which):
    """vq.nearest with z entirely zero (every row picks the code of smallest norm) and with the codebook entirely zero (every
    distance ties: index 0), on the specialised and the generic kernel: the fp64 argmin with the first-index tie rule.  The
    route returns indices only -- it exposes no distances whose finiteness could be asserted; a NaN or inf score inside the
    kernel would show as a wrong index here."""
    from lvt_amd.hip import vq
    P, n, num = 16, 7, 3
    g = torch.Generator().manual_seed(Dg + K)
    z, cb = torch.randn(n * P, num * Dg, generator=g), torch.randn(num, K, Dg, generator=g)
    if which == "z":
        z = torch.zeros_like(z)
    else:
        cb = torch.zeros_like(cb)
    idx = vq.nearest(z.to(DEV), cb.to(DEV), P).cpu()                       # (n, num, P)
    again = vq.nearest(z.to(DEV), cb.to(DEV), P).cpu()
    assert torch.equal(idx, again)
    for gi in range(num):
        rows = z[:, Dg * gi:Dg * (gi + 1)].double()
        d = ((rows[:, None, :] - cb[gi].double()[None]) ** 2).sum(-1)      # (rows, K): exact ties where an operand is zero
        dmin = d.min(-1, keepdim=True).values
        first = torch.where(d == dmin, torch.arange(K)[None, :], torch.tensor(K)).min(-1).values     # first index among the minima
        assert torch.equal(idx[:, gi].reshape(-1), first), (which, Dg, K, gi)
