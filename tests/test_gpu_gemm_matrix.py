"""Conformance matrix of lvt_gemm_f32 (lvt_amd/csrc/gemm_engine.hip) against an fp64 CPU reference, cell by cell.

Dispatch rules the cells target (lvt_gemm_f32, launch_tile, launch_wide):
  * wide kernel lvt_gemm_wide_kernel<ta, tb>: f16x2 arithmetic && M > 128 && K % 32 == 0 && a_kb % 32 == 0 && b_kb % 32 == 0
    && no CAUSAL_* flag; everything else runs lvt_gemm_kernel<(ta, tb) form, MATH 0 (f32) / 1 (bf16x3) / 2 (f16x2)>;
  * epilogue: vec_epi = N % 4 == 0 && C 16-byte aligned && ldc, sC_o, sC_i % 4 == 0 && (BIAS: bias aligned) && (RESIDUAL:
    res aligned, ldr % 4 == 0) && (MASK: mask aligned, ldm % 4 == 0); vec_epi && no PLANES / ACCUM / TANH -> the fast
    epilogue (epilogue_fast.h: eight compile-time subsets of {BIAS, RESIDUAL, RELU, MASK}, the run-time form for the rest);
    vec_epi otherwise -> lvt_epilogue_vec; !vec_epi -> the scalar lvt_epilogue;
  * splits > 1: k ranges of ceil(ceil(K / splits) / 32) * 32, partial tiles, lvt_reduce_splits_kernel (ACCUM: C += sum);
    a_colsum (ta == 1) reduced by a second lvt_reduce_splits_kernel launch;
  * CAUSAL_KMAX: a tile reduces k < m0 + 128; CAUSAL_KMIN: from k = m0; CAUSAL_TILE: tiles with n0 > m0 + 127 are written 0.

Per cell: every element within |C - C64| <= 1e-5 |alpha| (|A||B|)_mn + 2^-21 (|bias_n| + |res_mn| + |C_old,mn| + |C64_mn|)
(C64: the epilogue in fp64 in lvt_epilogue_vec's order: alpha acc, + bias, + res, relu / tanh, mask, + C_old for ACCUM); MASK
zeros and RELU signs exact; every float of the C buffer outside the logical C (ldc padding, batch gaps, 64 before and after)
still holds the NaN payload bit for bit; the operands sit in NaN-filled buffers the same way (lda / ldb padding, beyond the k
block, batch gaps), so a read of padding shows up as a NaN in C; in f16x2 the record of max |C| equals torch's; and a second
launch into fresh buffers gives the same bits."""
import pytest
import torch

from lvt_amd.hip import binding as L, gemm as G
from util_guard import PAD, PAYLOAD, Buf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS_ACC, EPS_EPI = 1e-5, 2.0 ** -21
B_, R_, U_, M_ = L.EPI_BIAS, L.EPI_RESIDUAL, L.EPI_RELU, L.EPI_MASK
T_, A_ = L.EPI_TANH, L.EPI_ACCUM
KMAX, KMIN, KTILE = L.CAUSAL_KMAX, L.CAUSAL_KMIN, L.CAUSAL_TILE


@pytest.fixture(params=["bf16x3", "f16x2", "f32"])
def mode(request):
    # the operand records cover the logical region only, while LVT_AMAX_CHECK would scan the whole NaN-padded view: off here
    before, check = L.get_math_mode(), L.AMAX_CHECK
    L.set_math_mode(request.param)
    L.AMAX_CHECK = False
    yield request.param
    L.AMAX_CHECK = check
    L.set_math_mode(before)


# ---- buffers ---------------------------------------------------------------------------------------------------------
def _r4(x):
    return (x + 3) // 4 * 4


def _zoff(bo, bi, s_o, s_i):
    zo, zi = torch.arange(bo).repeat_interleave(bi), torch.arange(bi).repeat(bo)
    return zo * s_o + zi * s_i


def _kidx(R, K, ld, kb, skb):
    """(R, K) offsets of element (r, k) at r ld + (k / kb) skb + k % kb (plain k-contiguous rows when kb == K)."""
    k = torch.arange(K)
    return torch.arange(R)[:, None] * ld + ((k // kb) * skb + k % kb)[None, :]


def _rand(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float() * (hi - lo) + lo


def _record(view, logical):
    """f16x2: attach to the operand the max |.| of its LOGICAL region -- the kernel must never read the padding."""
    if L.f16x2():
        L.set_amax(view, L.amax_slot(view.device).fill_(float(logical.abs().max())))


class Cell:
    def __init__(self, M, N, K, ta=0, tb=0, flags=0, alpha=1.0, splits=1, pa=4, pb=8, pc=4, bo=1, bi=1, gap=0,
                 a_kb=0, b_kb=0, colsum=False, bias_off=0, seed=0, name=None):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def __repr__(self):
        return self.name or "M%dN%dK%d_t%d%d_f%x_a%g_s%d_b%dx%d_g%d_kb%d.%d%s" % (
            self.M, self.N, self.K, self.ta, self.tb, self.flags, self.alpha, self.splits, self.bo, self.bi, self.gap,
            self.a_kb, self.b_kb, "_cs" if self.colsum else "")


def _operands(c):
    """Build A, B (and res / mask / bias / C_old) of cell `c` in their padded layouts; returns a dict."""
    g = torch.Generator().manual_seed(1000 + c.seed + c.M * 7 + c.N * 13 + c.K * 17 + c.flags)
    Z, M, N, K = c.bo * c.bi, c.M, c.N, c.K
    o = {"Z": Z}
    # A(z, m, k)
    if c.ta == 0:
        kb = c.a_kb or K
        lda = kb + c.pa
        skb = _r4(M * lda + (16 if c.a_kb else 0))
        a1 = _kidx(M, K, lda, kb, skb)
        o["lda"], o["a_kb"], o["a_skb"] = lda, (c.a_kb or 0), (skb if c.a_kb else 0)
    else:
        lda = M + c.pa
        a1 = torch.arange(K)[None, :] * lda + torch.arange(M)[:, None]
        o["lda"], o["a_kb"], o["a_skb"] = lda, 0, 0
    sa_i = _r4(int(a1.max()) + 1 + c.gap)
    sa_o = _r4(c.bi * sa_i + 2 * c.gap)
    o["sA"] = (sa_o, sa_i) if Z > 1 else (0, 0)
    aidx = _zoff(c.bo, c.bi, *o["sA"])[:, None, None] + a1[None]
    # B(z, k, n)
    if c.tb == 0:
        kb = c.b_kb or K
        ldb = kb + c.pb
        skb = _r4(N * ldb + (16 if c.b_kb else 0))
        b1 = _kidx(N, K, ldb, kb, skb).t()
        o["ldb"], o["b_kb"], o["b_skb"] = ldb, (c.b_kb or 0), (skb if c.b_kb else 0)
    else:
        ldb = N + c.pb
        b1 = torch.arange(K)[:, None] * ldb + torch.arange(N)[None, :]
        o["ldb"], o["b_kb"], o["b_skb"] = ldb, 0, 0
    sb_i = _r4(int(b1.max()) + 1 + 3 * c.gap)
    sb_o = _r4(c.bi * sb_i + c.gap)
    o["sB"] = (sb_o, sb_i) if Z > 1 else (0, 0)
    bidx = _zoff(c.bo, c.bi, *o["sB"])[:, None, None] + b1[None]
    # C(z, m, n); res / mask share its layout (their batch strides follow C's)
    ldc = N + c.pc
    sc_i = M * ldc + c.gap if c.splits > 1 else _r4(M * ldc + c.gap)
    sc_o = _r4(c.bi * sc_i + c.gap)
    o["ldc"], o["sC"] = ldc, ((sc_o, sc_i) if Z > 1 else (0, 0))
    o["cidx"] = _zoff(c.bo, c.bi, *o["sC"])[:, None, None] + (torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :])[None]
    A, Bm = _rand((Z, M, K), g), _rand((Z, K, N), g)
    m_, k_ = torch.arange(M)[:, None], torch.arange(K)[None, :]
    if c.flags & KMAX:
        A = A * (k_ <= m_)                   # A(m, k) == 0 for k > m
    if c.flags & KMIN:
        A = A * (k_ >= m_)                   # A(m, k) == 0 for k < m
    o["A"], o["B"] = A, Bm
    o["abuf"], o["bbuf"] = Buf(aidx, A), Buf(bidx, Bm)
    o["bias"] = _rand((N,), g)
    o["res"] = _rand((Z, M, N), g)
    o["mask"] = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, (Z, M, N), generator=g)]
    o["cold"] = _rand((Z, M, N), g)
    return o


def _launch(c, o, flags=None, cold=None, bias_off=None, planes=False):
    """One launch of cell `c` into fresh buffers; returns (C buffer, colsum tensor or None)."""
    flags = c.flags if flags is None else flags
    bias_off = c.bias_off if bias_off is None else bias_off
    kw = {}
    if flags & B_:
        bb = Buf(torch.arange(c.N), o["bias"], start=PAD + bias_off)
        kw["bias"] = bb.view
    if flags & R_:
        kw["res"], kw["ldr"] = Buf(o["cidx"], o["res"]).view, o["ldc"]
    if flags & M_:
        kw["mask"], kw["ldm"] = Buf(o["cidx"], o["mask"]).view, o["ldc"]
    cbuf = Buf(o["cidx"], o["cold"] if flags & A_ else None)
    colsum = torch.full((o["Z"], c.M), float("nan"), device=DEV) if c.colsum else None
    av, bv = o["abuf"].view, o["bbuf"].view
    _record(av, o["A"])
    _record(bv, o["B"])
    G.gemm(av, bv, cbuf.view, c.M, c.N, c.K, ta=c.ta, tb=c.tb, lda=o["lda"], ldb=o["ldb"], ldc=o["ldc"],
           a_kb=o["a_kb"], a_skb=o["a_skb"], b_kb=o["b_kb"], b_skb=o["b_skb"], batch_outer=c.bo, batch_inner=c.bi,
           sA=o["sA"], sB=o["sB"], sC=o["sC"], alpha=c.alpha, flags=flags, splits=c.splits, a_colsum=colsum, **kw)
    torch.cuda.synchronize()
    return cbuf, colsum


def _reference(c, o, flags):
    A, Bm = o["A"].double(), o["B"].double()
    acc, mag = A @ Bm, A.abs() @ Bm.abs()
    v = c.alpha * acc
    extra = torch.zeros_like(v)
    if flags & B_:
        v = v + o["bias"].double()
        extra += o["bias"].double().abs()
    if flags & R_:
        v = v + o["res"].double()
        extra += o["res"].double().abs()
    if flags & U_:
        v = v.clamp_min(0.0)
    if flags & T_:
        v = torch.tanh(v)
    if flags & M_:
        v = torch.where(o["mask"].double() > 0, v, torch.zeros_like(v))
    if flags & A_:
        v = v + o["cold"].double()
        extra += o["cold"].double().abs()
    tol = EPS_ACC * abs(c.alpha) * mag + EPS_EPI * (extra + v.abs())
    return v, tol


def _check_cell(c, o, cbuf, colsum, flags):
    got = cbuf.logical().double()
    ref, tol = _reference(c, o, flags)
    cmp = torch.ones_like(got, dtype=torch.bool)
    if flags & KTILE:
        m_, n_ = torch.arange(c.M)[:, None], torch.arange(c.N)[None, :]
        above = (n_ // 128) * 128 > (m_ // 128) * 128 + 127              # tiles wholly above the diagonal
        assert bool((got[:, above.expand(c.M, c.N)] == 0).all()), "CAUSAL_TILE: a tile above the diagonal is not 0"
        cmp = (n_ <= m_).expand_as(got)
    err = (got - ref).abs()
    bad = ~(err <= tol) & cmp
    assert not bool(bad.any()), "%d elements out of bound (first %s: got %r, ref %r, tol %r)" % (
        int(bad.sum()), tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(ref[bad][0]), float(tol[bad][0]))
    if flags & M_:
        # the masked epilogue value is exactly 0: C stays 0 -- or, with ACCUM, keeps its old value bit for bit
        want = o["cold"].double() if flags & A_ else torch.zeros_like(got)
        assert torch.equal(got[o["mask"] <= 0], want[o["mask"] <= 0]), "MASK: masked elements are not exactly 0 / C_old"
    if flags & U_ and not flags & A_:
        assert bool((got >= 0).all()), "RELU: negative value"
    assert cbuf.outside_untouched(), "a float outside the logical C was written"
    if colsum is not None:
        A = o["A"].double()
        cs_ref, cs_tol = A.sum(2), EPS_ACC * A.abs().sum(2)
        assert bool(((colsum.double().cpu() - cs_ref).abs() <= cs_tol).all()), "a_colsum"
    if L.f16x2() and c.splits <= 1:
        assert float(L.amax_of(cbuf.view)) == float(cbuf.logical().abs().max()), "c_amax"


# ---- the matrix ------------------------------------------------------------------------------------------------------
SUBSETS = [f for f in range(16)]                     # bit 0 BIAS, 1 RESIDUAL, 2 RELU, 3 MASK  ==  EPI_BIAS | RESIDUAL | RELU | MASK(16)


def _flags4(s):
    return (B_ if s & 1 else 0) | (R_ if s & 2 else 0) | (U_ if s & 4 else 0) | (M_ if s & 8 else 0)


CELLS = []
# all 16 subsets on the wide kernel (f16x2: M = 257 > 128, K % 32 == 0; N = 260 one quad past two 128-wide tiles) and on
# lvt_gemm_kernel (K = 68: K % 32 != 0 in every mode; M = 129 one past a tile), alpha != 1 on the odd subsets
for s in SUBSETS:
    CELLS.append(Cell(257, 260, 512, 0, 0, _flags4(s), alpha=(-0.75 if s & 1 else 1.0), seed=s))
    CELLS.append(Cell(129, 132, 68, 0, 1, _flags4(s), alpha=(1.5 if s & 1 else 1.0), seed=s))
# TANH and ACCUM (lvt_epilogue_vec), alone and with BIAS / RESIDUAL, on both kernels
for f in (T_, T_ | B_, T_ | R_, A_, A_ | B_, A_ | R_, A_ | B_ | R_ | U_ | M_):
    CELLS.append(Cell(255, 128, 512, 0, 1, f, alpha=0.5))
    CELLS.append(Cell(127, 28, 36, 0, 0, f))
# edge shapes: M, N, K over the sets of the issue; ta / tb forms
for M, N, K, ta, tb in [(1, 4, 4, 0, 0), (4, 28, 28, 0, 1), (127, 128, 36, 0, 0), (128, 132, 68, 1, 1), (129, 4, 512, 0, 1),
                        (255, 260, 1028, 0, 0), (257, 28, 512, 0, 1), (1000, 128, 512, 1, 1), (1000, 132, 68, 0, 1), (1000, 260, 512, 0, 0),
                        (256, 128, 1028, 1, 1), (4, 260, 512, 1, 1), (128, 4, 4, 1, 1)]:
    CELLS.append(Cell(M, N, K, ta, tb, B_ | R_, alpha=1.25))
# scalar epilogue: N % 4 != 0 (tb = 0), ldc % 4 != 0, a bias that is not 16-byte aligned
for M, K in [(257, 512), (129, 36)]:
    CELLS.append(Cell(M, 130, K, 0, 0, B_ | R_ | U_, pc=2))
    CELLS.append(Cell(M, 130, K, 0, 0, A_ | T_ | M_, alpha=-2.0))
    CELLS.append(Cell(M, 132, K, 0, 1, B_ | M_, pc=1))
    CELLS.append(Cell(M, 132, K, 0, 0, B_ | R_, bias_off=1))
# split-K: 33 k tiles over 2 and 7 ranges (K = 1028), an empty last range (K = 512, splits = 7: 96-wide ranges), ACCUM,
# column sums of A (ta = 1), a scalar partial store (N % 4 != 0)
for M, N, K, ta, tb, sp, f, cs in [(257, 28, 1028, 0, 0, 2, 0, False), (257, 28, 1028, 0, 0, 7, A_, False),
                                   (128, 132, 512, 1, 1, 7, 0, True), (256, 260, 512, 1, 1, 2, A_, True),
                                   (256, 128, 68, 1, 1, 7, 0, True), (128, 130, 1028, 0, 0, 7, A_, False),
                                   (1000, 128, 512, 0, 1, 1, A_, False)]:
    CELLS.append(Cell(M, N, K, ta, tb, f, splits=sp, pc=0, colsum=cs))
# batched with gaps between the batch strides of A, B and C, and two-level k on A / on B
for M, N, K, ta, tb, bo, bi, akb, bkb, sp, f in [
        (257, 128, 512, 0, 1, 2, 3, 0, 0, 1, B_ | R_ | U_), (129, 132, 68, 0, 0, 1, 2, 0, 0, 1, M_ | R_),
        (256, 128, 512, 0, 0, 2, 2, 64, 0, 1, A_), (256, 260, 512, 0, 0, 1, 3, 0, 128, 1, B_),
        (128, 128, 96, 0, 0, 2, 1, 32, 32, 1, T_), (256, 128, 1028, 1, 1, 2, 2, 0, 0, 7, 0),
        (255, 28, 512, 0, 0, 1, 3, 64, 64, 2, A_)]:
    CELLS.append(Cell(M, N, K, ta, tb, f, bo=bo, bi=bi, gap=(0 if sp > 1 else 36), a_kb=akb, b_kb=bkb, splits=sp,
                      pc=(0 if sp > 1 else 4), colsum=(ta == 1 and sp > 1)))
# causal attention products at the attention shape: 256-token blocks, B x H = 2 x 2 batches (vt_attention.py's backward)
CELLS += [Cell(256, 128, 256, 1, 1, KMIN, bo=2, bi=2, gap=12, name="causal_kmin_dV"),
          Cell(256, 256, 128, 0, 0, KTILE, bo=2, bi=2, gap=12, name="causal_tile_dP"),
          Cell(256, 128, 256, 0, 1, KMAX, bo=2, bi=2, gap=12, name="causal_kmax_dQ"),
          Cell(256, 128, 256, 1, 1, KMIN | A_, bo=2, bi=2, gap=12, alpha=0.5, name="causal_kmin_accum")]


@pytest.mark.parametrize("c", CELLS, ids=repr)
def test_cell(mode, c):
    o = _operands(c)
    cbuf, colsum = _launch(c, o)
    _check_cell(c, o, cbuf, colsum, c.flags)
    cbuf2, colsum2 = _launch(c, o)
    assert torch.equal(cbuf.bits(), cbuf2.bits()), "a second launch gave other bits"
    if colsum is not None:
        assert torch.equal(colsum.view(torch.int32), colsum2.view(torch.int32))


@pytest.mark.parametrize("c", [Cell(257, 260, 512, 0, 0, B_ | R_ | U_, alpha=-0.75), Cell(1000, 132, 68, 0, 1, R_ | M_),
                               Cell(256, 128, 512, 1, 1, 0), Cell(129, 28, 36, 0, 0, B_, alpha=1.5)], ids=repr)
def test_plain_equals_accum_into_zeros(mode, c):
    """The fast epilogue (epilogue_fast.h) and lvt_epilogue_vec (taken for ACCUM) promise the same bits: C = epi(..) against
    C = 0; C += epi(..)."""
    o = _operands(c)
    plain, _ = _launch(c, o)
    o["cold"] = torch.zeros_like(o["cold"])
    accum, _ = _launch(c, o, flags=c.flags | A_)
    assert torch.equal(plain.bits(), accum.bits())


@pytest.mark.parametrize("c", [Cell(257, 260, 512, 0, 0, B_ | R_ | U_ | M_, alpha=-0.75), Cell(129, 132, 68, 0, 1, B_, alpha=1.5),
                               Cell(255, 128, 512, 0, 1, B_ | T_, alpha=0.5), Cell(127, 28, 36, 0, 0, B_ | A_, alpha=3.0)],
                         ids=repr)
def test_vec_epilogue_equals_scalar_epilogue(mode, c):
    """Same launch, ldc = N, bias aligned (float4 epilogues) and bias one float off (the scalar lvt_epilogue): same bits."""
    c.pc = 0
    o = _operands(c)
    vec, _ = _launch(c, o, bias_off=0)
    sca, _ = _launch(c, o, bias_off=1)
    _check_cell(c, o, sca, None, c.flags)
    assert torch.equal(vec.bits(), sca.bits())


@pytest.mark.parametrize("c", [Cell(257, 132, 512, 0, 0, B_ | R_, alpha=1.5), Cell(129, 28, 68, 0, 1, T_),
                               Cell(256, 128, 256, 0, 1, 0, bo=1, bi=2, gap=4)], ids=repr)
def test_planes_are_the_exact_bf16_split(mode, c):
    """PLANES: p1 = RNE_bf16(v), p2 = RNE_bf16(v - p1), p3 = v - p1 - p2 exactly, v = the fp32 C of the same launch."""
    o = _operands(c)
    M, N = c.M, c.N
    ref, _ = _launch(c, o)
    v = ref.logical()
    plane = _r4(int(o["cidx"].max()) + 1 + 8)
    img = torch.zeros(PAD + 3 * plane + PAD, dtype=torch.bfloat16, device=DEV)
    _record(o["abuf"].view, o["A"])
    _record(o["bbuf"].view, o["B"])
    kw = {}
    if c.flags & B_:
        kw["bias"] = o["bias"].to(DEV)
    if c.flags & R_:
        kw["res"], kw["ldr"] = Buf(o["cidx"], o["res"]).view, o["ldc"]
    args = (o["abuf"].view, o["bbuf"].view, img[PAD:], M, N, c.K)
    kwargs = dict(ta=c.ta, tb=c.tb, lda=o["lda"], ldb=o["ldb"], ldc=o["ldc"], batch_outer=c.bo, batch_inner=c.bi, sA=o["sA"],
                  sB=o["sB"], sC=o["sC"], alpha=c.alpha, flags=c.flags | L.EPI_PLANES, c_plane=plane, **kw)
    if mode == "f32":
        with pytest.raises(L.LvtError):
            G.gemm(*args, **kwargs)
        return
    G.gemm(*args, **kwargs)
    im = img.cpu()[PAD:]
    p1, p2, p3 = (im[j * plane + o["cidx"]].float() for j in range(3))
    e1 = v.to(torch.bfloat16).float()
    e2 = (v - e1).to(torch.bfloat16).float()
    e3 = v - e1 - e2
    assert torch.equal(p1, e1) and torch.equal(p2, e2) and torch.equal(p3, e3)


def test_many_tile_wide_launch(mode):
    """8192 x 4096 x 512: 1024 wide tiles, two rounds of the 512 resident workgroup slots; a seeded sample of 640 rows
    against fp64, C inside a NaN-payload buffer, and the record of max |C|."""
    M, N, K = 8192, 4096, 512
    g = torch.Generator().manual_seed(5)
    A, Bt = _rand((M, K), g), _rand((N, K), g)
    bias = _rand((N,), g)
    a, b = A.to(DEV), Bt.to(DEV)
    _record(a, A)
    _record(b, Bt)
    cb = torch.full((PAD + M * N + PAD,), PAYLOAD, dtype=torch.int32, device=DEV).view(torch.float32)
    cv = cb[PAD:PAD + M * N]
    G.gemm(a, b, cv, M, N, K, flags=B_ | U_, bias=bias.to(DEV), alpha=0.5)
    rows = torch.cat([torch.tensor([0, M - 1]), torch.randperm(M, generator=g)[:638]])
    Cg = cv.view(M, N)[rows.to(DEV)].cpu().double()
    A64 = A[rows].double()
    ref = (0.5 * (A64 @ Bt.double().t()) + bias.double()).clamp_min(0)
    tol = EPS_ACC * 0.5 * (A64.abs() @ Bt.double().abs().t()) + EPS_EPI * (bias.double().abs() + ref.abs())
    assert bool(((Cg - ref).abs() <= tol).all())
    edge = cb.view(torch.int32)
    assert bool((edge[:PAD] == PAYLOAD).all()) and bool((edge[PAD + M * N:] == PAYLOAD).all())
    if L.f16x2():
        assert float(L.amax_of(cv)) == float(cv.abs().max())


def test_operand_spanning_two_tensors(mode):
    """a_also / b_also: batch 1 of A and B lives in another allocation (batch stride = address difference) with values 1000x
    larger; in f16x2 the operand scale must come from both records."""
    M, N, K = 257, 132, 512
    g = torch.Generator().manual_seed(9)
    A0, A1 = _rand((M, K), g), _rand((M, K), g) * 1000
    B0, B1 = _rand((K, N), g), _rand((K, N), g) * 1000
    a0, a1, b0, b1 = (t.to(DEV) for t in (A0, A1, B0, B1))
    for t, h in ((a0, A0), (a1, A1), (b0, B0), (b1, B1)):
        _record(t, h)
    out = torch.empty(2, M, N, device=DEV)
    G.gemm(a0, b0, out, M, N, K, ta=0, tb=1, batch_inner=2, sA=(0, (a1.data_ptr() - a0.data_ptr()) // 4),
           sB=(0, (b1.data_ptr() - b0.data_ptr()) // 4), sC=(0, M * N), a_also=a1, b_also=b1)
    for z, (A, Bm) in enumerate(((A0, B0), (A1, B1))):
        ref = A.double() @ Bm.double()
        tol = EPS_ACC * (A.double().abs() @ Bm.double().abs()) + EPS_EPI * ref.abs()
        assert bool(((out[z].cpu().double() - ref).abs() <= tol).all()), z


def test_written_views_and_split_k_leave_no_stale_record():
    """LVT_AMAX_CHECK semantics: a recorded C is rewritten through a view (1000x larger values) and by a split-K launch, then
    used as an f16x2 operand: no stale record may be used, and the product is fp64-accurate."""
    before, old_check = L.get_math_mode(), L.AMAX_CHECK
    L.set_math_mode("f16x2")
    L.AMAX_CHECK = True
    try:
        g = torch.Generator().manual_seed(11)
        A, Bt, W = _rand((512, 256), g), _rand((256, 256), g), _rand((128, 256), g)
        a, b, w = A.to(DEV), Bt.to(DEV), W.to(DEV)
        out = torch.empty(512, 256, device=DEV)
        G.gemm(a, b, out, 512, 256, 256)                                  # out carries a record ~ max |A B^T|
        big = a[:128] * 1000
        G.gemm(big, b, out[0:128], 128, 256, 256)                          # a view of out rewritten, 1000x larger
        # split-K: a weight-gradient style launch rewrites the whole of `out2` after a recorded launch wrote it
        out2 = torch.empty(256, 256, device=DEV)
        G.gemm(b, b, out2, 256, 256, 256)
        G.gemm(a * 1000, a, out2, 256, 256, 512, ta=1, tb=1, lda=256, ldb=256, splits=7)
        for C_ in (out, out2):
            y = torch.empty(C_.shape[0], 128, device=DEV)
            G.gemm(C_, w, y, C_.shape[0], 128, 256)
            Ch = C_.cpu().double()
            ref = Ch @ W.double().t()
            tol = EPS_ACC * (Ch.abs() @ W.double().abs().t())
            assert bool(((y.cpu().double() - ref).abs() <= tol).all())
    finally:
        L.AMAX_CHECK = old_check
        L.set_math_mode(before)
