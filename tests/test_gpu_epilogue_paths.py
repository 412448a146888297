"""The float4 epilogue of the matrix-core engine kernels (lvt_amd/csrc/epilogue_fast.h) against the library's scalar epilogue.

Reference: the same launch with a C pointer that is one float off a 16-byte boundary -- launch_wide / launch_tile then clear
vec_epi and the kernel runs the scalar lvt_epilogue, whose arithmetic is documented as identical.  Every case compares the two C
bit for bit (torch.equal) and the float4 one against fp64 with the bound of tests/test_gpu_gemm_matrix.py (EPS_ACC, EPS_EPI are
imported from there): |C - C64| <= EPS_ACC |alpha| (|A||B|) + EPS_EPI (|bias| + |res| + |C64|).

What the cases walk (f16x2 arithmetic, lvt_gemm_wide_kernel unless said otherwise):
  * the flag sets of the models' launches -- 0, BIAS, BIAS|RELU, BIAS|RESIDUAL, RESIDUAL, MASK, RESIDUAL|MASK -- in the NT / NN / TN
    forms, and the split-K partial store of the TN form (splits = 2, 3; the column sums of A with it).  A split-K launch stores
    through the workspace pointer, not through C, so its reference is assembled from one scalar-epilogue launch per k range, summed
    in lvt_reduce_splits_kernel's order;
  * M = 256 + 36, N = 128 + 4, K = 64: a full and a ragged tile in each direction, the ragged column quad in and out of range, rows
    past M in both 32-row rounds of a wave; and the exact single tile 256 x 128 x 32;
  * what decides between the forms of the float4 epilogue: alpha = 1 / 0.5, residual and mask with ldr == ldc and with a wider
    leading dimension (a column slice of a wider tensor), a batched launch (the second batch has a non-zero offset into C);
  * max |C|: the device scalar equals C.abs().max() bit for bit after every case, also when it held a smaller value before the
    launch; one that held a larger value keeps it;
  * the two frame row maps of lvt_conv_patch_kernel: a 3x3 256 -> 128 convolution on two 16x16 frames and the 4x4 stride-2
    transposed pass on two frames, against the implicit-GEMM route of the conv engine (the same frames as T = 2 of one clip fall
    outside the frame-resident geometry; lvt_conv3d_bwd_data without phase weights) and against fp64 (tests/util_conv.py).
No operand is zero everywhere (tests/test_gpu_degenerate_scale.py covers what f16x2 makes of one)."""
import ctypes as C

import pytest
import torch

import util_conv as U
from lvt_amd.hip import binding as L, gemm as G
from test_gpu_gemm_matrix import EPS_ACC, EPS_EPI
from util_guard import PAD, Buf, rows_idx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_, R_, U_, M_ = L.EPI_BIAS, L.EPI_RESIDUAL, L.EPI_RELU, L.EPI_MASK
FLAG_SETS = [0, B_, B_ | U_, B_ | R_, R_, M_, R_ | M_]
FORMS = {"NT": (0, 0), "NN": (0, 1), "TN": (1, 1)}
RAGGED = (256 + 36, 128 + 4, 64)
SINGLE = (256, 128, 32)


@pytest.fixture(autouse=True)
def f16x2():
    before, check = L.get_math_mode(), L.AMAX_CHECK
    L.set_math_mode("f16x2")
    L.AMAX_CHECK = False
    yield
    L.AMAX_CHECK = check
    L.set_math_mode(before)


def _rand(shape, g):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float() * 2.0 - 1.0


def _slot(value=0.0):
    return L.amax_slot(torch.device(DEV)).fill_(value)


# ---- operands and fp64 results: once per (shape, form, batch), shared, never modified ------------------------------------
_OPS = {}


def _ops(M, N, K, form, Z=1):
    key = (M, N, K, form, Z)
    if key not in _OPS:
        ta, tb = FORMS[form]
        g = torch.Generator().manual_seed(4000 + M * 7 + N * 13 + K * 17 + 5 * ta + 3 * tb + Z)
        A, Bm = _rand((Z, M, K), g), _rand((Z, K, N), g)
        o = dict(A=A, B=Bm, ta=ta, tb=tb)
        o["a"] = (A.transpose(1, 2) if ta else A).contiguous().to(DEV)           # (Z, K, M) m-contiguous / (Z, M, K)
        o["b"] = (Bm if tb else Bm.transpose(1, 2)).contiguous().to(DEV)         # (Z, K, N) n-contiguous / (Z, N, K)
        o["sa"], o["sb"] = _slot(float(A.abs().max())), _slot(float(Bm.abs().max()))
        o["bias"], o["res"] = _rand((N,), g), _rand((Z, M, N), g)
        o["mask"] = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, (Z, M, N), generator=g)]
        o["acc"], o["mag"] = A.double() @ Bm.double(), A.double().abs() @ Bm.double().abs()
        _OPS[key] = o
    return _OPS[key]


def _gemm(o, a, b, cview, M, N, K, ldc, flags=0, alpha=1.0, bias=None, res=None, ldr=0, mask=None, ldm=0, splits=1, colsum=None,
          c_slot=None, Z=1, sA=0, sB=0, sC=0):
    """lvt_gemm_f32 with explicit max |.| scalars (gemm.gemm attaches a fresh zeroed one to C)."""
    d = L.GemmDesc()
    d.M, d.N, d.K, d.ta, d.tb = M, N, K, o["ta"], o["tb"]
    d.A, d.lda = a.data_ptr(), (M if o["ta"] else K)
    d.B, d.ldb = b.data_ptr(), (N if o["tb"] else K)
    d.C, d.ldc = cview.data_ptr(), ldc
    d.batch_outer, d.batch_inner = 1, Z
    d.sA_o, d.sA_i, d.sB_o, d.sB_i, d.sC_o, d.sC_i = 0, sA, 0, sB, 0, sC
    d.alpha, d.flags = alpha, flags | L.math_flag()
    d.bias = bias.data_ptr() if bias is not None else None
    d.res, d.ldr = (res.data_ptr() if res is not None else None), (ldr or ldc)
    d.mask, d.ldm = (mask.data_ptr() if mask is not None else None), (ldm or ldc)
    d.splits = splits
    d.a_colsum = colsum.data_ptr() if colsum is not None else None
    d.a_amax, d.b_amax = o["sa"].data_ptr(), o["sb"].data_ptr()
    d.c_amax = c_slot.data_ptr() if c_slot is not None else None
    ws, nws = None, 0
    if splits > 1:
        nws = L.lib().lvt_gemm_workspace_bytes(C.byref(d))
        ws = L.workspace(nws, a.device, "gemm")
    L.check(L.lib().lvt_gemm_f32(C.byref(d), L.ptr(ws), nws, L.stream_ptr()), "lvt_gemm_f32")
    torch.cuda.synchronize()


def _wide_parent(t, ld, lead):
    """`t` (Z, M, N) as a column slice [lead, lead + N) of a (Z, M, ld) tensor of other values -> (view of the first element, ld)."""
    Z, M, N = t.shape
    parent = torch.full((Z, M, ld), 7.5)
    parent[:, :, lead:lead + N] = t
    dev = parent.to(DEV)
    return dev.view(-1)[lead:], dev


def _run(M, N, K, form, flags, alpha=1.0, aligned=True, pc=4, wide_ld=False, Z=1, seed=0.0):
    """One launch; C in a NaN-payload buffer with row pitch N + pc, its pointer 16-byte aligned or one float off.  Returns (C of
    the batches (Z, M, N), the whole buffer's bits, max |C| scalar)."""
    o = _ops(M, N, K, form, Z)
    ldc = N + pc
    sC = (M * ldc + 36 + 3) // 4 * 4 if Z > 1 else 0
    cidx = (torch.arange(Z) * sC)[:, None, None] + rows_idx(M, N, ldc)[None]
    cbuf = Buf(cidx, start=PAD if aligned else PAD + 1)
    kw, keep = {}, []
    if flags & B_:
        kw["bias"] = o["bias"].to(DEV)
    for f, name, ld in ((R_, "res", "ldr"), (M_, "mask", "ldm")):
        if flags & f:
            if wide_ld:                                    # a single batch: the operand follows C's batch stride otherwise
                assert Z == 1
                kw[name], parent = _wide_parent(o[name], ldc + 8, 4)
                kw[ld] = ldc + 8
                keep.append(parent)
            else:
                kw[name], kw[ld] = Buf(cidx, o[name]).view, ldc
    slot = _slot(seed)
    _gemm(o, o["a"], o["b"], cbuf.view, M, N, K, ldc, flags=flags, alpha=alpha, c_slot=slot, Z=Z, sA=M * K, sB=K * N, sC=sC, **kw)
    assert cbuf.outside_untouched(), "a float outside the logical C was written"
    return cbuf.logical(), slot


def _ref64(o, flags, alpha):
    v = alpha * o["acc"]
    extra = torch.zeros_like(v)
    if flags & B_:
        v = v + o["bias"].double()
        extra = extra + o["bias"].double().abs()
    if flags & R_:
        v = v + o["res"].double()
        extra = extra + o["res"].double().abs()
    if flags & U_:
        v = v.clamp_min(0.0)
    if flags & M_:
        v = torch.where(o["mask"].double() > 0, v, torch.zeros_like(v))
    return v, EPS_ACC * abs(alpha) * o["mag"] + EPS_EPI * (extra + v.abs())


def _check(M, N, K, form, flags, alpha=1.0, **kw):
    o = _ops(M, N, K, form, kw.get("Z", 1))
    got, slot = _run(M, N, K, form, flags, alpha, aligned=True, **kw)
    want, slot_ref = _run(M, N, K, form, flags, alpha, aligned=False, **kw)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "float4 and scalar epilogue differ in %d elements" % int(
        (got.view(torch.int32) != want.view(torch.int32)).sum())
    ref, tol = _ref64(o, flags, alpha)
    err = (got.double() - ref).abs()
    assert bool((err <= tol).all()), "worst error / bound %r" % float((err / tol.clamp_min(1e-300)).max())
    seed = kw.get("seed", 0.0)
    top = max(seed, float(got.abs().max()))
    assert float(slot) == top and float(slot_ref) == top, ("max |C|", float(slot), float(slot_ref), top)


# ---- the flag sets and forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "f%x" % f)
def test_flag_sets_ragged_tiles(form, flags):
    _check(*RAGGED, form, flags)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", [0, B_ | R_, R_ | M_], ids=lambda f: "f%x" % f)
def test_exact_single_tile(form, flags):
    _check(*SINGLE, form, flags, pc=0)


# ---- what selects the form of the float4 epilogue ------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("flags", [0, B_ | R_, B_ | U_, R_ | M_], ids=lambda f: "f%x" % f)
def test_alpha(flags, alpha):
    _check(*RAGGED, "NT", flags, alpha=alpha)
    _check(*SINGLE, "NN", flags, alpha=alpha, pc=0)


@pytest.mark.parametrize("wide_ld", [False, True], ids=["ldr_eq_ldc", "ldr_wider"])
@pytest.mark.parametrize("flags", [R_, M_, R_ | M_, B_ | R_], ids=lambda f: "f%x" % f)
def test_residual_and_mask_leading_dimension(flags, wide_ld):
    _check(*RAGGED, "NT", flags, wide_ld=wide_ld)
    _check(*SINGLE, "NT", flags, wide_ld=wide_ld, pc=0)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", [0, B_ | R_, R_ | M_], ids=lambda f: "f%x" % f)
def test_batched_launch_with_an_offset_into_c(form, flags):
    _check(*RAGGED, form, flags, Z=2)
    _check(*SINGLE, form, flags, Z=2, pc=0)


@pytest.mark.parametrize("seed", [2.0 ** -20, 1.0e6], ids=["smaller", "larger"])
@pytest.mark.parametrize("shape", [RAGGED, SINGLE], ids=["ragged", "single"])
def test_max_c_scalar_seeded_before_the_launch(shape, seed):
    _check(*shape, "NT", B_ | R_, seed=seed)
    _check(*shape, "TN", 0, seed=seed)


# ---- split-K partial store (TN, column sums of A) -------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("shape", [(256 + 36, 128 + 4, 64), (256, 128, 64)], ids=["ragged", "single"])
def test_split_k_partial_store(shape, splits):
    """C = sum over the k ranges of the partial tiles; a range's partial tile equals a splits = 1 launch over that range (same
    operand scales, alpha = 1, no flags) -- taken here through the scalar epilogue -- and lvt_reduce_splits_kernel adds the ranges
    in order into one running sum for fewer than five of them, then adds three zero sums."""
    M, N, K = shape
    o = _ops(M, N, K, "TN")
    cbuf = Buf(rows_idx(M, N, N))
    colsum = torch.full((1, M), float("nan"), device=DEV)
    _gemm(o, o["a"], o["b"], cbuf.view, M, N, K, N, splits=splits, colsum=colsum)
    assert cbuf.outside_untouched()
    got = cbuf.logical()
    per = ((K + splits - 1) // splits + 31) // 32 * 32
    total = None
    for s in range(splits):
        k0, k1 = min(s * per, K), min((s + 1) * per, K)
        if k1 > k0:
            part = Buf(rows_idx(M, N, N), start=PAD + 1)
            _gemm(o, o["a"][0, k0:k1], o["b"][0, k0:k1], part.view, M, N, k1 - k0, N)
            p = part.logical()
        else:
            p = torch.zeros(M, N)
        total = p if total is None else total + p
    total = (total + 0.0) + (0.0 + 0.0)
    assert torch.equal(got.view(torch.int32), total.view(torch.int32)), "%d elements differ" % int((got != total).sum())
    ref = o["acc"][0]
    assert bool(((got.double() - ref).abs() <= EPS_ACC * o["mag"][0] + EPS_EPI * ref.abs()).all())
    A = o["A"][0].double()
    assert bool(((colsum[0].double().cpu() - A.sum(1)).abs() <= EPS_ACC * A.abs().sum(1)).all()), "a_colsum"


# ---- the frame row maps of lvt_conv_patch_kernel --------------------------------------------------------------------------
def _conv_operands(c):
    x, w, dy = U.operands(c)
    xd, wd, dyd = U.to_cl(x, c.ci).to(DEV), w.to(DEV), U.to_cl(dy, c.co).to(DEV)
    g = torch.Generator().manual_seed(77)
    return x, w, dy, xd, wd, dyd, g


def _close(got, ref, mag, bias, res, what):
    tol = U.tol(mag, ref, bias, res)
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= tol).all()), "%s: worst error / bound %r" % (what, float((err / tol).max()))


@pytest.mark.parametrize("flags", [B_ | R_, R_ | M_], ids=lambda f: "f%x" % f)
def test_frame_row_map_of_the_3x3_convolution(flags):
    """3x3 / pad 1, 256 -> 128 channels, two 16x16 frames: lvt_conv_patch_kernel<0> (N = 2, T = 1) against the implicit GEMM that
    serves the same frames as N = 1, T = 2 (patch_conv_eligible wants Ti == 1)."""
    c = U.ConvCell("frames16_k3_256to128", (2, 1, 16, 16), 256, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    x, w, _, xd, wd, _, g = _conv_operands(c)
    g_patch = G.conv_geom(2, 1, 16, 16, 256, 128, c.kernel, c.stride, c.pad)
    g_gemm = G.conv_geom(1, 2, 16, 16, 256, 128, c.kernel, c.stride, c.pad)
    assert G.uses_patch_kernel(g_patch) and not G.uses_patch_kernel(g_gemm)
    shape = (2, 1, 16, 16, 128)
    bias, res = U.rand((128,), g), U.rand(shape, g)
    mask = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, shape, generator=g)]
    kw = dict(bias=bias.to(DEV) if flags & B_ else None, res=res.to(DEV) if flags & R_ else None,
              mask=mask.to(DEV) if flags & M_ else None)
    wp = G.pack_weight(g_patch, wd, 256, 128)
    y_patch = G.conv_fwd(g_patch, xd, wp, **kw)
    y_gemm = G.conv_fwd(g_gemm, xd.view(1, 2, 16, 16, 256), wp, **{k: (v.view(1, 2, 16, 16, 128) if v is not None and v.dim() == 5 else v)
                                                                    for k, v in kw.items()})
    torch.cuda.synchronize()
    acc = U.to_cl(U.conv_ref(x, w, c.kernel, c.stride, c.pad, c.out), 128)
    mag = U.to_cl(U.conv_ref(x.abs(), w.abs(), c.kernel, c.stride, c.pad, c.out), 128)
    ref = U.epilogue64(acc, flags, bias.double(), res.double(), mask.double())
    b64, r64 = (bias.double().expand_as(ref) if flags & B_ else None), (res.double() if flags & R_ else None)
    _close(y_patch, ref, mag, b64, r64, "frame-resident")
    _close(y_gemm.view(shape), ref, mag, b64, r64, "implicit GEMM")
    if flags & M_:
        assert torch.equal(y_patch.cpu()[mask <= 0], torch.zeros(int((mask <= 0).sum())))
    assert float(L.amax_of(y_patch)) == float(y_patch.abs().max()), "max |y|"


@pytest.mark.parametrize("flags", [B_ | R_, M_], ids=lambda f: "f%x" % f)
def test_frame_row_map_of_the_transposed_phases(flags):
    """Data gradient of the 4x4 / stride 2 / pad 1 convolution 128 -> 32 channels between 32x32 and 16x16 frames, two frames:
    lvt_conv_patch_kernel<1> (one phase per workgroup plane) against lvt_conv3d_bwd_data's implicit GEMM."""
    c = U.ConvCell("frames32_k4s2_128to32", (2, 1, 32, 32), 128, 32, (1, 4, 4), (1, 2, 2), (0, 1, 1))
    x, w, dy, _, wd, dyd, g = _conv_operands(c)
    geom = G.conv_geom(2, 1, 32, 32, 128, 32, c.kernel, c.stride, c.pad)
    assert G.bwd_data_by_phases(geom)
    shape = (2, 1, 32, 32, 128)
    bias, res = U.rand((128,), g), U.rand(shape, g)
    mask = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, shape, generator=g)]
    kw = dict(bias=bias.to(DEV) if flags & B_ else None, res=res.to(DEV) if flags & R_ else None,
              mask=mask.to(DEV) if flags & M_ else None)
    dx_patch = G.conv_bwd_data(geom, dyd, None, wph=G.pack_weight_phases(geom, wd, 128, 32), **kw)
    dx_gemm = G.conv_bwd_data(geom, dyd, G.pack_weight(geom, wd, 128, 32), **kw)
    torch.cuda.synchronize()
    b = U.bounds(c, x, w, dy)
    acc, mag = U.to_cl(b["dx"], 128), U.to_cl(b["mag_dx"], 128)
    ref = U.epilogue64(acc, flags, bias.double(), res.double(), mask.double())
    b64, r64 = (bias.double().expand_as(ref) if flags & B_ else None), (res.double() if flags & R_ else None)
    _close(dx_patch, ref, mag, b64, r64, "frame-resident")
    _close(dx_gemm, ref, mag, b64, r64, "implicit GEMM")
    if flags & M_:
        assert torch.equal(dx_patch.cpu()[mask <= 0], torch.zeros(int((mask <= 0).sum())))
    assert float(L.amax_of(dx_patch)) == float(dx_patch.abs().max()), "max |dx|"
