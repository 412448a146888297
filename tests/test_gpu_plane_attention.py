"""The plane attention kernels (csrc/attention_pipe.hip: lvt_attn_fwd_planes, lvt_attn_bwd_planes = kernels A16 and B16 + the
bank reduce) against an fp64 evaluation of the reference formula and its autograd backward (util_attention.reference): output,
the saved attention matrix, dq / dk / dv and the three bias-bank gradients; both block geometries, masked and not; the smallest
launch, a head count other than 8 and an odd sample count; zero rows; guard buffers; the host-side refusals; and the max-|.|
records that the plane AND the flash kernels hand to the next f16x2 GEMM.

The operands are built on the host as the exact 3-way bf16 split (util_attention.bf16x3_split) of fp32 tensors, and every test
first checks on the CPU that the planes restore the fp32 operand bit for bit: the fp64 reference then takes the fp32 operands."""
import ctypes as C
import math

import pytest
import torch

from util_attention import DA, S, bf16x3_split, judge, rand, reference, split_restores
from util_guard import Buf, dense, fbuf, obuf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOMS = [(1, 16, 16), (4, 8, 8)]
NAMES = ["o", "P", "dq", "dk", "dv", "ddt", "ddh", "ddw"]
REF_IDX = [0, 9, 3, 4, 5, 6, 7, 8]             # where util_attention.reference keeps them


@pytest.fixture
def math_mode():
    """set(mode) for the length of one test; the mode of the session is restored afterwards."""
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    yield L.set_math_mode
    L.set_math_mode(before)


def _split_checked(x):
    p = bf16x3_split(x)
    assert split_restores(x, p)
    return p


def _operands(q, k, v, go):
    """-> qkvp (3 operands, 3 planes, M, hd), dop (3 planes, M, hd) bf16 on the device."""
    return torch.stack([_split_checked(t) for t in (q, k, v)]).to(DEV).contiguous(), _split_checked(go).to(DEV).contiguous()


def _planes(q, k, v, go, banks, blk, masked):
    """Forward, then the backward fed the forward's own P and o (as the layer does) -> NAMES order."""
    from lvt_amd.hip import tx
    B, H = q.shape[0] // S, q.shape[1] // DA
    qkvp, dop = _operands(q, k, v, go)
    bd = [t.to(DEV).contiguous() for t in banks]
    P, o = tx.attn_fwd_planes(qkvp, B, H, S, DA, math.sqrt(DA), bd[0], bd[1], bd[2], blk, masked)
    dqkv, ddt, ddh, ddw = tx.attn_bwd_planes(qkvp, dop, P, o, B, H, S, DA, math.sqrt(DA), blk, masked)
    torch.cuda.synchronize()
    return [o, P, dqkv[0], dqkv[1], dqkv[2], ddt, ddh, ddw]


def _pick(ref):
    return [ref[i] for i in REF_IDX]


@pytest.mark.parametrize("BH", [(1, 8), (2, 4), (3, 8)], ids=lambda p: "B%dH%d" % p)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("blk", GEOMS)
def test_planes_vs_fp64(blk, masked, BH, math_mode):
    """o, P, dq, dk, dv and the bank gradients against fp64: err < max(2e-5 * scale, 4 * err32), err32 = the error of the same
    formula in fp32 torch.  (1, 8) is the smallest launch (8 pairs), (2, 4) indexes the banks with pair % 4, (3, 8) = 24 pairs
    wraps the pairing of block ids 8 apart.

    Worst err / err32 over the 12 cases on an MI355X (the test prints every figure): o 1.19, P 1.04, dq 1.19, dk 1.57, dv 1.38,
    ddt 1.72, ddh 0.41, ddw 0.44; the worst err / scale was 1.1e-6 (dq), so every case is also inside the 2e-5 * scale arm."""
    math_mode("bf16x3")                        # the arithmetic in which these kernels are the default path
    B, H = BH
    hd = H * DA
    q, k, v, go = (rand(B * S, hd, seed=s) for s in (1, 2, 3, 4))
    q = q * 3.0                                                                        # scores of a few units: a peaked softmax
    banks = [rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    ref = _pick(reference(q, k, v, go, banks, blk, masked))
    ref32 = _pick(reference(q, k, v, go, banks, blk, masked, dtype=torch.float32))
    got = _planes(q, k, v, go, banks, blk, masked)
    bank_scale = max(float(r.abs().max()) for r in ref[5:])
    for n, a, r, r32 in zip(NAMES, got, ref, ref32):
        assert a.shape == r.shape, (n, a.shape, r.shape)
        # (the gradient of a one-entry bank is sum_ij g_ij == 0 up to rounding: judged against the scale of the other banks)
        err, err32, scale = judge(n, a, r, r32, scale=bank_scale if n.startswith("dd") else None)
        print("planes_vs_fp64 %s masked=%d B=%d H=%d %s err=%.3e err32=%.3e ratio=%.3f rel=%.3e"
              % (blk, masked, B, H, n, err, err32, err / max(err32, 1e-300), err / scale))
    if masked:
        P = got[1].cpu()
        assert float(P.triu(1).abs().max()) == 0.0                   # structural zeros: exp(fill - m) == 0 exactly
        assert torch.isfinite(got[3]).all() and torch.isfinite(got[4]).all()


@pytest.mark.parametrize("blk", GEOMS)
def test_planes_zero_rows_and_zero_gradients(blk, math_mode):
    """The zero-row case of test_gpu_flash_attention.py on the plane kernels: a zero q row, zero k rows, a sample whose dO is
    zero, a (sample, head) whose dO is zero and one whose V is zero."""
    math_mode("bf16x3")
    B, H = 2, 8
    hd = H * DA
    q, k, v, go = (rand(B * S, hd, seed=s) for s in (11, 12, 13, 14))
    go[:S] = 0                                  # sample 0: no gradient at all
    go[S:, :DA] = 0                             # sample 1, head 0 alike
    v[S:, DA:2 * DA] = 0                        # sample 1, head 1: V == 0
    q[5] = 0; k[7] = 0; k[S + 9] = 0
    banks = [rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    for masked in (False, True):
        ref = _pick(reference(q, k, v, go, banks, blk, masked))
        got = _planes(q, k, v, go, banks, blk, masked)
        bank_scale = max(float(r.abs().max()) for r in ref[5:])
        for n, a, r in zip(NAMES, got, ref):
            assert torch.isfinite(a).all(), n
            scale = bank_scale if n.startswith("dd") else float(r.abs().max())
            assert float((a.double().cpu() - r).abs().max()) < 2e-5 * scale, (n, masked)
        assert float(got[2][:S].abs().max()) == 0.0 and float(got[4][:S].abs().max()) == 0.0     # sample 0: dq == dv == 0


def _bbuf(t):
    """bf16 tensor (even element count) -> Buf that holds its bits; .view is the bf16 device view."""
    bits = t.contiguous().view(-1).view(torch.float32)
    return Buf(dense(bits.numel()), bits, dtype=torch.bfloat16)


@pytest.mark.parametrize("masked", [False, True])
def test_planes_in_guard_buffers(masked):
    """Straight through the C entry points with every input, every output, the max-|.| slots and the workspace inside
    NaN-payload buffers: nothing outside a logical output changes, every logical element is written, no padding is read."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    blk, B, H = (4, 8, 8), 1, 8
    M, hd = B * S, H * DA
    q, k, v, go = (rand(M, hd, seed=s) for s in (21, 22, 23, 24))
    banks = [rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    qkvp = _bbuf(torch.stack([_split_checked(t) for t in (q, k, v)]))
    dop = _bbuf(_split_checked(go))
    bd = [fbuf(t) for t in banks]
    P, o, o_amax = obuf(B, H, S, S), obuf(M, hd), fbuf(torch.zeros(1))
    temper = math.sqrt(DA)
    L.check(lib.lvt_attn_fwd_planes(L.ptr(qkvp.view), M * hd, 3 * M * hd, B, H, S, DA, temper, L.ptr(bd[0].view), L.ptr(bd[1].view),
                                    L.ptr(bd[2].view), blk[0], blk[1], blk[2], int(masked), -1e4, L.ptr(P.view), L.ptr(o.view),
                                    L.ptr(o_amax.view), L.stream_ptr()), "lvt_attn_fwd_planes")
    nws = lib.lvt_attn_bwd_planes_workspace_bytes(B, H, S, blk[0], blk[1], blk[2])
    assert nws % 4 == 0
    ws = obuf(nws // 4)
    dq, dk, dv, d_amax = obuf(M, hd), obuf(M, hd), obuf(M, hd), fbuf(torch.zeros(1))
    dd = [obuf(H, 2 * n - 1) for n in blk]
    L.check(lib.lvt_attn_bwd_planes(L.ptr(qkvp.view), M * hd, 3 * M * hd, L.ptr(dop.view), L.ptr(P.view), L.ptr(o.view), B, H, S, DA,
                                    temper, blk[0], blk[1], blk[2], int(masked), L.ptr(dq.view), L.ptr(dk.view), L.ptr(dv.view),
                                    L.ptr(dd[0].view), L.ptr(dd[1].view), L.ptr(dd[2].view), L.ptr(d_amax.view), L.ptr(ws.view), nws,
                                    L.stream_ptr()), "lvt_attn_bwd_planes")
    torch.cuda.synchronize()
    outs = dict(P=P, o=o, dq=dq, dk=dk, dv=dv, ddt=dd[0], ddh=dd[1], ddw=dd[2], o_amax=o_amax, d_amax=d_amax)
    for n, b in outs.items():
        assert b.outside_untouched(), n
        val = b.logical()
        assert not torch.isnan(val).any(), n     # a payload NaN: an element nobody wrote; any other NaN: padding was read
    assert ws.outside_untouched()
    for b in (qkvp, dop, *bd):                   # (inputs are inputs)
        assert b.outside_untouched()
    ref = _pick(reference(q, k, v, go, banks, blk, masked))
    got = [outs[n].logical() for n in NAMES]
    bank_scale = max(float(r.abs().max()) for r in ref[5:])
    for n, a, r in zip(NAMES, got, ref):
        scale = bank_scale if n.startswith("dd") else float(r.abs().max())
        assert float((a.double().reshape(r.shape) - r).abs().max()) < 2e-5 * scale, n
    assert float(o_amax.logical()) == float(got[0].abs().max())
    assert float(d_amax.logical()) == max(float(got[i].abs().max()) for i in (2, 3, 4))


def test_planes_refusals():
    """Argument checks the entry points make on the host before any launch: an error code and a message, and not one output
    float changes."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    B, H, blk = 1, 8, (1, 16, 16)
    M, hd = B * S, H * DA
    # big enough for every (refused) shape below; nothing is ever read
    qkvp = torch.zeros(3, 3, M, hd, dtype=torch.bfloat16, device=DEV)
    dop = torch.zeros(3, M, hd, dtype=torch.bfloat16, device=DEV)
    banks = torch.zeros(H, 31, device=DEV)
    FILL = 7.0
    P = torch.full((B, H, S, S), FILL, device=DEV)
    o = torch.full((M + 1, hd), FILL, device=DEV)
    dqkv = torch.full((3, M + 1, hd), FILL, device=DEV)
    dd = torch.full((3, H, 31), FILL, device=DEV)
    amax = torch.full((1,), FILL, device=DEV)
    nws = lib.lvt_attn_bwd_planes_workspace_bytes(B, H, S, *blk)
    ws = torch.full((nws // 4,), FILL, device=DEV)
    temper = math.sqrt(DA)

    def fwd(B=B, H=H, S_=S, da=DA, blk=blk, ps=M * hd, o_off=0):
        return lib.lvt_attn_fwd_planes(L.ptr(qkvp), ps, 3 * M * hd, B, H, S_, da, temper, L.ptr(banks), L.ptr(banks), L.ptr(banks),
                                       blk[0], blk[1], blk[2], 0, -1e4, L.ptr(P), C.c_void_p(o.data_ptr() + 4 * o_off), L.ptr(amax),
                                       L.stream_ptr())

    def bwd(B=B, H=H, S_=S, da=DA, blk=blk, ps=M * hd, o_off=0, nws=nws):
        return lib.lvt_attn_bwd_planes(L.ptr(qkvp), ps, 3 * M * hd, L.ptr(dop), L.ptr(P), L.ptr(o), B, H, S_, da, temper, blk[0], blk[1],
                                       blk[2], 0, C.c_void_p(dqkv[0].data_ptr() + 4 * o_off), L.ptr(dqkv[1]), L.ptr(dqkv[2]),
                                       L.ptr(dd[0]), L.ptr(dd[1]), L.ptr(dd[2]), L.ptr(amax), L.ptr(ws), nws, L.stream_ptr())

    cases = [dict(H=4),                        # B * H = 4: no pairing per XCD
             dict(S_=512), dict(da=64), dict(blk=(2, 8, 16)),
             dict(ps=M * hd + 4),              # plane stride not a multiple of 8 elements
             dict(o_off=1)]                    # o / dq 4 bytes off a 16-byte boundary
    for kw in cases:
        for fn in (fwd, bwd):
            rc = fn(**kw)
            assert rc == -1, (fn.__name__, kw, rc)                                     # LVT_EINVAL
            assert len(lib.lvt_last_error()) > 0, (fn.__name__, kw)
    rc = fwd(H=4)
    assert rc == -1 and "multiple of 8" in lib.lvt_last_error().decode()
    rc = bwd(blk=(2, 8, 16))
    assert rc == -1 and "no instantiation" in lib.lvt_last_error().decode()
    rc = bwd(nws=nws - 1)
    assert rc == -2 and "workspace" in lib.lvt_last_error().decode()                    # LVT_EWORKSPACE
    torch.cuda.synchronize()
    for t in (P, o, dqkv, dd, amax, ws):
        assert bool((t == FILL).all())
    # the same buffers, legal arguments: accepted (the refusals above were about the arguments, not the buffers)
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool((o[:M] != FILL).any()) and bool((dqkv[:, :M] != FILL).any())


def _amax_case(where):
    """Operands whose backward maximum sits in dq (kernel A) or in dv (kernel B)."""
    B, H = 1, 8
    hd = H * DA
    q, k, v, go = (rand(B * S, hd, seed=s) for s in (31, 32, 33, 34))
    if where == "dq":
        k, v = k * 16.0, v * 16.0              # dq = dS K with dS ~ dO . V: both factors large; dv = P^T dO stays O(1)
    else:
        q, k, v = q * 0.25, k * 0.25, v * 0.25  # tiny dS; dv = P^T dO
        go = go * 8.0
    return B, H, q, k, v, go


@pytest.mark.parametrize("where", ["dq", "dv"])
def test_attention_outputs_carry_exact_amax_records(where, math_mode):
    """In the f16x2 arithmetic the next GEMM scales its operands by the max |.| that the attention kernels report: the record on
    `o` and on `dqkv` must equal torch's abs().max() of the tensor, whichever of the two backward kernels holds the maximum, and
    must come from the kernels (no stand-alone lvt_amax pass)."""
    from lvt_amd.hip import binding as L, tx
    math_mode("f16x2")
    blk, masked = (1, 16, 16), True
    B, H, q, k, v, go = _amax_case(where)
    banks = [(rand(H, 2 * n - 1, seed=5 + i) * 0.5).to(DEV) for i, n in enumerate(blk)]
    qkvp, dop = _operands(q, k, v, go)
    qkv = torch.stack([q, k, v]).to(DEV).contiguous()
    god = go.to(DEV).contiguous()
    temper = math.sqrt(DA)
    n0 = L.AMAX_FALLBACKS[0]

    def exact(t):
        return float(L.amax_of(t)) == float(t.abs().max())

    P, o = tx.attn_fwd_planes(qkvp, B, H, S, DA, temper, *banks, blk, masked)
    assert exact(o)
    dqkv, _, _, _ = tx.attn_bwd_planes(qkvp, dop, P, o, B, H, S, DA, temper, blk, masked)
    assert exact(dqkv)
    big = max(range(3), key=lambda i: float(dqkv[i].abs().max()))
    assert big == (0 if where == "dq" else 2), [float(dqkv[i].abs().max()) for i in range(3)]
    of, stats = tx.attn_fwd_flash(qkv, B, H, S, DA, temper, *banks, blk, masked)
    assert exact(of)
    for onepass in (True, False):
        dqkv, _, _, _ = tx.attn_bwd_flash(qkv, god, stats, B, H, S, DA, temper, *banks, blk, masked, o=of if onepass else None)
        assert exact(dqkv), onepass
        big = max(range(3), key=lambda i: float(dqkv[i].abs().max()))
        assert big == (0 if where == "dq" else 2), [float(dqkv[i].abs().max()) for i in range(3)]
    assert L.AMAX_FALLBACKS[0] == n0
