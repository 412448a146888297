"""The attention code that runs when neither the flash nor the plane kernels apply, against fp64, in NaN-payload guard buffers
(tests/util_guard.py):

  * lvt_attn_fwd_kernel<0,0,0> (csrc/attention.hip): the any-geometry instantiation of the fused forward -- every block other
    than (1,16,16) and (4,8,8); bank and coordinate look-ups per element, bw = 4 breaks the BW % 8 folding of the specialised ones;
  * lvt_attn_softmax_fwd / lvt_attn_softmax_bwd / lvt_attn_bank_grad_kernel (csrc/transformer.hip) at every S in {256, 512, 768,
    1024} (the `c < nc` chunk logic with nc > 1), every bank (the dt entries included), and their refusals;
  * the layer path of _BlockLocalAttentionFn off the flash / plane kernels: QK^T GEMM, softmax kernel, PV GEMM, and the backward
    through the CAUSAL_KMIN / CAUSAL_KMAX / CAUSAL_TILE products -- S != 256, da != 128, b * n_head % 8 != 0, a block-split volume.

Bounds.  The reference is the same formula in fp64 on the CPU; err32 is the distance of torch's fp32 CPU evaluation of that
formula from it (a property of the reference, never of the kernel).
  pointwise (P, dS), per row:          |got - ref64| <= max(4 err32_row, 2^-21 max |ref64_row|)
  reductions (bank gradients):         |got - ref64| <= max(4 err32, 2^-21 sum |terms|), the terms summed in fp64
  lvt_attn_fwd and the layer:          max |got - ref64| <= max(2e-5 scale, 4 err32), scale = max |ref64| -- for a bank gradient the
                                       largest bank gradient of the case (a one-entry bank has true value 0), as
                                       test_gpu_flash_attention.py::test_flash_attention_vs_fp64 judges them
[guard]: every float outside the logical output still holds the payload; [repeat]: a second launch gives the same bits."""
import math

import pytest
import torch

from lvt_amd.hip import binding as L, gemm as G, tx
from oracle import lvt_oracle as O
from util_guard import DEV, fbuf, obuf

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -21


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def _row_bound(got, ref64, ref32):
    """Pointwise bound per row (last dim): -> number of elements out of bound, worst ratio."""
    err = (got.double() - ref64).abs()
    err32 = (ref32.double() - ref64).abs().amax(-1, keepdim=True)
    tol = torch.maximum(4 * err32, EPS * ref64.abs().amax(-1, keepdim=True))
    bad = ~(err <= tol)
    return int(bad.sum()), float((err / tol.clamp_min(1e-300)).max())


def _bank_index(blk):
    """Flat (S*S) bank entry of (i, j) for each of the three banks."""
    t, h, w = blk
    it = torch.arange(t).view(t, 1, 1).expand(t, h, w).reshape(-1)
    ih = torch.arange(h).view(1, h, 1).expand(t, h, w).reshape(-1)
    iw = torch.arange(w).view(1, 1, w).expand(t, h, w).reshape(-1)
    return [(ix[:, None] - ix[None, :] + (n - 1)).reshape(-1) for ix, n in ((it, t), (ih, h), (iw, w))]


# ---- 1.1 lvt_attn_fwd, generic instantiation ------------------------------------------------------------------------
def _attn_ref(q, k, v, banks, blk, masked, B, H, dtype, fill=-1e4):
    S, da = 256, 128
    qh, kh, vh = (t.to(dtype).view(B, S, H, da).permute(0, 2, 1, 3) for t in (q, k, v))
    bias = O.rel_position_bias(*[x.to(dtype) for x in banks], blk).transpose(0, 1)
    sc = qh @ kh.transpose(2, 3) / math.sqrt(da) + bias
    if masked:
        sc = sc.masked_fill(torch.triu(torch.ones(S, S), 1).bool(), fill)
    P = torch.softmax(sc, -1)
    return P, (P @ vh).permute(0, 2, 1, 3).reshape(B * S, H * da)


def _attn_fwd_c(qkv, banks, blk, masked, B, H, S=256, da=128):
    """lvt_attn_fwd through the C entry point: inputs and outputs in guard buffers -> (rc, message, P buffer, o buffer)."""
    ib = [fbuf(t) for t in qkv]
    bb = [fbuf(t) for t in banks]
    P, o = obuf(B, H, S, S), obuf(B * S, H * da)
    rc = L.lib().lvt_attn_fwd(L.ptr(ib[0].view), L.ptr(ib[1].view), L.ptr(ib[2].view), B, H, S, da, math.sqrt(da),
                              L.ptr(bb[0].view), L.ptr(bb[1].view), L.ptr(bb[2].view), blk[0], blk[1], blk[2],
                              1 if masked else 0, -1e4, L.ptr(P.view), L.ptr(o.view), L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, P, o


@pytest.mark.parametrize("masked", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("BH", [(1, 3), (2, 1)], ids=lambda p: "B%dH%d" % p)
@pytest.mark.parametrize("blk", [(2, 8, 16), (16, 4, 4), (1, 8, 32), (8, 8, 4)], ids=lambda b: "%dx%dx%d" % b)
def test_attn_fwd_any_geometry(blk, BH, masked):
    B, H = BH
    S, da = 256, 128
    hd = H * da
    q, k, v = _rand(B * S, hd, seed=1) * 3.0, _rand(B * S, hd, seed=2), _rand(B * S, hd, seed=3)
    banks = [_rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    P64, o64 = _attn_ref(q, k, v, banks, blk, masked, B, H, torch.float64)
    P32, o32 = _attn_ref(q, k, v, banks, blk, masked, B, H, torch.float32)
    rc, msg, Pb, ob = _attn_fwd_c((q, k, v), banks, blk, masked, B, H)
    assert rc == 0, msg
    P, o = Pb.logical(), ob.logical()
    for name, got, r64, r32 in (("P", P, P64, P32), ("o", o, o64, o32)):
        err, err32 = float((got.double() - r64).abs().max()), float((r32.double() - r64).abs().max())
        print("%s: err %.3g err32 %.3g scale %.3g" % (name, err, err32, float(r64.abs().max())))
        assert err <= max(2e-5 * float(r64.abs().max()), 4 * err32), (name, err, err32)
    if masked:
        assert bool((P[:, :, torch.triu(torch.ones(S, S), 1).bool()] == 0).all()), "a masked probability is not exactly 0"
    assert Pb.outside_untouched() and ob.outside_untouched(), "a float outside P / o was written"
    # the three-launch path: QK^T GEMM, softmax kernel, PV GEMM
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    bd = [x.to(DEV).contiguous() for x in banks]
    P3 = torch.empty(B, H, S, S, device=DEV)
    G.gemm(qd, kd, P3, S, S, da, ta=0, tb=0, lda=hd, ldb=hd, ldc=S, batch_outer=B, batch_inner=H,
           sA=(S * hd, da), sB=(S * hd, da), sC=(H * S * S, S * S))
    tx.attn_softmax_fwd_(P3, math.sqrt(da), bd[0], bd[1], bd[2], blk, masked)
    o3 = torch.empty(B * S, hd, device=DEV)
    G.gemm(P3, vd, o3, S, da, S, ta=0, tb=1, lda=S, ldb=hd, ldc=hd, batch_outer=B, batch_inner=H,
           sA=(H * S * S, S * S), sB=(S * hd, da), sC=(S * hd, da))
    for name, got, other, r64, r32 in (("P", P, P3, P64, P32), ("o", o, o3, o64, o32)):
        d, err32 = float((got.double() - other.cpu().double()).abs().max()), float((r32.double() - r64).abs().max())
        assert d <= max(2e-5 * float(r64.abs().max()), 4 * err32), ("three-launch " + name, d, err32)
    # [repeat]
    rc, msg, Pb2, ob2 = _attn_fwd_c((q, k, v), banks, blk, masked, B, H)
    assert rc == 0 and torch.equal(Pb.bits(), Pb2.bits()) and torch.equal(ob.bits(), ob2.bits()), "a second launch gave other bits"


@pytest.mark.parametrize("blk,S,da,what", [((1, 4, 64), 256, 128, "block geometry"), ((2, 16, 16), 512, 128, "unsupported"),
                                           ((4, 8, 8), 256, 64, "unsupported")], ids=["bw64", "S512", "da64"])
def test_attn_fwd_refusals(blk, S, da, what):
    """2 bw - 1 > 64 bank entries, S != 256 and da != 128: an error code, a message, and not one float written."""
    B, H = 1, 1
    qkv = [_rand(B * S, H * da, seed=s) for s in (1, 2, 3)]
    banks = [_rand(H, 2 * n - 1, seed=5 + i) for i, n in enumerate(blk)]
    rc, msg, Pb, ob = _attn_fwd_c(qkv, banks, blk, True, B, H, S=S, da=da)
    assert rc == -1 and what in msg, (rc, msg)
    assert Pb.outside_untouched() and ob.outside_untouched()
    assert bool(torch.isnan(Pb.logical()).all()) and bool(torch.isnan(ob.logical()).all()), "a refused call wrote its output"


# ---- 1.2 lvt_attn_softmax_fwd / lvt_attn_softmax_bwd ------------------------------------------------------------------
GEOMS = [(256, (4, 8, 8)), (256, (2, 8, 16)), (256, (16, 4, 4)), (512, (8, 8, 8)), (512, (4, 8, 16)), (768, (12, 8, 8)),
         (1024, (16, 8, 8))]


def _softmax_ref(s, banks, blk, masked, fill, dP, dtype):
    """-> P, dS, [ddt, ddh, ddw], G = P (dP - sum_j P dP) summed over nothing (B, H, S, S), all in `dtype`."""
    S, da = s.shape[-1], 128
    sr = s.to(dtype).clone().requires_grad_(True)
    bl = [b.to(dtype).clone().requires_grad_(True) for b in banks]
    a = sr / math.sqrt(da) + O.rel_position_bias(*bl, blk).transpose(0, 1)
    if masked:
        a = a.masked_fill(torch.triu(torch.ones(S, S), 1).bool(), fill)
    P = torch.softmax(a, -1)
    if dP is None:
        return P.detach(), None, None, None
    P.backward(dP.to(dtype))
    Pd = P.detach()
    g = Pd * (dP.to(dtype) - (Pd * dP.to(dtype)).sum(-1, keepdim=True))
    return Pd, sr.grad, [b.grad for b in bl], g


def _softmax_fwd_c(s, banks, blk, masked, fill, B, H):
    S = s.shape[-1]
    sb = fbuf(s)
    bb = [fbuf(t) for t in banks]
    rc = L.lib().lvt_attn_softmax_fwd(L.ptr(sb.view), B, H, S, math.sqrt(128), L.ptr(bb[0].view), L.ptr(bb[1].view),
                                      L.ptr(bb[2].view), blk[0], blk[1], blk[2], 1 if masked else 0, fill, L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, sb


def _softmax_bwd_c(P, dP, blk, B, H):
    """-> rc, message, dP buffer (dS afterwards), [ddt, ddh, ddw] buffers, G buffer."""
    S = P.shape[-1]
    pb, db, gb = fbuf(P), fbuf(dP), obuf(H, S, S)
    dd = [obuf(H, 2 * n - 1) for n in blk]
    rc = L.lib().lvt_attn_softmax_bwd(L.ptr(pb.view), L.ptr(db.view), B, H, S, math.sqrt(128), blk[0], blk[1], blk[2],
                                      L.ptr(gb.view), L.ptr(dd[0].view), L.ptr(dd[1].view), L.ptr(dd[2].view), L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, db, dd, gb


def _check_softmax(S, blk, B, H, masked, fill, backward=True):
    s, dP = _rand(B, H, S, S, seed=1) * 4, _rand(B, H, S, S, seed=2)
    banks = [_rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    P64, dS64, dd64, g64 = _softmax_ref(s, banks, blk, masked, fill, dP, torch.float64)
    P32, dS32, dd32, _ = _softmax_ref(s, banks, blk, masked, fill, dP, torch.float32)
    # forward
    rc, msg, sb = _softmax_fwd_c(s, banks, blk, masked, fill, B, H)
    assert rc == 0, msg
    P = sb.logical()
    nbad, worst = _row_bound(P, P64, P32)
    print("P: worst err / bound %.3g" % worst)
    assert nbad == 0, ("P", nbad, worst)
    assert float((P.double().sum(-1) - 1).abs().max()) <= EPS, "a row of P does not sum to 1"
    if masked and fill == -1e4:
        assert bool((P[:, :, torch.triu(torch.ones(S, S), 1).bool()] == 0).all()), "a masked probability is not exactly 0"
    assert sb.outside_untouched(), "a float outside the scores was written"
    rc, msg, sb2 = _softmax_fwd_c(s, banks, blk, masked, fill, B, H)
    assert rc == 0 and torch.equal(sb.bits(), sb2.bits()), "a second forward gave other bits"
    if not backward:
        return
    # backward, from the kernel's own P (what the layer saves)
    rc, msg, db, dd, gb = _softmax_bwd_c(P, dP, blk, B, H)
    assert rc == 0, msg
    nbad, worst = _row_bound(db.logical(), dS64, dS32)
    print("dS: worst err / bound %.3g" % worst)
    assert nbad == 0, ("dS", nbad, worst)
    absg = g64.abs().sum(0).view(H, S * S)                                 # sum |terms| of a bank entry: the |g| that select it
    for name, buf, r64, r32, ix, n in zip(("ddt", "ddh", "ddw"), dd, dd64, dd32, _bank_index(blk), blk):
        terms = torch.zeros(H, 2 * n - 1, dtype=torch.float64).index_add_(1, ix, absg)
        err, err32 = (buf.logical().double() - r64).abs(), (r32.double() - r64).abs()
        tol = torch.maximum(4 * err32, EPS * terms)
        print("%s: worst err / bound %.3g" % (name, float((err / tol.clamp_min(1e-300)).max())))
        assert bool((err <= tol).all()), (name, float(err.max()), float(tol.min()))
        assert buf.outside_untouched(), name + ": a float outside the bank gradient was written"
    assert db.outside_untouched() and gb.outside_untouched(), "a float outside dS / G was written"
    rc, msg, db2, dd2, gb2 = _softmax_bwd_c(P, dP, blk, B, H)
    assert rc == 0 and torch.equal(db.bits(), db2.bits()) and torch.equal(gb.bits(), gb2.bits())
    assert all(torch.equal(a.bits(), b.bits()) for a, b in zip(dd, dd2)), "a second backward gave other bank gradients"


@pytest.mark.parametrize("masked", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("BH", [(1, 2), (3, 1)], ids=lambda p: "B%dH%d" % p)
@pytest.mark.parametrize("S,blk", GEOMS, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else "S%d" % x)
def test_attn_softmax_fwd_bwd(S, blk, BH, masked):
    _check_softmax(S, blk, BH[0], BH[1], masked, -1e4)


def test_attn_softmax_fill_that_does_not_underflow():
    """fill = -30: exp(fill - max) is an ordinary number, so the masked probabilities are the formula's value, not 0.  (Forward
    only: the backward kernel's dS = P (dP - sum P dP) / temper is the score gradient of a causal layer because P is exactly 0
    above the diagonal, which holds for the reference's fill of -1e4 and not for this one.)"""
    _check_softmax(256, (2, 8, 16), 1, 2, True, -30.0, backward=False)
    s = _rand(1, 2, 256, 256, seed=1) * 4
    banks = [_rand(2, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate((2, 8, 16))]
    rc, _, sb = _softmax_fwd_c(s, banks, (2, 8, 16), True, -30.0, 1, 2)
    assert rc == 0 and float(sb.logical()[:, :, 0, 1:].min()) > 0.0


OVER = [((2, 16, 16), 65), ((3, 16, 16), 67), ((4, 16, 16), 69)]


def test_attn_softmax_fwd_accepts_65_bank_entries():
    """The forward has no bank-entry limit: (2,16,16) at S = 512 is accepted and correct."""
    blk, B, H, S = (2, 16, 16), 1, 2, 512
    s = _rand(B, H, S, S, seed=1) * 4
    banks = [_rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    for masked in (False, True):
        P64 = _softmax_ref(s, banks, blk, masked, -1e4, None, torch.float64)[0]
        P32 = _softmax_ref(s, banks, blk, masked, -1e4, None, torch.float32)[0]
        rc, msg, sb = _softmax_fwd_c(s, banks, blk, masked, -1e4, B, H)
        assert rc == 0, msg
        nbad, worst = _row_bound(sb.logical(), P64, P32)
        assert nbad == 0 and sb.outside_untouched(), (masked, nbad, worst)


@pytest.mark.parametrize("blk,entries", OVER, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else "n%d" % x)
def test_attn_softmax_bwd_refuses_more_than_64_bank_entries(blk, entries):
    """lvt_attn_bank_grad_kernel gives one lane to each bank entry of a head: more than 64 are refused BEFORE the first launch
    (which overwrites dP), with an error that names the limit; dP keeps its bits."""
    B, H, S = 1, 1, blk[0] * 256
    P = torch.softmax(_rand(B, H, S, S, seed=1), -1)
    dP = _rand(B, H, S, S, seed=2)
    db = fbuf(dP)
    before = db.bits().clone()
    with pytest.raises(L.LvtError, match="%d bank entries per head" % entries):
        tx.attn_softmax_bwd_(P.to(DEV), db.view[:dP.numel()].view(B, H, S, S), math.sqrt(128), blk)
    torch.cuda.synchronize()
    assert torch.equal(db.bits(), before), "a refused backward changed dP"
    rc, msg, db2, dd, gb = _softmax_bwd_c(P, dP, blk, B, H)
    assert rc == -1 and "bank entries" in msg
    assert torch.equal(db2.bits(), before) and all(bool(torch.isnan(x.logical()).all()) for x in dd + [gb])


@pytest.mark.parametrize("S,blk", [(384, (6, 8, 8)), (1280, (20, 8, 8))], ids=["S384", "S1280"])
def test_attn_softmax_refuses_other_row_lengths(S, blk):
    B, H = 1, 1
    s = _rand(B, H, S, S, seed=1)
    banks = [_rand(H, 2 * n - 1, seed=5 + i) for i, n in enumerate(blk)]
    rc, msg, sb = _softmax_fwd_c(s, banks, blk, False, -1e4, B, H)
    assert rc == -1 and "unsupported" in msg and torch.equal(sb.logical(), s) and sb.outside_untouched()
    rc, msg, db, dd, gb = _softmax_bwd_c(torch.softmax(s, -1), s, blk, B, H)
    assert rc == -1 and "unsupported" in msg and torch.equal(db.logical(), s)
    assert all(bool(torch.isnan(x.logical()).all()) for x in dd + [gb])


# ---- 1.3 the layer off the flash / plane path --------------------------------------------------------------------------
LAYER_CASES = [
    # block, volume (None: the block), da, d, n_head, b
    ((8, 8, 8), None, 64, 128, 2, 2),
    ((2, 8, 16), None, 128, 256, 3, 1),              # lvt_attn_fwd<0,0,0> forward + the generic backward
    ((16, 8, 8), None, 32, 64, 1, 1),
    ((1, 16, 16), None, 128, 128, 4, 1),             # the shipped geometry with b * n_head % 8 != 0
    ((2, 8, 16), (4, 16, 16), 128, 128, 1, 1),       # block-split: lvt_row_gather and its inverse around the layer
]


def _oracle_layer(state, x5, gy5, block, masked, dtype):
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(v.dtype.is_floating_point and k.split(".")[-1] not in ("mask",))
         for k, v in state.items() if v is not None and v.dtype.is_floating_point}
    x = x5.to(dtype).clone().requires_grad_(True)
    y = O.block_local_attention(p, "", x, block, masked)
    y.backward(gy5.to(dtype))
    return y.detach(), x.grad, {k: v.grad for k, v in p.items() if v.grad is not None}


@pytest.mark.parametrize("masked", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("block,thw,da,d,n_head,b", LAYER_CASES,
                         ids=["8x8x8_da64", "2x8x16_da128", "16x8x8_da32", "1x16x16_bh4", "2x8x16_in_4x16x16"])
def test_layer_off_the_flash_path(block, thw, da, d, n_head, b, masked):
    import lvt_amd.modeling.autoregressive.vt_attention as A
    thw = thw or block
    S = block[0] * block[1] * block[2]
    vol = thw[0] * thw[1] * thw[2]
    pairs = b * (vol // S) * n_head
    assert not tx.attn_flash_supported(S, da, block, pairs) and not tx.attn_planes_supported(S, da, block, pairs)
    torch.manual_seed(3)
    layer = A.BlockLocalAttention(block, da, d, n_head, masked=masked).to(DEV)
    with torch.no_grad():
        layer.dt_bank.normal_(0, 0.3); layer.dh_bank.normal_(0, 0.3); layer.dw_bank.normal_(0, 0.3)
    state = {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}
    g = torch.Generator().manual_seed(17)
    x5 = torch.randn(b, d, *thw, generator=g)
    gy5 = torch.randn(b, d, *thw, generator=g)
    tok = lambda t: t.reshape(b, d, vol).transpose(1, 2).reshape(b * vol, d).contiguous()
    xx = tok(x5).to(DEV).requires_grad_(True)
    y = layer.forward_tokens(xx, thw)
    y.backward(tok(gy5).to(DEV))
    torch.cuda.synchronize()
    got = {"y": y.detach(), "dx": xx.grad}
    got.update({n: p.grad for n, p in layer.named_parameters()})
    y64, dx64, g64 = _oracle_layer(state, x5, gy5, block, masked, torch.float64)
    y32, dx32, g32 = _oracle_layer(state, x5, gy5, block, masked, torch.float32)
    ref64 = dict(g64, y=tok(y64), dx=tok(dx64))
    ref32 = dict(g32, y=tok(y32), dx=tok(dx32))
    assert set(got) == set(ref64), (sorted(got), sorted(ref64))
    bank_scale = max(float(ref64[n].abs().max()) for n in ("dt_bank", "dh_bank", "dw_bank"))
    for n in sorted(got):
        r64, r32 = ref64[n], ref32[n]
        scale = bank_scale if n.endswith("_bank") else float(r64.abs().max())
        err = float((got[n].double().cpu().reshape(r64.shape) - r64).abs().max())
        err32 = float((r32.double() - r64).abs().max())
        print("%s: err %.3g err32 %.3g scale %.3g" % (n, err, err32, scale))
        assert err <= max(2e-5 * scale, 4 * err32), (n, err, err32, scale)
