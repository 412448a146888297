"""The flash attention kernels (csrc/attention_flash.hip: lvt_attn_fwd_flash, lvt_attn_bwd_flash = kernels A and B + the bank
reduce) off the one launch shape of test_gpu_flash_attention.py: a (batch, heads) grid against fp64, a temper other than
sqrt(128), a row stride wider than H * 128 through the C entry points inside guard buffers, the host-side refusals, and
run-to-run bit equality of the fixed-order reductions.

The acceptance rule is util_attention.judge: err < max(2e-5 * scale, 4 * err32), err32 = the error of the same formula in fp32
torch against fp64; bank gradients are judged against the largest bank's scale.  Inputs are the draw of the flash tests:
rand(seed = 1..4), q * 3, banks * 0.5."""
import ctypes as C
import math

import pytest
import torch

from util_attention import DA, S, judge, rand, reference
from util_guard import Buf, dense, fbuf, float_bits, obuf, rows_idx, PAYLOAD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOMS = [(1, 16, 16), (4, 8, 8)]
NAMES = ["o", "m", "linv", "dq", "dk", "dv", "ddt", "ddh", "ddw"]
FORMS = [("onepass", True), ("twopass", False)]      # backward A: `o` handed over (delta = dO . O), or o == NULL
TEMPER = math.sqrt(DA)


def _ids(p):
    return "B%dH%d" % p


def _inputs(B, H, blk):
    hd = H * DA
    q, k, v, go = (rand(B * S, hd, seed=s) for s in (1, 2, 3, 4))
    banks = [rand(H, 2 * n - 1, seed=5 + i) * 0.5 for i, n in enumerate(blk)]
    return q * 3.0, k, v, go, banks                                 # scores of a few units: a peaked softmax


_KEPT = {}


def _case(B, H, blk, masked, temper=None):
    """-> (q, k, v, go, banks), fp64 reference, fp32 reference (NAMES order).  The (1, 8) cases are computed once and kept:
    the grid, the temper and the row-stride tests share them.  Nobody writes to what this returns."""
    key = (B, H, blk, masked, temper)
    if key in _KEPT:
        return _KEPT[key]
    ins = _inputs(B, H, blk)
    q, k, v, go, banks = ins
    ref = reference(q, k, v, go, banks, blk, masked, temper=temper)[:9]
    ref32 = reference(q, k, v, go, banks, blk, masked, dtype=torch.float32, temper=temper)[:9]
    if (B, H) == (1, 8):
        _KEPT[key] = (ins, ref, ref32)
    return ins, ref, ref32


def _judge(tag, names, got, ref, ref32):
    """judge() every output of `names` (got: the same order) and print the figures; the outputs that miss the rule are reported
    together (name, err, err32, scale each)."""
    bank_scale = max(float(ref[i].abs().max()) for i in (6, 7, 8))
    missed = []
    for n, a in zip(names, got):
        r, r32 = ref[NAMES.index(n)], ref32[NAMES.index(n)]
        assert a.shape == r.shape, (tag, n, a.shape, r.shape)
        try:
            # (the gradient of a one-entry bank is sum_ij g_ij == 0 up to rounding: judged against the scale of the other banks)
            err, err32, scale = judge(n, a, r, r32, scale=bank_scale if n.startswith("dd") else None)
        except AssertionError as e:
            missed.append(e.args[0])
            continue
        print("flash_matrix %s %s err=%.3e err32=%.3e ratio=%.3f rel=%.3e" % (tag, n, err, err32, err / max(err32, 1e-300), err / scale))
    assert not missed, (tag, missed)


def _flash_both(ins, B, H, blk, masked, temper):
    """One forward through the wrappers, then both backward forms from it -> [o, m, linv], {form: [dq .. ddw]}."""
    from lvt_amd.hip import binding as L, tx
    assert L.get_math_mode() == "f16x2"
    q, k, v, go, banks = ins
    qkv = torch.stack([q, k, v]).to(DEV).contiguous()
    god = go.to(DEV).contiguous()
    bd = [t.to(DEV).contiguous() for t in banks]
    o, stats = tx.attn_fwd_flash(qkv, B, H, S, DA, temper, bd[0], bd[1], bd[2], blk, masked)
    back = {}
    for form, onepass in FORMS:
        dqkv, ddt, ddh, ddw = tx.attn_bwd_flash(qkv, god, stats, B, H, S, DA, temper, bd[0], bd[1], bd[2], blk, masked,
                                                o=o if onepass else None)
        back[form] = [dqkv[0], dqkv[1], dqkv[2], ddt, ddh, ddw]
    torch.cuda.synchronize()
    return [o, stats[0], stats[1]], back


def _check_both(tag, ins, ref, ref32, B, H, blk, masked, temper):
    fwd, back = _flash_both(ins, B, H, blk, masked, temper)
    _judge(tag, NAMES[:3], fwd, ref, ref32)
    for form, _ in FORMS:
        _judge(tag + " " + form, NAMES[3:], back[form], ref, ref32)
        for t in back[form]:
            assert torch.isfinite(t).all(), (tag, form)


@pytest.mark.parametrize("BH", [(1, 8), (2, 4), (3, 8), (8, 1), (1, 24), (40, 1)], ids=_ids)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("blk", GEOMS)
def test_flash_grid_vs_fp64(blk, masked, BH):
    """All nine outputs against fp64, one forward and both backward forms from it.  (1, 8) is the smallest legal launch (8
    pairs); (2, 4) reaches the second sample's heads with H < 8; (3, 8) = 24 pairs wraps the pairing of block ids 8 apart;
    (8, 1) has one row per bank; (1, 24) is a head count that is no power of two (pair / H and pair % H do real work);
    (40, 1) has 2 B = 80 > 64 partials per bank entry: the second trip of the bank reduce's loop.

    Worst err / err32 over the 24 cases and both backward forms on an MI355X (the test prints every figure): o 0.93, m 0.87,
    linv 1.00, dq 1.15, dk 1.19, dv 1.21, ddt 2.20, ddh 0.86, ddw 0.50; the worst err / scale was 2.1e-6 (ddt, (40, 1)), so
    every case is also inside the 2e-5 * scale arm."""
    B, H = BH
    ins, ref, ref32 = _case(B, H, blk, masked)
    _check_both("%s masked=%d B=%d H=%d" % (blk, masked, B, H), ins, ref, ref32, B, H, blk, masked, TEMPER)


@pytest.mark.parametrize("blk", GEOMS)
def test_flash_temper(blk):
    """temper = 7.0, neither sqrt(128) nor a power of two: c1 = log2(e) / temper of the scores and inv_temper of dq / dk must be
    the same temper, and the one the caller passed."""
    B, H, masked, temper = 1, 8, True, 7.0
    ins, ref, ref32 = _case(B, H, blk, masked, temper)
    _check_both("%s temper=7 B=%d H=%d" % (blk, B, H), ins, ref, ref32, B, H, blk, masked, temper)


# ---- straight through the C entry points -----------------------------------------------------------------------------------
def _p(t, off=0):
    """Pointer `off` floats into tensor t (None: NULL)."""
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + 4 * off)


def _fwd(lib, q, k, v, ld, B, H, temper, banks, blk, masked, o, stats, amax, S_=S, da=DA):
    from lvt_amd.hip import binding as L
    return lib.lvt_attn_fwd_flash(q, k, v, ld, B, H, S_, da, temper, banks[0], banks[1], banks[2], blk[0], blk[1], blk[2],
                                  int(masked), -1e4, o, stats, amax, L.stream_ptr())


def _bwd(lib, q, k, v, go, ld, stats, o, B, H, temper, banks, blk, masked, dq, dk, dv, dd, amax, ws, nws, S_=S, da=DA):
    from lvt_amd.hip import binding as L
    return lib.lvt_attn_bwd_flash(q, k, v, go, ld, stats, o, B, H, S_, da, temper, banks[0], banks[1], banks[2], blk[0], blk[1],
                                  blk[2], int(masked), -1e4, dq, dk, dv, dd[0], dd[1], dd[2], amax, ws, nws, L.stream_ptr())


@pytest.mark.parametrize("gaps", ["nan", "3e38"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("blk", GEOMS)
def test_flash_row_stride_in_guard_buffers(blk, masked, gaps):
    """ld = 3 * H * 128 + 4: q, k and v are column blocks of ONE (M, ld) matrix (the packed projection output with a gap), dO,
    o, dq, dk and dv sit in buffers of the same pitch; stats, the bank gradients, the workspace and both max-|.| slots in dense
    guard buffers.  Nothing outside a logical output changes, every logical element is written, the results meet the fp64
    rule, the max-|.| records are exact, the inputs are unchanged.  The gap columns and the padding of q / k / v / dO hold the
    NaN payload in one run and 3.0e38 in the other: a row maximum built with fmaxf drops a NaN, but a row scale that swallowed
    3.0e38 wrecks the row."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    B, H = 1, 8
    M, hd = B * S, H * DA
    ld = 3 * hd + 4
    (q, k, v, go, banks), ref, ref32 = _case(B, H, blk, masked)
    pay = PAYLOAD if gaps == "nan" else float_bits(3.0e38)
    qkv = Buf(rows_idx(M, 3 * hd, ld), torch.cat([q, k, v], 1), payload=pay)
    god = Buf(rows_idx(M, hd, ld), go, payload=pay)
    bd = [fbuf(t) for t in banks]
    in_bits = [b.bits() for b in (qkv, god, *bd)]
    qp, kp, vp = _p(qkv.view), _p(qkv.view, hd), _p(qkv.view, 2 * hd)
    bp = [_p(b.view) for b in bd]
    o, stats, o_amax = Buf(rows_idx(M, hd, ld)), obuf(2, B * H * S), fbuf(torch.zeros(1))
    L.check(_fwd(lib, qp, kp, vp, ld, B, H, TEMPER, bp, blk, masked, _p(o.view), _p(stats.view), _p(o_amax.view)), "lvt_attn_fwd_flash")
    torch.cuda.synchronize()
    fwd_bits = [o.bits(), stats.bits()]
    nws = lib.lvt_attn_bwd_flash_workspace_bytes(B, H, S, blk[0], blk[1], blk[2])
    assert nws % 4 == 0
    outs = dict(o=o, stats=stats, o_amax=o_amax)
    got = {"": [o.logical(), stats.logical()[0], stats.logical()[1]]}
    spaces = []
    for form, onepass in FORMS:
        ws = obuf(nws // 4)
        dq, dk, dv = (Buf(rows_idx(M, hd, ld)) for _ in range(3))
        dd = [obuf(H, 2 * n - 1) for n in blk]
        d_amax = fbuf(torch.zeros(1))
        L.check(_bwd(lib, qp, kp, vp, _p(god.view), ld, _p(stats.view), _p(o.view) if onepass else None, B, H, TEMPER, bp, blk,
                     masked, _p(dq.view), _p(dk.view), _p(dv.view), [_p(b.view) for b in dd], _p(d_amax.view), _p(ws.view), nws),
                "lvt_attn_bwd_flash")
        torch.cuda.synchronize()
        spaces.append(ws)
        outs.update({form + " dq": dq, form + " dk": dk, form + " dv": dv, form + " ddt": dd[0], form + " ddh": dd[1],
                     form + " ddw": dd[2], form + " d_amax": d_amax})
        got[form] = [b.logical() for b in (dq, dk, dv, *dd)]
        assert float(d_amax.logical()) == max(float(t.abs().max()) for t in got[form][:3]), form
    assert float(o_amax.logical()) == float(got[""][0].abs().max())
    for n, b in outs.items():
        assert b.outside_untouched(), n
        assert not torch.isnan(b.logical()).any(), n     # a payload NaN: an element nobody wrote; any other NaN: a gap was read
    for ws in spaces:
        assert ws.outside_untouched()
    for b, before in zip((qkv, god, *bd), in_bits):      # (inputs are inputs: logical elements, gaps and padding alike)
        assert torch.equal(b.bits(), before)
    assert torch.equal(o.bits(), fwd_bits[0]) and torch.equal(stats.bits(), fwd_bits[1])      # (and so are o and stats, to the backward)
    tag = "%s masked=%d ld=%d gaps=%s" % (blk, masked, ld, gaps)
    _judge(tag, NAMES[:3], got[""], ref, ref32)
    for form, _ in FORMS:
        _judge(tag + " " + form, NAMES[3:], got[form], ref, ref32)


def test_flash_refusals():
    """Argument checks the two entry points make on the host before any launch: an error code and a message, and not one float
    of any output, the workspace or the max-|.| slot changes.  Then the same buffers with legal arguments are accepted."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    B, H, blk = 1, 8, (1, 16, 16)
    M, hd = B * S, H * DA
    # big enough for every (refused) shape and offset below; nothing is ever read
    qkv = torch.zeros(3, M + 1, hd, device=DEV)
    go = torch.zeros(M + 1, hd, device=DEV)
    banks = torch.zeros(H, 31, device=DEV)
    FILL = 7.0
    o = torch.full((M + 1, hd), FILL, device=DEV)
    stats = torch.full((2 * B * H * S + 4,), FILL, device=DEV)
    dqkv = torch.full((3, M + 1, hd), FILL, device=DEV)
    dd = torch.full((3, H, 31), FILL, device=DEV)
    amax = torch.full((1,), FILL, device=DEV)
    nws = lib.lvt_attn_bwd_flash_workspace_bytes(B, H, S, *blk)
    ws = torch.full((nws // 4 + 4,), FILL, device=DEV)
    bp = [_p(banks)] * 3

    def fwd(B=B, H=H, S_=S, da=DA, blk=blk, ld=hd, q_off=0, o_off=0, stats_off=0):
        return _fwd(lib, _p(qkv[0], q_off), _p(qkv[1]), _p(qkv[2]), ld, B, H, TEMPER, bp, blk, 0, _p(o, o_off), _p(stats, stats_off),
                    _p(amax), S_=S_, da=da)

    def bwd(B=B, H=H, S_=S, da=DA, blk=blk, ld=hd, q_off=0, stats_off=0, dq_off=0, o_in=True, o_off=0, ws_off=0, nws=nws, ws_null=False):
        return _bwd(lib, _p(qkv[0], q_off), _p(qkv[1]), _p(qkv[2]), _p(go), ld, _p(stats, stats_off), _p(o, o_off) if o_in else None,
                    B, H, TEMPER, bp, blk, 0, _p(dqkv[0], dq_off), _p(dqkv[1]), _p(dqkv[2]), [_p(dd[0]), _p(dd[1]), _p(dd[2])],
                    _p(amax), None if ws_null else _p(ws, ws_off), nws, S_=S_, da=da)

    def refused(fn, kw, code, word=None):
        rc = fn(**kw)
        msg = lib.lvt_last_error().decode()
        assert rc == code, (fn.__name__, kw, rc, msg)
        assert len(msg) > 0, (fn.__name__, kw)
        assert word is None or word in msg, (fn.__name__, kw, msg)

    both = [(dict(H=4), "multiple of 8"),                                    # B * H = 4: no pairing per XCD
            (dict(S_=512), "no instantiation"), (dict(da=64), "no instantiation"), (dict(blk=(2, 8, 16)), "no instantiation"),
            (dict(ld=hd + 2), None),                                         # rows off a 16-byte boundary
            (dict(ld=hd - 4), None),                                         # rows that overlap
            (dict(q_off=1), None), (dict(stats_off=1), None)]                # 4 bytes off a 16-byte boundary
    for kw, word in both:
        for fn in (fwd, bwd):
            refused(fn, kw, -1, word)                                        # LVT_EINVAL
    refused(fwd, dict(o_off=1), -1)
    refused(bwd, dict(dq_off=1), -1)
    refused(bwd, dict(o_off=1), -1)                                          # the optional o of the one-pass form
    for kw in (dict(nws=nws - 1), dict(ws_off=1), dict(ws_null=True)):
        for o_in in (True, False):
            refused(bwd, dict(kw, o_in=o_in), -2, "workspace")               # LVT_EWORKSPACE
    torch.cuda.synchronize()
    for t in (o, stats, dqkv, dd, amax, ws):
        assert bool((t == FILL).all())
    # the same buffers, legal arguments: accepted (the refusals above were about the arguments, not the buffers) and written
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool((o[:M] != FILL).all()) and bool((stats[:2 * B * H * S] != FILL).all()) and bool((dqkv[:, :M] != FILL).all())
    ddt = dd[0].view(-1)                                                     # (H, 1) dense at the head of its (H, 31) buffer
    assert bool((ddt[:H] != FILL).all()) and bool((dd[1:] != FILL).all())
    assert bool((ws[:B * H * S] != FILL).all())                              # delta, the head of the workspace
    assert bool((o[M:] == FILL).all()) and bool((stats[2 * B * H * S:] == FILL).all()) and bool((dqkv[:, M:] == FILL).all())
    assert bool((ddt[H:] == FILL).all()) and bool((ws[nws // 4:] == FILL).all())
    dqkv.fill_(FILL)
    assert bwd(o_in=False) == 0
    torch.cuda.synchronize()
    assert bool((dqkv[:, :M] != FILL).all()) and bool((dqkv[:, M:] == FILL).all())


@pytest.mark.parametrize("form,onepass", FORMS, ids=[f for f, _ in FORMS])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("blk", GEOMS)
def test_flash_runs_are_bit_equal(blk, masked, form, onepass):
    """The bank partials and the reduce kernel add in a fixed order, and nothing else in the three kernels depends on which
    workgroup ran first: two full forward + backward runs on the same inputs give all nine outputs bit for bit, with every
    output and the workspace re-filled with NaN in between.  24 pairs."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    B, H = 3, 8
    M, hd = B * S, H * DA
    q, k, v, go, banks = _inputs(B, H, blk)
    qkv = torch.stack([q, k, v]).to(DEV).contiguous()
    god = go.to(DEV).contiguous()
    bd = [t.to(DEV).contiguous() for t in banks]
    bp = [_p(t) for t in bd]
    nws = lib.lvt_attn_bwd_flash_workspace_bytes(B, H, S, blk[0], blk[1], blk[2])
    o, dq, dk, dv = (torch.empty(M, hd, device=DEV) for _ in range(4))
    stats = torch.empty(2, B * H * S, device=DEV)
    dd = [torch.empty(H, 2 * n - 1, device=DEV) for n in blk]
    ws = torch.empty(nws // 4, device=DEV)
    runs = []
    for _ in range(2):
        for t in (o, dq, dk, dv, stats, *dd, ws):
            t.fill_(float("nan"))
        L.check(_fwd(lib, _p(qkv[0]), _p(qkv[1]), _p(qkv[2]), hd, B, H, TEMPER, bp, blk, masked, _p(o), _p(stats), None),
                "lvt_attn_fwd_flash")
        L.check(_bwd(lib, _p(qkv[0]), _p(qkv[1]), _p(qkv[2]), _p(god), hd, _p(stats), _p(o) if onepass else None, B, H, TEMPER, bp,
                     blk, masked, _p(dq), _p(dk), _p(dv), [_p(t) for t in dd], None, _p(ws), nws), "lvt_attn_bwd_flash")
        torch.cuda.synchronize()
        runs.append([t.cpu().clone() for t in (o, stats[0], stats[1], dq, dk, dv, *dd)])
    for n, a, b in zip(NAMES, *runs):
        assert not torch.isnan(a).any(), n
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n
