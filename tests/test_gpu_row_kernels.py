"""The row kernels a transformer layer runs beside its GEMMs and attention core, each against a plain fp64 (or, for pure data
movement, a bit-exact) reference, at the sizes where their code takes another path, in NaN-payload guard buffers
(tests/util_guard.py): LayerNorm forward / P2 form / backward and lvt_splitsum_layernorm_fwd (csrc/elementwise.hip, smallm.hip),
lvt_xent_fwd / lvt_xent_bwd, lvt_embbag_fwd, lvt_permute3, the decode plumbing (csrc/transformer.hip), lvt_add_periodic, lvt_axpy,
lvt_row_gather, and the small-M GEMM paths no other test reaches (csrc/smallm.hip).

Bounds.  The reference is the same formula in fp64 on the CPU; err32 is the distance of torch's fp32 CPU evaluation of it from that
(a property of the reference, never of the kernel).
  pointwise outputs, per row:   |got - ref64| <= max(4 err32_row, 2^-21 max |ref64_row|)
  reductions over many rows:    |got - ref64| <= max(4 err32, 2^-21 sum |terms|), the terms summed in fp64
  small-M GEMM:                 1e-5 |alpha| (|A||B|)_mn + 2^-21 (|bias_n| + |res_mn| + |C64_mn|)   (test_gpu_gemm_matrix.py)
  gathers, order-defined sums:  bit-equal to numpy float32 / torch evaluated in the documented order
[guard]: every element outside the logical output still holds the payload, inputs sit in payload buffers too (index inputs sit in
ordinary tensors whose unused elements are VALID other indices: a misread index changes the result instead of the address);
[repeat]: a second launch into fresh buffers gives the same bits."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lvt_amd.hip import binding as L, ew, gemm as G
from util_f16_scale import _image_ref
from util_guard import DEV, Buf, IBuf, dense, fbuf, obuf, rows_idx

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -21


def _gen(*key):
    return torch.Generator().manual_seed(1000 + sum(int(k) * (7 + 6 * i) for i, k in enumerate(key)))


def _rand(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float() * (hi - lo) + lo


def _call(fn, *args):
    rc = fn(*args, L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg


def _p(b):
    return L.ptr(b.view) if b is not None else C.c_void_p(0)


def _rows_ok(got, ref64, ref32, what):
    """Pointwise bound per row (last dim)."""
    err = (got.double() - ref64).abs()
    err32 = (ref32.double() - ref64).abs().amax(-1, keepdim=True)
    tol = torch.maximum(4 * err32, EPS * ref64.abs().amax(-1, keepdim=True))
    bad = ~(err <= tol)
    assert not bool(bad.any()), "%s: %d elements out of bound (worst err / bound %.3g, first at %s)" % (
        what, int(bad.sum()), float((err / tol.clamp_min(1e-300))[bad].max()), tuple(bad.nonzero()[0].tolist()))


def _each_ok(got, ref64, ref32, what):
    """The pointwise bound with every element its own row (per-row scalars: mean, rstd, lse)."""
    _rows_ok(got.reshape(-1, 1), ref64.reshape(-1, 1), ref32.reshape(-1, 1), what)


def _sum_ok(got, ref64, ref32, terms, what):
    """Reduction bound: `terms` = sum |terms| in fp64, elementwise."""
    err = (got.double() - ref64).abs()
    tol = torch.maximum(4 * (ref32.double() - ref64).abs(), EPS * terms)
    assert bool((err <= tol).all()), "%s: worst err / bound %.3g" % (what, float((err / tol.clamp_min(1e-300)).max()))


def _same_bits(*pairs):
    return all(torch.equal(a.bits(), b.bits()) for a, b in pairs)


# ---- 2.1 LayerNorm --------------------------------------------------------------------------------------------------
LN_D = [4, 36, 252, 256, 260, 768, 1020, 1024]
HOT = [1e4, 1e3, 3.3e5, 7.7e6]


def _ln_input(rows, d, g):
    """Row classes, cycling: a one-hot row (1e4 first), a constant row (-1.5: d copies sum and divide exactly in fp32, so the
    variance is exactly 0 and rstd = eps^-1/2 in every summation order), a random row on a magnitude ladder 2^0 .. 2^-20 over the
    rows, a random row."""
    x = _rand((rows, d), g)
    for r in range(rows):
        c = r % 4
        if c == 0:
            x[r] = 0
            x[r, (5 * r) % d] = HOT[(r // 4) % 4]
        elif c == 1:
            x[r] = -1.5
        elif c == 2:
            x[r] *= 2.0 ** (-20.0 * r / max(rows - 1, 1))
    return x


def _ln_ref(x, w, b, dy, add, dtype):
    xr, wr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    y, mean, rstd = torch.native_layer_norm(xr, (x.shape[1],), wr, br, 1e-5)
    y.backward(dy.to(dtype))
    dx = xr.grad + (add.to(dtype) if add is not None else 0)
    return [t.detach() for t in (y, mean.reshape(-1), rstd.reshape(-1), dx, wr.grad, br.grad)]


def _ln_fwd_c(x, w, b, p2=False, amax=True):
    rows, d = x.shape
    xb, wb, bb = fbuf(x), fbuf(w), fbuf(b)
    y, mean, rstd, rec = obuf(rows, d), obuf(rows), obuf(rows), obuf(1)
    wa, ba = fbuf(w.abs().max().reshape(1)), fbuf(b.abs().max().reshape(1))
    img = obuf(rows, d) if p2 else None
    lib = L.lib()
    if p2:
        rc, msg = _call(lib.lvt_layernorm_fwd_p2, _p(xb), rows, d, 1e-5, _p(wb), _p(bb), _p(y), _p(img), _p(mean), _p(rstd), _p(rec),
                        _p(wa), _p(ba))
    else:
        rc, msg = _call(lib.lvt_layernorm_fwd, _p(xb), rows, d, 1e-5, _p(wb), _p(bb), _p(y), _p(mean), _p(rstd),
                        _p(rec) if amax else None, _p(wa) if amax else None, _p(ba) if amax else None)
    return rc, msg, y, mean, rstd, rec, img


def _ln_bwd_c(dy, x, mean, rstd, w, add):
    rows, d = x.shape
    ins = [fbuf(t) for t in (dy, x, mean, rstd, w)]
    ab = fbuf(add) if add is not None else None
    dx, dw, db, rec = obuf(rows, d), obuf(d), obuf(d), Buf(dense(1), torch.zeros(1))
    lib = L.lib()
    nws = max(lib.lvt_layernorm_bwd_workspace_bytes(d), 1)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc, msg = _call(lib.lvt_layernorm_bwd, *[_p(t) for t in ins], rows, d, _p(ab), _p(dx), _p(dw), _p(db), _p(rec), L.ptr(ws), nws)
    return rc, msg, dx, dw, db, rec


def _check_ln(rows, d, with_add):
    g = _gen(rows, d, with_add)
    x, w, b, dy = _ln_input(rows, d, g), _rand((d,), g), _rand((d,), g), _rand((rows, d), g)
    add = _rand((rows, d), g) if with_add else None
    r64, r32 = _ln_ref(x, w, b, dy, add, torch.float64), _ln_ref(x, w, b, dy, add, torch.float32)
    rc, msg, y, mean, rstd, rec, _ = _ln_fwd_c(x, w, b)
    assert rc == 0, msg
    _rows_ok(y.logical(), r64[0], r32[0], "y")
    _sum_ok(mean.logical(), r64[1], r32[1], x.double().abs().sum(1) / d, "mean")      # a sum of d terms x_i / d that may cancel
    _each_ok(rstd.logical(), r64[2], r32[2], "rstd")
    assert all(t.outside_untouched() for t in (y, mean, rstd, rec)), "forward wrote outside its outputs"
    rc, msg, y2, mean2, rstd2, rec2, _ = _ln_fwd_c(x, w, b)
    assert rc == 0 and _same_bits((y, y2), (mean, mean2), (rstd, rstd2), (rec, rec2)), "a second forward gave other bits"
    # without the weight bounds the record is the reduced max |y| (no record at all: same y)
    rc, msg, y3, _, _, _, _ = _ln_fwd_c(x, w, b, amax=False)
    assert rc == 0 and torch.equal(y3.bits(), y.bits())
    # backward from the kernel's own statistics
    rc, msg, dx, dw, db, drec = _ln_bwd_c(dy, x, mean.logical(), rstd.logical(), w, add)
    assert rc == 0, msg
    _rows_ok(dx.logical(), r64[3], r32[3], "dx")
    xh = (x.double() - r64[1][:, None]) * r64[2][:, None]
    _sum_ok(dw.logical(), r64[4], r32[4], (dy.double() * xh).abs().sum(0), "dw")
    _sum_ok(db.logical(), r64[5], r32[5], dy.double().abs().sum(0), "db")
    assert float(drec.logical()) == float(dx.logical().abs().max()), "the record on dx is not max |dx|"
    assert all(t.outside_untouched() for t in (dx, dw, db, drec)), "backward wrote outside its outputs"
    rc, msg, dx2, dw2, db2, drec2 = _ln_bwd_c(dy, x, mean.logical(), rstd.logical(), w, add)
    assert rc == 0 and _same_bits((dx, dx2), (dw, dw2), (db, db2), (drec, drec2)), "a second backward gave other bits"


@pytest.mark.parametrize("d", LN_D)
def test_layernorm_fwd_bwd(d):
    for rows in (1, 3, 5, 67):
        for with_add in (False, True):
            _check_ln(rows, d, with_add)


def test_layernorm_bwd_ragged_workgroups():
    """4101 x 36: 9 rows per workgroup, 456 workgroups (fewer than the 512 the partial sums are laid out for), 6 rows in the last."""
    _check_ln(4101, 36, True)


def test_layernorm_record_bounds_one_hot_rows():
    """f16x2 bookkeeping: the scalar lvt_layernorm_fwd leaves on y must be >= max |y|, with no tolerance -- one-hot rows with
    w = 1, b = 0 reach sqrt(d - 1) up to fp32 rounding, for every d % 4 == 0 up to 1024."""
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    try:
        worst, fails = 0.0, []
        for d in range(4, 1025, 4):
            x = torch.zeros(4, d)
            for r in range(4):
                x[r, (7 * r + d // 3) % d] = HOT[r]
            y, _, _ = ew.layernorm_fwd(x.to(DEV), torch.ones(d, device=DEV), torch.zeros(d, device=DEV))
            rec, top = float(L._valid_amax(y)), float(y.abs().max())
            assert abs(rec - math.sqrt(d - 1.0)) <= 1e-5 * rec
            if not rec >= top:
                fails.append((d, rec, top))
            worst = max(worst, top / rec)
        print("max |y| / record: worst %.9g, %d of 256 d above the record" % (worst, len(fails)))
        assert not fails, "%d of 256 d: max |y| above the record, first (d, record, max |y|) = %r" % (len(fails), fails[0])
    finally:
        L.set_math_mode(before)


def test_layernorm_record_through_the_wrapper():
    """The record ew.layernorm_fwd leaves on y (read through binding._valid_amax) bounds max |y| on the mixed input; the one
    ew.layernorm_bwd leaves on dx equals max |dx|."""
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    try:
        for d in (4, 260, 1024):
            g = _gen(d, 99)
            x, w, b, dy = _ln_input(67, d, g).to(DEV), _rand((d,), g).to(DEV), _rand((d,), g).to(DEV), _rand((67, d), g).to(DEV)
            y, mean, rstd = ew.layernorm_fwd(x, w, b)
            assert float(L._valid_amax(y)) >= float(y.abs().max())
            dx, _, _ = ew.layernorm_bwd(dy, x, mean, rstd, w)
            assert float(L._valid_amax(dx)) == float(dx.abs().max())
    finally:
        L.set_math_mode(before)


@pytest.mark.parametrize("d", [32, 96, 512, 1024])
def test_layernorm_p2_form(d):
    """lvt_layernorm_fwd_p2: y bit-identical to the plain form, the image byte-equal to the split of y under the stored bound."""
    for rows in (3, 67):
        g = _gen(rows, d, 5)
        x, w, b = _ln_input(rows, d, g), _rand((d,), g), _rand((d,), g)
        rc, msg, y, mean, rstd, rec, _ = _ln_fwd_c(x, w, b)
        assert rc == 0, msg
        rc, msg, yp, meanp, rstdp, recp, img = _ln_fwd_c(x, w, b, p2=True)
        assert rc == 0, msg
        assert _same_bits((y, yp), (mean, meanp), (rstd, rstdp), (rec, recp)), "the P2 form computes other bits"
        ref = _image_ref(yp.logical(), float(recp.logical()))
        got = img.logical().view(torch.float16).view(rows, d // 32, 2, 32)
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), "image bytes"
        assert img.outside_untouched() and yp.outside_untouched()


@pytest.mark.parametrize("d,p2", [(6, False), (1028, False), (36, True)], ids=["d6", "d1028", "p2_d36"])
def test_layernorm_refusals(d, p2):
    x, w, b = torch.ones(3, d), torch.ones(d), torch.zeros(d)
    rc, msg, y, mean, rstd, rec, img = _ln_fwd_c(x, w, b, p2=p2)
    assert rc == -1 and "layernorm_fwd" in msg, (rc, msg)
    for t in (y, mean, rstd, rec) + ((img,) if p2 else ()):
        assert t.outside_untouched() and bool(torch.isnan(t.logical()).all()), "a refused call wrote an output"
    if not p2:
        rc, msg, dx, dw, db, drec = _ln_bwd_c(x, x, torch.zeros(3), torch.ones(3), w, None)
        assert rc == -1 and "layernorm_bwd" in msg
        assert all(bool(torch.isnan(t.logical()).all()) for t in (dx, dw, db)) and float(drec.logical()) == 0.0


# ---- 2.2 lvt_splitsum_layernorm_fwd ---------------------------------------------------------------------------------
def _ssln_c(parts, bias, res, ldr, w, b):
    splits, rows, d = parts.shape
    pb, wb, bb = fbuf(parts), fbuf(w), fbuf(b)
    biasb = fbuf(bias) if bias is not None else None
    resb = Buf(rows_idx(rows, d, ldr), res) if res is not None else None
    xo, y = obuf(rows, d), obuf(rows, d)
    rc, msg = _call(L.lib().lvt_splitsum_layernorm_fwd, _p(pb), splits, rows, d, _p(biasb), _p(resb), ldr, _p(xo), 1e-5, _p(wb),
                    _p(bb), _p(y))
    return rc, msg, xo, y


@pytest.mark.parametrize("d", [4, 260, 1024])
@pytest.mark.parametrize("splits", [1, 2, 9, 17])
def test_splitsum_layernorm(d, splits):
    for rows in (1, 5):
        for has_bias, has_res in ((False, False), (True, False), (False, True), (True, True)):
            g = _gen(d, splits, rows, has_bias, 2 * has_res)
            parts, w, b = _rand((splits, rows, d), g), _rand((d,), g), _rand((d,), g)
            bias = _rand((d,), g) if has_bias else None
            res = _rand((rows, d), g, -2, 2) if has_res else None
            ldr = d + 8
            ref = []
            for dt in (torch.float64, torch.float32):
                x = parts.to(dt).sum(0)
                if has_bias:
                    x = x + bias.to(dt)
                if has_res:
                    x = x + res.to(dt)
                ref.append((x, F.layer_norm(x, (d,), w.to(dt), b.to(dt), 1e-5)))
            rc, msg, xo, y = _ssln_c(parts, bias, res, ldr, w, b)
            assert rc == 0, msg
            _rows_ok(xo.logical(), ref[0][0], ref[1][0], "x")
            _rows_ok(y.logical(), ref[0][1], ref[1][1], "y")
            assert xo.outside_untouched() and y.outside_untouched()
            rc, msg, xo2, y2 = _ssln_c(parts, bias, res, ldr, w, b)
            assert rc == 0 and _same_bits((xo, xo2), (y, y2))


# ---- 2.3 cross entropy --------------------------------------------------------------------------------------------------
IGN = -100


def _xent_case(V, B, P, layout, ignored, g):
    rows = B * P
    logits = _rand((rows, V), g, -3, 3)
    logits[0] = -80.0
    logits[0, int(torch.randint(0, V, (1,), generator=g))] = 80.0          # one +80 among -80
    if rows > 1:
        logits[rows - 1] = 0.375                                            # an all-equal row
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[0] = 0
    tgt[rows - 1] = V - 1
    if rows > 2:
        tgt[1] = V - 1
        tgt[2] = 0
    if ignored == "some":
        tgt[torch.rand(rows, generator=g) < 0.3] = IGN
        tgt[rows // 2] = IGN
    elif ignored == "all":
        tgt[:] = IGN
    # the holder: every element the kernel must NOT read is another valid target
    if layout == "channel":                                                  # channel 1 of (B, nc = 3, P), as the model passes it
        hold = torch.randint(0, V, (B, 3, P), generator=g)
        hold[:, 1] = tgt.view(B, P)
        first, sb, sp = hold[0, 1], 3 * P, 1
    else:                                                                    # (P, B): position-major
        hold = tgt.view(B, P).t().contiguous()
        first, sb, sp = hold, 1, B
    return logits, tgt, hold, first, sb, sp


def _xent_ref(logits, tgt, gout, scale, dtype):
    lg = logits.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(lg, tgt, ignore_index=IGN) * scale
    lse = torch.logsumexp(lg.detach(), -1)
    if bool((tgt != IGN).any()):
        (loss * gout).backward()
        dl = lg.grad
    else:
        dl = torch.zeros_like(lg)
    return loss.detach(), lse, dl


def _xent_c(logits, hold, first, sb, sp, P, gout, scale):
    rows, V = logits.shape
    lib = L.lib()
    lb = fbuf(logits)
    hd = hold.to(DEV)
    tptr = C.c_void_p(hd.data_ptr() + first.storage_offset() * 8)
    row_loss, lse, loss, count = obuf(rows), obuf(rows), obuf(1), obuf(1)
    nws = lib.lvt_xent_workspace_bytes()
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc, msg = _call(lib.lvt_xent_fwd, _p(lb), tptr, sb, sp, P, rows, V, IGN, scale, _p(row_loss), _p(lse), _p(loss), _p(count),
                    L.ptr(ws), nws)
    if rc:
        return rc, msg, (row_loss, lse, loss, count), None
    dl, rec = obuf(rows, V), obuf(1)
    gb = fbuf(torch.tensor([gout]))
    rc, msg = _call(lib.lvt_xent_bwd, _p(lb), tptr, sb, sp, P, rows, V, IGN, L.ptr(lse.view), L.ptr(count.view), _p(gb), scale,
                    _p(dl), _p(rec))
    return rc, msg, (row_loss, lse, loss, count), (dl, rec)


def _check_xent(V, B, P, layout, ignored):
    g = _gen(V, B, P, len(layout), len(ignored))
    logits, tgt, hold, first, sb, sp = _xent_case(V, B, P, layout, ignored, g)
    gout, scale = 1.75, 0.25
    (l64, lse64, dl64), (l32, lse32, dl32) = (_xent_ref(logits, tgt, gout, scale, dt) for dt in (torch.float64, torch.float32))
    rc, msg, fw, bw = _xent_c(logits, hold, first, sb, sp, P, gout, scale)
    assert rc == 0, msg
    row_loss, lse, loss, count = fw
    dl, rec = bw
    keep = tgt != IGN
    n = int(keep.sum())
    assert float(count.logical()) == n, "count"
    _each_ok(lse.logical(), lse64, lse32, "lse")
    if n == 0:
        assert math.isnan(float(loss.logical())) and math.isnan(float(l64)), "all rows ignored: the loss is NaN, as torch's"
        assert bool((dl.logical() == 0).all()), "all rows ignored: dlogits must be exactly 0"
    else:
        terms = (lse64 - logits.double().gather(1, tgt.clamp_min(0)[:, None])[:, 0]).abs()[keep].sum() * scale / n
        _sum_ok(loss.logical().reshape(()), l64, l32, terms, "loss")
        _rows_ok(dl.logical(), dl64, dl32, "dlogits")
        assert bool((dl.logical()[~keep] == 0).all()) and bool((row_loss.logical()[~keep] == 0).all()), "ignored rows must be exactly 0"
        assert float(rec.logical()) >= float(dl.logical().abs().max()), "dl_amax is not a bound of max |dlogits|"
        assert float(rec.logical()) == abs(float(torch.tensor(gout) * torch.tensor(scale) / torch.tensor(float(n))))
    assert all(t.outside_untouched() for t in fw + bw), "a float outside an output was written"
    rc, msg, fw2, bw2 = _xent_c(logits, hold, first, sb, sp, P, gout, scale)
    assert rc == 0 and _same_bits(*zip(fw + bw, fw2 + bw2)), "a second launch gave other bits"


@pytest.mark.parametrize("ignored", ["none", "some", "all"])
@pytest.mark.parametrize("layout", ["channel", "transposed"])
@pytest.mark.parametrize("V", [256, 768, 4096])
def test_xent_fwd_bwd(V, layout, ignored):
    for B, P in ((1, 1), (3, 5), (2, 300)):
        _check_xent(V, B, P, layout, ignored)


@pytest.mark.parametrize("ignored", ["none", "some"])
def test_xent_many_partial_workgroups(ignored):
    """rows = 2050 at V = 256: 513 row workgroups with a ragged last one, 9 partial-sum workgroups."""
    _check_xent(256, 2, 1025, "channel", ignored)


@pytest.mark.parametrize("V", [260, 4352])
def test_xent_refusals(V):
    logits = torch.zeros(4, V)
    hold = torch.zeros(4, dtype=torch.int64)
    rc, msg, fw, _ = _xent_c(logits, hold, hold, 4, 1, 4, 1.0, 1.0)
    assert rc == -1 and "unsupported" in msg, (rc, msg)
    assert all(t.outside_untouched() and bool(torch.isnan(t.logical()).all()) for t in fw)


# ---- 2.4 embedding bag ------------------------------------------------------------------------------------------------------
def _iarr(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _embbag_c(idx, bstride, P, rows, off, tab, table, D, bias, btable, bindex):
    tb = fbuf(table)
    bb = fbuf(bias) if bias is not None else None
    btb = fbuf(btable) if btable is not None else None
    bi = bindex.to(DEV) if bindex is not None else None
    out = obuf(rows, D)
    idev = idx.to(DEV)
    rc = L.lib().lvt_embbag_fwd(L.ptr(idev), bstride, P, rows, len(off), _iarr(off), _iarr(tab), _p(tb), D, _p(bb), _p(btb), L.ptr(bi),
                                _p(out), L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, out


@pytest.mark.parametrize("slots", [1, 7, 9, 32])
@pytest.mark.parametrize("D", [4, 36, 128, 260])
def test_embbag_is_the_slot_ordered_fp32_sum(D, slots):
    """out = bias, + slot 0 .. n-1 in order, + btable: bit-equal to numpy float32 additions in that order (slots are gathered eight at
    a time; 7 / 9 / 32 cover a short group, a group plus one and four full groups)."""
    for B, P in ((1, 1), (3, 5)):
        for has_bias, has_bt in ((False, False), (True, True), (True, False), (False, True)):
            g = _gen(D, slots, B, P, has_bias, 2 * has_bt)
            sizes = [3 + (5 * s) % 11 for s in range(slots)]                     # non-uniform tables
            tab = [sum(sizes[:s]) for s in range(slots)]
            off = [s * P for s in range(slots)]
            bstride = slots * P + 13                                             # larger than the packed size
            idx = torch.randint(0, 3, (B, bstride), generator=g)                 # the gap holds valid indices of every table
            for s in range(slots):
                idx[:, s * P:(s + 1) * P] = torch.randint(-1, sizes[s], (B, P), generator=g)
            idx[B - 1, torch.arange(slots) * P + (P - 1)] = -1                   # one row whose every slot is -1
            table = _rand((sum(sizes), D), g)
            bias = _rand((D,), g) if has_bias else None
            btable = _rand((5, D), g) if has_bt else None
            bindex = torch.randint(0, 5, (B,), generator=g) if has_bt else None
            rows = B * P
            ref = np.zeros((rows, D), np.float32)
            tn = table.numpy()
            for r in range(rows):
                bq, pos = divmod(r, P)
                acc = bias.numpy().copy() if has_bias else np.zeros(D, np.float32)
                for s in range(slots):
                    i = int(idx[bq, off[s] + pos])
                    if i >= 0:
                        acc = acc + tn[tab[s] + i]
                if has_bt:
                    acc = acc + btable.numpy()[int(bindex[bq])]
                ref[r] = acc
            rc, msg, out = _embbag_c(idx, bstride, P, rows, off, tab, table, D, bias, btable, bindex)
            assert rc == 0, msg
            assert torch.equal(out.logical(), torch.from_numpy(ref)), (B, P, has_bias, has_bt)
            assert out.outside_untouched()


def test_embbag_refuses_33_slots():
    idx = torch.zeros(1, 33, dtype=torch.int64)
    rc, msg, out = _embbag_c(idx, 33, 1, 1, list(range(33)), [0] * 33, torch.ones(4, 4), 4, None, None, None)
    assert rc == -1 and "embbag_fwd" in msg and bool(torch.isnan(out.logical()).all()) and out.outside_untouched()


# ---- 2.5 small glue kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 36, 512])
def test_add_periodic(d):
    for rows in (1, 7, 1000):
        for P in (1, 3, 7, 1000):
            g = _gen(d, rows, P)
            x, tab = _rand((rows, d), g), _rand((P, d), g)
            xb, tb = fbuf(x), fbuf(tab)
            rc, msg = _call(L.lib().lvt_add_periodic, _p(xb), _p(tb), rows, P, d)
            assert rc == 0, msg
            assert torch.equal(xb.logical(), x + tab[torch.arange(rows) % P]) and xb.outside_untouched(), (rows, P)


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_axpy(n):
    for has_dev, has_add in ((False, False), (True, False), (False, True), (True, True)):
        g = _gen(n, has_dev, 2 * has_add)
        x, add, adev = _rand((n,), g), _rand((n,), g), torch.tensor([-0.625])
        xb, ab, db, out = fbuf(x), fbuf(add) if has_add else None, fbuf(adev) if has_dev else None, obuf(n)
        rc, msg = _call(L.lib().lvt_axpy, _p(xb), _p(ab), n, _p(db), 1.7, _p(out))
        assert rc == 0, msg
        a = torch.tensor(1.7, dtype=torch.float32) * (adev[0] if has_dev else torch.tensor(1.0))     # formed in float32
        ref = a.double() * x.double() + (add.double() if has_add else 0)
        tol = 2.0 ** -23 * ((a.double() * x.double()).abs() + (add.double().abs() if has_add else 0))
        assert bool(((out.logical().double() - ref).abs() <= tol).all()) and out.outside_untouched()


def _permute3_c(src, strides, shape, offset=0):
    sb, out = fbuf(src), obuf(*shape)
    rc = L.lib().lvt_permute3(C.c_void_p(sb.view.data_ptr() + 4 * offset), strides[0], strides[1], strides[2], shape[0], shape[1], shape[2],
                              _p(out), L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    assert rc == 0, msg
    ref = torch.as_strided(src.reshape(-1), shape, strides, offset).contiguous()
    assert torch.equal(out.logical().view(torch.int32), ref.view(torch.int32)) and out.outside_untouched(), (strides, shape)


def test_permute3():
    g = _gen(3)
    de, ncnv, KK = 12, 10, 6
    # conv weight (de, nc*nv, KK) -> packed (KK, nc*nv, de), and the gradient's way back (videotransformer.py)
    _permute3_c(_rand((de, ncnv, KK), g), (1, KK, ncnv * KK), (KK, ncnv, de))
    _permute3_c(_rand((KK * ncnv, de), g), (1, de, ncnv * de), (de, ncnv, KK))
    # a zero stride and a dimension of 1: column block `d..` of a (rows, fin) weight, transposed (the channel predictor's U_k)
    fin, d0, ncols, rws = 20, 8, 12, 7
    _permute3_c(_rand((rws, fin), g), (1, fin, 0), (ncols, rws, 1), offset=d0)
    _permute3_c(_rand((5, 9), g), (9, 0, 1), (5, 3, 9))                       # a broadcast middle dimension
    _permute3_c(_rand((1, 6, 5), g), (30, 1, 5), (1, 5, 6))                  # a leading dimension of 1, transposed
    # more than 8192 x 256 elements: the grid is capped and every thread strides
    n0, n1, n2 = 33, 257, 256
    _permute3_c(_rand((n1, n0, n2), g), (n2, n0 * n2, 1), (n0, n1, n2))


@pytest.mark.parametrize("d", [4, 132])
@pytest.mark.parametrize("S", [1, 6, 1024])
def test_row_gather(S, d):
    for B in (1, 3):
        g = _gen(S, d, B)
        x = _rand((B * S, d), g)
        perm = torch.randperm(S, generator=g)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(S)
        xb, out = fbuf(x), obuf(B * S, d)
        rc, msg = _call(L.lib().lvt_row_gather, _p(xb), L.ptr(perm.to(DEV)), B, S, d, _p(out))
        assert rc == 0, msg
        ref = x.view(B, S, d)[:, perm].reshape(B * S, d)
        assert torch.equal(out.logical(), ref) and out.outside_untouched()
        back = obuf(B * S, d)
        rc, msg = _call(L.lib().lvt_row_gather, L.ptr(out.view), L.ptr(inv.to(DEV)), B, S, d, _p(back))
        assert rc == 0 and torch.equal(back.logical(), x) and back.outside_untouched(), "the inverse does not restore the input"
    # the wrapper hands the record of x on in f16x2 mode (a permutation of the rows: same max |.|)
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    try:
        xd = x.to(DEV)
        slot = L.amax_of(xd)
        o = ew.row_gather(xd, perm.to(DEV), S)
        assert L._valid_amax(o) is slot and float(slot) == float(x.abs().max()) and torch.equal(o.cpu(), ref)
    finally:
        L.set_math_mode(before)


@pytest.mark.parametrize("rows", [1, 300])
def test_decode_gather_and_commit(rows):
    """The documented clamps: the cursor is clamped to [0, S) for the gather; neighbour entries < 0 or >= S1 read the padded
    slot S1 - 1; commit writes column `cursor` only for 0 <= cursor < S1 - 1 and with `drawn`, and always increments."""
    S, taps = 9, 5
    S1 = S + 1
    g = _gen(rows, 11)
    codes = torch.randint(0, 512, (rows, S1), generator=g)
    codes[:, S] = -7                                                           # the padded slot
    nb = torch.randint(0, S1, (S, taps), generator=g)
    nb[:, 0] = -3                                                              # < 0       -> padded slot
    nb[:, 1] = S1 + 4                                                          # >= S1     -> padded slot
    nb[:, 2] = S                                                               # == S: the padded slot itself
    lib = L.lib()
    for cur in (-2, 0, 4, S - 1, S, S + 5):
        pos = torch.tensor([cur], dtype=torch.int32, device=DEV)
        cb, nbb, out = IBuf(dense(rows, S1), codes), IBuf(dense(S, taps), nb), IBuf(dense(rows, taps))
        rc, msg = _call(lib.lvt_decode_gather_codes, _p(cb), _p(nbb), L.ptr(pos), rows, S1, taps, _p(out))
        assert rc == 0, msg
        c = min(max(cur, 0), S - 1)
        n = nb[c].clone()
        n[(n < 0) | (n >= S1)] = S
        assert torch.equal(out.logical(), codes[:, n]) and out.outside_untouched(), cur
        assert int(pos) == cur and torch.equal(cb.bits(), IBuf(dense(rows, S1), codes).bits())
        drawn = torch.randint(1000, 2000, (rows,), generator=g)
        for with_drawn in (True, False):
            pos = torch.tensor([cur], dtype=torch.int32, device=DEV)
            cb, db = IBuf(dense(rows, S1), codes), IBuf(dense(rows), drawn)
            rc, msg = _call(lib.lvt_decode_commit, _p(db) if with_drawn else None, rows, S1, _p(cb), L.ptr(pos))
            assert rc == 0, msg
            want = codes.clone()
            if with_drawn and 0 <= cur < S1 - 1:
                want[:, cur] = drawn
            assert torch.equal(cb.logical(), want) and cb.outside_untouched(), (cur, with_drawn)
            assert int(pos) == cur + 1, "commit must always advance the cursor"


# ---- 2.6 small-M GEMM paths nobody runs -----------------------------------------------------------------------------
B_, R_, U_ = L.EPI_BIAS, L.EPI_RESIDUAL, L.EPI_RELU


def _r4(x):
    return (x + 3) // 4 * 4


class SCell:
    def __init__(self, M, N, K, tb=0, flags=0, alpha=1.0, batch=1, pc=4, cur=None, c_pos=0, r_pos=0, name=None):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def __repr__(self):
        return self.name or "M%dN%dK%d_tb%d_f%x_a%g_b%d_pc%d%s" % (self.M, self.N, self.K, self.tb, self.flags, self.alpha, self.batch,
                                                                   self.pc, "" if self.cur is None else "_pos%d" % self.cur)


def _small_operands(c):
    g = _gen(c.M, c.N, c.K, c.tb, c.flags, c.batch)
    M, N, K, Z = c.M, c.N, c.K, c.batch
    o = {}
    o["A"], o["B"] = _rand((M, K), g), _rand((Z, K, N), g)
    o["lda"] = K + 4
    o["abuf"] = Buf(rows_idx(M, K, o["lda"]), o["A"])
    if c.tb == 0:
        o["ldb"] = K + 8
        b1 = rows_idx(N, K, o["ldb"]).t()
    else:
        o["ldb"] = N + 4
        b1 = rows_idx(K, N, o["ldb"])
    o["sB"] = _r4(int(b1.max()) + 1 + 12) if Z > 1 else 0
    o["bbuf"] = Buf(torch.arange(Z)[:, None, None] * o["sB"] + b1[None], o["B"])
    o["ldc"] = N + c.pc
    o["sC"] = M * o["ldc"] + 20 if Z > 1 else 0
    shift = (c.cur or 0) * c.c_pos
    o["cidx"] = shift + torch.arange(Z)[:, None, None] * o["sC"] + rows_idx(M, N, o["ldc"])[None]
    o["ldr"] = N + 8
    o["ridx"] = (c.cur or 0) * c.r_pos + rows_idx(M, N, o["ldr"])
    o["bias"], o["res"] = _rand((N,), g), _rand((M, N), g)
    return o


def _small_launch(c, o, through_wrapper=False):
    cbuf = Buf(o["cidx"])
    bias = fbuf(o["bias"]) if c.flags & B_ else None
    res = Buf(o["ridx"], o["res"]) if c.flags & R_ else None
    pos = torch.tensor([c.cur], dtype=torch.int32, device=DEV) if c.cur is not None else None
    if through_wrapper:
        G.gemm_small(o["abuf"].view, o["bbuf"].view, cbuf.view, c.M, c.N, c.K, tb=c.tb, lda=o["lda"], ldb=o["ldb"], ldc=o["ldc"],
                     batch=c.batch, sB=o["sB"], sC=o["sC"], alpha=c.alpha, flags=c.flags, bias=bias.view if bias else None,
                     res=res.view if res else None, ldr=o["ldr"], pos=pos, c_pos=c.c_pos, r_pos=c.r_pos)
        torch.cuda.synchronize()
        return 0, "", cbuf
    rc, msg = _call(L.lib().lvt_gemm_smallm_f32, c.M, c.N, c.K, c.tb, _p(o["abuf"]), o["lda"], _p(o["bbuf"]), o["ldb"], _p(cbuf), o["ldc"],
                    c.batch, o["sB"], o["sC"], c.alpha, c.flags, _p(bias), _p(res), o["ldr"], L.ptr(pos), c.c_pos, c.r_pos)
    return rc, msg, cbuf


def _small_check(c, o, cbuf):
    A, Bm = o["A"].double(), o["B"].double()
    v = c.alpha * (A @ Bm)
    extra = torch.zeros_like(v)
    if c.flags & B_:
        v = v + o["bias"].double()
        extra += o["bias"].double().abs()
    if c.flags & R_:
        v = v + o["res"].double()
        extra += o["res"].double().abs()
    if c.flags & U_:
        v = v.clamp_min(0.0)
    tol = 1e-5 * abs(c.alpha) * (A.abs() @ Bm.abs()) + EPS * (extra + v.abs())
    got = cbuf.logical().double()
    bad = ~((got - v).abs() <= tol)
    assert not bool(bad.any()), "%d elements out of bound (first %s)" % (int(bad.sum()), tuple(bad.nonzero()[0].tolist()))
    if c.flags & U_:
        assert bool((got >= 0).all())
    assert cbuf.outside_untouched(), "a float outside the logical C was written"


SCELLS = [
    # lvt_gemm_smallm_kernel<0>: tb = 0 with K % 8 == 4
    SCell(1, 16, 4), SCell(7, 100, 132, flags=B_ | R_, alpha=1.25), SCell(64, 48, 260, flags=U_, alpha=-0.75),
    # <1>
    SCell(5, 20, 36, tb=1, flags=B_ | R_ | U_, alpha=1.5),
    # the MFMA kernel: a ragged second 32-row tile, N = 40, K = 24 (the zero-filled half step), three 64-row blocks
    SCell(33, 40, 24, flags=B_), SCell(130, 40, 64, flags=R_, alpha=0.5),
    # batch = 3 with sB / sC and ldc > N through the device cursor: the q / k / v call of a decode step
    SCell(5, 40, 64, batch=3, pc=120, cur=2, c_pos=40, name="qkv_decode_step"),
    # cursor with c_pos and r_pos on all three kernels
    SCell(7, 100, 132, flags=B_ | R_, cur=2, c_pos=52, r_pos=36), SCell(5, 20, 36, tb=1, flags=R_, cur=2, c_pos=24, r_pos=8),
    SCell(33, 40, 24, flags=R_ | U_, cur=2, c_pos=44, r_pos=12),
]
# every epilogue subset on one cell of each kernel
for s in range(8):
    f = (B_ if s & 1 else 0) | (R_ if s & 2 else 0) | (U_ if s & 4 else 0)
    SCELLS += [SCell(7, 20, 36, flags=f, alpha=-1.5), SCell(6, 20, 36, tb=1, flags=f, alpha=-1.5), SCell(40, 36, 72, flags=f, alpha=-1.5)]


@pytest.mark.parametrize("c", SCELLS, ids=repr)
def test_gemm_small_m(c):
    o = _small_operands(c)
    rc, msg, cbuf = _small_launch(c, o)
    assert rc == 0, msg
    _small_check(c, o, cbuf)
    rc, msg, cbuf2 = _small_launch(c, o)
    assert rc == 0 and torch.equal(cbuf.bits(), cbuf2.bits()), "a second launch gave other bits"


def test_gemm_small_m_split_k_with_cursor():
    """gemm_small at K = 1024: four k ranges through lvt_gemm_smallm_splitk_f32, with the device cursor, ldc > N and a residual."""
    c = SCell(3, 36, 1024, flags=B_ | R_ | U_, alpha=0.5, pc=12, cur=2, c_pos=48, r_pos=44)
    assert G._smallm_splits(c.N, c.K) == 4
    o = _small_operands(c)
    _, _, cbuf = _small_launch(c, o, through_wrapper=True)
    _small_check(c, o, cbuf)
    _, _, cbuf2 = _small_launch(c, o, through_wrapper=True)
    assert torch.equal(cbuf.bits(), cbuf2.bits())


@pytest.mark.parametrize("c", [SCell(70, 16, 16, tb=1), SCell(4, 16, 6)], ids=["M70_tb1", "K6"])
def test_gemm_small_m_refusals(c):
    o = _small_operands(c) if c.K % 4 == 0 else _small_operands(SCell(4, 16, 8))
    rc, msg, cbuf = _small_launch(c, o)
    assert rc == -1 and "gemm_smallm" in msg, (rc, msg)
    assert bool((cbuf.bits() == 0x7FC0DEAD).all()), "a refused call wrote C"
