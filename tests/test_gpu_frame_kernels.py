"""The frame-boundary and pixel-loss kernels at the top of csrc/elementwise.hip and lvt_colsum (csrc/gemm_engine.hip), each C entry
point against a plain fp64 (or, for pure data movement, a bit-exact) reference in NaN-payload guard buffers (tests/util_guard.py):
lvt_to_channels_last / lvt_to_channels_first, lvt_mse_fwd / lvt_l1_fwd, lvt_mse_bwd / lvt_l1_bwd / lvt_mse_bwd_plus /
lvt_l1_bwd_plus / lvt_tanh_bwd / lvt_sigmoid_bwd, lvt_colsum.  All but lvt_colsum are grid-stride kernels under a grid cap (1024
workgroups for the loss sums, 2048 for a launch that reports max |out|, 8192 otherwise): every family has one case past its cap,
where the loop takes a second trip.

Bounds (tests/util_vq_ref.py): pointwise outputs per row, reductions against sum |terms|, layout mode 0 bit-exact.  A gradient
tensor is one row: its maximum is the scale its consumers work under.
[guard]: every element outside the logical output still holds the payload, inputs sit in payload buffers too;
[repeat]: a second launch into fresh buffers gives the same bits."""
import ctypes as C

import pytest
import torch

from lvt_amd.hip import binding as L
from util_guard import DEV, Buf, dense, fbuf, obuf, rows_idx
from util_vq_ref import rows_ok, sum_ok

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")


def _gen(*key):
    return torch.Generator().manual_seed(3000 + sum(int(k) * (5 + 8 * i) for i, k in enumerate(key)))


def _rand(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float() * (hi - lo) + lo


def _call(fn, *args):
    rc = fn(*args, L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg


def _p(b):
    return L.ptr(b.view) if b is not None else C.c_void_p(0)


def _untouched(*bufs):
    return all(b.outside_untouched() and bool((b.bits() == b.payload).all()) for b in bufs)


# ---- B1 layout -------------------------------------------------------------------------------------------------------
LAYOUT = [(1, 4), (3, 4), (4, 4), (5, 8), (3, 12)]


def _affine(Cc, g):
    """Per-channel (a, s) of both directions: s in 0.3 .. 0.7, a in 0.4 .. 0.6."""
    return _rand((Cc,), g, 0.4, 0.6), _rand((Cc,), g, 0.3, 0.7)


def _to_last(x, ldo, mode, a, s, amax0=0.0):
    B, Cc, R = x.shape
    xb, ab, sb = fbuf(x), fbuf(a), fbuf(s)
    out, rec = obuf(B, R, ldo), Buf(dense(1), torch.tensor([amax0]))
    rc, msg = _call(L.lib().lvt_to_channels_last, _p(xb), B, Cc, R, ldo, mode, _p(ab), _p(sb), _p(out), _p(rec))
    return rc, msg, out, rec


def _to_first(x, ldi, mode, a, s, lo, hi):
    """x (B, R, C) logical, stored with pitch ldi; the padding columns hold the NaN payload."""
    B, R, Cc = x.shape
    xb = Buf(rows_idx(B * R, Cc, ldi), x.reshape(B * R, Cc))
    ab, sb = fbuf(a), fbuf(s)
    out = obuf(B, Cc, R)
    rc, msg = _call(L.lib().lvt_to_channels_first, _p(xb), B, Cc, R, ldi, mode, _p(ab), _p(sb), lo, hi, _p(out))
    return rc, msg, out


def _check_to_last(B, Cc, R, ldo, mode):
    g = _gen(B, Cc, R, ldo, mode)
    x = _rand((B, Cc, R), g, -2.0, 2.0)
    a, s = _affine(Cc, g)
    rc, msg, out, rec = _to_last(x, ldo, mode, a, s)
    assert rc == 0, msg
    got = out.logical()
    xt = x.transpose(1, 2)                                                     # (B, R, C)
    if mode == 0:
        assert torch.equal(got[:, :, :Cc].view(torch.int32), xt.contiguous().view(torch.int32)), "mode 0 is a copy"
    else:
        rows_ok(got[:, :, :Cc], (xt.double() - a.double()) / s.double(), (xt - a) / s, "(x - a) / s")
    assert bool((got[:, :, Cc:].view(torch.int32) == 0).all()), "the pad channels are not exact zeros"
    assert float(rec.logical()) == float(got.abs().max()), "the record is not max |out|"
    assert out.outside_untouched() and rec.outside_untouched()
    rc, msg, out2, rec2 = _to_last(x, ldo, mode, a, s)
    assert rc == 0 and torch.equal(out.bits(), out2.bits()) and torch.equal(rec.bits(), rec2.bits()), "a second launch gave other bits"


def _check_to_first(B, Cc, R, ldi, mode):
    g = _gen(B, Cc, R, ldi, mode, 1)
    x = _rand((B, R, Cc), g, -4.0, 4.0)
    a, s = _affine(Cc, g)
    lo, hi = 0.0, 1.0                                                          # x s + a spans at least -0.6 .. 1.6: binds on both sides
    rc, msg, out = _to_first(x, ldi, mode, a, s, lo, hi)
    assert rc == 0, msg
    got = out.logical()
    assert not bool(torch.isnan(got).any()), "input padding reached the output"
    xt = x.transpose(1, 2)                                                     # (B, C, R)
    if mode == 0:
        assert torch.equal(got.view(torch.int32), xt.contiguous().view(torch.int32)), "mode 0 is a copy"
    else:
        pre64 = xt.double() * s.double()[:, None] + a.double()[:, None]
        pre32 = xt * s[:, None] + a[:, None]
        rows_ok(got, pre64.clamp(lo, hi), pre32.clamp(lo, hi), "clamp(x s + a)")
        slack = 2.0 ** -20
        assert bool((got[pre64 > hi + slack] == hi).all()) and bool((got[pre64 < lo - slack] == lo).all()), "not exact where the clamp binds"
        if R > 1:
            assert int((pre64 > hi + slack).sum()) and int((pre64 < lo - slack).sum()), "the clamp does not bind on both sides"
    assert out.outside_untouched()
    rc, msg, out2 = _to_first(x, ldi, mode, a, s, lo, hi)
    assert rc == 0 and torch.equal(out.bits(), out2.bits()), "a second launch gave other bits"


@pytest.mark.parametrize("Cc,pitch", LAYOUT)
def test_to_channels_last(Cc, pitch):
    """lvt_to_channels_last_kernel, modes 0 and 1, B in {1, 3}, R in {1, 4097}: at most 3 x 4097 x 12 = 147492 outputs, below the
    2048 x 256 outputs of one trip of the capped grid (a record is asked for)."""
    for B in (1, 3):
        for R in (1, 4097):
            for mode in (0, 1):
                _check_to_last(B, Cc, R, pitch, mode)


@pytest.mark.parametrize("Cc,pitch", LAYOUT)
def test_to_channels_first(Cc, pitch):
    """lvt_to_channels_first_kernel, modes 0 and 2 (per-channel a, s; the clamp binds on both sides), B in {1, 3}, R in {1, 4097},
    input pitch > C with payload padding: one trip of the 8192-workgroup grid."""
    for B in (1, 3):
        for R in (1, 4097):
            for mode in (0, 2):
                _check_to_first(B, Cc, R, pitch, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_to_channels_last_past_the_grid_cap(mode):
    """B R ldo = 2 x 70000 x 4 = 560000 outputs with a record: more than 2048 workgroups x 256, the loop's second trip."""
    _check_to_last(2, 3, 70000, 4, mode)


@pytest.mark.parametrize("mode", [0, 2])
def test_to_channels_first_past_the_grid_cap(mode):
    """B C R = 2 x 3 x 350003 = 2100018 outputs: more than 8192 workgroups x 256, the loop's second trip."""
    _check_to_first(2, 3, 350003, 4, mode)


def test_layout_refuses_the_other_direction_s_mode():
    """lvt_to_channels_last knows modes {0, 1}, lvt_to_channels_first {0, 2}: every other mode is LVT_EINVAL and nothing is
    written (mode 2 / mode 1 used to return LVT_OK after applying no transform)."""
    g = _gen(9)
    x, (a, s) = _rand((2, 3, 5), g), _affine(3, g)
    for mode in (2, 3, -1):
        rc, msg, out, rec = _to_last(x, 4, mode, a, s)
        assert rc == -1 and "to_channels_last" in msg, (mode, rc, msg)
        assert _untouched(out) and float(rec.logical()) == 0.0
    for mode in (1, 3, -1):
        rc, msg, out = _to_first(x.transpose(1, 2).contiguous(), 4, mode, a, s, 0.0, 1.0)
        assert rc == -1 and "to_channels_first" in msg, (mode, rc, msg)
        assert _untouched(out)


def test_to_channels_first_keeps_nan_and_clamps_inf():
    """Mode 2 on NaN and +-inf pixels: the reference's clamp_ keeps a NaN a NaN (fminf(fmaxf(v, lo), hi) returned lo) and takes
    +-inf to the bounds; mode 0 copies the bits."""
    g = _gen(10)
    x, (a, s) = _rand((1, 9, 3), g, -1.2, 1.2), _affine(3, g)
    x[0, 2, 0], x[0, 3, 1], x[0, 4, 2], x[0, 5, 0] = NAN, INF, -INF, NAN
    rc, msg, out = _to_first(x, 4, 2, a, s, 0.0, 1.0)
    assert rc == 0, msg
    got = out.logical()
    want = (x.transpose(1, 2) * s[:, None] + a[:, None]).clamp_(0.0, 1.0)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 2, "a NaN pixel did not stay NaN"
    assert float(got[0, 1, 3]) == 1.0 and float(got[0, 2, 4]) == 0.0, "+-inf pixels do not land on the bounds"
    fin = ~torch.isnan(want)
    rows_ok(got[fin][None], want.double()[fin][None], want[fin][None], "finite pixels")
    rc, msg, out0 = _to_first(x, 4, 0, a, s, 0.0, 1.0)
    assert rc == 0 and torch.equal(out0.logical().view(torch.int32), x.transpose(1, 2).contiguous().view(torch.int32))


def test_to_channels_first_finite_bits_as_recorded(golden):
    """Fixture frame_to_first_mode2 (B 1, C 3, pitch 4, R 4097, the clamp binding on 1112 + 981 of 12291 outputs): the output the
    fminf / fmaxf form of the kernel gave on an MI355X before the comparison form replaced it.  Finite inputs: the same bits."""
    f = golden("frame_to_first_mode2")
    rc, msg, out = _to_first(f["x"], 4, 2, f["a"], f["s"], float(f["lo"]), float(f["hi"]))
    assert rc == 0, msg
    assert torch.equal(out.logical().view(torch.int32), f["out"].view(torch.int32))


# ---- B2 loss forward -----------------------------------------------------------------------------------------------
BIG_FWD = 4 * (1024 * 1024 + 3077)


def _loss_fwd(l1, a, b, denom, scale, ws_bytes=None, n=None):
    lib = L.lib()
    ab, bb, out = fbuf(a), fbuf(b), obuf(1)
    full = lib.lvt_reduce_workspace_bytes()
    ws = torch.empty(full, dtype=torch.uint8, device=DEV)
    nws = full if ws_bytes is None else ws_bytes
    rc, msg = _call(lib.lvt_l1_fwd if l1 else lib.lvt_mse_fwd, _p(ab), _p(bb), a.numel() if n is None else n, float(denom), scale,
                    _p(out), L.ptr(ws) if nws else C.c_void_p(0), nws)
    return rc, msg, out


@pytest.mark.parametrize("n", [4, 4092, 4096, BIG_FWD])
@pytest.mark.parametrize("l1", [False, True], ids=["mse", "l1"])
def test_loss_fwd(l1, n):
    """lvt_sqdiff_partial_kernel<L1> + lvt_scalar_finish_kernel: one float4 (one thread), 1023 and 1024 float4 (the last thread
    of a 4-float4-per-thread workgroup idle / busy), and 1024 x 1024 + 3077 float4: past 1024 workgroups x 1024, where 3077
    threads take a fifth float4.  Reduction bound against the fp64 sum of the fp32 operands' exact differences."""
    g = _gen(n, l1)
    a, b = _rand((n,), g), _rand((n,), g)
    d = a.double() - b.double()
    terms64 = d.abs().sum() if l1 else (d * d).sum()
    d32 = a - b
    terms32 = d32.abs().sum() if l1 else (d32 * d32).sum()
    for denom in (n, 1):
        rc, msg, out = _loss_fwd(l1, a, b, denom, 0.7)
        assert rc == 0, msg
        k = 0.7 / denom
        sum_ok(out.logical(), k * terms64.reshape(1), (terms32 * torch.tensor(k, dtype=torch.float32)).reshape(1), k * terms64.reshape(1),
               "loss, denom %d" % denom)
        assert out.outside_untouched()
        rc, msg, out2 = _loss_fwd(l1, a, b, denom, 0.7)
        assert rc == 0 and torch.equal(out.bits(), out2.bits()), "a second launch gave other bits"


@pytest.mark.parametrize("l1", [False, True], ids=["mse", "l1"])
def test_loss_fwd_refusals(l1):
    a = torch.ones(8)
    full = L.lib().lvt_reduce_workspace_bytes()
    for kw in (dict(n=6), dict(denom=0.0), dict(denom=-1.0), dict(ws_bytes=full - 1), dict(ws_bytes=0)):
        rc, msg, out = _loss_fwd(l1, a, a, kw.get("denom", 8.0), 0.7, kw.get("ws_bytes"), kw.get("n"))
        assert rc == -1 and "_fwd" in msg, (kw, rc, msg)
        assert _untouched(out), kw


# ---- B3 loss backward --------------------------------------------------------------------------------------------
BIG_BWD = 4 * (524288 + 777)                 # past 2048 workgroups x 256 float4 (a record is asked for)
BIG_BWD_NOREC = 4 * (8192 * 256 + 777)       # past 8192 workgroups x 256 float4 (no record)


def _loss_bwd_ref(kind, dt, a, b, c, gout, add, tanh_of_a, g2, G):
    a, b = a.to(dt), b.to(dt)
    d = a - b
    if kind.startswith("l1"):
        d = torch.sign(d)
    coef = torch.tensor(c, dtype=dt) * (gout.to(dt) if gout is not None else 1)
    r = d * coef
    if G is not None:
        r = r + g2.to(dt) * G.to(dt)
    if tanh_of_a:
        r = r * (1 - a * a)
    if add is not None:
        r = r + add.to(dt)
    return r


def _loss_bwd(kind, a, b, denom, scale, gout=None, add=None, tanh_of_a=0, g2=None, G=None, amax0=0.0, n=None, ins=None):
    """`ins`: a list that keeps the input buffers from one launch to the next (they are read-only)."""
    lib = L.lib()
    ins = [] if ins is None else ins
    if not ins:
        ins.extend(fbuf(t) if t is not None else None for t in (a, b, gout, add, g2, G))
    ab, bb, gb, addb, g2b, Gb = ins
    out = obuf(a.numel())
    rec = Buf(dense(1), torch.tensor([amax0])) if amax0 is not None else None
    n = a.numel() if n is None else n
    if kind in ("mse", "l1"):
        rc, msg = _call(getattr(lib, "lvt_%s_bwd" % kind), _p(ab), _p(bb), n, float(denom), scale, _p(gb), _p(addb), tanh_of_a,
                        _p(out), _p(rec))
    else:
        rc, msg = _call(getattr(lib, "lvt_%s_bwd_plus" % kind[:-5]), _p(ab), _p(bb), n, float(denom), scale, _p(gb), _p(g2b), _p(Gb),
                        _p(out), _p(rec))
    return rc, msg, out, rec


def _finite_max(t):
    return float(torch.where(torch.isfinite(t), t.abs(), torch.zeros(())).max())


def _check_loss_bwd(kind, n, with_gout, with_add, tanh_of_a, record=True):
    g = _gen(n, len(kind), with_gout, with_add, tanh_of_a)
    a, b = _rand((n,), g, -0.95, 0.95), _rand((n,), g)
    l1 = kind.startswith("l1")
    if l1 and n >= 8:
        b[1], b[5] = a[1], a[5]                                                 # a == b
        a[2], b[2], a[6], b[6] = 0.0, -0.0, -0.0, 0.0                           # +0 against -0
    gout = torch.tensor([1.7]) if with_gout else None
    add = _rand((n,), g) if with_add else None
    plus = kind.endswith("_plus")
    g2, G = (torch.tensor([-0.6]), _rand((n,), g)) if plus else (None, None)
    denom, scale = 3.0 * n, 0.7 * n                                             # gradients of order 1
    scale = float(torch.tensor(scale, dtype=torch.float32))                   # the entry point takes a float
    c = float(torch.tensor((1.0 if l1 else 2.0) * scale / denom, dtype=torch.float32))
    ins = []
    rc, msg, out, rec = _loss_bwd(kind, a, b, denom, scale, gout, add, tanh_of_a, g2, G, 0.0 if record else None, ins=ins)
    assert rc == 0, msg
    got = out.logical()
    r64, r32 = (_loss_bwd_ref(kind, dt, a, b, c, gout, add, tanh_of_a, g2, G) for dt in (torch.float64, torch.float32))
    rows_ok(got[None], r64[None], r32[None], "%s_bwd" % kind)
    if l1 and n >= 8 and not plus:
        z = torch.tensor([1, 2, 5, 6])
        want = add[z] if with_add else torch.zeros(4)
        assert torch.equal(got[z], want), "l1: a == b does not give an exact 0"
    assert out.outside_untouched()
    if record:
        assert float(rec.logical()) == float(got.abs().max()) and rec.outside_untouched(), "the record is not max |out|"
    rc, msg, out2, rec2 = _loss_bwd(kind, a, b, denom, scale, gout, add, tanh_of_a, g2, G, 0.0 if record else None, ins=ins)
    assert rc == 0 and torch.equal(out.bits(), out2.bits()), "a second launch gave other bits"
    if record and n <= 1028:
        # a larger value already in the slot survives
        rc, msg, _, rec3 = _loss_bwd(kind, a, b, denom, scale, gout, add, tanh_of_a, g2, G, 1.0e30, ins=ins)
        assert rc == 0 and float(rec3.logical()) == float(torch.tensor(1.0e30))


@pytest.mark.parametrize("n", [4, 1028, BIG_BWD])
@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_loss_bwd(kind, n):
    """lvt_mse_bwd_kernel<L1, 0>: gout null / given x add null / given x tanh_of_a 0 / 1; one float4, 257 float4 (two
    workgroups, one thread in the second) and 524288 + 777 float4: past the 2048-workgroup grid of a launch with a record."""
    for with_gout in (False, True):
        for with_add in (False, True):
            for tanh_of_a in (0, 1):
                _check_loss_bwd(kind, n, with_gout, with_add, tanh_of_a)


@pytest.mark.parametrize("n", [4, 1028, BIG_BWD])
@pytest.mark.parametrize("kind", ["mse_plus", "l1_plus"])
def test_loss_bwd_plus(kind, n):
    """lvt_mse_bwd_kernel<L1, 1> (lvt_mse_bwd_plus / lvt_l1_bwd_plus): gout null / given, the second term g2[0] G; sizes as
    test_loss_bwd."""
    for with_gout in (False, True):
        _check_loss_bwd(kind, n, with_gout, False, 0)


def test_loss_bwd_past_the_uncapped_grid():
    """lvt_mse_bwd_kernel<0, 0> with out_amax = NULL and 8192 x 256 + 777 float4: the second trip of the 8192-workgroup grid."""
    _check_loss_bwd("mse", BIG_BWD_NOREC, True, True, 1, record=False)


def _act_bwd(kind, gv, y, amax0=0.0):
    gb, yb, out = fbuf(gv), fbuf(y), obuf(gv.numel())
    rec = Buf(dense(1), torch.tensor([amax0])) if amax0 is not None else None
    rc, msg = _call(getattr(L.lib(), "lvt_%s_bwd" % kind), _p(gb), _p(yb), gv.numel(), _p(out), _p(rec))
    return rc, msg, out, rec


def _act_ref(kind, dt, gv, y):
    gv, y = gv.to(dt), y.to(dt)
    return gv * (1 - y * y) if kind == "tanh" else gv * (y * (1 - y))


@pytest.mark.parametrize("n", [4, 1028, BIG_BWD])
@pytest.mark.parametrize("kind", ["tanh", "sigmoid"])
def test_activation_bwd(kind, n):
    """lvt_tanh_bwd_kernel / lvt_sigmoid_bwd_kernel from the saved output y; sizes as test_loss_bwd (BIG_BWD: second trip of the
    2048-workgroup grid), and once without a record."""
    g = _gen(n, len(kind), 4)
    gv = _rand((n,), g)
    y = _rand((n,), g, -0.99, 0.99) if kind == "tanh" else _rand((n,), g, 0.01, 0.99)
    for amax0 in (0.0, None):
        rc, msg, out, rec = _act_bwd(kind, gv, y, amax0)
        assert rc == 0, msg
        got = out.logical()
        rows_ok(got[None], _act_ref(kind, torch.float64, gv, y)[None], _act_ref(kind, torch.float32, gv, y)[None], kind + "_bwd")
        assert out.outside_untouched()
        if rec is not None:
            assert float(rec.logical()) == float(got.abs().max()) and rec.outside_untouched(), "the record is not max |out|"
        rc, msg, out2, _ = _act_bwd(kind, gv, y, amax0)
        assert rc == 0 and torch.equal(out.bits(), out2.bits()), "a second launch gave other bits"
    rc, msg, _, rec3 = _act_bwd(kind, gv, y, 1.0e30)
    assert rc == 0 and float(rec3.logical()) == float(torch.tensor(1.0e30)), "a larger record did not survive"


def test_record_is_the_max_over_finite_outputs():
    """out_amax (lvt_absf): an inf or NaN element of `out` does not raise the slot, which equals the max over the finite
    elements bit for bit -- every kernel that reports one."""
    n = 1028
    g = _gen(n, 55)
    a, b, x = _rand((n,), g, -0.95, 0.95), _rand((n,), g), _rand((n,), g)
    x[3], x[700], x[1027] = INF, -INF, NAN
    runs = []
    for kind in ("mse", "l1"):
        rc, msg, out, rec = _loss_bwd(kind, a, b, 3.0, 0.7, None, x, 0)
        runs.append((kind, rc, out, rec))
        rc, msg, out, rec = _loss_bwd(kind + "_plus", a, b, 3.0, 0.7, None, None, 0, torch.tensor([0.5]), x)
        runs.append((kind + "_plus", rc, out, rec))
    for kind in ("tanh", "sigmoid"):
        rc, msg, out, rec = _act_bwd(kind, x, a * 0.5 + 0.5)
        runs.append((kind, rc, out, rec))
    for kind, rc, out, rec in runs:
        got = out.logical()
        assert rc == 0 and int((~torch.isfinite(got)).sum()) == 3, kind
        assert float(rec.logical()) == _finite_max(got) and _finite_max(got) > 0, kind


def test_loss_bwd_refusals():
    a = torch.ones(8)
    for kind in ("mse", "l1", "mse_plus", "l1_plus"):
        extra = dict(g2=torch.ones(1), G=a) if kind.endswith("_plus") else {}
        for kw in (dict(n=6), dict(denom=0.0)):
            rc, msg, out, rec = _loss_bwd(kind, a, a, kw.get("denom", 8.0), 0.7, n=kw.get("n"), **extra)
            assert rc == -1 and "_bwd" in msg, (kind, kw, rc, msg)
            assert _untouched(out) and float(rec.logical()) == 0.0, (kind, kw)


# ---- B4 lvt_colsum ---------------------------------------------------------------------------------------------------
def _colsum(x, ld, ws_bytes=None, N=None):
    lib = L.lib()
    M, n_ = x.shape
    N = n_ if N is None else N
    xb, out = Buf(rows_idx(M, n_, ld), x), obuf(n_)
    full = lib.lvt_colsum_workspace_bytes(M, N)
    ws = torch.empty(max(full, 16), dtype=torch.uint8, device=DEV)
    nws = full if ws_bytes is None else ws_bytes
    rc, msg = _call(lib.lvt_colsum, _p(xb), M, N, ld, _p(out), L.ptr(ws) if nws else C.c_void_p(0), nws)
    return rc, msg, out


@pytest.mark.parametrize("N", [4, 12, 260, 1024, 1028])
def test_colsum(N):
    """lvt_colsum_kernel: N / 4 float4 columns against 256 threads -- 1 column x 256 row lanes (N 4), 3 x 85 with an idle thread
    (12), 65 x 3 with 61 idle (260), 256 x 1 (1024), and 257 columns: a second column pass with one busy thread (1028).  M 1
    (one stage, most row lanes empty), 64 (one full stage), 65 and 4097 (two and three 64-row stages with a ragged last
    workgroup), 131072 (N 4: the 128-row stage, then 64-row stages).  ld = N and N + 8 with payload padding."""
    for M in (1, 64, 65, 4097) + ((131072,) if N == 4 else ()):
        g = _gen(N, M)
        x = _rand((M, N), g)
        ref64, ref32, terms = x.double().sum(0), x.sum(0), x.double().abs().sum(0)
        for ld in (N, N + 8):
            rc, msg, out = _colsum(x, ld)
            assert rc == 0, msg
            sum_ok(out.logical(), ref64, ref32, terms, "colsum M %d ld %d" % (M, ld))
            assert out.outside_untouched()
            rc, msg, out2 = _colsum(x, ld)
            assert rc == 0 and torch.equal(out.bits(), out2.bits()), "a second launch gave other bits"


def test_colsum_refusals():
    x = torch.ones(70, 8)
    full = L.lib().lvt_colsum_workspace_bytes(70, 8)
    for kw, want in ((dict(N=6), -1), (dict(ld=10), -1), (dict(ws_bytes=full - 1), -2), (dict(ws_bytes=0), -2)):
        rc, msg, out = _colsum(x, kw.get("ld", 8), kw.get("ws_bytes"), kw.get("N"))
        assert rc == want and "colsum" in msg, (kw, rc, msg)
        assert _untouched(out), kw
