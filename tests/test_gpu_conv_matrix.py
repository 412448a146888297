"""Conformance matrix of the convolution entry points of lvt_amd/csrc/gemm_engine.hip -- lvt_conv3d_fwd, lvt_conv3d_bwd_data,
lvt_conv3d_bwd_weight (with db) -- against the fp64 reference of tests/util_conv.py, off the 64x64 workload's grid.

Routes the cells (util_conv.CELLS) target:
  * forward: ALoader<A_CONV_K> on the 128x128 tile (Co > 32) and the 128x32 tile (Co <= 32); the 1x1 shortcut to the wide kernel
    (f16x2 && Ci % 32 == 0 && M > 128); the thin image-side kernel (f16x2, 4 -> 128, k4 s2 p1, Wo % 32 == 0);
  * data gradient: ALoader<A_CONVT_K> + BLoader<B_CONVT_W>, one grid plane per stride class, the phase decode of the epilogues, on
    the 128x128 (Ci > 32) and 128x32 tiles; the 1x1 shortcut (f16x2 && Co % 32 == 0 && M > 128);
  * weight gradient: ALoader<A_CONV_M> on the 64x128 (taps Ci <= 64) and 128x128 tiles, bwd_weight_splits (>= 2 ranges of a
    multiple of 32 positions: with fewer than 32 positions the second range is empty), the column sums of dy, and the two unpack
    kernels (tiled: Co % 64 == 0, no channel padding, the tile within 64 KB of LDS; generic: everything else);
  * none of the cells is served by a frame-resident kernel: the near misses assert that through the four predicates.

Per cell and pass: every element within |got - ref64| <= 1e-5 mag + 2^-21 (|bias| + |res| + |ref64|) (EPS_ACC / EPS_EPI of
tests/test_gpu_gemm_matrix.py; mag = sum |x||w|, sum |dy||w|, sum |x||dy|), db within 1e-5 sum |dy|; masked elements exactly 0,
ReLU outputs >= 0, pad channels of y / dx exactly 0 (sigmoid: through LVT_EPI_PAD); operands, outputs and the weight-gradient
workspace live in NaN-payload buffers (tests/util_guard.py), so a read of padding or of a partial row nobody wrote arrives as a NaN,
an element never written keeps its payload bits and a write outside the logical output changes them; in f16x2 the record of
max |y| equals torch's; a second launch into fresh buffers gives equal bits.  Each check prints its worst error / bound ratio
("RATIO pass mode cell value")."""
import copy
import ctypes as C

import pytest
import torch

import util_conv as U
from lvt_amd.hip import binding as L, gemm as G
from util_guard import PAD, PAYLOAD, Buf, dense, fbuf, obuf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_, R_, U_, M_ = L.EPI_BIAS, L.EPI_RESIDUAL, L.EPI_RELU, L.EPI_MASK
T_, S_, LK_, LKM_ = L.EPI_TANH, L.EPI_SIGMOID, L.EPI_LEAKY, L.EPI_LEAKY_MASK
assert (B_, R_, U_, T_, M_, S_, LK_, LKM_) == (U.EPI_BIAS, U.EPI_RESIDUAL, U.EPI_RELU, U.EPI_TANH, U.EPI_MASK, U.EPI_SIGMOID,
                                                U.EPI_LEAKY, U.EPI_LEAKY_MASK)


@pytest.fixture(params=["bf16x3", "f16x2", "f32"])
def mode(request):
    # the operand records cover the logical region only, while LVT_AMAX_CHECK would scan the whole NaN-padded view: off here
    before, check = L.get_math_mode(), L.AMAX_CHECK
    L.set_math_mode(request.param)
    L.AMAX_CHECK = False
    yield request.param
    L.AMAX_CHECK = check
    L.set_math_mode(before)


# ---- reference (computed once per cell, shared, never modified) ----------------------------------------------------------
_REF = {}


def _ref(c):
    key = (c.name, c.ci_real, c.co_real)
    if key not in _REF:
        x, w, dy = U.operands(c)
        _REF[key] = (x, w, dy, U.bounds(c, x, w, dy))
    return _REF[key]


def _geom(c):
    return G.conv_geom(c.N, c.ins[0], c.ins[1], c.ins[2], c.ci, c.co, c.kernel, c.stride, c.pad, out=c.out)


def _record(view, logical):
    """f16x2: attach to the operand the max |.| of its LOGICAL region -- the kernel must never read the padding."""
    if L.f16x2():
        L.set_amax(view, L.amax_slot(view.device).fill_(float(logical.abs().max())))


def _opbuf(t):
    b = fbuf(t)
    _record(b.view, t)
    return b


def _pad_noise(shape, seed):
    """Random non-zero values for the pad channels of dy (the engine may read them: the packed weight's pad rows are 0)."""
    g = torch.Generator().manual_seed(seed)
    return U.rand(shape, g, 0.25, 1.0)


def _packed(c, g, w):
    """lvt_conv3d_pack_weight into a guard buffer: [taps][Ci][Co], zero padded, every element written, nothing else."""
    taps = c.kernel[0] * c.kernel[1] * c.kernel[2]
    wb = fbuf(w)
    wp = obuf(taps, c.ci, c.co)
    L.check(L.lib().lvt_conv3d_pack_weight(C.byref(g), L.ptr(wb.view), c.ci_real, c.co_real, L.ptr(wp.view), L.stream_ptr()),
            "lvt_conv3d_pack_weight")
    torch.cuda.synchronize()
    want = torch.zeros(taps, c.ci, c.co)
    want[:, :c.ci_real, :c.co_real] = w.reshape(c.co_real, c.ci_real, taps).permute(2, 1, 0)
    assert torch.equal(wp.logical(), want) and wp.outside_untouched(), "lvt_conv3d_pack_weight"
    _record(wp.view, w)
    return wp


class Operands:
    """The device operands of one cell, built once per test and shared by its launches."""

    def __init__(self, c):
        self.c, self.g = c, _geom(c)
        self.x, self.w, self.dy, self.b = _ref(c)
        self.xb = _opbuf(U.to_cl(self.x, c.ci))                                                       # zero pad channels
        self.dyb = _opbuf(U.to_cl(self.dy, c.co, fill=_pad_noise((c.N,) + c.out + (c.co,), 11)))      # noise in the pads
        self.wp = _packed(c, self.g, self.w)


def _epi_operands(shape, creal, seed):
    """bias (C), res and mask (shape) for an output of channels-last `shape`; bias and res are 0 in the pad channels."""
    g = torch.Generator().manual_seed(seed)
    bias, res = U.rand(shape[-1:], g), U.rand(shape, g)
    bias[creal:] = 0.0
    res[..., creal:] = 0.0
    mask = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, shape, generator=g)]
    return bias, res, mask


def _ratio(err, tol):
    """max err / tol over the elements with a positive bound; the others must be exact."""
    pos = tol > 0
    assert bool((err[~pos] == 0).all()), "an element with a zero bound is not exact"
    return float((err[pos] / tol[pos]).max()) if bool(pos.any()) else 0.0


def _report(what, c, ratio):
    print("RATIO %s %s %s %.4f" % (what, L.get_math_mode(), c.name, ratio))


def _complete(buf, what):
    got = buf.logical()
    assert not bool((got.view(torch.int32) == PAYLOAD).any()), "%s: an element of the output was never written" % what
    assert not bool(torch.isnan(got).any()), "%s: NaN in the output (padding or an unwritten partial was read)" % what
    assert buf.outside_untouched(), "%s: a float outside the logical output was written" % what
    return got


def _launch_epi(o, data, flags, epi):
    """One lvt_conv3d_fwd (data = False) / lvt_conv3d_bwd_data (True) launch into a fresh guard buffer."""
    c, g = o.c, o.g
    shape = ((c.N,) + c.ins + (c.ci,)) if data else ((c.N,) + c.out + (c.co,))
    bias, res, mask = epi
    bb = Buf(torch.arange(shape[-1]), bias) if flags & B_ else None
    rb = fbuf(res) if flags & R_ else None
    mb = fbuf(mask) if flags & M_ else None
    out = obuf(*shape)
    src = o.dyb if data else o.xb
    io = L.amax_io(src.view, o.wp.view, out.view)
    fn = L.lib().lvt_conv3d_bwd_data if data else L.lib().lvt_conv3d_fwd
    L.check(fn(C.byref(g), L.ptr(src.view), L.ptr(o.wp.view), L.ptr(bb.view if bb else None), L.ptr(rb.view if rb else None),
               L.ptr(mb.view if mb else None), L.ptr(out.view), flags | L.math_flag(), L.io_ref(io), L.stream_ptr()),
            "lvt_conv3d_bwd_data" if data else "lvt_conv3d_fwd")
    torch.cuda.synchronize()
    return out


def _check_epi(o, data, flags, seed=0):
    """Launch, judge against fp64, launch again: equal bits."""
    c = o.c
    creal, cpad = (c.ci_real, c.ci) if data else (c.co_real, c.co)
    what = "bwd_data" if data else "fwd"
    if flags & S_:
        flags |= L.epi_pad(cpad - creal)
    acc = U.to_cl(o.b["dx" if data else "y"], cpad)
    mag = U.to_cl(o.b["mag_dx" if data else "mag_y"], cpad)
    epi = _epi_operands(tuple(acc.shape), creal, 100 + seed + flags % 4096)
    bias, res, mask = (t.double() for t in epi)
    ref = U.epilogue64(acc, flags, bias, res, mask, npad=cpad - creal)
    tol = U.tol(mag, ref, bias.expand_as(ref) if flags & B_ else None, res if flags & R_ else None)
    out = _launch_epi(o, data, flags, epi)
    got = _complete(out, what).double()
    err = (got - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), "%s: %d elements out of bound (first %s: got %r, ref %r, tol %r)" % (
        what, int(bad.sum()), tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(ref[bad][0]), float(tol[bad][0]))
    _report(what, c, _ratio(err, tol))
    if flags & M_ and not flags & LKM_:
        assert bool((got[epi[2] <= 0] == 0).all()), "%s MASK: masked elements are not exactly 0" % what
    if flags & U_:
        assert bool((got >= 0).all()), "%s RELU: negative value" % what
    assert bool((got[..., creal:] == 0).all()), "%s: a pad channel is not exactly 0" % what
    if L.f16x2():
        assert float(L.amax_of(out.view)) == float(got.abs().max()), "%s: record of max |.|" % what
    again = _launch_epi(o, data, flags, epi)
    assert torch.equal(out.bits(), again.bits()), "%s: a second launch gave other bits" % what


def _launch_wgrad(o, short=0):
    """One lvt_conv3d_bwd_weight launch (with db) into fresh guard buffers, the workspace all payload."""
    c, g = o.c, o.g
    lib = L.lib()
    nws = lib.lvt_conv3d_bwd_weight_workspace_bytes(C.byref(g))
    assert nws % 4 == 0 and nws > 0
    ws = Buf(dense(nws // 4))
    dw, db = obuf(c.co_real, c.ci_real, *c.kernel), obuf(c.co_real)
    io = L.amax_io(o.xb.view, o.dyb.view)
    rc = lib.lvt_conv3d_bwd_weight(C.byref(g), L.ptr(o.xb.view), L.ptr(o.dyb.view), L.ptr(dw.view), L.ptr(db.view), c.ci_real,
                                   c.co_real, L.math_flag(), L.io_ref(io), L.ptr(ws.view), nws - short, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dw, db, ws


def _check_wgrad(o):
    c = o.c
    rc, dw, db, ws = _launch_wgrad(o)
    L.check(rc, "lvt_conv3d_bwd_weight")
    assert ws.outside_untouched(), "bwd_weight: a float outside the workspace was written"
    got = _complete(dw, "bwd_weight dw").double()
    err, tol = (got - o.b["dw"]).abs(), U.tol(o.b["mag_dw"], o.b["dw"])
    bad = ~(err <= tol)
    assert not bool(bad.any()), "dw: %d elements out of bound (first %s: got %r, ref %r, tol %r)" % (
        int(bad.sum()), tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(o.b["dw"][bad][0]), float(tol[bad][0]))
    _report("bwd_weight", c, _ratio(err, tol))
    gdb = _complete(db, "bwd_weight db").double()
    err, tol = (gdb - o.b["db"]).abs(), U.EPS_ACC * o.b["mag_db"]
    assert bool((err <= tol).all()), "db: worst error / bound %r" % float((err / tol).max())
    _report("bwd_weight_db", c, _ratio(err, tol))
    rc, dw2, db2, _ = _launch_wgrad(o)
    L.check(rc, "lvt_conv3d_bwd_weight")
    assert torch.equal(dw.bits(), dw2.bits()) and torch.equal(db.bits(), db2.bits()), "bwd_weight: a second launch gave other bits"


# ---- the matrix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", U.CELLS, ids=repr)
def test_cell(mode, c):
    """The three passes of one cell; forward and data gradient with BIAS | RESIDUAL."""
    o = Operands(c)
    _check_epi(o, False, B_ | R_)
    _check_epi(o, True, B_ | R_)
    _check_wgrad(o)


@pytest.mark.parametrize("c", [c for c in U.CELLS if c.near_miss], ids=repr)
def test_near_miss_is_served_by_no_frame_resident_kernel(mode, c):
    g, lib = _geom(c), L.lib()
    assert lib.lvt_conv3d_uses_patch_kernel(C.byref(g), L.math_flag()) == 0
    if c.stride == (1, 1, 1):                                    # (the data gradient as a forward convolution: convnet's route)
        assert not G.bwd_data_as_conv(g)
    assert lib.lvt_conv3d_fwd_uses_parity_kernel(C.byref(g), L.math_flag()) == 0
    assert lib.lvt_conv3d_bwd_data_uses_phase_kernel(C.byref(g), L.math_flag()) == 0
    assert lib.lvt_conv3d_bwd_weight_fuses_bias(C.byref(g), L.math_flag() | L.WGRAD_DB_OF_X) == 0


def _flags4(s):
    return (B_ if s & 1 else 0) | (R_ if s & 2 else 0) | (U_ if s & 4 else 0) | (M_ if s & 8 else 0)


@pytest.mark.parametrize("s", range(16))
def test_epilogue_subsets(mode, s):
    """All 16 subsets of {BIAS, RESIDUAL, RELU, MASK}: forward on the 7x5 34 -> 33 cell, data gradient on the strided 10x6 12 -> 128
    cell (the phase decode of both epilogues and of the two-phase MASK form).  Those two run the 128x128 forward tile (the fast
    epilogue of epilogue_fast.h) and the 128x32 data-gradient tile; the other two tiles -- the forward with Co <= 32, whose MASK
    forms take lvt_epilogue_vec, and the data gradient with Ci > 32 -- run the subsets on the 6x10 12 -> 32 and the strided
    128 -> 12 cell.  The image-side 6x64 cell runs them through the four <RES, MASK> forms of the thin kernel in f16x2 (3 output
    rows: 6 tiles of 32 positions over two workgroups of four waves, two waves of the second idle)."""
    _check_epi(Operands(U.CELL["r7x5_34to33"]), False, _flags4(s), seed=s)
    _check_epi(Operands(U.CELL["s10x6_12to128_p1"]), True, _flags4(s), seed=s)
    _check_epi(Operands(U.CELL["r6x10_k5_12to32"]), False, _flags4(s), seed=s)
    _check_epi(Operands(U.CELL["s10x6_128to12_p1"]), True, _flags4(s), seed=s)
    _check_epi(Operands(U.CELL["i6x64_3to128"]), False, _flags4(s), seed=s)


ACTS = [("leaky_bias", LK_ | B_, 0), ("leaky_mask", M_ | LKM_, 0), ("leaky_leaky_mask", LK_ | M_ | LKM_, 0), ("tanh_bias", T_ | B_, 0),
        ("sigmoid_pad1", S_, 1), ("sigmoid_pad3", S_, 3)]


@pytest.mark.parametrize("name", ["r6x10_k5_12to32", "r7x5_34to33"])
@pytest.mark.parametrize("data", [False, True], ids=["fwd", "bwd_data"])
@pytest.mark.parametrize("act", ACTS, ids=[a[0] for a in ACTS])
def test_epilogue_activations(mode, act, data, name):
    """LEAKY, LEAKY_MASK, TANH and SIGMOID (1 and 3 pad channels, stored as 0) on a cell of the 128x32 tile (12 -> 32) and one of
    the 128x128 tile (36 -> 36), forward and data gradient."""
    c = U.CELL[name]
    _, flags, npad = act
    if npad:
        c = c.with_real(ci_real=c.ci - npad) if data else c.with_real(co_real=c.co - npad)
    _check_epi(Operands(c), data, flags)


# ---- refusals: host-side, nothing is written, lvt_last_error is set --------------------------------------------------------------
def _refused(rc, outs, text):
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.lib().lvt_last_error().decode()
    assert text in msg, msg
    for b in outs:
        assert bool((b.bits() == PAYLOAD).all()), "a refused call wrote something"


def _bare(c):
    """Payload-only buffers of the cell's shapes (a refused call reads and writes nothing)."""
    taps = c.kernel[0] * c.kernel[1] * c.kernel[2]
    return (obuf(c.N, *c.ins, c.ci), obuf(c.N, *c.out, c.co), obuf(taps, c.ci, c.co))


def _io():
    if not L.f16x2():
        return None
    io = L.AmaxIO()
    io.a = io.b = L.amax_slot(torch.device(DEV)).fill_(1.0).data_ptr()
    return io


@pytest.mark.parametrize("name,nthw,text", [("k3_s2", (1, 1, 8, 8), "kernel extents must be multiples of the strides"),
                                            ("h7_s2", (1, 1, 7, 8), "input extents must be multiples of the strides")])
def test_bwd_data_refuses(mode, name, nthw, text):
    k = (1, 3, 3) if name == "k3_s2" else (1, 4, 4)
    c = U.ConvCell(name, nthw, 12, 12, k, (1, 2, 2), (0, 1, 1))
    assert not c.bwd_data_ok
    dx, dy, wp = _bare(c)
    io = _io()
    rc = L.lib().lvt_conv3d_bwd_data(C.byref(_geom(c)), L.ptr(dy.view), L.ptr(wp.view), None, None, None, L.ptr(dx.view),
                                     L.math_flag(), L.io_ref(io), L.stream_ptr())
    _refused(rc, (dx, dy, wp), text)


def test_channel_count_not_a_multiple_of_4_is_refused(mode):
    c = U.ConvCell("ci6", (1, 1, 4, 4), 8, 12, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    x, y, wp = _bare(c)
    g = _geom(c)
    g.Ci = 6
    lib, io = L.lib(), _io()
    _refused(lib.lvt_conv3d_fwd(C.byref(g), L.ptr(x.view), L.ptr(wp.view), None, None, None, L.ptr(y.view), L.math_flag(),
                                L.io_ref(io), L.stream_ptr()), (x, y, wp), "must be multiples of 4")
    _refused(lib.lvt_conv3d_bwd_data(C.byref(g), L.ptr(y.view), L.ptr(wp.view), None, None, None, L.ptr(x.view), L.math_flag(),
                                     L.io_ref(io), L.stream_ptr()), (x, y, wp), "must be multiples of 4")
    ws, dw = obuf(1 << 16), obuf(12, 6, 1, 3, 3)
    _refused(lib.lvt_conv3d_bwd_weight(C.byref(g), L.ptr(x.view), L.ptr(y.view), L.ptr(dw.view), None, 6, 12, L.math_flag(),
                                       L.io_ref(io), L.ptr(ws.view), 4 << 16, L.stream_ptr()), (x, y, dw, ws), "must be multiples of 4")
    _refused(lib.lvt_conv3d_pack_weight(C.byref(g), L.ptr(dw.view), 6, 12, L.ptr(wp.view), L.stream_ptr()), (dw, wp),
             "must be multiples of 4")


def test_pack_weight_t_refuses_a_strided_geometry(mode):
    c = U.CELL["s10x6_12to28_p1"]
    w, wt = obuf(c.co, c.ci, *c.kernel), obuf(16, c.co, c.ci)
    _refused(L.lib().lvt_conv3d_pack_weight_t(C.byref(_geom(c)), L.ptr(w.view), c.ci, c.co, L.ptr(wt.view), L.stream_ptr()),
             (w, wt), "stride-1 convolutions only")
    with pytest.raises(L.LvtError, match="stride-1"):
        G.PackBatch().t(_geom(c), w.view, c.ci, c.co)


def test_workspace_one_byte_short_is_refused(mode):
    o = Operands(U.CELL["r1x1_12to28"])
    rc, dw, db, ws = _launch_wgrad(o, short=1)
    _refused(rc, (dw, db, ws), "workspace")


# ---- whole stacks on frames that are not 64x64 -----------------------------------------------------------------------------------
TOL = 2e-5            # one engine launch against its output's max (tests/test_gpu_engine.py)


def _nchw(y, c):
    return y.reshape(y.shape[0], y.shape[-3], y.shape[-2], y.shape[-1])[..., :c].permute(0, 3, 1, 2).cpu()


def _twin_forward(seq, plan, outs, h):
    """fp64 forward through a deep copy of a stack's `layers`, layer by layer of its plan (tests/test_gpu_resshuffle.py and
    tests/test_gpu_convcoders.py: _twin_forward).  Every ReLU / LeakyReLU takes each element's branch from the sign of the GPU's
    own activation (outs[i], stored post-activation) instead of the sign of the fp64 value: the derivative jumps at 0, and an
    element within the engine's error of 0 is a valid reference for its own branch only.  The disagreements are checked to be
    exactly that: fp64 values within TOL of the layer's max of 0.  The activation is applied where the plan stores it, so the
    explicit activation modules behind a layer are already done when the walk reaches them.
    -> (output, number of elements that took the GPU's branch against fp64's)."""
    from torch import nn
    state = {"i": -1, "flips": 0}

    def act(h):
        ly = plan[state["i"]]
        if ly.act in ("relu", "leaky"):
            pos = _nchw(outs[state["i"]], ly.cout) > 0
            differ = pos != (h.detach() > 0)
            assert float(h.detach().abs()[differ].max() if differ.any() else 0.0) <= TOL * float(h.detach().abs().max())
            state["flips"] += int(differ.sum())
            return h * (pos.double() if ly.act == "relu" else torch.where(pos, 1.0, U.LEAKY_SLOPE).double())
        return {"": lambda t: t, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[ly.act](h)

    def conv(m, h):
        state["i"] += 1
        ly = plan[state["i"]]
        assert ly.kind == ("convT" if isinstance(m, nn.ConvTranspose2d) else "conv") and ly.norm == ""
        return m(h)

    for m in seq:
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            h = act(conv(m, h))
        elif isinstance(m, (nn.AvgPool2d, nn.Upsample)):
            state["i"] += 1
            assert plan[state["i"]].kind == ("pool" if isinstance(m, nn.AvgPool2d) else "up") and plan[state["i"]].act == ""
            h = m(h)
        elif type(m).__name__ == "ResBlock":
            t = act(conv(m.block[1], h))
            t = conv(m.block[3], t)
            assert plan[state["i"]].res_from >= 0
            h = act(h + t)
        else:
            assert isinstance(m, (nn.ReLU, nn.LeakyReLU, nn.Tanh, nn.Sigmoid))
    assert state["i"] == len(plan) - 1
    return h, state["flips"]


def _gpu_pass(mod, x, gy=None):
    """Forward (and, with gy, backward) of the module on the device, and the activations of that pass again, layer by layer (the
    kernels are deterministic).  -> (y, input gradient or None, outs)."""
    from lvt_amd.hip import convnet
    from lvt_amd.modeling import convstack
    xd = x.to(DEV).requires_grad_(gy is not None)
    y = mod(xd)
    if gy is not None:
        (y * gy.to(DEV)).sum().backward()
    with torch.no_grad():
        outs, _ = convnet.stack_forward(mod._plan, convstack.nchw_to_cl(x.to(DEV)), convstack.plan_params(mod._owners))
    return y.detach(), xd.grad, outs


def _twin(mod):
    twin = copy.deepcopy(mod.layers).cpu().double()
    for p in twin.parameters():
        p.grad = None
    return twin


def _stack_against_fp64(mod, x_shape, launches, seed):
    """Output, input gradient and every parameter gradient of `mod` within launches x 2e-5 of their own max."""
    from conftest import rel_err
    n_conv = sum(ly.kind in ("conv", "convT") for ly in mod._plan)
    assert launches == 3 * n_conv                  # forward, weight-gradient and data-gradient launch of every convolution
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*x_shape, generator=g)
    y, gx, outs = _gpu_pass(mod, x, None)
    gy = torch.randn(*y.shape, generator=g)
    for p in mod.parameters():
        p.grad = None
    y, gx, outs = _gpu_pass(mod, x, gy)
    twin = _twin(mod)
    x64 = x.double().requires_grad_(True)
    y64, flips = _twin_forward(twin, mod._plan, outs, x64)
    print("elements on the GPU's side of an activation kink against fp64's: %d" % flips)
    assert flips <= 5
    assert y.shape == y64.shape
    (y64 * gy.double()).sum().backward()
    err = rel_err(y, y64.detach())
    print("output %.2e" % err)
    assert err < launches * TOL
    err = rel_err(gx, x64.grad)
    print("input gradient %.2e" % err)
    assert err < launches * TOL
    n = 0
    for (k, p), (k2, q) in zip(mod.layers.named_parameters(), twin.named_parameters()):
        assert k == k2 and p.grad is not None
        err = rel_err(p.grad, q.grad)
        print("%-22s %.2e" % (k, err))
        assert err < launches * TOL, k
        n += 1
    assert n == 2 * n_conv


def _res_encoder():
    from lvt_amd.modeling.encoder import ResEncoder
    return ResEncoder(3, 64, 32, "", False, 1, "", 4).to(DEV)


def _res_decoder():
    from lvt_amd.modeling.generator import ResDecoder
    return ResDecoder(64, 64, 32, 3, "", False, 1, "tanh", 4).to(DEV)


@pytest.mark.parametrize("frames", [(2, 24, 40), (1, 64, 32)], ids=["2x24x40", "1x64x32"])
def test_res_encoder_off_the_grid_against_fp64(mode, frames):
    """ResEncoder(3, 64, 32, "", False, 1, "", 4) on 2 frames of 24 x 40 (latents 6 x 10: nothing lands on a frame-resident or thin
    kernel) and on 1 frame of 64 x 32 (32 x 16 and 16 x 8 inside: near misses of the 32 x 32 / 16 x 16 kernels), against its
    deep-copied `layers` in fp64.  The plan is conv4x4s2, conv4x4s2, conv3x3, ResBlock (conv3x3, conv1x1): 5 forward, 5
    weight-gradient and 5 data-gradient engine launches (the frame's gradient is asked for), L = 15; output and every gradient
    within L x 2e-5 of its own max."""
    torch.manual_seed(41)
    enc = _res_encoder()
    assert [ly.kind for ly in enc._plan] == ["conv"] * 5
    n, h, w = frames
    _stack_against_fp64(enc, (n, 3, h, w), 15, 411)


@pytest.mark.parametrize("frames", [(2, 6, 10), (1, 16, 8)], ids=["2x24x40", "1x64x32"])
def test_res_decoder_off_the_grid_against_fp64(mode, frames):
    """ResDecoder(64, 64, 32, 3, "", False, 1, "tanh", 4) on the latents of the same frames (6 x 10 and 16 x 8).  The plan is
    conv3x3, ResBlock (conv3x3, conv1x1), convT4x4s2, convT4x4s2 (tanh): 5 forward, 5 weight-gradient and 5 data-gradient
    launches (the latent's gradient is asked for), L = 15."""
    torch.manual_seed(43)
    dec = _res_decoder()
    assert [ly.kind for ly in dec._plan] == ["conv", "conv", "conv", "convT", "convT"]
    n, h, w = frames
    _stack_against_fp64(dec, (n, 64, h, w), 15, 431)


def test_conv_encoder_off_the_grid_against_fp64(mode):
    """ConvEncoder at the smallest width of the configurations (NF 16, N_LAYERS 1, 256 output channels) on 2 frames of 24 x 40:
    conv3x3 x 3, pool, conv3x3 x 2 with LeakyReLU between them -- 5 convolutions, L = 15 (the pool moves fp32 values at 1e-7)."""
    from lvt_amd.modeling.encoder import ConvEncoder
    torch.manual_seed(45)
    enc = ConvEncoder(3, 16, 256, "", False, 1, "").to(DEV)
    assert [ly.kind for ly in enc._plan] == ["conv", "conv", "conv", "pool", "conv", "conv"]
    _stack_against_fp64(enc, (2, 3, 24, 40), 15, 451)


def test_conv_decoder_off_the_grid_against_fp64(mode):
    """ConvDecoder (NF 16, N_LAYERS 1, 256 input channels, tanh) on 2 latent frames of 12 x 20 -> 24 x 40: conv3x3 x 2, upsample,
    conv3x3 x 2 -- 4 convolutions, L = 12."""
    from lvt_amd.modeling.generator import ConvDecoder
    torch.manual_seed(47)
    dec = ConvDecoder(256, 16, 3, "", False, 1, "tanh").to(DEV)
    assert [ly.kind for ly in dec._plan] == ["conv", "conv", "up", "conv", "conv"]
    _stack_against_fp64(dec, (2, 256, 12, 20), 12, 471)


def test_res_encoder_30x30_forward_matches_and_backward_is_refused(mode):
    """A 30 x 30 frame: 15 x 15 behind the first stride-2 convolution, 7 x 7 behind the second.  The forward matches fp64 (5
    launches); the backward reaches the data gradient of the second convolution, whose input extent 15 is no multiple of its
    stride: lvt_conv3d_bwd_data refuses and the LvtError comes out of backward() instead of numbers."""
    from conftest import rel_err
    torch.manual_seed(49)
    enc = _res_encoder()
    g = torch.Generator().manual_seed(491)
    x = torch.randn(1, 3, 30, 30, generator=g)
    y, _, outs = _gpu_pass(enc, x)
    assert y.shape == (1, 64, 7, 7)
    y64, flips = _twin_forward(_twin(enc), enc._plan, outs, x.double())
    assert flips <= 5
    err = rel_err(y, y64.detach())
    print("output %.2e" % err)
    assert err < 5 * TOL
    xd = x.to(DEV).requires_grad_(True)
    loss = enc(xd).sum()
    with pytest.raises(L.LvtError, match="input extents must be multiples of the strides"):
        loss.backward()
    assert xd.grad is None
