"""Residual dropout of the video transformer on the GPU (csrc/dropout.hip, MODEL.AUTOREGRESSIVE.VT.DROPOUT):

  * lvt_dropout_add / lvt_dropout_bwd against the float32 numpy statement of lvt_amd/hip/dropout.py, bit for bit, in NaN-payload
    guard buffers (tests/util_guard.py): one element, a partial group, exact multiples, many workgroups with a tail (262156 =
    65536 * 4 + 12), and 2100000 elements, whose 525000 groups are more than the 2048 * 256 threads of the largest grid, so the
    grid-stride loop runs a second time; with and without res, out aliasing z, T = 0, the max |out| record, refusals;
  * one attention layer in training mode against an fp64 and an fp32 CPU evaluation of the same graph with the same two masks
    (the bound of test_gpu_attention_fallback.py: err <= max(2e-5 scale, 4 err32), err32 the fp32 evaluation's own distance from
    fp64; bank gradients on the common bank scale) -- generic path, block-split path, the shipped flash geometry;
  * off is off: at rate 0 and in eval mode the model issues the C-ABI calls it issues without the keyword and the same logits
    bits; in training each of the 8 sites of a 2 + 2 layer model appears once per direction under one pass index;
  * run-to-run determinism of the loss and the gradients, and what changes them (seed, pass)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seeded
from lvt_amd.hip import binding as L
from lvt_amd.hip import dropout as D
from oracle import lvt_oracle as O
from util_guard import DEV, fbuf, obuf
from util_models import dsfvt_cfg

pytestmark = pytest.mark.gpu

SEED, SR, PASS = 0x9E3779B97F4A7C15, D.site_rank(3, 1, 2), 5
# 2100000: 525000 groups, more than the 2048 * 256 threads of the largest grid -- some threads take a second group
NS = [1, 5, 4096, 32792, 262156, 2100000]


@functools.lru_cache(maxsize=None)
def _data(n):
    g = torch.Generator().manual_seed(1000 + n % 977)
    z = torch.randn(n, generator=g) * 3
    z[z == 0] = 1.0
    return z, torch.randn(n, generator=g)


@functools.lru_cache(maxsize=None)
def _ref(n, p, with_res):
    """The numpy statement, computed once per case and shared."""
    z, r = _data(n)
    out = torch.from_numpy(D.dropout_add_reference(z.numpy(), r.numpy() if with_res else None, SEED, SR, PASS, p))
    keep = torch.from_numpy(D.keep_mask(SEED, SR, PASS, n, p))
    return out, keep


def _bits(t):
    return t.contiguous().view(torch.int32)


def _add_c(zb, rb, n, T, s, ob, slot=None):
    rc = L.lib().lvt_dropout_add(L.ptr(zb.view), L.ptr(rb.view) if rb is not None else None, n, SEED, SR, PASS, T, s,
                                 L.ptr(ob.view), L.ptr(slot), L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg


def _bwd_c(gb, n, T, s, ob, slot=None):
    rc = L.lib().lvt_dropout_bwd(L.ptr(gb.view), n, SEED, SR, PASS, T, s, L.ptr(ob.view), L.ptr(slot), L.stream_ptr())
    msg = L.lib().lvt_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", NS)
def test_dropout_add_bit_for_bit(n, p, with_res):
    z, r = _data(n)
    want, keep = _ref(n, p, with_res)
    T, s = D.threshold(p), float(D.scale(p))
    zb, rb, ob = fbuf(z), (fbuf(r) if with_res else None), obuf(n)
    slot = torch.zeros(1, device=DEV)
    rc, msg = _add_c(zb, rb, n, T, s, ob, slot)
    assert rc == 0, msg
    got = ob.logical()
    assert torch.equal(_bits(got), _bits(want)), "kernel and numpy statement differ in %d of %d elements" % (
        int((_bits(got) != _bits(want)).sum()), n)
    assert ob.outside_untouched() and zb.outside_untouched(), "a float outside the tensor was written"
    assert torch.equal(zb.logical(), z), "the input changed"
    assert float(slot) >= float(got.abs().max()), "max |out| record"
    if not with_res:
        assert torch.equal(got == 0, ~keep) and not bool(torch.signbit(got[~keep]).any())
    # [repeat]
    ob2 = obuf(n)
    rc, msg = _add_c(zb, rb, n, T, s, ob2)
    assert rc == 0 and torch.equal(ob.bits(), ob2.bits()), "a second launch gave other bits"
    # out aliasing z
    rc, msg = _add_c(zb, rb, n, T, s, zb)
    assert rc == 0, msg
    assert torch.equal(_bits(zb.logical()), _bits(want)) and zb.outside_untouched(), "in place"


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", NS)
def test_dropout_bwd_zeroes_what_the_forward_zeroed(n, p):
    g, r = _data(n)
    fwd, keep = _ref(n, p, True)
    want, _ = _ref(n, p, False)
    T, s = D.threshold(p), float(D.scale(p))
    gb, ob = fbuf(g), obuf(n)
    slot = torch.zeros(1, device=DEV)
    rc, msg = _bwd_c(gb, n, T, s, ob, slot)
    assert rc == 0, msg
    got = ob.logical()
    assert torch.equal(_bits(got), _bits(want)) and ob.outside_untouched()
    assert torch.equal(got == 0, ~keep), "the backward's zeros are not the forward's"
    assert torch.equal(_bits(fwd)[~keep], _bits(r)[~keep]), "a dropped element of the forward is not the residual"
    assert float(slot) >= float(got.abs().max())
    ob2 = obuf(n)
    assert _bwd_c(gb, n, T, s, ob2)[0] == 0 and torch.equal(ob.bits(), ob2.bits())


@pytest.mark.parametrize("n", [5, 32792])
def test_threshold_zero_is_a_plain_add(n):
    z, r = _data(n)
    ob = obuf(n)
    rc, msg = _add_c(fbuf(z), fbuf(r), n, 0, 1.0, ob)
    assert rc == 0, msg
    assert torch.equal(_bits(ob.logical()), _bits(r + z))


@pytest.mark.parametrize("n", [5, 262156])
def test_wrappers_and_the_amax_record(n):
    z, r = (t.to(DEV) for t in _data(n))
    want, _ = _ref(n, 0.1, True)
    wantb, _ = _ref(n, 0.1, False)
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    try:
        fallbacks = L.AMAX_FALLBACKS[0]
        out = D.dropout_add(z, r, (SEED, SR, PASS), 0.1)
        assert out is not z and torch.equal(_bits(out.cpu()), _bits(want))
        assert float(L.amax_of(out)) >= float(out.abs().max())
        dz = D.dropout_bwd(z, (SEED, SR, PASS), 0.1)
        assert torch.equal(_bits(dz.cpu()), _bits(wantb)) and float(L.amax_of(dz)) >= float(dz.abs().max())
        z2 = z.clone()
        L.amax_of(z2)                                              # a record that the in-place launch must replace
        fallbacks += 1
        same = D.dropout_add(z2, r, (SEED, SR, PASS), 0.1, inplace=True)
        assert same is z2 and torch.equal(_bits(z2.cpu()), _bits(want)) and float(L.amax_of(z2)) >= float(z2.abs().max())
        assert L.AMAX_FALLBACKS[0] == fallbacks, "an output carried no max |.| record"
    finally:
        L.set_math_mode(before)


def test_refusals_launch_nothing():
    z, r = _data(32)
    zb, ob = fbuf(z), obuf(32)
    T, s = D.threshold(0.5), 2.0
    lib = L.lib()
    null = None
    cases = [
        lib.lvt_dropout_add(L.ptr(zb.view), null, 0, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_add(L.ptr(zb.view), null, -4, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_add(null, null, 32, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_add(L.ptr(zb.view), null, 32, SEED, SR, PASS, T, s, null, null, L.stream_ptr()),
        lib.lvt_dropout_add(L.ptr(zb.view[1:]), null, 16, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_add(L.ptr(zb.view), L.ptr(zb.view[2:]), 16, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_add(L.ptr(zb.view), null, 16, SEED, SR, PASS, T, s, L.ptr(ob.view[3:]), null, L.stream_ptr()),
        lib.lvt_dropout_bwd(L.ptr(zb.view), 0, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_bwd(null, 32, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_bwd(L.ptr(zb.view), 32, SEED, SR, PASS, T, s, null, null, L.stream_ptr()),
        lib.lvt_dropout_bwd(L.ptr(zb.view[1:]), 16, SEED, SR, PASS, T, s, L.ptr(ob.view), null, L.stream_ptr()),
        lib.lvt_dropout_bwd(L.ptr(zb.view), 16, SEED, SR, PASS, T, s, L.ptr(ob.view[1:]), null, L.stream_ptr()),
    ]
    assert cases == [-1] * len(cases), cases
    # the wrappers turn them into LvtError
    zd = zb.view[:32]
    with pytest.raises(L.LvtError, match="lvt_dropout_add"):
        D.dropout_add(zd[:0], None, (SEED, SR, PASS), 0.5)
    with pytest.raises(L.LvtError, match="aligned"):
        D.dropout_add(zd[1:9], None, (SEED, SR, PASS), 0.5, inplace=True)
    with pytest.raises(L.LvtError, match="aligned"):
        D.dropout_add(zd[:8], zd[9:17], (SEED, SR, PASS), 0.5, inplace=True)
    with pytest.raises(L.LvtError, match="lvt_dropout_bwd"):
        D.dropout_bwd(zd[1:9], (SEED, SR, PASS), 0.5)
    with pytest.raises(L.LvtError):
        D.dropout_add(zd[:8].cpu(), None, (SEED, SR, PASS), 0.5)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ob.logical()).all()) and ob.outside_untouched(), "a refused call wrote its output"
    assert torch.equal(zb.logical(), z) and zb.outside_untouched(), "a refused in-place call wrote"


# ---- one layer in training mode against fp64 -------------------------------------------------------------------------------
LAYER_CASES = [
    # block, volume (None: the block), da, d, n_head, b
    ((8, 8, 8), None, 64, 128, 2, 2),
    ((2, 8, 16), (4, 16, 16), 128, 128, 1, 1),       # block-split: the masks index the permuted rows the node sees
    ((1, 16, 16), None, 128, 512, 8, 1),             # the shipped flash geometry
]
P_LAYER, LAYER_NO, LAYER_PASS, LAYER_SEED = 0.25, 3, 1, 0x0123456789ABCDEF


def _oracle_layer(state, x5, gy5, block, masked, dtype, m1, m2):
    """block_local_attention of the oracle with both residual branches dropped: its pieces, same order of operations."""
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(k.split(".")[-1] not in ("mask",))
         for k, v in state.items() if v is not None and v.dtype.is_floating_point}
    x = x5.to(dtype).clone().requires_grad_(True)
    b, c, T, H, W = x.shape
    t, h, w = block
    s = float(D.scale(P_LAYER))
    m1, m2 = m1.to(dtype) * s, m2.to(dtype) * s
    B = O.rel_position_bias(p["dt_bank"], p["dh_bank"], p["dw_bank"], block)

    def layer(tok):
        y1 = tok + (O.multi_head_attention(p, "mha.", tok, B, masked) - tok) * m1
        f = O.layer_norm(y1, p["ffn.0.weight"], p["ffn.0.bias"])
        f = torch.relu(F.linear(f, p["ffn.1.weight"], p["ffn.1.bias"]))
        f = F.linear(f, p["ffn.3.weight"], p["ffn.3.bias"])
        return y1 + f * m2

    if (T, H, W) == (t, h, w):
        y = layer(x.view(b, c, -1).transpose(1, 2).contiguous()).transpose(1, 2).contiguous().view(b, c, T, H, W)
    else:
        nt, nh, nw = T // t, H // h, W // w
        xb = x.view(b, c, nt, t, nh, h, nw, w).permute(0, 2, 4, 6, 1, 3, 5, 7)
        tok = layer(xb.reshape(b * nt * nh * nw, c, t * h * w).transpose(1, 2).contiguous())
        y = tok.transpose(1, 2).reshape(b, nt, nh, nw, c, t, h, w).permute(0, 4, 1, 5, 2, 6, 3, 7).contiguous().view(b, c, T, H, W)
    y.backward(gy5.to(dtype))
    return y.detach(), x.grad, {k: v.grad for k, v in p.items() if v.grad is not None}


@pytest.mark.parametrize("masked", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("block,thw,da,d,n_head,b", LAYER_CASES, ids=["8x8x8_da64", "2x8x16_in_4x16x16", "1x16x16_flash"])
def test_layer_with_dropout_vs_fp64(block, thw, da, d, n_head, b, masked):
    import lvt_amd.modeling.autoregressive.vt_attention as A
    thw = thw or block
    S = block[0] * block[1] * block[2]
    vol = thw[0] * thw[1] * thw[2]
    torch.manual_seed(3)
    layer = A.BlockLocalAttention(block, da, d, n_head, masked=masked, dropout=P_LAYER).to(DEV)
    state_obj = D.DropoutState(LAYER_SEED)
    state_obj.set_next_pass(LAYER_PASS)
    assert state_obj.begin_pass() == LAYER_PASS
    layer.bind_dropout(state_obj, LAYER_NO)
    assert layer.training
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
    # the node sees (b * vol, d) rows, block by block in the split case: the masks of the flat tensor, viewed as (blocks, S, d)
    m1, m2 = (torch.from_numpy(D.keep_mask(LAYER_SEED, D.site_rank(LAYER_NO, br), LAYER_PASS, b * vol * d, P_LAYER))
              .view(b * vol // S, S, d) for br in (0, 1))
    assert 0.7 < float(m1.float().mean()) < 0.8 and not torch.equal(m1, m2)
    y64, dx64, g64 = _oracle_layer(state, x5, gy5, block, masked, torch.float64, m1, m2)
    y32, dx32, g32 = _oracle_layer(state, x5, gy5, block, masked, torch.float32, m1, m2)
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
    # eval mode: the layer without dropout, bit for bit
    layer.eval()
    plain = A.BlockLocalAttention(block, da, d, n_head, masked=masked).to(DEV)
    plain.load_state_dict(layer.state_dict())
    with torch.no_grad():
        assert torch.equal(layer.forward_tokens(xx.detach(), thw), plain.forward_tokens(xx.detach(), thw))


# ---- the model: off is off, sites and passes, determinism ------------------------------------------------------------------
_HOST_ONLY = ("_bytes", "_uses_", "_fuses_", "_supported", "_is_gather", "_partials", "lvt_last_error", "lvt_version",
              "lvt_device_info")
_DROP_ARGS = {"lvt_dropout_add": (4, 5), "lvt_dropout_bwd": (3, 4)}            # (site_rank, pass) among the arguments


class _Recorder:
    """Stands in for the ctypes handle: every enqueued entry point is logged by name, the dropout entries with site and pass."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lvt_") or any(s in name for s in _HOST_ONLY):
            return fn

        def logged(*a):
            self._calls.append((name,) + tuple(a[i] for i in _DROP_ARGS[name]) if name in _DROP_ARGS else name)
            return fn(*a)
        return logged


def _small_cfg(dropout):
    cfg = dsfvt_cfg(DEV)
    vt = cfg.MODEL.AUTOREGRESSIVE.VT
    vt.BLOCKS_E, vt.N_HEAD_E = tuple(vt.BLOCKS_E[:2]), tuple(vt.N_HEAD_E[:2])
    vt.BLOCKS_D, vt.N_HEAD_D = tuple(vt.BLOCKS_D[:2]), tuple(vt.N_HEAD_D[:2])
    vt.DROPOUT = dropout
    return cfg


@functools.lru_cache(maxsize=None)
def _batch():
    return tuple(O.prepare_slices(seeded.seeded_codes("drop%d" % i, (16, 4, 16, 16), 11), (6, 0, 0), (16, 1, 1), (7, 1, 1), 1)
                 for i in range(2))


@pytest.fixture(scope="module")
def models():
    """Three 2 + 2 layer DSFVT models with the same weights: built without the keyword, with DROPOUT 0.0, with DROPOUT 0.1."""
    from lvt_amd.modeling import build_model
    from lvt_amd.modeling.autoregressive.videotransformer import VideoTransformer
    torch.manual_seed(5)
    off = build_model(_small_cfg(0.0))
    on = build_model(_small_cfg(0.1))
    plain = build_model(_small_cfg(0.0))
    v = plain.cfg.MODEL.AUTOREGRESSIVE.VT
    plain.model = VideoTransformer(v.NC, v.NV, v.DA, v.DE, v.D, v.BLOCKS_E, v.N_HEAD_E, v.KERNEL, v.STRIDE, v.BLOCKS_D, v.N_HEAD_D,
                                   v.PAD_VALUE, v.SHARE_P, v.SHARE_EMBEDDINGS, v.CLASS_NUM).to(DEV)
    sd = off.model.state_dict()
    with torch.no_grad():                                           # (banks start at zero: give them values)
        for k in sd:
            if k.endswith("_bank"):
                sd[k].normal_(0, 0.3)
    for m in (on, plain):
        assert list(m.model.state_dict()) == list(sd)
        m.model.load_state_dict(sd)
    return plain, off, on


def _step(model, train, backward=True):
    """One supervised pass -> (C-ABI calls, loss, gradients)."""
    from lvt_amd.utils.events import EventStorage
    model.train(train)
    model.zero_grad(set_to_none=True)
    real, calls = L.lib, []
    handle = real()
    L.lib = lambda: _Recorder(handle, calls)
    try:
        with EventStorage(0), torch.set_grad_enabled(backward):
            loss = model(list(_batch()), mode="supervised")["loss_cross_entropy"]
        if backward:
            loss.backward()
        torch.cuda.synchronize()
    finally:
        L.lib = real
    grads = {n: p.grad.clone() for n, p in model.model.named_parameters() if p.grad is not None}
    return calls, loss.detach().clone(), grads


def _logits(model, train):
    d = _batch()
    ctx, sl, si = (torch.stack([x[k] for x in d]).to(DEV) for k in ("context", "slice", "slice_idx"))
    model.train(train)
    with torch.no_grad():
        model._begin_pass()
        return model.model.logits_tokens(ctx.contiguous(), sl.contiguous(), si.contiguous())


def test_off_is_off(models):
    plain, off, on = models
    pass_before = on.model.dropout_state.pass_
    for m in (plain, off):                                          # (whatever a model's first pass does once is done)
        _step(m, True)
    want, loss0, grads0 = _step(plain, True)
    assert want and not any(isinstance(c, tuple) for c in want)
    calls, loss, grads = _step(off, True)
    assert calls == want and torch.equal(_bits(loss), _bits(loss0))
    assert set(grads) == set(grads0) and all(torch.equal(grads[n], grads0[n]) for n in grads0)
    assert off.model.dropout_state.pass_ == 0
    # rate 0.1 in eval mode: the same calls, the same bits
    for m in (plain, on):
        _step(m, False, backward=False)
    want_eval, loss0, _ = _step(plain, False, backward=False)
    calls, loss, _ = _step(on, False, backward=False)
    assert calls == want_eval and not any(isinstance(c, tuple) for c in calls) and torch.equal(_bits(loss), _bits(loss0))
    for a, b in zip(_logits(on, False), _logits(off, False)):
        assert torch.equal(a, b)
    assert on.model.dropout_state.pass_ == pass_before, "an eval-mode forward advanced the pass index"


def test_every_site_once_per_direction(models):
    plain, off, on = models
    on.model.dropout_state.set_next_pass(0)
    for want_pass in (0, 1):
        calls, _, _ = _step(on, True)
        adds = [c for c in calls if isinstance(c, tuple) and c[0] == "lvt_dropout_add"]
        bwds = [c for c in calls if isinstance(c, tuple) and c[0] == "lvt_dropout_bwd"]
        assert [c[1] for c in adds] == list(range(8)), adds
        assert sorted(c[1] for c in bwds) == list(range(8)), bwds
        assert {c[2] for c in adds + bwds} == {want_pass}
        names = [c[0] if isinstance(c, tuple) else c for c in calls]
        assert names.count("lvt_dropout_add") == 8 and names.count("lvt_dropout_bwd") == 8


def test_model_determinism_seed_and_pass(models):
    plain, off, on = models
    st = on.model.dropout_state
    on.model.set_dropout_seed(1234)
    st.set_next_pass(0)
    _, loss_a, grads_a = _step(on, True)
    st.set_next_pass(0)
    _, loss_b, grads_b = _step(on, True)
    assert torch.equal(_bits(loss_a), _bits(loss_b)) and set(grads_a) == set(grads_b)
    assert all(torch.equal(_bits(grads_a[n]), _bits(grads_b[n])) for n in grads_a), "same seed and pass, other gradient bits"
    _, loss_next, _ = _step(on, True)                                # one pass later
    assert st.pass_ == 1 and float(loss_next) != float(loss_a)
    on.model.set_dropout_seed(4321)
    st.set_next_pass(0)
    _, loss_seed, _ = _step(on, True)
    assert float(loss_seed) != float(loss_a)
    _, loss_off, _ = _step(off, True)
    assert float(loss_off) != float(loss_a)


def test_sampling_ignores_dropout(models):
    plain, off, on = models
    video = seeded.seeded_codes("dropvideo", (16, 4, 16, 16), 8).transpose(0, 1)[None].contiguous().to(DEV)
    outs, pass_before = [], on.model.dropout_state.pass_
    for m in (on, off):
        m.eval()
        with torch.no_grad():
            torch.manual_seed(0)
            outs.append(m.sample_video(video, n_prime=15))
    assert torch.equal(outs[0], outs[1]) and on.model.dropout_state.pass_ == pass_before
