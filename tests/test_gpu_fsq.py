"""Finite scalar quantisation (MODEL.CODEBOOK.FSQ.LEVELS, csrc/fsq.hip) on the device.  The reference has no FSQ: the
yardstick is lvt_amd/modeling/vq/fsq.py in float64 on the CPU.

Bounds.  Kernels: indices equal wherever the float64 bound is further than 2^-14 from a half-integer (16 fp32 ulps at the largest
magnitude a bound takes, 32), one of the two neighbours elsewhere, and at most 1 % of a case's elements may be elsewhere
(tests/util_fsq.py; tests/test_host_fsq.py checks that share on the CPU); z_q within one fp32 ulp of the float64 value at equal
digits; pad columns exactly 0; decode(idx) == z_q bit for bit; the max |.| record at least the true maximum; two runs equal bits.
Backward: err <= max(2e-5 scale, 4 err32), err32 the same rule in fp32 torch (the project's bound, tests/test_gpu_vt_dropout.py).
Module and model: the exempt set is wider by half_l x the engine's bound on the projection (tests/test_gpu_gemm_matrix.py: 1e-5
sum |a||b| + 2^-21 (|bias| + |c|)); values within the engine's bound, gradients within max(2e-5, 4 x the CPU fp32 evaluation's
distance) of the float64 evaluation with the same indices, the loss 2e-4 relative -- the model-level check of
tests/test_gpu_cosine_codebook.py, which also lends the 2 % the model's exempt share may reach."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import seeded
import util_fsq as U
from conftest import ROOT, rel_err
from util_models import MEAN, STD, dsfvt_cfg, vqvae_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 23


def _bits(t):
    return t.contiguous().view(torch.int32)


def _digits_of_idx(idx, levels):
    """(n, num, P) int64 on any device -> digits (n * P, num * d) on the CPU."""
    from lvt_amd.modeling.vq import fsq as R
    n, num, P = idx.shape
    return R.digits_of(idx.cpu().permute(0, 2, 1).reshape(n * P, num), levels)


def _amax_ok(t):
    from lvt_amd.hip import binding as L
    if not L.f16x2():
        return
    assert L._valid_amax(t) is not None, "no max |.| record"
    assert float(L.amax_of(t)) >= float(t.abs().max())


# ---- the kernels against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", U.KERNEL_CASES, ids=U.case_id)
def test_forward_and_decode_against_fp64(c):
    from lvt_amd.hip import fsq as K
    from lvt_amd.modeling.vq import fsq as R
    rows, num, levels, scale, extra = c
    k = U.kernel_case(*c)
    nd, ld = k["nd"], k["ld"]
    z = k["z_p"].to(DEV)
    z_q, idx = K.fsq_fwd(z, num, levels)                                    # P = rows: idx (1, num, rows)
    assert torch.equal(z.cpu(), k["z_p"])                                   # out of place: the input is untouched
    assert tuple(z_q.shape) == (rows, ld) and tuple(idx.shape) == (1, num, rows) and idx.dtype == torch.int64
    dig = _digits_of_idx(idx, levels)
    assert int(idx.min()) >= 0 and int(idx.max()) < math.prod(levels)
    U.check_digits(dig, k["b"], k["dig"], levels, k["exempt"], U.case_id(c))
    same = dig == k["dig"]
    got = z_q.cpu()[:, :nd].double()
    assert bool(((got - k["z_q"]).abs() <= U.ulp32(k["z_q"]))[same].all())                       # one fp32 ulp at equal digits
    own = R.value_of(dig, levels)
    assert bool(((got - own).abs() <= U.ulp32(own)).all())                                      # and z_q is the value of idx
    assert float(got.abs().max()) <= 1.0
    assert bool((_bits(z_q[:, nd:]) == 0).all())                                                # pad columns: +0
    _amax_ok(z_q)
    # decode(idx) == z_q bit for bit, pads included
    back = K.fsq_decode(idx, levels, ld)
    assert torch.equal(_bits(back), _bits(z_q))
    _amax_ok(back)
    # either output alone, another P, a second run: the same bits
    only_q, none = K.fsq_fwd(z, num, levels, want_idx=False)
    none2, only_i = K.fsq_fwd(z, num, levels, want_zq=False)
    assert none is None and none2 is None
    assert torch.equal(_bits(only_q), _bits(z_q)) and torch.equal(only_i, idx)
    z_q1, idx1 = K.fsq_fwd(z, num, levels, P=1)                             # idx (rows, num, 1)
    assert torch.equal(idx1[:, :, 0], idx[0].t()) and torch.equal(_bits(z_q1), _bits(z_q))
    assert torch.equal(_bits(K.fsq_decode(idx1, levels, ld)), _bits(z_q))
    z_q2, idx2 = K.fsq_fwd(z, num, levels)
    assert torch.equal(_bits(z_q2), _bits(z_q)) and torch.equal(idx2, idx)


def test_code_layout_with_several_samples():
    """rows = 6 samples x 35 positions: idx is (6, num, 35), the layout of the other quantisers' searches."""
    from lvt_amd.hip import fsq as K
    num, levels, n, P = 4, (8, 5, 5, 5), 6, 35
    z = torch.randn(n * P, 16, generator=torch.Generator().manual_seed(3)).to(DEV) * 2
    z_q, idx = K.fsq_fwd(z, num, levels, P=P)
    _, flat = K.fsq_fwd(z, num, levels, P=1)
    assert tuple(idx.shape) == (n, num, P)
    assert torch.equal(idx.permute(0, 2, 1).reshape(n * P, num), flat[:, :, 0])
    assert torch.equal(_bits(K.fsq_decode(idx, levels)), _bits(z_q))


@pytest.mark.parametrize("c", U.KERNEL_CASES, ids=U.case_id)
def test_backward_against_fp64(c):
    from lvt_amd.hip import fsq as K
    rows, num, levels, scale, extra = c
    k = U.kernel_case(*c)
    nd = k["nd"]
    z, g = k["z_p"].to(DEV), k["g"].to(DEV)
    dz = K.fsq_bwd(g, z, num, levels)
    assert torch.equal(z.cpu(), k["z_p"]) and torch.equal(g.cpu(), k["g"])
    ref = k["dz_p"]
    err = float((dz.cpu()[:, :nd].double() - ref).abs().max())
    err32 = float((k["dz_p32"].double() - ref).abs().max())
    sc = float(ref.abs().max())
    print("%s: err %.3g err32 %.3g scale %.3g" % (U.case_id(c), err, err32, sc))
    assert err <= max(2e-5 * sc, 4 * err32), (err, err32, sc)
    assert bool((_bits(dz[:, nd:]) == 0).all())
    _amax_ok(dz)
    assert torch.equal(_bits(K.fsq_bwd(g, z, num, levels)), _bits(dz))


# ---- FSQEmbedding against fsq.step ---------------------------------------------------------------------------------------------
def _module(num, levels, dim, params):
    from lvt_amd.modeling.vq import FSQEmbedding
    q = FSQEmbedding(num, levels, dim)
    q.load_state_dict({"proj_in.weight": params["w_in"], "proj_in.bias": params["b_in"], "proj_out.weight": params["w_out"],
                       "proj_out.bias": params["b_out"]})
    return q.to(DEV)


def _rule(k, levels, idx_rows, dtype):
    """fsq.step on the case's rows with the device's codes forced -> (out, gradients at z_e and the four parameters)."""
    from lvt_amd.modeling.vq import fsq as R
    p = {n: v.detach().clone().to(dtype).requires_grad_(True) for n, v in k["params"].items()}     # (copies: the case is shared)
    z = k["rows64"].detach().clone().to(dtype).requires_grad_(True)
    out = R.step(z, p["w_in"], p["b_in"], p["w_out"], p["b_out"], levels, force_idx=idx_rows)
    g_rows = k["g"].permute(0, 2, 3, 1).reshape(z.shape).to(dtype)
    out["z_out"].backward(g_rows)
    return out, dict({"z": z.grad}, **{n: v.grad for n, v in p.items()})


@pytest.mark.parametrize("c", U.MODULE_CASES, ids=U.module_case_id)
def test_module_three_modes_and_backward(c):
    from lvt_amd.modeling.vq import fsq as R
    num, levels, dim, (n, h, w) = c
    k = U.module_case(*c)
    q = _module(num, levels, dim, k["params"])
    z = k["z"].to(DEV).requires_grad_(True)
    idx = q(z.detach())                                                      # mode "": (n, num, h, w) int64
    assert tuple(idx.shape) == (n, num, h, w) and idx.dtype == torch.int64
    idx_rows = idx.cpu().permute(0, 2, 3, 1).reshape(-1, num)
    dig64 = R.digits(R.project_in(k["rows64"], k["params"]["w_in"].double(), k["params"]["b_in"].double()), levels)
    U.check_digits(R.digits_of(idx_rows, levels), k["b"], dig64, levels, k["exempt"], U.module_case_id(c))
    st, bar = q(z, "st")
    assert bar is st and tuple(st.shape) == (n, dim, h, w)
    assert torch.equal(q.last_indices, idx)
    ref, g64 = _rule(k, levels, idx_rows, torch.float64)
    _, g32 = _rule(k, levels, idx_rows, torch.float32)
    p64 = {name: v.double() for name, v in k["params"].items()}
    tol = U.engine_bound(ref["z_q"].detach(), p64["w_out"], p64["b_out"], ref["z_out"].detach())
    got = st.detach().cpu().permute(0, 2, 3, 1).reshape(-1, dim).double()
    assert bool(((got - ref["z_out"].detach()).abs() <= tol).all())
    # "emb": the decoder input from the codes alone -- the tensor the "st" pass produced, bit for bit
    emb = q(idx, "emb")
    assert tuple(emb.shape) == (n, h, w, dim)
    assert torch.equal(_bits(emb), _bits(st.detach().permute(0, 2, 3, 1)))
    st.backward(k["g"].to(DEV))
    mine = {"z": z.grad.cpu().permute(0, 2, 3, 1).reshape(-1, dim), "w_in": q.proj_in.weight.grad, "b_in": q.proj_in.bias.grad,
            "w_out": q.proj_out.weight.grad, "b_out": q.proj_out.bias.grad}
    for name in sorted(mine):
        assert tuple(mine[name].shape) == tuple(g64[name].shape), name
        sc = float(g64[name].abs().max())
        err = float((mine[name].double().cpu() - g64[name]).abs().max())
        err32 = float((g32[name].double() - g64[name]).abs().max())
        print("%s %s: err %.3g err32 %.3g scale %.3g" % (U.module_case_id(c), name, err, err32, sc))
        assert err <= max(2e-5 * sc, 4 * err32), (name, err, err32, sc)


def test_module_is_the_same_function_in_eval_mode_and_run_to_run():
    c = (4, (8, 8, 8), 256, (3, 5, 7))
    k = U.module_case(*c)
    q = _module(c[0], c[1], c[2], k["params"])
    z = k["z"].to(DEV)
    with torch.no_grad():
        a, ia = q.train()(z, "st")[0], q.last_indices
        b, ib = q.eval()(z, "st")[0], q.last_indices
        a2 = q.train()(z, "st")[0]
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(a2)) and torch.equal(ia, ib)
    assert q.normalise_cl(z) is z and q.health_scalars() is None


# ---- the model ---------------------------------------------------------------------------------------------------------------------
LEVELS = (8, 8, 8)


def _model():
    from lvt_amd.modeling import build_model
    cfg = vqvae_cfg(DEV)
    cfg.MODEL.CODEBOOK.EMA = False
    cfg.MODEL.CODEBOOK.FSQ.LEVELS = list(LEVELS)
    torch.manual_seed(SEED)
    model = build_model(cfg)
    model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, SEED, "enc."))
    model.generator.load_state_dict(seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, SEED, "dec."))
    gen = torch.Generator().manual_seed(SEED)
    model.codebook.load_state_dict({"proj_in.weight": torch.randn(12, 256, generator=gen) / 16.0,
                                    "proj_in.bias": 0.2 * torch.randn(12, generator=gen),
                                    "proj_out.weight": torch.randn(256, 12, generator=gen) / 12 ** 0.5,
                                    "proj_out.bias": 0.2 * torch.randn(256, generator=gen)})
    return model


def _frames(tag, n=4):
    return torch.stack([seeded.seeded_input("fsq.%s.%d" % (tag, i), (3, 64, 64), SEED) for i in range(n)])


def _snapshot(model):
    cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
    return cpu(model.encoder.state_dict()), cpu(model.generator.state_dict()), cpu(model.codebook.state_dict())


def _oracle_step(enc, dec, cb, x, idx_rows, dtype):
    """The float64 (float32) statement of the supervised step at the given parameters with the device's codes forced ->
    (loss, gradients by name)."""
    from oracle import lvt_oracle as O
    from lvt_amd.modeling.vq import fsq as R
    pe = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in enc.items()}
    pd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in dec.items()}
    pc = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in cb.items()}
    xn = O.normalize(x, MEAN, STD).to(dtype)
    z_e = O.res_encoder(pe, xn)
    n, d, h, w = z_e.shape
    out = R.step(z_e.permute(0, 2, 3, 1).reshape(-1, d), pc["proj_in.weight"], pc["proj_in.bias"], pc["proj_out.weight"],
                 pc["proj_out.bias"], LEVELS, force_idx=idx_rows)
    x_tilde = O.res_decoder(pd, out["z_out"].view(n, h, w, d).permute(0, 3, 1, 2))
    loss = F.mse_loss(x_tilde, xn)
    loss.backward()
    grads = {"enc.layers.0.weight": pe["layers.0.weight"].grad, "dec.layers.0.weight": pd["layers.0.weight"].grad,
             "proj_in.weight": pc["proj_in.weight"].grad, "proj_in.bias": pc["proj_in.bias"].grad,
             "proj_out.weight": pc["proj_out.weight"].grad, "proj_out.bias": pc["proj_out.bias"].grad}
    return loss.detach(), grads


def test_model_three_train_steps_against_fp64():
    """PR-DVQVAE2 with EMA False and LEVELS [8, 8, 8], 4 seeded frames, three consecutive train steps (Adam in between), each
    against the float64 statement evaluated at the device's own pre-step parameters with the device's codes forced."""
    from lvt_amd.modeling.vq import FSQEmbedding, fsq as R
    from lvt_amd.utils.events import EventStorage
    model = _model().train()
    assert isinstance(model.codebook, FSQEmbedding) and model.fsq
    opts, _ = model.configure_optimizers_and_checkpointers()
    assert len(opts) == 3
    enc_fwd = model.encoder.forward_cl
    seen = {}

    def forward_cl(x_cl):
        seen["z_e"] = enc_fwd(x_cl)
        return seen["z_e"]

    model.encoder.forward_cl = forward_cl
    try:
        for step in range(3):
            x = _frames("s%d" % step)
            enc, dec, cb = _snapshot(model)
            with EventStorage(step):
                losses = model([{"image": x[i].numpy()} for i in range(4)], mode="supervised")
            assert set(losses) == {"loss_reconstruction"}                        # no loss_commitment, no loss_dict
            sum(losses.values()).backward()
            idx = model.codebook.last_indices
            assert tuple(idx.shape) == (4, 4, 16, 16) and idx.dtype == torch.int64
            idx_rows = idx.cpu().permute(0, 2, 3, 1).reshape(-1, 4)
            # the device's codes against the float64 rule on the device's own z_e
            z_e = seen["z_e"].detach().cpu().reshape(-1, 256).double()
            b, exempt = U.projected_exempt(z_e, cb["proj_in.weight"].double(), cb["proj_in.bias"].double(), LEVELS)
            share = float(exempt.double().mean())
            dig64 = R.digits(R.project_in(z_e, cb["proj_in.weight"].double(), cb["proj_in.bias"].double()), LEVELS)
            dig = R.digits_of(idx_rows, LEVELS)
            print("step %d: exempt %.3g %%, %d codes in use" % (step, 100 * share, int(torch.unique(idx).numel())))
            assert share <= 0.02
            assert torch.equal(dig[~exempt], dig64[~exempt])
            assert bool(((dig - dig64).abs() <= 1).all())
            l64, g64 = _oracle_step(enc, dec, cb, x, idx_rows, torch.float64)
            l32, g32 = _oracle_step(enc, dec, cb, x, idx_rows, torch.float32)
            a, r = float(losses["loss_reconstruction"]), float(l64)
            print("step %d: loss_reconstruction %.9g float64 %.9g" % (step, a, r))
            assert abs(a - r) < 2e-4 * r
            mine = {"enc.layers.0.weight": model.encoder.state_dict(keep_vars=True)["layers.0.weight"].grad,
                    "dec.layers.0.weight": model.generator.state_dict(keep_vars=True)["layers.0.weight"].grad,
                    **{k: v.grad for k, v in model.codebook.state_dict(keep_vars=True).items()}}
            for name in sorted(g64):
                e_mine, e_cpu = rel_err(mine[name], g64[name]), rel_err(g32[name], g64[name])
                print("step %d: gradient of %s %.3g (CPU fp32 %.3g)" % (step, name, e_mine, e_cpu))
                assert e_mine <= max(2e-5, 4 * e_cpu), (step, name, e_mine, e_cpu)
            for o in opts:
                o["optimizer"].step()
            for o in opts:
                o["optimizer"].zero_grad()
            after = _snapshot(model)[2]
            assert all(not torch.equal(after[k], cb[k]) for k in cb)             # the optimizer moved all four tensors
    finally:
        del model.encoder.forward_cl


def test_model_inference_encode_decode_and_a_transformer_on_top():
    from oracle import lvt_oracle as O
    from lvt_amd.modeling import build_model
    from lvt_amd.modeling.vq import fsq as R
    model = _model().eval()
    x = _frames("eval", 16)
    xn = O.normalize(x, MEAN, STD).to(DEV)
    enc, dec, cb = _snapshot(model)
    with torch.no_grad():
        out = model([{"image": x[i].numpy()} for i in range(16)], mode="inference")
        lat = model.encode(xn)
        rec = model.decode(lat)
        pix = model.decode_pixels(lat)
        direct = model.codebook(model.encoder(xn))
    assert tuple(lat.shape) == (16, 4, 16, 16) and lat.dtype == torch.int64
    assert int(lat.min()) >= 0 and int(lat.max()) < 512
    assert torch.equal(torch.stack([o["latent"] for o in out]), lat) and torch.equal(direct, lat)
    recon = torch.stack([o["reconstruction"] for o in out])
    assert tuple(recon.shape) == (16, 3, 64, 64) and torch.equal(recon, pix)
    # the round trip against the float64 decode of the same codes
    rows = lat.cpu().permute(0, 2, 3, 1).reshape(-1, 4)
    z_out = R.decode(rows, cb["proj_out.weight"].double(), cb["proj_out.bias"].double(), LEVELS)
    want = O.res_decoder({k: v.double() for k, v in dec.items()}, z_out.view(16, 16, 16, 256).permute(0, 3, 1, 2))
    err = float((rec.double().cpu() - want).abs().max())
    err_pix = float((recon.double().cpu() - O.back_normalize(want, MEAN, STD).clamp(0.0, 1.0)).abs().max())
    print("decode(encode(x)): %.3g   inference pixels: %.3g" % (err, err_pix))
    assert err < 5e-4 and err_pix < 5e-4                                          # (the bound of tests/test_gpu_convcoders.py)
    # a DSFVT train pass on the codes: NV 512, NC 4 match
    vt = build_model(dsfvt_cfg(DEV)).train()
    v = vt.cfg.MODEL.AUTOREGRESSIVE.VT
    assert (v.NV, v.NC) == (512, 4)
    data = [O.prepare_slices(lat.cpu(), (a, 0, 0), (16, 1, 1), (7, 1, 1), 1) for a in (3, 9)]
    loss = vt.compute_supervised_loss(*vt.preprocess_data(data)[:4])["loss_cross_entropy"]
    loss.backward()
    assert bool(torch.isfinite(loss)) and 1.0 < float(loss) < 2 * math.log(512)


# ---- off is off ------------------------------------------------------------------------------------------------------------------------
_HOST_ONLY = ("_bytes", "_uses_", "_fuses_", "_supported", "_is_gather", "lvt_last_error", "lvt_version", "lvt_device_info",
              "_partials")


class _Recorder:
    """Stands in for the ctypes handle: every enqueued entry point is logged by name (the pattern of tests/test_gpu_convcoders.py)."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lvt_") or any(s in name for s in _HOST_ONLY):
            return fn

        def logged(*a):
            self._calls.append(name)
            return fn(*a)
        return logged


def record_train_step_calls(levels=None, ema=None):
    """C-ABI calls, by name, of one PR-DVQVAE2 supervised step (forward + backward, 2 frames, f16x2 arithmetic)."""
    from lvt_amd.hip import binding as L
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.events import EventStorage
    cfg = vqvae_cfg(DEV)
    if levels is not None:
        cfg.MODEL.CODEBOOK.FSQ.LEVELS = levels
    if ema is not None:
        cfg.MODEL.CODEBOOK.EMA = ema
    torch.manual_seed(3)
    model = build_model(cfg)
    model.train()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    before, real, calls = L.get_math_mode(), L.lib, []
    L.set_math_mode("f16x2")
    handle = real()
    L.lib = lambda: _Recorder(handle, calls)
    try:
        with EventStorage(0):
            losses = model([{"image": x[i].numpy()} for i in range(2)], mode="supervised")
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        L.lib = real
        L.set_math_mode(before)
    return calls


# Recorded from the parent commit with record_train_step_calls() (that commit's package, which has no FSQ key):
PARENT_TRAIN_STEP_CALLS = """
    lvt_amax_multi lvt_to_channels_last lvt_conv3d_pack_weights_multi lvt_conv3d_weight_images lvt_conv3d_fwd
    lvt_conv3d_fwd_parity lvt_conv3d_fwd lvt_conv3d_fwd lvt_conv3d_fwd lvt_conv3d_fwd lvt_conv3d_fwd lvt_vq_nearest
    lvt_vq_gather lvt_amax lvt_vq_ema_accumulate lvt_conv3d_pack_weights_multi lvt_conv3d_weight_images lvt_conv3d_fwd
    lvt_conv3d_fwd lvt_conv3d_fwd lvt_conv3d_fwd lvt_conv3d_fwd lvt_conv3d_bwd_data_phases lvt_convt4_fwd_act
    lvt_vq_ema_finalize lvt_vq_gather lvt_amax lvt_mse_fwd lvt_mse_fwd lvt_mse_bwd lvt_mse_bwd lvt_tanh_bwd
    lvt_conv3d_bwd_weight lvt_colsum lvt_conv3d_fwd lvt_conv3d_bwd_weight lvt_conv3d_fwd_parity lvt_conv3d_bwd_weight
    lvt_conv3d_bwd_data lvt_conv3d_bwd_weight lvt_conv3d_fwd lvt_conv3d_bwd_weight lvt_conv3d_bwd_data lvt_conv3d_bwd_weight
    lvt_conv3d_fwd lvt_conv3d_bwd_weight lvt_conv3d_fwd lvt_amax lvt_conv3d_bwd_weight lvt_conv3d_bwd_data
    lvt_conv3d_bwd_weight lvt_conv3d_fwd lvt_conv3d_bwd_weight lvt_conv3d_bwd_data lvt_conv3d_bwd_weight lvt_conv3d_fwd
    lvt_conv3d_bwd_weight lvt_conv3d_fwd lvt_conv3d_bwd_weight lvt_conv3d_bwd_data_phases lvt_conv3d_bwd_weight
"""


def test_off_issues_the_calls_of_the_parent_commit():
    want = PARENT_TRAIN_STEP_CALLS.split()
    assert record_train_step_calls([]) == want
    assert record_train_step_calls(None) == want
    on = record_train_step_calls([8, 8, 8], ema=False)
    assert [n for n in on if n.startswith("lvt_fsq_")] == ["lvt_fsq_fwd", "lvt_fsq_bwd"]
    assert not any(n.startswith("lvt_vq_") for n in on)                          # no search, gather, EMA
    assert not any(n.startswith("lvt_fsq_") for n in want)


# ---- tools/train_net.py ----------------------------------------------------------------------------------------------------------------
def test_train_net_runs_with_the_key_set(tmp_path):
    out = str(tmp_path / "fsq")
    r = subprocess.run([sys.executable, "tools/train_net.py", "--config-file", "configs/vqvae/PR-DVQVAE2.yaml", "--synthetic",
                        "--max-iter", "40", "OUTPUT_DIR", out, "SOLVER.IMS_PER_BATCH", "4", "SOLVER.MAX_ITER", "40",
                        "MODEL.CODEBOOK.EMA", "False", "MODEL.CODEBOOK.FSQ.LEVELS", "[8, 8, 8]"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = r.stdout + r.stderr
    assert "loss_commitment" not in log and "loss_dict" not in log
    vals = [float(v) for v in re.findall(r"iter \d+ .*?loss_reconstruction: ([0-9.eE+-]+|nan|inf)", log)]
    print("loss_reconstruction at the logged iterations:", vals)
    assert len(vals) >= 2 and all(math.isfinite(v) for v in vals) and vals[-1] < vals[0]
    ck = torch.load(os.path.join(out, "netC", "model_final.pth"))
    assert sorted(ck["model"]) == ["proj_in.bias", "proj_in.weight", "proj_out.bias", "proj_out.weight"]
    assert all(bool(torch.isfinite(v).all()) for v in ck["model"].values())
