"""Output activations of the conv stacks on the GPU: the sigmoid epilogue of every kernel that accepts the tanh one, against
fp64 CPU torch (bounds: those of the tanh twin of each call in tests/test_gpu_engine.py / tests/test_gpu_norm.py);
PR-DVQVAE2 with the OUT_ACTIVATION pairs of fixture G27 (captured from the reference; bounds of tests/test_gpu_norm.py); the
eval fold, determinism, the model's modes and a short training run."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seeded
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5          # conv outputs (tests/test_gpu_engine.py)
ATOL = 2e-5         # reconstructions (tests/test_gpu_norm.py)


@pytest.fixture(params=["f16x2", "f32"])
def math_mode(request):
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode(request.param)
    yield request.param
    L.set_math_mode(before)


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def _nhwc(x, cp=None):   # (N,C,H,W) -> (N,1,H,W,Cp) contiguous, channels zero-padded
    n, c, h, w = x.shape
    out = torch.zeros(n, 1, h, w, cp or c)
    out[:, 0, :, :, :c] = x.permute(0, 2, 3, 1)
    return out


def _nchw(y):   # (N,1,H,W,C) -> (N,C,H,W)
    return y.squeeze(1).permute(0, 3, 1, 2).contiguous()


def _pad4(c):
    return (c + 3) // 4 * 4


def _spread_bias(c):
    """Biases from -30 to 30: the pre-activations reach both saturated ends of the sigmoid."""
    return torch.linspace(-30.0, 30.0, c) if c > 1 else torch.tensor([30.0])


def _check_sigmoid_out(got_cl, pre64, c, tol):
    """got_cl: (N,1,H,W,Cp) device output; pre64: (N,C,H,W) fp64 pre-activation."""
    from lvt_amd.hip import binding as L
    assert float(pre64.min()) < -20 and float(pre64.max()) > 20          # both ends exercised
    o = got_cl.cpu()
    assert bool(torch.isfinite(o).all())
    err = rel_err(_nchw(o)[:, :c], torch.sigmoid(pre64))
    print("sigmoid rel_err %.3g (bound %.3g)" % (err, tol))
    assert err < tol
    assert torch.equal(o[..., c:], torch.zeros_like(o[..., c:]))            # pad channels exactly 0
    assert float(o.min()) >= 0.0 and float(o.max()) <= 1.0
    if L.f16x2():
        assert float(L.amax_of(got_cl)) >= float(o.abs().max())


# ---- kernels ----------------------------------------------------------------------------------------------------------
# (N, H, W, Ci, Co, k, stride, pad, residual): the first two are the cases of the issue; then the three frame-resident kernels at
# their smallest served shapes (3x3 on 16x16 frames, 4x4 / stride 2 by parity classes, both f16x2 only: f32 takes the tile
# engine) and a 1x1 with more than 128 rows (the wide kernel in f16x2)
CONV_FWD = [(2, 16, 16, 32, 64, 3, 1, 1, True), (1, 8, 8, 64, 3, 1, 1, 0, False), (1, 16, 16, 32, 128, 3, 1, 1, True),
            (1, 32, 32, 32, 128, 4, 2, 1, False), (1, 16, 16, 64, 6, 1, 1, 0, True)]


@pytest.mark.parametrize("N,H,W,Ci,Co,k,s,p,with_res", CONV_FWD)
def test_conv_fwd_sigmoid(N, H, W, Ci, Co, k, s, p, with_res, math_mode):
    from lvt_amd.hip import gemm as G, binding as L
    x, w, b = _rand(N, Ci, H, W), _rand(Co, Ci, k, k, seed=1) * 0.1, _spread_bias(Co)
    pre = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p)
    res = _rand(*pre.shape, seed=2) * 3 if with_res else None
    if with_res:
        pre = pre + res.double()
    cop = _pad4(Co)
    g = G.conv_geom(N, 1, H, W, Ci, cop, (1, k, k), (1, s, s), (0, p, p))
    wd = w.to(DEV)
    wp = G.pack_weight(g, wd, Ci, Co)
    wq = G.pack_weight_parity(g, wd, Ci, Co) if G.fwd_by_parity(g) else None
    bias = torch.cat([b, torch.zeros(cop - Co)]).to(DEV)
    y = G.conv_fwd(g, _nhwc(x).to(DEV), wp, bias=bias, res=_nhwc(res, cop).to(DEV) if with_res else None,
                   flags=L.EPI_SIGMOID | L.epi_pad(cop - Co), wq=wq)
    _check_sigmoid_out(y, pre, Co, TOL)


# (N, Hi, Wi, Cin, Cout): ConvTranspose2d(Cin -> Cout, k4 s2 p1); the case of the issue (the tile engine, phase by phase),
# the frame-resident phase kernel at its smallest served shape (f16x2), and 3 output channels carried as 4
CONVT = [(2, 8, 8, 32, 16), (1, 16, 16, 32, 128), (2, 8, 8, 32, 3)]


@pytest.mark.parametrize("N,Hi,Wi,Cin,Cout", CONVT)
def test_conv_bwd_data_by_phases_sigmoid(N, Hi, Wi, Cin, Cout, math_mode):
    from lvt_amd.hip import gemm as G, binding as L
    x, w, b = _rand(N, Cin, Hi, Wi), _rand(Cin, Cout, 4, 4, seed=1) * 0.1, _spread_bias(Cout)
    pre = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    cop = _pad4(Cout)
    g = G.conv_geom(N, 1, 2 * Hi, 2 * Wi, cop, Cin, (1, 4, 4), (1, 2, 2), (0, 1, 1))
    wd = w.to(DEV)
    wp = G.pack_weight(g, wd, Cout, Cin)
    wph = G.pack_weight_phases(g, wd, Cout, Cin) if G.bwd_data_by_phases(g) else None
    bias = torch.cat([b, torch.zeros(cop - Cout)]).to(DEV)
    y = G.conv_bwd_data(g, _nhwc(x).to(DEV), wp, bias=bias, flags=L.EPI_SIGMOID | L.epi_pad(cop - Cout), wph=wph)
    _check_sigmoid_out(y, pre, Cout, TOL)


# (N, Hi, Wi, Ci, Cr, tol): the case of the issue and a ragged one on the fp32 FMA kernel, then the matrix-core kernel's shape
# (Ci 128, 8 x 32 bands; f16x2); bounds of test_thin_conv_transpose_forward for the same kernels
CONVT4 = [(2, 16, 16, 16, 3, 2e-6), (1, 5, 7, 32, 2, 2e-6), (1, 8, 32, 128, 3, 4e-6)]


@pytest.mark.parametrize("N,Hi,Wi,Ci,Cr,tol", CONVT4)
@pytest.mark.parametrize("act", ["sigmoid", ""])
def test_convt4_fwd_activation_codes(N, Hi, Wi, Ci, Cr, tol, act, math_mode):
    from lvt_amd.hip import gemm as G, binding as L
    x, w, b = _rand(N, Ci, Hi, Wi), _rand(Ci, Cr, 4, 4, seed=1) * 0.1, _spread_bias(Cr)
    if Cr == 2:
        b = torch.tensor([-30.0, 30.0])
    pre = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    y = G.convT4_fwd(_nhwc(x).to(DEV), w.to(DEV), b.to(DEV), L.EPI_SIGMOID if act else 0)
    assert y.shape == (N, 1, 2 * Hi, 2 * Wi, 4)
    if act:
        _check_sigmoid_out(y, pre, Cr, tol)
    else:
        o = y.cpu()
        assert rel_err(_nchw(o)[:, :Cr], pre) < tol
        assert torch.equal(o[..., Cr:], torch.zeros_like(o[..., Cr:]))
        if L.f16x2():
            assert float(L.amax_of(y)) >= float(o.abs().max())


def test_convt4_old_entry_point_keeps_its_meaning():
    """lvt_convt4_fwd(act_tanh) still is tanh / none, bit for bit the new entry with the matching code."""
    from lvt_amd.hip import gemm as G, binding as L
    x, w, b = _nhwc(_rand(2, 16, 8, 8)).to(DEV), (_rand(16, 3, 4, 4, seed=1) * 0.1).to(DEV), _rand(3, seed=2).to(DEV)
    for flag, code in ((1, L.EPI_TANH), (0, 0)):
        y = torch.empty(2, 1, 16, 16, 4, device=DEV)
        io = L.amax_io(x, w)
        L.check(L.lib().lvt_convt4_fwd(L.ptr(x), L.ptr(w), L.ptr(b), 2, 8, 8, 16, 3, flag, L.ptr(y), L.math_flag(), L.io_ref(io),
                                       L.stream_ptr()), "lvt_convt4_fwd")
        assert torch.equal(y, G.convT4_fwd(x, w, b, code))
        assert torch.equal(y, G.convT4_fwd(x, w, b, bool(flag)))
    y = torch.empty(2, 1, 16, 16, 4, device=DEV)
    rc = L.lib().lvt_convt4_fwd_act(L.ptr(x), L.ptr(w), L.ptr(b), 2, 8, 8, 16, 3, L.EPI_RELU, L.ptr(y), L.math_flag(),
                                    L.io_ref(L.amax_io(x, w)), L.stream_ptr())
    assert rc != 0                                                          # an activation code the kernel does not have


def _rows(M, C, seed):
    """(M, Cp) rows with zero pad channels, |.| up to 30."""
    g = torch.Generator().manual_seed(seed)
    cp = _pad4(C)
    y = torch.zeros(M, cp)
    y[:, :C] = (torch.rand(M, C, generator=g) * 2 - 1) * 30
    return y, cp, g


@pytest.mark.parametrize("M,C", [(37, 3), (4099, 64)])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_apply_sigmoid(M, C, with_res, math_mode):
    from lvt_amd.hip import binding as L, norm as BN
    y, cp, g = _rows(M, C, M + C)
    scale, shift = torch.zeros(cp), torch.zeros(cp)                         # (what finalize leaves in the pad channels)
    scale[:C], shift[:C] = torch.rand(C, generator=g) * 0.5 + 0.5, torch.randn(C, generator=g)
    res = torch.zeros(M, cp)
    res[:, :C] = torch.randn(M, C, generator=g)
    pre = y[:, :C].double() * scale[:C].double() + shift[:C].double() + (res[:, :C].double() if with_res else 0.0)
    assert float(pre.min()) < -20 and float(pre.max()) > 20
    out = BN.apply(y.to(DEV), scale.to(DEV), shift.to(DEV), res=res.to(DEV) if with_res else None,
                   act=L.EPI_SIGMOID | L.epi_pad(cp - C))
    o = out.cpu()
    err = rel_err(o[:, :C], torch.sigmoid(pre))
    print("bn_apply sigmoid rel_err %.3g" % err)
    assert err < 1e-6
    assert bool(torch.isfinite(o).all())
    assert torch.equal(o[:, C:], torch.zeros(M, cp - C))                    # pad channels exactly 0
    if L.f16x2():
        assert float(L.amax_of(out)) >= float(o.abs().max())


def test_sigmoid_bwd(math_mode):
    from lvt_amd.hip import binding as L, ew
    M, C = 4099, 64
    x, _, g = _rows(M, C, 5)
    y = torch.sigmoid(x)                                                    # saved fp32 output: exactly 1 / 1e-13 at the ends
    assert float(y.max()) == 1.0 and float(y.min()) < 1e-12
    gout = torch.randn(M, C, generator=g)
    out = ew.sigmoid_bwd(gout.to(DEV), y.to(DEV))
    o = out.cpu()
    ref = gout.double() * y.double() * (1.0 - y.double())
    err = rel_err(o, ref)
    print("sigmoid_bwd rel_err %.3g" % err)
    assert err < 1e-6
    assert bool(torch.isfinite(o).all())
    if L.f16x2():
        assert float(L.amax_of(out)) >= float(o.abs().max())


def test_bounded_activation_must_end_the_stack():
    """Tanh or sigmoid anywhere but the last layer, and a ReLU-terminated stack, stay LvtError."""
    from lvt_amd.hip import binding as L, convnet
    x = _nhwc(_rand(1, 16, 8, 8)).to(DEV)
    w = [(_rand(16, 16, 1, 1, seed=i).to(DEV), _rand(16, seed=9 + i).to(DEV)) for i in range(2)]
    for acts in (("sigmoid", ""), ("tanh", ""), ("", "relu")):
        layers = [convnet.Layer("conv", (1, 1, 1), (1, 1, 1), (0, 0, 0), 16, 16, act=a) for a in acts]
        outs, saved = convnet.stack_forward(layers, x, w)
        with pytest.raises(L.LvtError):
            convnet.stack_backward(layers, x, outs, saved, torch.ones_like(outs[-1]))


# ---- PR-DVQVAE2 against G27 ----------------------------------------------------------------------------------------------
GRADS = {"enc_first": ("encoder", "layers.0.0.weight"), "enc_res3": ("encoder", "layers.5.block.1.0.weight"),
         "dec_ct1": ("generator", "layers.4.0.weight")}                    # tests/golden/make_golden_norm.py


def _state(module, prefix, seed):
    """make_golden_norm.py:seeded_norm_state / seeded_conv_state on the lvt_amd module tree (same keys)."""
    st = {}
    for name, m in module.named_modules():
        if not hasattr(m, "running_mean"):
            continue
        c = m.running_mean.numel()
        r = seeded._rng(seed, prefix + "norm." + name)
        st[name + ".weight"] = torch.from_numpy((1.0 + 0.2 * r.standard_normal(c)).astype(np.float32))
        st[name + ".bias"] = torch.from_numpy((0.1 * r.standard_normal(c)).astype(np.float32))
        st[name + ".running_mean"] = torch.from_numpy((0.05 * r.standard_normal(c)).astype(np.float32))
        st[name + ".running_var"] = torch.from_numpy(r.uniform(0.5, 2.0, c).astype(np.float32))
    norm_owner = lambda k: hasattr(module.get_submodule(k.rsplit(".", 1)[0]), "running_mean")  # noqa: E731
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()
              if (k.endswith(".weight") or k.endswith(".bias")) and v.dim() >= 1 and not norm_owner(k)}
    st.update(seeded.seeded_params(shapes, seed, prefix))
    return st


def act_cfg(norm, enc_act, dec_act):
    from util_models import vqvae_cfg
    cfg = vqvae_cfg(DEV)
    cfg.MODEL.ENCODER.NORM = cfg.MODEL.GENERATOR.NORM = norm
    cfg.MODEL.ENCODER.OUT_ACTIVATION, cfg.MODEL.GENERATOR.OUT_ACTIVATION = enc_act, dec_act
    return cfg


def act_model(g, combo):
    from lvt_amd.modeling import build_model
    tag, norm, enc_act, dec_act = combo.split("|")
    model = build_model(act_cfg(norm, enc_act, dec_act))
    wseed = int(g["wseed"])
    for part, pre in (("encoder", "enc."), ("generator", "dec.")):
        mod = getattr(model, part)
        missing, unexpected = mod.load_state_dict(_state(mod, pre, wseed), strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    cb = seeded.seeded_codebook_state(wseed, scale=float(g[tag + ".scale"]))
    model.codebook.load_state_dict(cb)
    return model, cb, tag, norm


def _data(g, n=4):
    return [{"image": seeded.seeded_input("g27.f%d" % i, (3, 64, 64), int(g["seed"])).numpy()} for i in range(n)]


def _run_g27(golden, combo):
    from lvt_amd.utils.events import EventStorage
    g = golden("g27_out_activation")
    assert combo in [str(c) for c in g["combos"]]
    model, cb, tag, norm = act_model(g, combo)
    rows, nrec = int(g["rows"]), int(g["rec_frames"])
    assert float(g[tag + ".eval.clear_share"]) >= 0.99
    # ---- one train step: the bounds of _check_step (tests/test_gpu_norm.py) ----
    model.train()
    with EventStorage(0):
        losses = model(_data(g), mode="supervised")
    sum(losses.values()).backward()
    lr, lc = float(losses["loss_reconstruction"]), float(losses["loss_commitment"])
    wr, wc = float(g[tag + ".train.loss_reconstruction"]), float(g[tag + ".train.loss_commitment"])
    print("%s: loss_reconstruction %.9g (want %.9g, rel %.3g)  loss_commitment %.9g (want %.9g, rel %.3g)"
          % (tag, lr, wr, abs(lr - wr) / wr, lc, wc, abs(lc - wc) / wc))
    assert abs(lr - wr) < 1e-5 * wr, lr
    assert abs(lc - wc) < 2e-4 * wc, lc
    for key, (part, name) in GRADS.items():
        p = dict(getattr(model, part).named_parameters())[name if norm else name.replace(".0.weight", ".weight")]
        err = rel_err(p.grad[:rows], g[tag + ".train.grad." + key])
        print("%s: grad %s rel_err %.3g" % (tag, key, err))
        assert err < 5e-3, key
    for part in ("encoder", "generator"):
        for k, v in getattr(model, part).state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                assert rel_err(v, g[tag + ".after.%s.%s" % (part, k)]) < 1e-5, k
    # ---- eval: latents and reconstructions (the bounds of _run_g26) ----
    model.eval()
    model.codebook.load_state_dict(cb)
    with torch.no_grad():
        out = model(_data(g), mode="inference")
    lat = torch.stack([o["latent"] for o in out]).cpu()
    rec = torch.stack([o["reconstruction"] for o in out]).cpu()[:nrec]
    want, clear = g[tag + ".eval.latent"], g[tag + ".eval.clear"]
    assert torch.equal(lat[clear], want[clear])
    keep = torch.ones(4, 64, 64, dtype=torch.bool)
    for t, i, y, x in (lat != want).nonzero().tolist():
        keep[t, max(0, 4 * (y - 4)):4 * (y + 5), max(0, 4 * (x - 4)):4 * (x + 5)] = False      # receptive field (G6)
    print("%s: %d latents differ, %.3f of the pixels kept" % (tag, int((lat != want).sum()), float(keep.float().mean())))
    assert float(keep.float().mean()) > 0.8
    k3 = keep[:nrec, None].expand_as(rec)
    ref = g[tag + ".eval.reconstruction"]
    err = float((rec - ref).abs()[k3].max() / ref.abs().max())
    print("%s: reconstruction err %.3g" % (tag, err))
    assert err < ATOL


COMBOS = ["plain_sigmoid|||sigmoid", "tanh_plain||tanh|", "sigmoid_tanh||sigmoid|tanh", "bn.plain_sigmoid|BN||sigmoid"]


@pytest.mark.parametrize("combo", COMBOS)
def test_g27_against_reference(golden, combo, math_mode):
    _run_g27(golden, combo)


def test_g27_sigmoid_head_under_amax_check(golden):
    """Every max |.| record that an engine launch of the sigmoid-head step reads is verified against its tensor."""
    from lvt_amd.hip import binding as L
    assert L.get_math_mode() == "f16x2"
    old, L.AMAX_CHECK = L.AMAX_CHECK, True
    try:
        _run_g27(golden, COMBOS[0])
    finally:
        L.AMAX_CHECK = old


# ---- further checks ------------------------------------------------------------------------------------------------------
def test_eval_fold_of_a_sigmoid_stride2_decoder(monkeypatch):
    """The stride-2 decoder normalises and then activates its only ConvTranspose: under no_grad the norms are folded into the
    weights (one `fold`, no other norm wrapper) and the sigmoid rides on the plain stack's last launch."""
    from lvt_amd.hip import norm as BN
    from lvt_amd.modeling.generator.resdecoder import ResDecoder
    torch.manual_seed(3)
    dec = ResDecoder(in_channels=64, nf=64, res_channels=32, out_channels=3, norm="BN", use_spectral_norm=False, n_layers=1,
                     out_activation="sigmoid", stride=2).to(DEV)
    with torch.no_grad():
        for m in dec.modules():
            if hasattr(m, "running_mean"):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(), m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.5, 2.0)
        dec.layers[-2][1].weight.mul_(8.0)                                  # spread the head's input over the sigmoid
    dec.eval()
    assert isinstance(dec.layers[-1], torch.nn.Sigmoid) and dec._plan[-1].norm == "bn" and dec._plan[-1].act == "sigmoid"
    z = torch.randn(2, 64, 16, 16, device=DEV)
    with torch.enable_grad():
        ref = dec(z.clone().requires_grad_(True)).detach()
    calls = []
    for name in ("stats", "finalize", "apply", "bwd_reduce", "bwd_apply", "fold"):
        fn = getattr(BN, name)
        monkeypatch.setattr(BN, name, lambda *a, _f=fn, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    with torch.no_grad():
        out = dec(z)
    assert calls == ["fold"]
    assert out.shape == (2, 3, 32, 32) and float(ref.min()) < 0.1 and float(ref.max()) > 0.9
    assert rel_err(out, ref) < 1e-5


def test_sigmoid_tanh_training_trajectory_bit_reproducible():
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.events import EventStorage

    def run():
        torch.manual_seed(11)
        model = build_model(act_cfg("", "sigmoid", "tanh"))
        model.train()
        opts, _ = model.configure_optimizers_and_checkpointers()
        g = torch.Generator().manual_seed(5)
        losses = []
        for i in range(3):
            clips = torch.rand(2, 16, 3, 64, 64, generator=g).to(DEV)
            with EventStorage(i):
                ls = model([{"image_sequence": clips[j]} for j in range(2)], mode="supervised")
            sum(ls.values()).backward()
            for o in opts:
                o["optimizer"].step()
            for o in opts:
                o["optimizer"].zero_grad()
            losses.append({k: float(v.detach()) for k, v in ls.items()})
        state = {n: t.detach().clone() for n, t in list(model.named_parameters()) + list(model.named_buffers())}
        return losses, state

    (la, sa), (lb, sb) = run(), run()
    assert la == lb and all(np.isfinite(v) for d in la for v in d.values())
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_every_mode_of_a_sigmoid_head_model(golden):
    """supervised, generator, inference, encoder, encoder_decoder and interpolate_first_last once, sigmoid decoder head."""
    from lvt_amd.utils.events import EventStorage
    g = golden("g27_out_activation")
    model, cb, tag, _ = act_model(g, COMBOS[0])
    data = _data(g)
    model.eval()
    with torch.no_grad():
        inf = model(data, mode="inference")
        lat = model(data, mode="encoder")
        ed = model(data, mode="encoder_decoder")
        itp = model(data, mode="interpolate_first_last")
    assert torch.equal(lat, torch.stack([o["latent"] for o in inf]))
    assert ed.shape == (4, 3, 64, 64) and float(ed.min()) >= 0.0 and float(ed.max()) <= 1.0
    rec = torch.stack([o["reconstruction"] for o in inf])
    assert rel_err(rec, (ed * 0.5 + 0.5).clamp(0.0, 1.0)) < 1e-6            # back_normalizer of PR-DVQVAE2 (mean / std 0.5)
    assert itp.shape == (4, 3, 64, 64) and float(itp.min()) >= 0.0 and float(itp.max()) <= 1.0
    model.train()
    losses = {}
    for mode in ("supervised", "generator"):
        model.codebook.load_state_dict(cb)
        with EventStorage(0):
            losses[mode] = {k: float(v) for k, v in model(data, mode=mode).items()}
    assert losses["supervised"] == losses["generator"]
    assert abs(losses["supervised"]["loss_reconstruction"] - float(g[tag + ".train.loss_reconstruction"])) \
        < 1e-5 * float(g[tag + ".train.loss_reconstruction"])


def test_train_net_runs_a_short_sigmoid_config(tmp_path):
    out = str(tmp_path / "vq")
    r = subprocess.run([sys.executable, "tools/train_net.py", "--config-file", "configs/vqvae/PR-DVQVAE2.yaml", "--synthetic",
                        "--max-iter", "3", "OUTPUT_DIR", out, "SOLVER.IMS_PER_BATCH", "4", "SOLVER.MAX_ITER", "3",
                        "MODEL.GENERATOR.OUT_ACTIVATION", "sigmoid"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "loss_reconstruction" in r.stdout + r.stderr
    ck = torch.load(os.path.join(out, "netG", "model_final.pth"))
    assert "layers.6.weight" in ck["model"]                                 # the head's ConvTranspose; the Sigmoid has no keys
