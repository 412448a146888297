"""Batch normalisation of the conv stacks on the GPU (csrc/norm.hip, hip/convnet.py): the kernels against fp64 CPU torch,
PR-DVQVAE2 with NORM "BN" / "FrozenBN" against fixture G26 (captured from the reference), the eval fold, determinism and
a short training run.  Tolerances of the model-level checks are those of G5 / G6 (tests/test_gpu_vqvae.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 2e-5


# ---- kernels ----------------------------------------------------------------------------------------------------------
def _act(M, C, ratio=1e3, seed=0):
    """(M, Cp) channels-last activation, pad channels zero, per-channel |mean| / std = ratio."""
    g = torch.Generator().manual_seed(seed)
    cp = (C + 3) // 4 * 4
    std = torch.rand(C, generator=g) * 2 + 0.1
    mean = std * ratio * torch.where(torch.rand(C, generator=g) > 0.5, 1.0, -1.0)
    y = torch.zeros(M, cp)
    y[:, :C] = torch.randn(M, C, generator=g) * std + mean
    return y, cp


SHAPES = [(1, 64), (37, 3), (4099, 64), (70001, 128), (65536 + 333, 256), (20000, 3)]


@pytest.mark.parametrize("M,C", SHAPES)
def test_stats_accuracy_at_large_mean(M, C):
    from lvt_amd.hip import norm as BN
    y, cp = _act(M, C)
    st = BN.stats(y.to(DEV)).cpu().double()
    yd = y[:, :C].double()
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    # the mean to 1e-5 of the spread, plus the rounding of an fp32 result (|mean| 2^-24)
    assert bool(((st[0, :C] - mean).abs() <= 1e-5 * var.sqrt() + 2.0 ** -24 * mean.abs()).all())
    if M > 1:
        assert float(((st[1, :C] - var).abs() / var).max()) <= 1e-5
    assert torch.equal(st[:, C:], torch.zeros(2, cp - C, dtype=torch.float64))


@pytest.mark.parametrize("M,C", SHAPES[1:])
@pytest.mark.parametrize("act", ["", "relu", "tanh"])
def test_forward_backward_against_fp64(M, C, act):
    from lvt_amd.hip import binding as L, norm as BN
    y, cp = _act(M, C, ratio=3.0, seed=M + C)
    g = torch.Generator().manual_seed(1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    res = torch.zeros(M, cp)
    res[:, :C] = torch.randn(M, C, generator=g)
    gout = torch.zeros(M, cp)
    gout[:, :C] = torch.randn(M, C, generator=g)
    d = lambda t: t.to(DEV)  # noqa: E731
    rm_d, rv_d, nbt = d(rm.clone()), d(rv.clone()), torch.zeros((), dtype=torch.int64, device=DEV)
    st = BN.stats(d(y))
    scale, shift, saved = BN.finalize(C, cp, d(gamma), d(beta), rm_d, rv_d, stats=st, count=M, num_batches_tracked=nbt,
                                      flags=L.BN_UPDATE | L.BN_UNBIASED | L.BN_COUNT)
    flag = {"": 0, "relu": L.EPI_RELU, "tanh": L.EPI_TANH}[act]
    out = BN.apply(d(y), scale, shift, res=d(res), act=flag)
    # fp64 reference: torch batch_norm in train mode with the same running buffers
    yd = y[:, :C].double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rmr, rvr = rm.double().clone(), rv.double().clone()
    z = torch.nn.functional.batch_norm(yd, rmr, rvr, gd, bd, training=True, momentum=0.1, eps=1e-5)
    pre = z + res[:, :C].double()
    ref = {"": pre, "relu": torch.relu(pre), "tanh": torch.tanh(pre)}[act]
    o = out.cpu()
    assert rel_err(o[:, :C], ref) < 1e-6
    assert torch.equal(o[:, C:], torch.zeros(M, cp - C))                    # pad channels exactly 0
    assert rel_err(rm_d.cpu(), rmr) < 1e-6 and rel_err(rv_d.cpu(), rvr) < 1e-6 and int(nbt) == 1
    if L.f16x2():
        assert float(L.amax_of(out)) >= float(o.abs().max())
    # backward at the normalised output (the activation's backward is the producer's business: g is given there)
    z.backward(gout[:, :C].double())
    sums = BN.bwd_reduce(d(gout), d(y), saved)
    dy = BN.bwd_apply(d(gout), d(y), scale, saved, sums, n=M, train=True)
    assert rel_err(dy.cpu()[:, :C], yd.grad) < 1e-5
    assert torch.equal(dy.cpu()[:, C:], torch.zeros(M, cp - C))
    assert rel_err(sums[1, :C].cpu(), gd.grad) < 1e-5 and rel_err(sums[0, :C].cpu(), bd.grad) < 1e-5
    if L.f16x2():
        assert float(L.amax_of(dy)) >= float(dy.abs().max())
    # running statistics (eval / frozen): scale g
    sc2, sh2, sv2 = BN.finalize(C, cp, d(gamma), d(beta), d(rm), d(rv), flags=L.BN_RUNNING)
    ref_sc = gamma.double() / (rv.double() + 1e-5).sqrt()
    assert rel_err(sc2.cpu()[:C], ref_sc) < 1e-6
    assert rel_err(sh2.cpu()[:C], beta.double() - rm.double() * ref_sc) < 1e-6
    dy2 = BN.bwd_apply(d(gout), None, sc2, train=False)
    assert rel_err(dy2.cpu()[:, :C], gout[:, :C].double() * ref_sc) < 1e-6


def test_kernels_bit_reproducible():
    from lvt_amd.hip import binding as L, norm as BN
    y, cp = _act(70001, 128, ratio=10.0)
    y = y.to(DEV)
    g = torch.randn(y.shape, device=DEV)
    one = torch.ones(128, device=DEV)
    outs = []
    for _ in range(2):
        st = BN.stats(y)
        sc, sh, sv = BN.finalize(128, cp, one, one * 0.5, torch.zeros(128, device=DEV), torch.ones(128, device=DEV), stats=st,
                                 count=y.shape[0], flags=0)
        s = BN.bwd_reduce(g, y, sv)
        outs.append([st, sc, sh, s, BN.apply(y, sc, sh, act=L.EPI_RELU), BN.bwd_apply(g, y, sc, sv, s, n=y.shape[0])])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_fold_conv_and_transposed():
    """One launch folds a conv and a ConvTranspose (output channel = weight dim 1): w scale[co], bias = shift (Cp long)."""
    from torch import nn
    from lvt_amd.hip import binding as L, norm as BN
    layers, want = [], []
    for transposed, (ci, co, k) in ((False, (32, 64, 3)), (True, (64, 30, 4))):
        shape = (ci, co, k, k) if transposed else (co, ci, k, k)
        w = torch.randn(shape, device=DEV)
        nm = nn.BatchNorm2d(co).to(DEV)
        with torch.no_grad():
            nm.weight.uniform_(0.5, 1.5), nm.bias.normal_(), nm.running_mean.normal_(), nm.running_var.uniform_(0.5, 2.0)
        cp = (co + 3) // 4 * 4
        layers.append((w, transposed, nm, cp))
        sc = (nm.weight.double() * (1.0 / torch.sqrt(nm.running_var.double() + 1e-5))).float()
        view = (1, -1, 1, 1) if transposed else (-1, 1, 1, 1)
        sh = torch.zeros(cp, device=DEV)
        sh[:co] = (nm.bias.double() - nm.running_mean.double() * sc.double()).float()
        want.append((w * sc.view(view), sh, co))
    got = BN.fold(layers)
    for (w2, b2), (wr, br, co) in zip(got, want):
        assert rel_err(w2, wr) < 1e-6 and rel_err(b2, br) < 1e-6
        assert not bool(b2[co:].any())                                    # pad channels of the bias exactly 0
        if L.f16x2():
            assert float(L.amax_of(w2)) >= float(w2.abs().max())


# ---- PR-DVQVAE2 with normalised conv stacks against G26 -----------------------------------------------------------------
SEED = 2626


def _norm_state(module, prefix):
    """make_golden_norm.py:seeded_norm_state / seeded_conv_state on the lvt_amd module tree (same keys)."""
    st = {}
    for name, m in module.named_modules():
        if not hasattr(m, "running_mean"):
            continue
        c = m.running_mean.numel()
        r = seeded._rng(SEED, prefix + "norm." + name)
        st[name + ".weight"] = torch.from_numpy((1.0 + 0.2 * r.standard_normal(c)).astype(np.float32))
        st[name + ".bias"] = torch.from_numpy((0.1 * r.standard_normal(c)).astype(np.float32))
        st[name + ".running_mean"] = torch.from_numpy((0.05 * r.standard_normal(c)).astype(np.float32))
        st[name + ".running_var"] = torch.from_numpy(r.uniform(0.5, 2.0, c).astype(np.float32))
    norm_owner = lambda k: hasattr(module.get_submodule(k.rsplit(".", 1)[0]), "running_mean")  # noqa: E731
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()
              if (k.endswith(".weight") or k.endswith(".bias")) and v.dim() >= 1 and not norm_owner(k)}
    st.update(seeded.seeded_params(shapes, SEED, prefix))
    return st


def norm_model(norm, scale=1.0, device=DEV):
    from lvt_amd.modeling import build_model
    from util_models import vqvae_cfg
    cfg = vqvae_cfg(device)
    cfg.MODEL.ENCODER.NORM = cfg.MODEL.GENERATOR.NORM = norm
    model = build_model(cfg)
    for part, pre in (("encoder", "enc."), ("generator", "dec.")):
        mod = getattr(model, part)
        missing, unexpected = mod.load_state_dict(_norm_state(mod, pre), strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    cb = seeded.seeded_codebook_state(SEED, scale=scale)
    model.codebook.load_state_dict(cb)
    return model, cb


def _data(n=4):
    return [{"image": seeded.seeded_input("g26.f%d" % i, (3, 64, 64), SEED).numpy()} for i in range(n)]


GRADS = {"enc_first": ("encoder", "layers.0.0.weight"), "enc_res3": ("encoder", "layers.5.block.1.0.weight"),
         "dec_ct1": ("generator", "layers.4.0.weight")}
NORM_LAYERS = {"enc0": ("encoder", "layers.0.1"), "enc_res1": ("encoder", "layers.6.block.3.1"),
               "dec_ct1": ("generator", "layers.4.1")}


def _check_step(model, g, tag, rows):
    from lvt_amd.utils.events import EventStorage
    with EventStorage(0):
        losses = model(_data(), mode="supervised")
    sum(losses.values()).backward()
    lr, lc = float(losses["loss_reconstruction"]), float(losses["loss_commitment"])
    assert abs(lr - float(g[tag + "loss_reconstruction"])) < 1e-5 * float(g[tag + "loss_reconstruction"]), lr
    assert abs(lc - float(g[tag + "loss_commitment"])) < 2e-4 * float(g[tag + "loss_commitment"]), lc
    for key, (part, name) in GRADS.items():
        p = dict(getattr(model, part).named_parameters())[name]
        assert rel_err(p.grad[:rows], g[tag + "grad." + key]) < 5e-3, key
    for key, (part, name) in NORM_LAYERS.items():
        m = getattr(model, part).get_submodule(name)
        for t in ("weight", "bias"):
            if (tag + "grad.%s.%s" % (key, t)) in g:
                assert rel_err(getattr(m, t).grad, g[tag + "grad.%s.%s" % (key, t)]) < 5e-3, (key, t)


def _run_g26(golden, norm):
    g = golden("g26_batchnorm")
    rows = int(g["rows"])
    model, cb = norm_model(norm, float(g[norm + ".scale"]))
    model.train()
    _check_step(model, g, norm + ".train.", rows)
    for part in ("encoder", "generator"):
        for k, v in getattr(model, part).state_dict().items():
            key = norm + ".after.%s.%s" % (part, k)
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(g[key]) == 1, k
            elif k.endswith("running_mean") or k.endswith("running_var"):
                assert rel_err(v, g[key]) < 1e-5, k
    # eval after the step: latents and reconstructions of the fold path
    model.eval()
    model.codebook.load_state_dict(cb)
    with torch.no_grad():
        out = model(_data(), mode="inference")
    lat = torch.stack([o["latent"] for o in out]).cpu()
    rec = torch.stack([o["reconstruction"] for o in out]).cpu()
    want, clear = g[norm + ".eval.latent"], g[norm + ".eval.clear"]
    assert torch.equal(lat[clear], want[clear])
    keep = torch.ones(4, 64, 64, dtype=torch.bool)
    for t, i, y, x in (lat != want).nonzero().tolist():
        keep[t, max(0, 4 * (y - 4)):4 * (y + 5), max(0, 4 * (x - 4)):4 * (x + 5)] = False      # receptive field (G6)
    assert float(keep.float().mean()) > 0.8
    k3 = keep[:, None].expand_as(rec)
    ref = g[norm + ".eval.reconstruction"]
    assert float((rec - ref).abs()[k3].max() / ref.abs().max()) < ATOL
    # eval with gradients: no fold, running statistics with their backward
    model.zero_grad()
    model.codebook.load_state_dict(cb)
    _check_step(model, g, norm + ".evalgrad.", rows)


@pytest.fixture(params=["f16x2", "f32"])
def math_mode(request):
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode(request.param)
    yield request.param
    L.set_math_mode(before)


@pytest.mark.parametrize("norm", ["BN", "FrozenBN"])
def test_g26_against_reference(golden, norm, math_mode):
    _run_g26(golden, norm)


def test_g26_bn_under_amax_check(golden):
    """Every max |.| record that an engine launch of the BN step reads is verified against its tensor."""
    from lvt_amd.hip import binding as L
    assert L.get_math_mode() == "f16x2"
    old, L.AMAX_CHECK = L.AMAX_CHECK, True
    try:
        _run_g26(golden, "BN")
    finally:
        L.AMAX_CHECK = old


def test_eval_fold_runs_no_norm_kernels_and_matches_unfolded(monkeypatch):
    from lvt_amd.hip import norm as BN
    model, _ = norm_model("BN", 0.2)
    model.eval()
    x = torch.stack([torch.from_numpy(d["image"]) for d in _data()]).to(DEV)
    xin = model.normalizer(x)
    # unfolded: grad enabled -> apply with running statistics
    with torch.enable_grad():
        z_ref = model.encoder(xin.clone().requires_grad_(True)).detach()
        r_ref = model.generator(z_ref.clone().requires_grad_(True)).detach()
    calls = []
    for name in ("stats", "finalize", "apply", "bwd_reduce", "bwd_apply", "fold"):
        fn = getattr(BN, name)
        monkeypatch.setattr(BN, name, lambda *a, _f=fn, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    with torch.no_grad():
        z = model.encoder(xin)
        r = model.generator(z)
    assert calls == ["fold", "fold"]                # one fold launch per stack, then the plain stack's kernels
    assert rel_err(z, z_ref) < 1e-5 and rel_err(r, r_ref) < 1e-5


def test_bn_training_trajectory_bit_reproducible():
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.events import EventStorage
    from util_models import vqvae_cfg

    def run():
        cfg = vqvae_cfg(DEV)
        cfg.MODEL.ENCODER.NORM = cfg.MODEL.GENERATOR.NORM = "BN"
        torch.manual_seed(11)
        model = build_model(cfg)
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
    assert la == lb
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert int(sa["encoder.layers.0.1.num_batches_tracked"]) == 3


def test_train_net_runs_a_short_bn_config(tmp_path):
    out = str(tmp_path / "vq")
    r = subprocess.run([sys.executable, "tools/train_net.py", "--config-file", "configs/vqvae/PR-DVQVAE2.yaml", "--synthetic",
                        "--max-iter", "3", "OUTPUT_DIR", out, "SOLVER.IMS_PER_BATCH", "4", "SOLVER.MAX_ITER", "3",
                        "MODEL.ENCODER.NORM", "BN", "MODEL.GENERATOR.NORM", "BN"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "loss_reconstruction" in r.stdout + r.stderr
    ck = torch.load(os.path.join(out, "netE", "model_final.pth"))
    assert int(ck["model"]["layers.0.1.num_batches_tracked"]) == 3
