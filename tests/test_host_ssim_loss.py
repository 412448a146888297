"""Host side of the SSIM loss term (LOSS.SSIM.LAMBDA): the plain-torch statement of the rule (evaluation/quality.py
ssim_loss_reference) against its closed-form gradient and against the evaluator's SSIM, the config key and its refusals, the
off-means-unchanged structure of the loss module, and the argument validation of the new C entries (before any device work)."""
import os
import re

import pytest
import torch

from conftest import ROOT

MEAN, STD = [0.4, 0.5, 0.6], [0.2, 0.25, 0.5]
NEW = ("lvt_ssim_loss_partials", "lvt_ssim_loss_fwd", "lvt_ssim_loss_finish", "lvt_mse_bwd_plus", "lvt_l1_bwd_plus")


def _norm(u, mean=MEAN, std=STD):
    c = u.shape[1]
    m, s = torch.tensor(mean[:c], dtype=torch.float64).view(1, c, 1, 1), torch.tensor(std[:c], dtype=torch.float64).view(1, c, 1, 1)
    return (u.double() - m) / s


def _cases():
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    smooth = torch.nn.functional.avg_pool2d(r(2, 3, 28, 34), 5, stride=1)          # (2, 3, 24, 30)
    yield "noise", r(2, 3, 24, 30), r(2, 3, 24, 30), 1.0
    yield "smooth+0.05", smooth + 0.05 * torch.randn(smooth.shape, generator=g, dtype=torch.float64), smooth, 1.0
    yield "bright flat", 0.9 + 1e-3 * r(2, 3, 24, 30), 0.9 + 1e-3 * r(2, 3, 24, 30), 1.0
    yield "out of range", 3 * r(2, 3, 24, 30) - 1, r(2, 3, 24, 30), 1.0
    yield "L=255", 255 * r(1, 3, 11, 13), 255 * r(1, 3, 11, 13), 255.0
    yield "one channel", r(3, 1, 11, 11), r(3, 1, 11, 11), 1.0


@pytest.mark.parametrize("name,ux,uy,L", list(_cases()), ids=[c[0] for c in _cases()])
def test_closed_form_gradient_equals_autograd(name, ux, uy, L):
    from lvt_amd.evaluation.quality import ssim_loss_closed_form, ssim_loss_reference
    c = ux.shape[1]
    mean, std = ([255 * v for v in MEAN[:c]], [255 * v for v in STD[:c]]) if L == 255.0 else (MEAN[:c], STD[:c])
    x = _norm(ux, mean, std).requires_grad_(True)
    y = _norm(uy, mean, std)
    loss = ssim_loss_reference(x, y, mean, std, L, 0.7)
    assert loss.dtype == torch.float64 and loss.dim() == 0
    g, = torch.autograd.grad(loss, x)
    closed = ssim_loss_closed_form(x.detach(), y, mean, std, L, 0.7)
    assert float(g.abs().max()) > 0
    assert float((closed - g).abs().max()) <= 1e-12 * float(g.abs().max())


def test_value_is_the_evaluators_ssim_on_denormalised_frames():
    from lvt_amd.evaluation import frame_quality_reference, ssim_loss_reference
    for name, ux, uy, L in _cases():
        c = ux.shape[1]
        mean, std = ([255 * v for v in MEAN[:c]], [255 * v for v in STD[:c]]) if L == 255.0 else (MEAN[:c], STD[:c])
        x, y = _norm(ux, mean, std), _norm(uy, mean, std)
        m, s = torch.tensor(mean, dtype=torch.float64).view(1, c, 1, 1), torch.tensor(std, dtype=torch.float64).view(1, c, 1, 1)
        want = 0.3 * (1 - frame_quality_reference(x * s + m, y * s + m, L)[1].mean())
        got = ssim_loss_reference(x, y, mean, std, L, 0.3)
        assert abs(float(got) - float(want)) <= 1e-14, name


def test_reference_properties():
    """Equal frames: exactly 0.  Any dtype, gradient to both arguments, refusals as ValueError."""
    from lvt_amd.evaluation import ssim_loss_reference
    g = torch.Generator().manual_seed(0)
    a = torch.rand(2, 3, 12, 15, generator=g)
    assert float(ssim_loss_reference(a, a.clone(), MEAN, STD, 1.0, 0.5)) == 0.0
    out = ssim_loss_reference(a, a.flip(0), MEAN, STD, 1.0, 0.5)
    assert out.dtype == torch.float32 and 0.0 < float(out) < 1.0
    assert ssim_loss_reference(a.bfloat16(), a.flip(0).bfloat16(), MEAN, STD, 1.0, 0.5).dtype == torch.bfloat16
    assert float(ssim_loss_reference(a, a.flip(0), MEAN, STD, 1.0, 0.0)) == 0.0
    x, y = a.double().requires_grad_(True), a.flip(0).double().requires_grad_(True)
    ssim_loss_reference(x, y, MEAN, STD, 1.0, 1.0).backward()
    assert x.grad is not None and y.grad is not None
    for bad in (lambda: ssim_loss_reference(a[..., :10], a[..., :10], MEAN, STD, 1.0, 1.0),
                lambda: ssim_loss_reference(a, a[:1], MEAN, STD, 1.0, 1.0),
                lambda: ssim_loss_reference(a, a, MEAN[:2], STD[:2], 1.0, 1.0),
                lambda: ssim_loss_reference(a, a, MEAN, STD, 0.0, 1.0),
                lambda: ssim_loss_reference(a, a, MEAN, STD, float("nan"), 1.0)):
        with pytest.raises(ValueError):
            bad()


# ---- config ----------------------------------------------------------------------------------------------------------------------
def _cfg(path="configs/vqvae/PR-DVQVAE2.yaml"):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, path))
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def test_default_is_off_in_every_shipped_config():
    from lvt_amd.config import get_cfg
    assert get_cfg().LOSS.SSIM.LAMBDA == 0.0
    for sub in ("vqvae", "vt"):
        for name in sorted(os.listdir(os.path.join(ROOT, "configs", sub))):
            cfg = get_cfg()
            cfg.merge_from_file(os.path.join(ROOT, "configs", sub, name))
            assert cfg.LOSS.SSIM.LAMBDA == 0.0, name
    cfg = get_cfg()
    cfg.merge_from_list(["LOSS.SSIM.LAMBDA", "0.5"])
    assert cfg.LOSS.SSIM.LAMBDA == 0.5


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("arch", ["VQVAEModel", "AutoEncoderModel"])
def test_bad_values_are_refused_when_the_model_is_built(bad, arch):
    from lvt_amd.modeling import build_model
    cfg = _cfg()
    cfg.MODEL.META_ARCHITECTURE = arch
    cfg.LOSS.SSIM.LAMBDA = bad
    with pytest.raises(ValueError, match="LOSS.SSIM.LAMBDA"):
        build_model(cfg)


@pytest.mark.parametrize("mode", ["l2", "l1"])
def test_off_is_the_pixel_loss_path(monkeypatch, mode):
    """LAMBDA == 0: the loss module of the VQ-VAE wraps the same PixelLoss, and its forward is one call of that PixelLoss with the
    arguments of the step before the term existed (the plain mse for AutoEncoderModel); nothing of the SSIM path is touched."""
    from lvt_amd.hip import ew
    from lvt_amd.modeling import build_model
    from lvt_amd.modeling.loss import PixelLoss, ReconstructionLoss
    from lvt_amd.modeling.loss import loss as loss_mod
    cfg = _cfg()
    cfg.LOSS.PIXEL.MODE = mode
    cfg.LOSS.PIXEL.LAMBDA = 0.75
    model = build_model(cfg)
    rl = model.reconstruction_loss
    assert isinstance(rl, ReconstructionLoss) and rl.ssim_lambda == 0.0
    assert isinstance(rl.pixel_loss, PixelLoss) and model.pixel_loss is rl.pixel_loss
    assert rl.pixel_loss._fn is (loss_mod.l1 if mode == "l1" else loss_mod.mse) and rl.pixel_loss._lambda == 0.75
    assert not list(rl.state_dict())                                    # the checkpoint layout does not change
    calls = []
    monkeypatch.setattr(loss_mod._MseFn, "apply", staticmethod(lambda *a: (calls.append(a), "pix")[1]))
    monkeypatch.setattr(loss_mod._PixelSsimFn, "apply", staticmethod(lambda *a: pytest.fail("SSIM node with LAMBDA == 0")))
    monkeypatch.setattr(ew, "ssim_loss_fwd", lambda *a, **k: pytest.fail("SSIM kernel with LAMBDA == 0"))
    a, b = torch.zeros(2, 1, 12, 12, 4), torch.ones(2, 1, 12, 12, 4)
    assert rl(a, b, denom=864) == {"loss_reconstruction": "pix"}
    assert len(calls) == 1 and calls[0][0] is a and calls[0][1] is b and calls[0][2:4] == (864.0, 0.75)
    assert (calls[0][4:] == (True,)) if mode == "l1" else (calls[0][4:] == ())
    # AutoEncoderModel: the plain mse under its own key
    cfg = _cfg()
    cfg.MODEL.META_ARCHITECTURE = "AutoEncoderModel"
    ae = build_model(cfg)
    assert ae.reconstruction_loss.pixel_loss is None and ae.reconstruction_loss.ssim_lambda == 0.0
    del calls[:]
    assert ae.reconstruction_loss(a, b, denom=864, key="loss_ae_mse") == {"loss_ae_mse": "pix"}
    assert len(calls) == 1 and calls[0][2:] == (864.0, 1.0)


def test_on_builds_with_the_inference_data_range():
    from lvt_amd.modeling import build_model
    cfg = _cfg()
    cfg.LOSS.SSIM.LAMBDA = 0.5
    assert build_model(cfg).reconstruction_loss.data_range == 1.0
    cfg.INPUT.SCALE_TO_ZEROONE = False
    rl = build_model(cfg).reconstruction_loss
    assert rl.data_range == 255.0 and rl.ssim_lambda == 0.5


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_table_and_header():
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    declared = set(re.findall(r"\b(lvt_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(L.declared_symbols())
    lib = L.lib()
    assert lib.lvt_ssim_loss_partials(2, 64, 64, 4) == 2 * 16 and lib.lvt_ssim_loss_partials(1, 11, 43, 8) == 2 * 3
    assert lib.lvt_ssim_loss_partials(1, 10, 64, 4) == -1 and lib.lvt_ssim_loss_partials(1, 64, 64, 3) == -1


def test_c_entries_refuse_before_any_device_work():
    import ctypes
    from lvt_amd.hip import binding as L
    lib = L.lib()
    p = ctypes.c_void_p(1 << 20)                                            # aligned, never dereferenced: every call below is refused
    ok = dict(N=2, H=16, W=16, Cp=4, C=3, rng=1.0, lam=0.5, n=2)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.lvt_ssim_loss_fwd(p, p, a["N"], a["H"], a["W"], a["Cp"], a["C"], p, p, a["rng"], a["lam"], p, a["n"], p, None)

    for kw, word in ((dict(H=10), "window"), (dict(W=10), "window"), (dict(C=5), "padded"), (dict(Cp=8), "padded"), (dict(N=0), "frames"),
                     (dict(rng=0.0), "data_range"), (dict(rng=float("nan")), "data_range"), (dict(rng=float("inf")), "data_range"),
                     (dict(lam=-1.0), "lam"), (dict(lam=float("nan")), "lam"), (dict(n=3), "partials")):
        assert fwd(**kw) == -1, kw
        assert word in lib.lvt_last_error().decode(), (kw, lib.lvt_last_error())
    assert lib.lvt_ssim_loss_fwd(None, p, 2, 16, 16, 4, 3, p, p, 1.0, 0.5, p, 2, p, None) == -1
    assert lib.lvt_ssim_loss_fwd(ctypes.c_void_p((1 << 20) + 4), p, 2, 16, 16, 4, 3, p, p, 1.0, 0.5, p, 2, p, None) == -1
    assert lib.lvt_ssim_loss_finish(p, 3, 2, 16, 16, 3, 0.5, p, None) == -1
    assert lib.lvt_ssim_loss_finish(None, 2, 2, 16, 16, 3, 0.5, p, None) == -1
    for fn in (lib.lvt_mse_bwd_plus, lib.lvt_l1_bwd_plus):
        assert fn(p, p, 16, 16.0, 1.0, p, None, p, p, None, None) == -1       # the second operand pair is required
        assert fn(p, p, 16, 16.0, 1.0, p, p, None, p, None, None) == -1
        assert fn(p, p, 15, 16.0, 1.0, p, p, p, p, None, None) == -1


def test_wrappers_refuse_cpu_tensors():
    from lvt_amd.hip import binding as L, ew
    a = torch.zeros(1, 1, 12, 12, 4)
    with pytest.raises(L.LvtError):
        ew.ssim_loss_fwd(a, a, MEAN, STD, 1.0, 0.5)
    with pytest.raises(L.LvtError):
        ew.mse_bwd(a, a, 1.0, g_plus=torch.ones(1), plus=a)
