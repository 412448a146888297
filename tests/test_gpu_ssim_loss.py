"""The SSIM term of the reconstruction loss on the GPU (csrc/ssim_loss.hip, LOSS.SSIM.LAMBDA): the kernel against
fp64 autograd of the plain-torch rule (evaluation/quality.py ssim_loss_reference), the merged backward launch
(lvt_mse_bwd_plus / lvt_l1_bwd_plus), PR-DVQVAE2 and AutoEncoderModel with the term on, off-is-off, determinism and a short
tools/train_net.py run.

Tolerance of every comparison with fp64: the yardstick err_t is computed here, on the CPU, from the same inputs -- the error of plain
fp32 torch autograd of the rule against the fp64 gradient g64, relative to max |g64| -- and the kernel's error in the same measure
must be <= max(4 err_t, 32 * 2^-24): the factor 4 because both sides are fp32 evaluations in different summation orders, the floor
for the rounding of the ~30 fp32 operations of two 11-tap passes and a ratio.  The loss value: the same rule with floor 2^-22."""
import os
import subprocess
import sys

import pytest
import torch

import seeded
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [0.4, 0.5, 0.6], [0.2, 0.25, 0.5]
LAM = 0.5
SHAPES = [(1, 1, 11, 11), (2, 3, 11, 43), (3, 3, 13, 37), (1, 3, 27, 75), (2, 4, 16, 16), (1, 6, 12, 12), (2, 3, 64, 64)]
CLASSES = ["noise", "smooth_noise_0.05", "smooth_noise_1e-3", "bright_flat", "out_of_range", "L255", "equal"]


def _tables(C, L=1.0):
    mean = [(MEAN * 2)[c] * L for c in range(C)]
    std = [(STD * 2)[c] * L for c in range(C)]
    return mean, std


def _normalise(u, mean, std):
    """pixel space (fp64) -> the network's normalised space, rounded to fp32: what the kernel and every reference start from."""
    C = u.shape[1]
    m, s = torch.tensor(mean, dtype=torch.float64).view(1, C, 1, 1), torch.tensor(std, dtype=torch.float64).view(1, C, 1, 1)
    return ((u - m) / s).float()


def make_inputs(cls, shape, seed=0):
    """-> (xt, x, mean, std, L): fp32 normalised (F, C, H, W) reconstruction and target of one input class."""
    g = torch.Generator().manual_seed(seed)
    F, C, H, W = shape
    r = lambda: torch.rand(shape, generator=g, dtype=torch.float64)  # noqa: E731
    n = lambda: torch.randn(shape, generator=g, dtype=torch.float64)  # noqa: E731
    L = 255.0 if cls == "L255" else 1.0
    mean, std = _tables(C, L)
    if cls in ("noise", "L255"):
        ut, u = L * r(), L * r()
    elif cls.startswith("smooth_noise_"):
        big = torch.rand(F, C, H + 4, W + 4, generator=g, dtype=torch.float64)
        u = torch.nn.functional.avg_pool2d(big, 5, stride=1)
        ut = u + float(cls.rsplit("_", 1)[1]) * n()
    elif cls == "bright_flat":
        ut, u = 0.9 + 1e-3 * n(), 0.9 + 1e-3 * n()
    elif cls == "out_of_range":
        ut, u = 3 * r() - 1, r()
    elif cls == "equal":
        u = torch.nn.functional.avg_pool2d(torch.rand(F, C, H + 4, W + 4, generator=g, dtype=torch.float64), 5, stride=1)
        ut = u
    else:
        raise KeyError(cls)
    return _normalise(ut, mean, std), _normalise(u, mean, std), mean, std, L


_REF = {}


def reference(cls, shape):
    """Computed once per (class, shape) and left unchanged: inputs, fp64 loss and gradient, and the fp32 torch yardstick."""
    key = (cls, shape)
    if key not in _REF:
        from lvt_amd.evaluation import ssim_loss_reference
        xt, x, mean, std, L = make_inputs(cls, shape)
        a = xt.double().requires_grad_(True)
        l64 = ssim_loss_reference(a, x.double(), mean, std, L, LAM)
        g64, = torch.autograd.grad(l64, a)
        b = xt.clone().requires_grad_(True)
        l32 = ssim_loss_reference(b, x, mean, std, L, LAM)
        g32, = torch.autograd.grad(l32, b)
        _REF[key] = dict(xt=xt, x=x, mean=mean, std=std, L=L, l64=float(l64.detach()), g64=g64, l32=float(l32.detach()), g32=g32)
    return _REF[key]


def to_cl(t):
    from lvt_amd.modeling import convstack
    return convstack.nchw_to_cl(t.to(DEV).contiguous())


def from_cl(t, C):
    return t.detach().cpu()[:, 0, :, :, :C].permute(0, 3, 1, 2).contiguous()


def run_kernel(ref, want_grad=True):
    from lvt_amd.hip import ew
    mean = torch.tensor(ref["mean"], dtype=torch.float32, device=DEV)
    std = torch.tensor(ref["std"], dtype=torch.float32, device=DEV)
    return ew.ssim_loss_fwd(to_cl(ref["xt"]), to_cl(ref["x"]), mean, std, ref["L"], LAM, want_grad=want_grad)


def check_against_fp64(ref, loss, G, tag):
    C = ref["xt"].shape[1]
    g64 = ref["g64"]
    scale = float(g64.abs().max())
    err_t = float((ref["g32"].double() - g64).abs().max()) / scale
    err_k = float((from_cl(G, C).double() - g64).abs().max()) / scale
    lerr_t, lerr_k = abs(ref["l32"] - ref["l64"]), abs(float(loss) - ref["l64"])
    print("%s: gradient err_kernel %.3e (err_t %.3e), loss err_kernel %.3e (err_t %.3e), loss %.8f" % (tag, err_k, err_t, lerr_k, lerr_t, ref["l64"]))
    assert err_k <= max(4 * err_t, 32 * 2.0 ** -24), (tag, err_k, err_t)
    assert lerr_k <= max(4 * lerr_t, 2.0 ** -22), (tag, lerr_k, lerr_t)
    assert torch.equal(G.cpu()[..., C:], torch.zeros_like(G.cpu()[..., C:]))             # pad channels exactly 0


# ---- the kernel against fp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_shapes_against_fp64(shape):
    ref = reference("noise", shape)
    loss, G = run_kernel(ref)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and G.shape == to_cl(ref["xt"]).shape
    check_against_fp64(ref, loss, G, "noise %s" % (shape,))


@pytest.mark.parametrize("cls", CLASSES[:-1])
def test_kernel_input_classes_against_fp64(cls):
    ref = reference(cls, SHAPES[-1])
    loss, G = run_kernel(ref)
    check_against_fp64(ref, loss, G, cls)


def test_bitwise_equal_frames_give_zero():
    """Loss exactly 0; the gradient at most 4 times the rounding residue fp32 torch autograd leaves on the same frames."""
    ref = reference("equal", SHAPES[-1])
    assert torch.equal(ref["xt"], ref["x"])
    loss, G = run_kernel(ref)
    print("equal frames: loss %r, max |G| %.3e, fp32 torch autograd leaves %.3e" % (float(loss), float(G.abs().max()), float(ref["g32"].abs().max())))
    assert float(loss) == 0.0
    assert float(G.abs().max()) <= 4 * float(ref["g32"].abs().max())


def test_two_runs_give_equal_bits_and_forward_only_gives_the_same_loss():
    for cls, shape in (("noise", SHAPES[3]), ("smooth_noise_0.05", SHAPES[-1]), ("noise", SHAPES[5])):
        ref = reference(cls, shape)
        (l1, g1), (l2, g2) = run_kernel(ref), run_kernel(ref)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)
        l3, g3 = run_kernel(ref, want_grad=False)
        assert g3 is None and torch.equal(l1, l3)


def test_refusals_launch_nothing():
    from lvt_amd.hip import binding as L, ew
    ok = torch.zeros(2, 1, 12, 12, 4, device=DEV)
    mean, std = torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)
    bad = [lambda: ew.ssim_loss_fwd(ok[:, :, :10].contiguous(), ok[:, :, :10].contiguous(), mean, std, 1.0, LAM),     # H < 11
           lambda: ew.ssim_loss_fwd(ok[:, :, :, :10].contiguous(), ok[:, :, :, :10].contiguous(), mean, std, 1.0, LAM),   # W < 11
           lambda: ew.ssim_loss_fwd(ok, ok[:1], mean, std, 1.0, LAM),                                     # shapes differ
           lambda: ew.ssim_loss_fwd(ok.double(), ok.double(), mean, std, 1.0, LAM),                       # not fp32
           lambda: ew.ssim_loss_fwd(ok, ok.half(), mean, std, 1.0, LAM),
           lambda: ew.ssim_loss_fwd(ok.cpu(), ok.cpu(), mean, std, 1.0, LAM),                             # CPU tensors
           lambda: ew.ssim_loss_fwd(ok, ok.cpu(), mean, std, 1.0, LAM),
           lambda: ew.ssim_loss_fwd(ok, ok, mean, std, 0.0, LAM),                                         # data_range
           lambda: ew.ssim_loss_fwd(ok, ok, mean, std, -1.0, LAM),
           lambda: ew.ssim_loss_fwd(ok, ok, mean, std, float("nan"), LAM),
           lambda: ew.ssim_loss_fwd(ok, ok, mean, std, float("inf"), LAM),
           lambda: ew.ssim_loss_fwd(ok, ok, torch.ones(5, device=DEV), torch.ones(5, device=DEV), 1.0, LAM),      # len(mean) != C
           lambda: ew.ssim_loss_fwd(ok, ok, mean, std[:2], 1.0, LAM),
           lambda: ew.ssim_loss_fwd(ok, ok, MEAN + [0.5, 0.5], STD + [0.5, 0.5], 1.0, LAM)]
    lib = L.lib()
    launched = []
    real_fwd, real_fin = lib.lvt_ssim_loss_fwd, lib.lvt_ssim_loss_finish
    try:
        lib.lvt_ssim_loss_fwd = lambda *a: (launched.append("fwd"), real_fwd(*a))[1]
        lib.lvt_ssim_loss_finish = lambda *a: (launched.append("finish"), real_fin(*a))[1]
        for i, call in enumerate(bad):
            with pytest.raises(L.LvtError):
                call()
            assert not launched, i
        ew.ssim_loss_fwd(ok, ok, mean, std, 1.0, LAM)
        assert launched == ["fwd", "finish"]
    finally:
        lib.lvt_ssim_loss_fwd, lib.lvt_ssim_loss_finish = real_fwd, real_fin


# ---- the merged backward launch ------------------------------------------------------------------------------------------------
@pytest.fixture(params=["f16x2", "f32"])
def math_mode(request):
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode(request.param)
    yield request.param
    L.set_math_mode(before)


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_plus_launch_scales_its_halves_independently(l1, math_mode):
    """out = g_rec c (a - b | sign) + g_ssim G.  Each element is a difference, two products and one fused multiply-add of fp32
    values, c = 2 scale / denom rounded once: at most 6 roundings of 2^-24 of the two terms' magnitudes.  With one of the two
    device scalars zero the launch gives the other half's bits exactly."""
    from lvt_amd.hip import binding as L, ew
    g = torch.Generator().manual_seed(7)
    shape = (3, 1, 13, 37, 4)
    a, b, G = (torch.randn(shape, generator=g) for _ in range(3))
    for t in (a, b, G):
        t[..., 3] = 0.0
    b[0, 0, :5] = a[0, 0, :5]                                               # equal elements: sign(0) = 0 in the l1 form
    ad, bd, Gd = a.to(DEV), b.to(DEV), G.to(DEV)
    denom, scale = float(a.numel() // 4 * 3), 0.75
    g_rec, g_ssim = torch.tensor([1.7], device=DEV), torch.tensor([0.37], device=DEV)
    out = ew.mse_bwd(ad, bd, denom, scale, gout=g_rec, l1=l1, g_plus=g_ssim, plus=Gd)
    d = a.double() - b.double()
    t1 = 1.7 * (scale / denom * torch.sign(d) if l1 else 2 * scale / denom * d)
    t2 = 0.37 * G.double()
    o = out.cpu()
    assert bool(((o.double() - (t1 + t2)).abs() <= 6 * 2.0 ** -24 * (t1.abs() + t2.abs()) + 1e-45).all())
    assert torch.equal(o[..., 3], torch.zeros_like(o[..., 3]))            # pad channels of the merged gradient exactly 0
    if math_mode == "f16x2":
        assert float(L.amax_of(out)) >= float(out.abs().max()) > 0
    zero = torch.zeros(1, device=DEV)
    assert torch.equal(ew.mse_bwd(ad, bd, denom, scale, gout=g_rec, l1=l1, g_plus=zero, plus=Gd), ew.mse_bwd(ad, bd, denom, scale, gout=g_rec, l1=l1))
    assert torch.equal(ew.mse_bwd(ad, bd, denom, scale, gout=zero, l1=l1, g_plus=g_ssim, plus=Gd), g_ssim * Gd)
    assert torch.equal(ew.mse_bwd(ad, bd, denom, scale, gout=g_rec, l1=l1, g_plus=g_ssim, plus=Gd), out)      # two runs, equal bits
    with pytest.raises(L.LvtError):
        ew.mse_bwd(ad, bd, denom, scale, gout=g_rec, l1=l1, plus=Gd)
    with pytest.raises(L.LvtError):
        ew.mse_bwd(ad, bd, denom, scale, gout=g_rec, l1=l1, g_plus=g_ssim, plus=Gd[:1])


# ---- model level ---------------------------------------------------------------------------------------------------------------
SEED = 11


def _cfg(lam=None, arch=None, mode=None):
    from util_models import vqvae_cfg
    cfg = vqvae_cfg(DEV)
    if lam is not None:
        cfg.LOSS.SSIM.LAMBDA = lam
    if arch is not None:
        cfg.MODEL.META_ARCHITECTURE = arch
    if mode is not None:
        cfg.LOSS.PIXEL.MODE = mode
    return cfg


def _vqvae(lam=None, mode=None):
    from lvt_amd.modeling import build_model
    model = build_model(_cfg(lam, mode=mode))
    model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, SEED, "enc."))
    model.generator.load_state_dict(seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, SEED, "dec."))
    model.codebook.load_state_dict(seeded.seeded_codebook_state(SEED, scale=0.05))
    model.train()
    return model


def _frames(n=4):
    return torch.stack([seeded.seeded_input("ssim.f%d" % i, (3, 64, 64), SEED) for i in range(n)])


def _total_reference(x_tilde, x, cfg, pixel_scale, l1, dtype):
    """pixel + ssim of the returned channels-last tensors in `dtype` on the CPU -> (loss_pixel, loss_ssim, d(sum)/d x_tilde)."""
    from lvt_amd.evaluation import ssim_loss_reference
    C = len(cfg.MODEL.PIXEL_MEAN)
    a = from_cl(x_tilde, C).to(dtype).requires_grad_(True)
    b = from_cl(x, C).to(dtype)
    pix = pixel_scale * ((a - b).abs().mean() if l1 else ((a - b) ** 2).mean())
    ssim = ssim_loss_reference(a, b, list(cfg.MODEL.PIXEL_MEAN), list(cfg.MODEL.PIXEL_STD), 1.0 if cfg.INPUT.SCALE_TO_ZEROONE else 255.0,
                               cfg.LOSS.SSIM.LAMBDA)
    g, = torch.autograd.grad(pix + ssim, a)
    return float(pix), float(ssim), g


def _check_model_step(losses, x, x_tilde, cfg, pixel_scale, l1, key, tag):
    C = len(cfg.MODEL.PIXEL_MEAN)
    p64, s64, g64 = _total_reference(x_tilde, x, cfg, pixel_scale, l1, torch.float64)
    p32, s32, g32 = _total_reference(x_tilde, x, cfg, pixel_scale, l1, torch.float32)
    scale = float(g64.abs().max())
    err_t = float((g32.double() - g64).abs().max()) / scale
    grad = x_tilde.grad
    err_k = float((from_cl(grad, C).double() - g64).abs().max()) / scale
    lerr_t, lerr_k = abs(s32 - s64), abs(float(losses["loss_ssim"]) - s64)
    print("%s: d(pixel + ssim)/d x_tilde err_kernel %.3e (err_t %.3e); loss_ssim %.8f err_kernel %.3e (err_t %.3e)"
          % (tag, err_k, err_t, s64, lerr_k, lerr_t))
    assert err_k <= max(4 * err_t, 32 * 2.0 ** -24), (tag, err_k, err_t)
    assert lerr_k <= max(4 * lerr_t, 2.0 ** -22), (tag, lerr_k, lerr_t)
    assert abs(float(losses[key]) - p64) <= 1e-5 * p64
    assert torch.equal(grad.cpu()[..., C:], torch.zeros_like(grad.cpu()[..., C:]))


def _vqvae_step(mode="l2"):
    from lvt_amd.hip import binding as L
    model = _vqvae(LAM, mode)
    xin = model.normalizer(_frames().to(DEV))
    L.bump_epoch()
    losses, x, x_tilde = model.compute_supervised_loss(xin, return_x=True)
    assert list(losses) == ["loss_reconstruction", "loss_ssim", "loss_commitment"]
    x_tilde.retain_grad()
    sum(losses.values()).backward()
    if L.f16x2():
        assert float(L.amax_of(x_tilde.grad)) >= float(x_tilde.grad.abs().max()) > 0
    _check_model_step(losses, x, x_tilde, model.cfg, model.cfg.LOSS.PIXEL.LAMBDA, mode == "l1", "loss_reconstruction", "VQVAEModel " + mode)
    g = model.encoder.layers[0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


@pytest.mark.parametrize("mode", ["l2", "l1"])
def test_vqvae_step_against_fp64(math_mode, mode):
    _vqvae_step(mode)


def test_vqvae_step_under_amax_check():
    from lvt_amd.hip import binding as L
    assert L.get_math_mode() == "f16x2"
    old, L.AMAX_CHECK = L.AMAX_CHECK, True
    try:
        _vqvae_step()
    finally:
        L.AMAX_CHECK = old


def test_autoencoder_step_against_fp64(math_mode):
    from lvt_amd.hip import binding as L
    from lvt_amd.modeling import build_model
    torch.manual_seed(3)
    model = build_model(_cfg(LAM, arch="AutoEncoderModel"))
    model.train()
    seen = []
    inner = model.reconstruction_loss.forward

    def spy(inp, tgt, **kw):
        if inp.requires_grad:
            inp.retain_grad()
        seen.append((inp, tgt))
        return inner(inp, tgt, **kw)

    model.reconstruction_loss.forward = spy
    xin = model.normalizer(_frames(2).to(DEV))
    L.bump_epoch()
    losses = model.compute_supervised_loss(xin)
    assert list(losses) == ["loss_ae_mse", "loss_ssim"]
    sum(losses.values()).backward()
    (x_tilde, x), = seen
    _check_model_step(losses, x, x_tilde, model.cfg, 1.0, False, "loss_ae_mse", "AutoEncoderModel")
    with torch.no_grad():                                                  # eval: the forward without a gradient buffer, same rule
        ev = model.compute_supervised_loss(xin)
    assert torch.equal(ev["loss_ssim"], losses["loss_ssim"])


# ---- off is off ----------------------------------------------------------------------------------------------------------------
def _train_step(model):
    from lvt_amd.utils.events import EventStorage
    data = [{"image": f.numpy()} for f in _frames()]
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    return ({k: v.detach().clone() for k, v in losses.items()}, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})


def test_lambda_zero_is_the_step_without_the_key(monkeypatch):
    from lvt_amd.hip import ew
    from lvt_amd.modeling.loss import loss as loss_mod
    calls = []
    for name in ("ssim_loss_fwd", "mse_bwd"):
        fn = getattr(ew, name)
        monkeypatch.setattr(ew, name, lambda *a, _f=fn, _n=name, **k: (calls.append((_n, k.get("plus") is not None)), _f(*a, **k))[1])
    real = loss_mod._PixelSsimFn.apply
    monkeypatch.setattr(loss_mod._PixelSsimFn, "apply", staticmethod(lambda *a: (calls.append(("node", True)), real(*a))[1]))
    la, ga = _train_step(_vqvae(None))
    plain = list(calls)
    del calls[:]
    lb, gb = _train_step(_vqvae(0.0))
    assert calls == plain and plain and all(n == "mse_bwd" and not plus for n, plus in plain)
    assert list(la) == list(lb) == ["loss_reconstruction", "loss_commitment"]
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    assert ga.keys() == gb.keys() and len(ga) > 10
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    del calls[:]
    lc, _ = _train_step(_vqvae(LAM))                                       # and on: one node, one kernel pair, one merged backward
    assert calls.count(("node", True)) == 1 and calls.count(("ssim_loss_fwd", False)) == 1 and calls.count(("mse_bwd", True)) == 1
    assert torch.equal(lc["loss_reconstruction"], la["loss_reconstruction"]) and float(lc["loss_ssim"]) > 0


def test_training_trajectory_bit_reproducible():
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.events import EventStorage

    def run():
        torch.manual_seed(11)
        model = build_model(_cfg(LAM))
        model.train()
        opts, _ = model.configure_optimizers_and_checkpointers()
        g = torch.Generator().manual_seed(5)
        losses = []
        for i in range(3):
            frames = torch.rand(4, 3, 64, 64, generator=g)
            with EventStorage(i):
                ls = model([{"image": f.numpy()} for f in frames], mode="supervised")
            sum(ls.values()).backward()
            for o in opts:
                o["optimizer"].step()
            for o in opts:
                o["optimizer"].zero_grad()
            losses.append({k: float(v.detach()) for k, v in ls.items()})
        return losses, {n: t.detach().clone() for n, t in list(model.named_parameters()) + list(model.named_buffers())}

    (la, sa), (lb, sb) = run(), run()
    assert la == lb and all("loss_ssim" in d and d["loss_ssim"] > 0 for d in la)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_train_net_logs_the_term(tmp_path):
    out = str(tmp_path / "vq")
    r = subprocess.run([sys.executable, "tools/train_net.py", "--config-file", "configs/vqvae/PR-DVQVAE2.yaml", "--synthetic",
                        "--max-iter", "3", "OUTPUT_DIR", out, "SOLVER.IMS_PER_BATCH", "4", "SOLVER.MAX_ITER", "3",
                        "LOSS.SSIM.LAMBDA", "0.5"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "loss_ssim" in r.stdout + r.stderr
    assert os.path.exists(os.path.join(out, "netG", "model_final.pth"))
