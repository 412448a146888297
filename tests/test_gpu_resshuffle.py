"""ResShuffleDecoder on the GPU: the pixel-shuffle kernels (csrc/shuffle.hip) against CPU torch, a conv / shuffle plan and the
stride-2 module against fp64 torch modules, the VQ-VAE with the decoder against fixture G29 (captured from the reference), the eval
fold, the max |.| records under AMAX_CHECK, bit reproducibility of training, the model surface and a short tools/train_net.py run.
Tolerances of the model-level checks are those of G6 / G26 (tests/test_gpu_norm.py); an engine launch is held to 2e-5 of its
output's max as in tests/test_gpu_engine.py."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import convcoders_cfg as CC
import seeded
import shuffle_cfg as SC
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5            # one engine launch (tests/test_gpu_engine.py)
ATOL = 2e-5           # G6


@pytest.fixture
def f16x2():
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    yield
    L.set_math_mode(before)


@pytest.fixture(params=["f16x2", "f32"])
def math_mode(request):
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode(request.param)
    yield request.param
    L.set_math_mode(before)


def _cl(x, cp=None):
    """(N,C,H,W) -> (N,H,W,Cp) channels-last on the device, channels zero-padded to a multiple of 4."""
    n, c, h, w = x.shape
    cp = cp or (c + 3) // 4 * 4
    out = torch.zeros(n, h, w, cp, dtype=x.dtype)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out.to(DEV)


def _nchw(y, c):
    return y.reshape(y.shape[0], y.shape[-3], y.shape[-2], y.shape[-1])[..., :c].permute(0, 3, 1, 2).cpu()


# ---- the kernels -----------------------------------------------------------------------------------------------------------
# N, H, W, C of the coarse side.  A thread owns one channel of a coarse pixel and the grid is capped at 8 x 256 workgroups of 256
# threads (524288 threads): (5, 32, 32, 128) is 655360 threads, 2560 workgroups, so the grid-stride loop runs a second round there.
# The last shape does the same with pad channels (37 carried as 40) and an odd width: 2 * 160 * 165 * 40 threads, four rounds.
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (1, 5, 7, 6), (3, 4, 4, 8), (2, 16, 16, 128), (5, 32, 32, 128), (2, 160, 165, 37)]
ACTS = ["", "relu", "tanh", "sigmoid"]
_ACT64 = {"": lambda t: t, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


assert all(n * h * w * c > 8 * 256 * 256 for n, h, w, c in SHAPES[-2:])


@functools.lru_cache(maxsize=None)
def _case(shape):
    """x (N,4C,H,W) with exact zeros sprinkled in, its shuffle in fp32 and fp64, and a fine-side gradient whose pad channels hold
    garbage (made once per shape)."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + c)
    x = torch.randn(n, 4 * c, h, w, generator=g)
    x[torch.rand(n, 4 * c, h, w, generator=g) < 0.05] = 0.0
    cp = (c + 3) // 4 * 4
    grad = torch.randn(n, cp, 2 * h, 2 * w, generator=g)
    if cp > c:
        grad[:, c:] = float("nan")
        grad[:, c:, ::2] = 1e30
    return dict(x=x, x_dev=_cl(x), ps=F.pixel_shuffle(x, 2), ps64=F.pixel_shuffle(x.double(), 2), grad=grad,
                unshuffled=F.pixel_unshuffle(grad[:, :c], 2))


def _raw_shuffle(x_dev, shape, flag):
    """lvt_pixel_shuffle2 at the C ABI into NaN-filled memory -> (rc, out)."""
    from lvt_amd.hip import binding as L
    n, h, w, c = shape
    out = torch.full((n, 2 * h, 2 * w, (max(c, 1) + 3) // 4 * 4), float("nan"), device=DEV)
    rc = L.lib().lvt_pixel_shuffle2(L.ptr(x_dev), n, h, w, c, flag, L.ptr(out), None, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_pixel_shuffle_against_torch(shape, act, f16x2):
    from lvt_amd.hip import binding as L, ew
    n, h, w, c = shape
    k = _case(shape)
    rc, raw = _raw_shuffle(k["x_dev"], shape, ew._SHUFFLE_ACTS[act])
    assert rc == 0
    assert not bool(torch.isnan(raw).any())                       # every element of the NaN-filled output was written
    assert not bool(raw[..., c:].any())                           # pads: exact zeros, sigmoid included
    out = ew.pixel_shuffle2(k["x_dev"], c, act)
    assert out.shape == (n, 2 * h, 2 * w, (c + 3) // 4 * 4) and torch.equal(out, raw)
    got = _nchw(out, c)
    if act == "":
        assert torch.equal(got, k["ps"])
    elif act == "relu":
        assert torch.equal(got, torch.relu(k["ps"]))
    else:
        err = rel_err(got, _ACT64[act](k["ps64"]))
        print("%s %s rel_err %.2e" % (shape, act, err))
        assert err < 1e-6
    assert float(L.amax_of(out)) >= float(out.abs().max())
    # 5-d frames (N,1,H,W,C), as the conv stacks carry them, and the flag form of convnet._act_flag (sigmoid with its pad count)
    assert torch.equal(ew.pixel_shuffle2(k["x_dev"].unsqueeze(1), c, act).squeeze(1), out)
    if act == "sigmoid":
        assert torch.equal(ew.pixel_shuffle2(k["x_dev"], c, L.EPI_SIGMOID | L.epi_pad((-c) % 4)), out)


@pytest.mark.parametrize("shape", SHAPES)
def test_unshuffle_inverts_the_shuffle_and_ignores_pads(shape, f16x2):
    from lvt_amd.hip import binding as L, ew
    n, h, w, c = shape
    k = _case(shape)
    back = ew.pixel_unshuffle2(ew.pixel_shuffle2(k["x_dev"], c), c)
    assert back.shape == k["x_dev"].shape and torch.equal(back, k["x_dev"])
    g_dev = _cl(k["grad"])
    out = ew.pixel_unshuffle2(g_dev, c)
    assert out.shape == (n, h, w, 4 * c)
    assert torch.equal(_nchw(out, 4 * c), k["unshuffled"])
    assert float(L.amax_of(out)) >= float(out.abs().max())       # the garbage of the pads is not in the record's way either
    assert float(L.amax_of(out)) < 1e3
    assert torch.equal(ew.pixel_unshuffle2(g_dev.unsqueeze(1), c).squeeze(1), out)


def test_shuffle_refusals():
    from lvt_amd.hip import binding as L, ew
    shape = (2, 3, 5, 3)
    k = _case(shape)
    for flag in (L.EPI_RELU | L.EPI_TANH, L.EPI_LEAKY, L.EPI_SIGMOID | L.epi_pad(1), L.EPI_BIAS, 3):
        rc, out = _raw_shuffle(k["x_dev"], shape, flag)
        assert rc == -1 and bool(torch.isnan(out).all()), flag
    rc, out = _raw_shuffle(k["x_dev"], (2, 3, 5, 0), 0)
    assert rc == -1 and bool(torch.isnan(out).all())
    g_dev = torch.zeros(2, 6, 10, 4, device=DEV)
    back = torch.full((2, 3, 5, 12), float("nan"), device=DEV)
    for dims in ((2, 3, 5, 0), (0, 3, 5, 3), (2, -1, 5, 3)):
        assert L.lib().lvt_pixel_unshuffle2(L.ptr(g_dev), *dims, L.ptr(back), None, L.stream_ptr()) == -1
    assert L.lib().lvt_pixel_unshuffle2(None, 2, 3, 5, 3, L.ptr(back), None, L.stream_ptr()) == -1
    assert L.lib().lvt_pixel_unshuffle2(g_dev.data_ptr() + 4, 2, 3, 5, 3, L.ptr(back), None, L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(back).all())
    with pytest.raises(L.LvtError, match="4 \\* C"):
        ew.pixel_shuffle2(k["x_dev"], 4)
    with pytest.raises(L.LvtError, match="act"):
        ew.pixel_shuffle2(k["x_dev"], 3, "leaky")
    with pytest.raises(L.LvtError, match="shuffle of C"):
        ew.pixel_unshuffle2(g_dev, 5)
    with pytest.raises(L.LvtError, match="frames only"):
        ew.pixel_shuffle2(torch.zeros(5, 12, device=DEV), 3)


# ---- fp64 twins of a plan --------------------------------------------------------------------------------------------------
def _twin_forward(seq, plan, outs, h):
    """fp64 forward through torch modules laid out like a stack's `layers`, layer by layer of its plan.  Every ReLU takes each
    element's branch from the sign of the GPU's own activation (outs[i], stored post-activation) instead of the sign of the fp64
    value, as tests/test_gpu_convcoders.py:_twin_forward does for LeakyReLU and for the same reason: the derivative jumps at 0,
    and an element within the engine's error of 0 is a valid reference for its own branch only.  The disagreements are checked to
    be exactly that: fp64 values within TOL of the layer's max of 0.  The activation is applied where the plan stores it, so the
    explicit (in-place) ReLU modules behind a layer are already done when the walk reaches them.
    -> (output, number of elements that took the GPU's branch against fp64's)."""
    state = {"i": -1, "flips": 0}

    def act(h):
        ly = plan[state["i"]]
        if ly.act == "relu":
            pos = _nchw(outs[state["i"]], ly.cout) > 0
            differ = pos != (h.detach() > 0)
            assert float(h.detach().abs()[differ].max() if differ.any() else 0.0) <= TOL * float(h.detach().abs().max())
            state["flips"] += int(differ.sum())
            return h * pos.double()
        return {"": lambda t: t, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[ly.act](h)

    def conv(m, h):
        state["i"] += 1
        assert plan[state["i"]].kind == "conv" and plan[state["i"]].norm == ""
        return m(h)

    for m in seq:
        if isinstance(m, nn.Conv2d):
            h = act(conv(m, h))
        elif isinstance(m, nn.PixelShuffle):
            state["i"] += 1
            assert plan[state["i"]].kind == "shuffle"
            h = act(m(h))
        elif type(m).__name__ == "ResBlock":
            t = act(conv(m.block[1], h))
            t = conv(m.block[3], t)
            assert plan[state["i"]].res_from >= 0
            h = act(h + t)
        else:
            assert isinstance(m, (nn.ReLU, nn.Tanh, nn.Sigmoid))
    assert state["i"] == len(plan) - 1
    return h, state["flips"]


def _plan_modules(seed):
    from lvt_amd.hip.convnet import Layer
    torch.manual_seed(seed)
    seq = nn.Sequential(nn.Conv2d(16, 32, 3, 1, 1), nn.PixelShuffle(2), nn.ReLU(), nn.Conv2d(8, 12, 3, 1, 1), nn.PixelShuffle(2),
                        nn.Tanh())
    k3 = ((1, 3, 3), (1, 1, 1), (0, 1, 1))
    plan = [Layer("conv", *k3, 16, 32), Layer.shuffle(8, "relu"), Layer("conv", *k3, 8, 12), Layer.shuffle(3, "tanh")]
    return seq, plan


def test_conv_shuffle_plan_against_fp64(math_mode):
    """conv(16 -> 32) -> shuffle(relu) -> conv(8 -> 12) -> shuffle(tanh) on 2 frames of 8 x 8 through stack_forward /
    stack_backward, against the same layers as torch modules in fp64 (see _twin_forward for the signs at the ReLU).
    Bound: an engine launch is within TOL = 2e-5 of its output's max and the errors of a chain add at worst linearly.  The chain
    has L = 6 engine launches: 2 forward convolutions, 2 weight-gradient and 2 data-gradient launches (the input gradient is
    asked for); the shuffles and the tanh backward move or scale fp32 values at 1e-7.  Output and every gradient: L x 2e-5 of
    its own max."""
    from lvt_amd.hip import convnet
    L_ = 6
    seq, plan = _plan_modules(29)
    g = torch.Generator().manual_seed(292)
    x = torch.randn(2, 16, 8, 8, generator=g)
    gy = torch.randn(2, 3, 32, 32, generator=g)
    params = [(m.weight.detach().to(DEV), m.bias.detach().to(DEV)) if isinstance(m, nn.Conv2d) else (None, None)
              for m in seq if isinstance(m, (nn.Conv2d, nn.PixelShuffle))]
    x_cl = _cl(x).unsqueeze(1)
    with torch.no_grad():
        outs, saved = convnet.stack_forward(plan, x_cl, params)
        assert [tuple(o.shape) for o in outs] == [(2, 1, 8, 8, 32), (2, 1, 16, 16, 8), (2, 1, 16, 16, 12), (2, 1, 32, 32, 4)]
        gx, grads, norm_grads = convnet.stack_backward(plan, x_cl, outs, saved, _cl(gy).unsqueeze(1), need_input_grad=True)
    assert norm_grads == [] and grads[1] == (None, None) and grads[3] == (None, None)
    assert not bool(outs[-1][..., 3:].any())
    twin = copy.deepcopy(seq).double()
    xd = x.double().requires_grad_(True)
    y, flips = _twin_forward(twin, plan, outs, xd)
    print("elements on the GPU's side of a ReLU kink against fp64's: %d" % flips)
    assert flips <= 5
    (y * gy.double()).sum().backward()
    err = rel_err(_nchw(outs[-1], 3), y.detach())
    print("output %.2e" % err)
    assert err < L_ * TOL
    err = rel_err(_nchw(gx, 16), xd.grad)
    print("input gradient %.2e" % err)
    assert err < L_ * TOL
    for i, m in ((0, twin[0]), (2, twin[3])):
        dw, db = grads[i]
        for name, got, want in (("weight", dw.view(m.weight.shape), m.weight.grad), ("bias", db, m.bias.grad)):
            err = rel_err(got, want)
            print("layer %d %s %.2e" % (i, name, err))
            assert err < L_ * TOL, (i, name)


def test_shuffle_behind_an_activation_is_refused(f16x2):
    from lvt_amd.hip import binding as L, convnet
    seq, plan = _plan_modules(29)
    plan[2].act = "relu"
    params = [(seq[0].weight.detach().to(DEV), seq[0].bias.detach().to(DEV)), (None, None),
              (seq[3].weight.detach().to(DEV), seq[3].bias.detach().to(DEV)), (None, None)]
    x_cl = torch.randn(2, 1, 8, 8, 16, device=DEV)
    with torch.no_grad():
        outs, saved = convnet.stack_forward(plan, x_cl, params)
        with pytest.raises(L.LvtError, match="pixel shuffle"):
            convnet.stack_backward(plan, x_cl, outs, saved, torch.randn(2, 1, 32, 32, 4, device=DEV))


def test_stride_2_module_against_fp64(math_mode):
    """ResShuffleDecoder(256, 64, 32, 3, "", False, 1, "tanh", stride=2) on 2 latent frames of 8 x 8 against its deep-copied
    `layers` in fp64 (the module tree is the reference's; _twin_forward walks it along the plan).
    The plan is conv3x3, ResBlock (conv3x3, conv1x1), conv3x3, shuffle(tanh): 4 forward, 4 weight-gradient and 4 data-gradient
    engine launches (the latent's gradient is asked for), L = 12; output and every gradient within L x 2e-5 of its own max."""
    from lvt_amd.hip import convnet
    from lvt_amd.modeling import convstack
    from lvt_amd.modeling.generator import ResShuffleDecoder
    L_ = 12
    torch.manual_seed(31)
    dec = ResShuffleDecoder(256, 64, 32, 3, "", False, 1, "tanh", stride=2).to(DEV)
    assert [ly.kind for ly in dec._plan] == ["conv", "conv", "conv", "conv", "shuffle"]
    g = torch.Generator().manual_seed(293)
    z = torch.randn(2, 256, 8, 8, generator=g)
    gy = torch.randn(2, 3, 16, 16, generator=g)
    zd = z.to(DEV).requires_grad_(True)
    y = dec(zd)
    assert y.shape == (2, 3, 16, 16)
    (y * gy.to(DEV)).sum().backward()
    with torch.no_grad():
        outs, _ = convnet.stack_forward(dec._plan, convstack.nchw_to_cl(z.to(DEV)), convstack.plan_params(dec._owners))
    twin = copy.deepcopy(dec.layers).cpu().double()
    for p in twin.parameters():
        p.grad = None
    z64 = z.double().requires_grad_(True)
    y64, flips = _twin_forward(twin, dec._plan, outs, z64)
    print("elements on the GPU's side of a ReLU kink against fp64's: %d" % flips)
    assert flips <= 5
    (y64 * gy.double()).sum().backward()
    err = rel_err(y.detach(), y64.detach())
    print("output %.2e" % err)
    assert err < L_ * TOL
    err = rel_err(zd.grad, z64.grad)
    print("latent gradient %.2e" % err)
    assert err < L_ * TOL
    n = 0
    for (k, p), (k2, q) in zip(dec.layers.named_parameters(), twin.named_parameters()):
        assert k == k2 and p.grad is not None
        err = rel_err(p.grad, q.grad)
        print("%-22s %.2e" % (k, err))
        assert err < L_ * TOL, k
        n += 1
    assert n == 8


# ---- G29: the VQ-VAE with ResShuffleDecoder against the reference --------------------------------------------------------------
def _g29_state(module, prefix, seed):
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


def shuffle_model(name, seed, scale=None, over=None):
    from lvt_amd.modeling import build_model
    from util_models import vqvae_cfg
    cfg = SC.apply(vqvae_cfg(DEV), dict(SC.overrides(name), **(over or {})))
    model = build_model(cfg)
    for part, pre in (("encoder", "enc."), ("generator", "dec.")):
        mod = getattr(model, part)
        missing, unexpected = mod.load_state_dict(_g29_state(mod, pre, seed), strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    cb = None
    if scale is not None:
        cb = seeded.seeded_codebook_state(seed, scale=scale)
        model.codebook.load_state_dict(cb)
    return model, cb


def _data(seed, n=4):
    return [{"image": seeded.seeded_input("g29.f%d" % i, (3, 64, 64), seed).numpy()} for i in range(n)]


def _check_step(model, g, name, pre, seed, rows):
    """One `supervised` forward + backward against the recording `pre` of the fixture (bounds: test_gpu_norm.py:_check_step)."""
    from lvt_amd.utils.events import EventStorage
    norm = SC.CONFIGS[name]["norm"]
    with EventStorage(0):
        losses = model(_data(seed), mode="supervised")
    sum(losses.values()).backward()
    lr, lc = float(losses["loss_reconstruction"]), float(losses["loss_commitment"])
    assert abs(lr - float(g[pre + "loss_reconstruction"])) < 1e-5 * float(g[pre + "loss_reconstruction"]), lr
    assert abs(lc - float(g[pre + "loss_commitment"])) < 2e-4 * float(g[pre + "loss_commitment"]), lc
    sub = ".0" if norm else ""
    params = dict(model.generator.named_parameters())
    for key, pname in (("dec0", "layers.0%s.weight" % sub), ("dec4", "layers.4%s.weight" % sub), ("dec7", "layers.7.weight")):
        assert tuple(g[pre + "grad." + key].shape) == (rows,) + tuple(params[pname].shape[1:])
        assert rel_err(params[pname].grad[:rows], g[pre + "grad." + key]) < 5e-3, key
    assert rel_err(params["layers.7.bias"].grad, g[pre + "grad.dec7.bias"]) < 5e-3
    if norm:
        for t in ("weight", "bias"):
            assert rel_err(params["layers.4.1." + t].grad, g[pre + "grad.dec4n." + t]) < 5e-3, t


def _run_g29(golden, name):
    g = golden("g29_res_shuffle")
    seed, rows, tag = int(g["seed"]), int(g["rows"]), name + "."
    c = SC.CONFIGS[name]
    assert float(g[tag + "clear_share"]) >= 0.98 and float(g[tag + "eval.clear"].float().mean()) >= 0.98
    model, cb = shuffle_model(name, seed, float(g[tag + "scale"]))
    model.train()
    _check_step(model, g, name, tag + "train.", seed, rows)
    seen = 0
    for part in ("encoder", "generator"):
        for k, v in getattr(model, part).state_dict().items():
            key = tag + "after.%s.%s" % (part, k)
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(g[key]) == 1, k
            elif k.endswith("running_mean") or k.endswith("running_var"):
                assert rel_err(v, g[key]) < 1e-5, k
                seen += 1
    assert seen == (2 * (7 + 6) if c["norm"] else 0)
    # eval after the step: latents on the clear rows; reconstructions outside the receptive field of a differing code
    model.eval()
    model.codebook.load_state_dict(cb)
    with torch.no_grad():
        out = model(_data(seed), mode="inference")
        dec = model.decode(g[tag + "eval.latent"].long()).cpu()
    lat = torch.stack([o["latent"] for o in out]).cpu()
    rec = torch.stack([o["reconstruction"] for o in out]).cpu()
    want, clear = g[tag + "eval.latent"].long(), g[tag + "eval.clear"]
    assert lat.shape == want.shape == (4, 4, 16, 16)
    assert torch.equal(lat[clear], want[clear])
    # a code at latent row y reaches rows y-4 .. y+4 of the 16 x 16 grid (four 3x3 convolutions), 2y-8 .. 2y+9 of the 32 x 32
    # grid behind the first shuffle, 2y-9 .. 2y+10 behind the 3x3 convolution there, pixel rows 4y-18 .. 4y+21 of the image
    keep = torch.ones(4, 64, 64, dtype=torch.bool)
    for t, i, y, x in (lat != want).nonzero().tolist():
        keep[t, max(0, 4 * y - 18):4 * y + 22, max(0, 4 * x - 18):4 * x + 22] = False
    share = float(keep.float().mean())
    print("%s: %d latents differ, %.3f of the pixels compared" % (name, int((lat != want).sum()), share))
    assert share >= 0.8
    # the fixture stores the reference's decode; its inference reconstruction IS decode * std + mean in fp32 (asserted bit for
    # bit by make_golden_shuffle.py when the fixture is made)
    ref = g[tag + "eval.decode"] * c["std"] + c["mean"]
    err = float((rec - ref).abs()[keep[:, None].expand_as(rec)].max() / ref.abs().max())
    print("%s: reconstruction %.2e" % (name, err))
    assert err < ATOL
    # decode of the FIXTURE's latents: no latent can differ, every pixel counts
    assert dec.shape == (4, 3, 64, 64)
    err = rel_err(dec, g[tag + "eval.decode"])
    print("%s: decode %.2e" % (name, err))
    assert err < ATOL
    # eval with gradients (no fold: running statistics with their backward).  Without a norm the reference's eval step equals its
    # train step bit for bit, and the fixture says so instead of storing it twice
    model.zero_grad()
    model.codebook.load_state_dict(cb)
    same = int(g[tag + "evalgrad.same_as_train"])
    assert same == (0 if c["norm"] else 1)
    _check_step(model, g, name, tag + ("train." if same else "evalgrad."), seed, rows)
    return model, cb


@pytest.mark.parametrize("name", SC.NAMES)
def test_g29_against_reference(golden, name, math_mode):
    _run_g29(golden, name)


def test_g29_plain_under_amax_check(golden, f16x2):
    """Every max |.| record that an engine launch of the step reads -- those the shuffle kernels wrote included -- is verified
    against its tensor."""
    from lvt_amd.hip import binding as L
    assert L.get_math_mode() == "f16x2"
    old, L.AMAX_CHECK = L.AMAX_CHECK, True
    try:
        _run_g29(golden, "p")
    finally:
        L.AMAX_CHECK = old


def test_g29_eval_fold_runs_no_norm_kernels_and_matches_unfolded(golden, f16x2, monkeypatch):
    from lvt_amd.hip import norm as BN
    g = golden("g29_res_shuffle")
    seed = int(g["seed"])
    model, _ = shuffle_model("b", seed, float(g["b.scale"]))
    model.eval()
    x = torch.stack([torch.from_numpy(d["image"]) for d in _data(seed)]).to(DEV)
    xin = model.normalizer(x)
    with torch.enable_grad():
        z_ref = model.encoder(xin.clone().requires_grad_(True)).detach()
        r_ref = model.generator(z_ref.clone().requires_grad_(True)).detach()
    calls = []
    for fname in ("stats", "finalize", "apply", "bwd_reduce", "bwd_apply", "fold"):
        fn = getattr(BN, fname)
        monkeypatch.setattr(BN, fname, lambda *a, _f=fn, _n=fname, **k: (calls.append(_n), _f(*a, **k))[1])
    with torch.no_grad():
        z = model.encoder(xin)
        r = model.generator(z)
    assert calls == ["fold", "fold"]                # one fold launch per stack, then the plain stack's kernels
    assert rel_err(z, z_ref) < 1e-5 and rel_err(r, r_ref) < 1e-5


def test_training_trajectory_bit_reproducible():
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.events import EventStorage
    from util_models import vqvae_cfg

    def run():
        cfg = SC.apply(vqvae_cfg(DEV), SC.overrides("b"))
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
    assert sa.keys() == sb.keys() and "generator.layers.7.weight" in sa
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert int(sa["generator.layers.4.1.num_batches_tracked"]) == 3


# ---- model surface -----------------------------------------------------------------------------------------------------------
def test_autoencoder_with_conv_encoder_in_front_trains_a_step(f16x2):
    from lvt_amd.modeling import build_model
    from lvt_amd.modeling.encoder import ConvEncoder
    from lvt_amd.modeling.generator import ResShuffleDecoder
    from lvt_amd.utils.events import EventStorage
    from util_models import vqvae_cfg
    over = dict(CC.overrides("a"), **{"MODEL.GENERATOR.NAME": "ResShuffleDecoder", "MODEL.GENERATOR.NF": 64,
                                      "MODEL.GENERATOR.RES_CHANNELS": 32})
    cfg = CC.apply(vqvae_cfg(DEV), over)
    cfg.MODEL.META_ARCHITECTURE = "AutoEncoderModel"
    torch.manual_seed(3)
    ae = build_model(cfg)
    assert isinstance(ae.encoder, ConvEncoder) and isinstance(ae.generator, ResShuffleDecoder)
    ae.train()
    with EventStorage(0):
        loss = ae(_data(2929), mode="supervised")
    assert list(loss) == ["loss_ae_mse"] and bool(torch.isfinite(loss["loss_ae_mse"]))
    loss["loss_ae_mse"].backward()
    for k, p in list(ae.encoder.named_parameters()) + list(ae.generator.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


def test_decode_of_codes_is_the_generator_on_their_embeddings(golden, math_mode):
    """`vqvae.decode(codes)` as VTSampler calls it (eval, no grad, (T, nc, h, w) codes) against the gather and the generator
    composed by hand.  Both run the decoder's 6 engine launches on the same values: bit for bit in f32 arithmetic.  In f16x2
    arithmetic the two routes may hand the first launch different (valid) upper bounds of max |z_q|, which scale its operand, so
    there the outputs are held to the launches' bound."""
    g = golden("g29_res_shuffle")
    seed = int(g["seed"])
    model, _ = shuffle_model("p", seed, float(g["p.scale"]))
    model.eval()
    codes = torch.randint(0, 512, (3, 4, 16, 16), generator=torch.Generator().manual_seed(7)).to(DEV)
    with torch.no_grad():
        got = model.decode(codes)
        emb = torch.cat([model.codebook.ve[i].embedding.weight[codes[:, i]] for i in range(4)], dim=-1)      # (T, h, w, 256)
        want = model.generator(emb.permute(0, 3, 1, 2).contiguous())
    assert got.shape == want.shape == (3, 3, 64, 64)
    if math_mode == "f32":
        assert torch.equal(got, want)
    else:
        assert rel_err(got, want) < 6 * TOL


def test_train_net_runs_the_shuffle_decoder(tmp_path):
    out = str(tmp_path / "vq")
    r = subprocess.run([sys.executable, "tools/train_net.py", "--config-file", "configs/vqvae/PR-DVQVAE2.yaml", "--synthetic",
                        "--max-iter", "3", "OUTPUT_DIR", out, "SOLVER.IMS_PER_BATCH", "4", "SOLVER.MAX_ITER", "3",
                        "MODEL.GENERATOR.NAME", "ResShuffleDecoder"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "loss_reconstruction" in r.stdout + r.stderr
    ck = torch.load(os.path.join(out, "netG", "model_final.pth"))
    assert tuple(ck["model"]["layers.7.weight"].shape) == (12, 128, 3, 3)
