"""ConvEncoder / ConvDecoder on the GPU: the 2x2 pool / upsample kernels (csrc/resample.hip) and the engine's LeakyReLU epilogue
and mask against fp64 CPU torch, the VQ-VAE built from the two stacks against fixture G28 (captured from the reference), a
whole-model gradient check against fp64 torch modules, the C-ABI call sequence of a Res stack (unchanged by the parameter-less
layers the executor learned), and a short tools/train_net.py run.  Tolerances of the model-level checks are those of G5 / G6
(tests/test_gpu_vqvae.py, tests/test_gpu_norm.py); the engine bounds are those of tests/test_gpu_engine.py."""
import copy
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convcoders_cfg as CC
import seeded
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5            # tests/test_gpu_engine.py: the ReLU epilogues at the same shapes
ATOL = 2e-5           # G6


@pytest.fixture
def f16x2():
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode("f16x2")
    yield
    L.set_math_mode(before)


def _cl(x, cp=None):
    """(N,C,H,W) -> (N,H,W,Cp) channels-last on the device, channels zero-padded to a multiple of 4."""
    n, c, h, w = x.shape
    cp = cp or (c + 3) // 4 * 4
    out = torch.zeros(n, h, w, cp)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out.to(DEV)


def _nchw(y, c):
    return y.reshape(y.shape[0], y.shape[-3], y.shape[-2], y.shape[-1])[..., :c].permute(0, 3, 1, 2).cpu()


def _leaky_grad(m):
    """torch's leaky_relu_backward factor from the saved output: an exact 0 takes the 0.2 branch."""
    return torch.where(m > 0, 1.0, 0.2).double()


# ---- resample kernels ------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 2, 3), (3, 6, 10, 32), (2, 64, 64, 3), (5, 16, 16, 256), (1, 34, 2, 68)]          # N, H, W, C


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and fp64 references of one shape, made once: x (N,C,H,W) with exact zeros sprinkled in; its 2x2 average pool and
    nearest upsample; gradients g_small (N,C,H/2,W/2) and g_big (N,C,2H,2W)."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + c)
    x = torch.randn(n, c, h, w, generator=g)
    x[torch.rand(n, c, h, w, generator=g) < 0.05] = 0.0
    return dict(x=x, pool=F.avg_pool2d(x.double(), 2), up=F.interpolate(x.double(), scale_factor=2, mode="nearest"),
                g_small=torch.randn(n, c, h // 2, w // 2, generator=g), g_big=torch.randn(n, c, 2 * h, 2 * w, generator=g))


def _pads_zero(y, c):
    return not bool(y[..., c:].any())


@pytest.mark.parametrize("shape", SHAPES)
def test_upsample_is_a_bit_exact_copy(shape, f16x2):
    from lvt_amd.hip import binding as L, ew
    c = shape[3]
    k = _case(shape)
    out = ew.upsample2x2(_cl(k["x"]))
    assert out.shape == (shape[0], 2 * shape[1], 2 * shape[2], (c + 3) // 4 * 4)
    assert torch.equal(_nchw(out, c), k["up"].float())
    assert _pads_zero(out, c)
    assert float(L.amax_of(out)) >= float(out.abs().max())
    assert torch.equal(out, ew.upsample2x2(_cl(k["x"])))


@pytest.mark.parametrize("shape", SHAPES)
def test_average_pool_against_fp64(shape, f16x2):
    from lvt_amd.hip import binding as L, ew
    c = shape[3]
    k = _case(shape)
    out = ew.pool2x2(_cl(k["x"]))
    assert out.shape == (shape[0], shape[1] // 2, shape[2] // 2, (c + 3) // 4 * 4)
    assert rel_err(_nchw(out, c), k["pool"]) < 1e-6
    assert _pads_zero(out, c)
    assert float(L.amax_of(out)) >= float(out.abs().max())
    assert torch.equal(out, ew.pool2x2(_cl(k["x"])))
    # 5-d frames (N,1,H,W,C), as the conv stacks carry them
    assert torch.equal(ew.pool2x2(_cl(k["x"]).unsqueeze(1)).squeeze(1), out)


@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_roles_with_activation_mask(shape, leaky, f16x2):
    """Upsample with scale 0.25 is the pool's backward, pool with scale 1 the upsample's; the mask is the saved output of the
    (Leaky)ReLU in front, exact zeros included, and the reference is torch autograd in fp64 through act -> pool / upsample."""
    from lvt_amd.hip import binding as L, ew
    c = shape[3]
    k = _case(shape)
    act = (lambda t: F.leaky_relu(t, 0.2)) if leaky else torch.relu
    for role, gname in (("pool", "g_small"), ("up", "g_big")):
        pre = k["x"].double().requires_grad_(True)
        y = act(pre)
        z = F.avg_pool2d(y, 2) if role == "pool" else F.interpolate(y, scale_factor=2, mode="nearest")
        z.backward(k[gname].double())
        mask = _cl(y.detach().float())
        assert bool((mask == 0).any())
        gd = _cl(k[gname])
        fn = (lambda: ew.upsample2x2(gd, 0.25, mask=mask, leaky=leaky)) if role == "pool" else \
            (lambda: ew.pool2x2(gd, 1.0, mask=mask, leaky=leaky))
        out = fn()
        assert out.shape == mask.shape
        assert rel_err(_nchw(out, c), pre.grad) < 1e-6, role
        assert _pads_zero(out, c)
        assert float(L.amax_of(out)) >= float(out.abs().max())
        assert torch.equal(out, fn())


def test_scaled_unmasked_forms_against_fp64(f16x2):
    from lvt_amd.hip import ew
    k = _case(SHAPES[1])
    assert rel_err(_nchw(ew.upsample2x2(_cl(k["x"]), 0.25), 32), 0.25 * k["up"]) < 1e-6
    assert rel_err(_nchw(ew.pool2x2(_cl(k["x"]), 1.0), 32), 4.0 * k["pool"]) < 1e-6


def test_resample_refusals():
    from lvt_amd.hip import binding as L, ew
    with pytest.raises(L.LvtError, match="even"):
        ew.pool2x2(torch.zeros(1, 3, 4, 4, device=DEV))
    with pytest.raises(L.LvtError, match="even"):
        ew.pool2x2(torch.zeros(1, 4, 5, 4, device=DEV))
    with pytest.raises(L.LvtError, match="mask"):
        ew.pool2x2(torch.zeros(1, 4, 4, 4, device=DEV), mask=torch.zeros(1, 4, 4, 4, device=DEV))
    x = torch.zeros(1, 4, 4, 4, device=DEV)
    out = torch.empty(1, 2, 2, 4, device=DEV)
    # mask flags without a mask, and a channel count that is no multiple of 4, at the C ABI
    rc = L.lib().lvt_pool2x2(L.ptr(x), 1, 4, 4, 4, 0.25, None, L.EPI_MASK, L.ptr(out), None, L.stream_ptr())
    assert rc == -1
    rc = L.lib().lvt_upsample2x2(L.ptr(x), 1, 4, 8, 2, 1.0, None, 0, L.ptr(out), None, L.stream_ptr())
    assert rc == -1


# ---- engine: leaky epilogue and leaky mask ------------------------------------------------------------------------------
@pytest.fixture(params=["bf16x3", "f16x2", "f32"])
def math_mode(request):
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode(request.param)
    yield request.param
    L.set_math_mode(before)


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def _mask_src(*shape, seed=0):
    m = _rand(*shape, seed=seed)
    m[_rand(*shape, seed=seed + 1) > 0.9] = 0.0
    return m


# 3x3 / stride 1 / pad 1 convolutions.  route: "resident" = the frame-resident kernel (16x16 frames; its epilogue is the
# straightened one of csrc/epilogue_fast.h); "fast" = the implicit-GEMM tile kernel with 128 x 128 tiles, whose aligned launches
# take the straightened epilogue too; "slow" = 128 x 32 tiles (Co <= 32), which keep the general float4 epilogue; "scalar" = the
# same with a bias that is not 16-byte aligned, which takes the scalar epilogue.  Co_real < Co: pad channels.
CONV_CASES = [  # route, N, H, Ci, Co, Co_real
    ("resident", 3, 16, 128, 128, 128),
    ("fast", 2, 24, 32, 64, 64),
    ("slow", 2, 24, 64, 32, 30),
    ("scalar", 1, 10, 8, 32, 32),
]


def _assert_route(g, route, math_mode):
    from lvt_amd.hip import binding as L
    patch = L.lib().lvt_conv3d_uses_patch_kernel(ctypes.byref(g), L.math_flag())
    assert patch == (1 if route == "resident" and math_mode != "f32" else 0)
    # the tile kernel picks 128 x 32 tiles for Co <= 32 (gemm_engine.hip: lvt_conv3d_fwd), the straightened epilogue needs 64 x 64
    # wave sub-tiles
    assert (g.Co <= 32) == (route in ("slow", "scalar"))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("route,N,H,Ci,Co,Cr", CONV_CASES)
def test_conv_forward_leaky_epilogue(route, N, H, Ci, Co, Cr, with_res, math_mode):
    from lvt_amd.hip import gemm as G, binding as L
    x, w, b = _rand(N, Ci, H, H), _rand(Cr, Ci, 3, 3, seed=1) * 0.1, _rand(Cr, seed=2)
    res = _rand(N, Cr, H, H, seed=4) if with_res else None
    pre = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = F.leaky_relu(pre + res.double() if with_res else pre, 0.2)
    g = G.conv_geom(N, 1, H, H, Ci, Co, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    _assert_route(g, route, math_mode)
    bias = torch.zeros(Co + 1, device=DEV)
    off = 1 if route == "scalar" else 0                      # an offset view: 4 bytes past a 16-byte boundary
    bias[off:off + Cr] = b.to(DEV)
    bias = bias[off:off + Co]
    assert (bias.data_ptr() % 16 != 0) == (route == "scalar")
    yd = G.conv_fwd(g, _cl(x).unsqueeze(1), G.pack_weight(g, w.to(DEV), Ci, Cr), bias=bias,
                    res=_cl(res, Co).unsqueeze(1) if with_res else None, flags=L.EPI_LEAKY)
    assert rel_err(_nchw(yd, Cr), ref) < TOL
    assert _pads_zero(yd, Cr)                                # leaky(0) = 0
    if L.f16x2():
        assert float(L.amax_of(yd)) >= float(yd.abs().max())


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("route,N,H,Ci,Co,Cr", CONV_CASES[:3])
def test_conv_backward_data_leaky_mask(route, N, H, Ci, Co, Cr, with_res, math_mode):
    """dx = (conv_transpose(gy, w) (+ res)) * (mask > 0 ? 1 : 0.2), mask with exact zeros: through lvt_conv3d_bwd_data (the general
    float4 epilogue's mask form) and, for the 16x16 frames, as a forward convolution over the transposed weights (the straightened
    epilogue of the frame-resident kernel)."""
    from lvt_amd.hip import gemm as G, binding as L
    gy, w = _rand(N, Co, H, H, seed=5), _rand(Co, Ci, 3, 3, seed=1) * 0.1
    rx = _rand(N, Ci, H, H, seed=6) if with_res else None
    m = _mask_src(N, Ci, H, H, seed=7)
    pre = F.conv_transpose2d(gy.double(), w.double(), stride=1, padding=1)
    ref = (pre + rx.double() if with_res else pre) * _leaky_grad(m)
    g = G.conv_geom(N, 1, H, H, Ci, Co, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    args = dict(res=_cl(rx).unsqueeze(1) if with_res else None, mask=_cl(m).unsqueeze(1), flags=L.EPI_LEAKY_MASK)
    gd = _cl(gy).unsqueeze(1)
    dx = G.conv_bwd_data(g, gd, G.pack_weight(g, w.to(DEV), Ci, Co), **args)
    assert rel_err(_nchw(dx, Ci), ref) < TOL
    # the ReLU rule on the same operands is what the flag changes
    dx0 = G.conv_bwd_data(g, gd, G.pack_weight(g, w.to(DEV), Ci, Co), res=args["res"], mask=args["mask"])
    assert rel_err(_nchw(dx0, Ci), (pre + rx.double() if with_res else pre) * (m > 0)) < TOL
    if route == "resident":
        assert G.bwd_data_as_conv(g) == (math_mode != "f32")
        dx2 = G.conv_bwd_data(g, gd, None, wt=G.pack_weight_t(g, w.to(DEV), Ci, Co), **args)
        assert rel_err(_nchw(dx2, Ci), ref) < TOL


def test_transposed_forward_and_strided_forms_take_the_leaky_flag(math_mode):
    """lvt_conv3d_bwd_data as a ConvTranspose forward (bias + leaky), its phase form and the parity form of the strided forward
    (4x4 / stride 2 between 32x32 and 16x16 frames; frame-resident outside f32 mode)."""
    from lvt_amd.hip import gemm as G, binding as L
    N, Cin, Cout, H = 1, 32, 128, 16
    x, w, b = _rand(N, Cin, H, H), _rand(Cin, Cout, 4, 4, seed=1) * 0.1, _rand(Cout, seed=2)
    m = _mask_src(N, Cout, 2 * H, 2 * H, seed=5)
    pre = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    g = G.conv_geom(N, 1, 2 * H, 2 * H, Cout, Cin, (1, 4, 4), (1, 2, 2), (0, 1, 1))
    assert G.bwd_data_by_phases(g) == (math_mode != "f32")
    xd, wd = _cl(x).unsqueeze(1), w.to(DEV)
    forms = [dict(wp=G.pack_weight(g, wd, Cout, Cin))]
    if math_mode != "f32":
        forms.append(dict(wp=None, wph=G.pack_weight_phases(g, wd, Cout, Cin)))
    for f in forms:
        y = G.conv_bwd_data(g, xd, f["wp"], bias=b.to(DEV), flags=L.EPI_LEAKY, wph=f.get("wph"))
        assert rel_err(_nchw(y, Cout), F.leaky_relu(pre, 0.2)) < TOL
        y = G.conv_bwd_data(g, xd, f["wp"], bias=b.to(DEV), mask=_cl(m).unsqueeze(1), flags=L.EPI_LEAKY_MASK, wph=f.get("wph"))
        assert rel_err(_nchw(y, Cout), pre * _leaky_grad(m)) < TOL
    # strided forward, Ci -> Co
    Ci, Co = 32, 128
    x, w, b = _rand(N, Ci, 32, 32), _rand(Co, Ci, 4, 4, seed=1) * 0.1, _rand(Co, seed=2)
    m = _mask_src(N, Co, 16, 16, seed=5)
    pre = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    g = G.conv_geom(N, 1, 32, 32, Ci, Co, (1, 4, 4), (1, 2, 2), (0, 1, 1))
    assert G.fwd_by_parity(g) == (math_mode != "f32")
    forms = [dict(wp=G.pack_weight(g, w.to(DEV), Ci, Co))]
    if math_mode != "f32":
        forms.append(dict(wp=None, wq=G.pack_weight_parity(g, w.to(DEV), Ci, Co)))
    for f in forms:
        y = G.conv_fwd(g, _cl(x).unsqueeze(1), f["wp"], bias=b.to(DEV), flags=L.EPI_LEAKY, wq=f.get("wq"))
        assert rel_err(_nchw(y, Co), F.leaky_relu(pre, 0.2)) < TOL
        y = G.conv_fwd(g, _cl(x).unsqueeze(1), f["wp"], bias=b.to(DEV), mask=_cl(m).unsqueeze(1), flags=L.EPI_LEAKY_MASK, wq=f.get("wq"))
        assert rel_err(_nchw(y, Co), pre * _leaky_grad(m)) < TOL


@pytest.mark.parametrize("M,N,K", [(256, 384, 512), (1000, 132, 68)])
def test_gemm_leaky_epilogue_and_mask(M, N, K, math_mode):
    from lvt_amd.hip import gemm as G, binding as L
    a, w, b, r = _rand(M, K), _rand(N, K, seed=1), _rand(N, seed=2), _rand(M, N, seed=3)
    m = _mask_src(M, N, seed=4)
    pre = a.double() @ w.double().t()
    out = torch.empty(M, N, device=DEV)
    G.gemm(a.to(DEV), w.to(DEV), out, M, N, K, flags=L.EPI_BIAS | L.EPI_RESIDUAL | L.EPI_LEAKY, bias=b.to(DEV), res=r.to(DEV))
    assert rel_err(out, F.leaky_relu(pre + b.double() + r.double(), 0.2)) < TOL
    G.gemm(a.to(DEV), w.to(DEV), out, M, N, K, flags=L.EPI_BIAS | L.EPI_LEAKY, bias=b.to(DEV))
    assert rel_err(out, F.leaky_relu(pre + b.double(), 0.2)) < TOL
    G.gemm(a.to(DEV), w.to(DEV), out, M, N, K, flags=L.EPI_MASK | L.EPI_LEAKY_MASK, mask=m.to(DEV), ldm=N)
    assert rel_err(out, pre * _leaky_grad(m)) < TOL


@pytest.mark.parametrize("M,C", [(37, 3), (4099, 64), (20000, 30)])
def test_bn_apply_leaky(M, C, f16x2):
    """lvt_bn_apply with the leaky flag against fp64, at the bound of tests/test_gpu_norm.py."""
    from lvt_amd.hip import binding as L, norm as BN
    g = torch.Generator().manual_seed(M + C)
    cp = (C + 3) // 4 * 4
    y, res = torch.zeros(M, cp), torch.zeros(M, cp)
    y[:, :C], res[:, :C] = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    scale, shift = torch.zeros(cp), torch.zeros(cp)
    scale[:C], shift[:C] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    out = BN.apply(y.to(DEV), scale.to(DEV), shift.to(DEV), res=res.to(DEV), act=L.EPI_LEAKY)
    ref = F.leaky_relu(y.double() * scale.double() + shift.double() + res.double(), 0.2)
    assert rel_err(out[:, :C], ref[:, :C]) < 1e-6
    assert _pads_zero(out, C)
    assert float(L.amax_of(out)) >= float(out.abs().max())


def test_flag_combinations_refused(f16x2):
    from lvt_amd.hip import gemm as G, binding as L, norm as BN
    N, H, C = 1, 8, 32
    g = G.conv_geom(N, 1, H, H, C, C, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    x = torch.zeros(N, 1, H, H, C, device=DEV)
    wp = G.pack_weight(g, torch.zeros(C, C, 3, 3, device=DEV), C, C)
    for bad in (L.EPI_RELU, L.EPI_TANH, L.EPI_SIGMOID):
        with pytest.raises(L.LvtError, match="LEAKY"):
            G.conv_fwd(g, x, wp, flags=L.EPI_LEAKY | bad)
        with pytest.raises(L.LvtError, match="LEAKY"):
            G.conv_bwd_data(g, x, wp, flags=L.EPI_LEAKY | bad)
        with pytest.raises(L.LvtError, match="LEAKY"):
            BN.apply(x.view(-1, C), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), act=L.EPI_LEAKY | bad)
    with pytest.raises(L.LvtError, match="LEAKY_MASK"):
        G.conv_fwd(g, x, wp, flags=L.EPI_LEAKY_MASK)            # qualifies a mask that is not there
    out = torch.empty(64, 64, device=DEV)
    with pytest.raises(L.LvtError, match="LEAKY"):
        G.gemm(torch.zeros(64, 64, device=DEV), torch.zeros(64, 64, device=DEV), out, 64, 64, 64, flags=L.EPI_LEAKY | L.EPI_RELU)


# ---- G28: the VQ-VAE on ConvEncoder / ConvDecoder against the reference ---------------------------------------------------
def _g28_state(module, prefix, seed):
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


def conv_model(name, seed, scale=None, arch=None):
    from lvt_amd.modeling import build_model
    from util_models import vqvae_cfg
    cfg = CC.apply(vqvae_cfg(DEV), CC.overrides(name))
    if arch is not None:
        cfg.MODEL.META_ARCHITECTURE = arch
    model = build_model(cfg)
    for part, pre in (("encoder", "enc."), ("generator", "dec.")):
        mod = getattr(model, part)
        missing, unexpected = mod.load_state_dict(_g28_state(mod, pre, seed), strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    cb = None
    if scale is not None:
        cb = seeded.seeded_codebook_state(seed, scale=scale)
        model.codebook.load_state_dict(cb)
    return model, cb


def _data(seed, n=4):
    return [{"image": seeded.seeded_input("g28.f%d" % i, (3, 64, 64), seed).numpy()} for i in range(n)]


def _conv_names(module):
    return [n for n, m in module.named_modules() if isinstance(m, torch.nn.Conv2d)]


def _run_g28(golden, name):
    from lvt_amd.utils.events import EventStorage
    g = golden("g28_conv_coders")
    seed, rows, tag = int(g["seed"]), int(g["rows"]), name + "."
    assert float(g[tag + "clear_share"]) >= 0.99 and float(g[tag + "eval.clear"].float().mean()) >= 0.99
    model, cb = conv_model(name, seed, float(g[tag + "scale"]))
    model.train()
    with EventStorage(0):
        losses = model(_data(seed), mode="supervised")
    sum(losses.values()).backward()
    lr, lc = float(losses["loss_reconstruction"]), float(losses["loss_commitment"])
    assert abs(lr - float(g[tag + "train.loss_reconstruction"])) < 1e-5 * float(g[tag + "train.loss_reconstruction"]), lr
    assert abs(lc - float(g[tag + "train.loss_commitment"])) < 2e-4 * float(g[tag + "train.loss_commitment"]), lc
    enc, dec = _conv_names(model.encoder), _conv_names(model.generator)
    grads = {"enc_first": ("encoder", enc[0]), "enc_mid": ("encoder", enc[3]), "dec_first": ("generator", dec[0]),
             "dec_last": ("generator", dec[-1])}
    for key, (part, mod) in grads.items():
        p = getattr(model, part).get_submodule(mod).weight
        assert rel_err(p.grad[:rows], g[tag + "train.grad." + key]) < 5e-3, key
    if CC.CONFIGS[name]["norm"]:
        en = [n for n, m in model.encoder.named_modules() if hasattr(m, "running_mean")]
        dn = [n for n, m in model.generator.named_modules() if hasattr(m, "running_mean")]
        for key, (part, mod) in {"enc0": ("encoder", en[0]), "enc_last": ("encoder", en[-1]), "dec1": ("generator", dn[1])}.items():
            m = getattr(model, part).get_submodule(mod)
            for t in ("weight", "bias"):
                assert rel_err(getattr(m, t).grad, g[tag + "train.grad.%s.%s" % (key, t)]) < 5e-3, (key, t)
        seen = 0
        for part in ("encoder", "generator"):
            for k, v in getattr(model, part).state_dict().items():
                key = tag + "after.%s.%s" % (part, k)
                if k.endswith("num_batches_tracked"):
                    assert int(v) == int(g[key]) == 1, k
                elif k.endswith("running_mean") or k.endswith("running_var"):
                    assert rel_err(v, g[key]) < 1e-5, k
                    seen += 1
        assert seen == 2 * (7 + 4)
    # eval after the step: latents on the clear rows, reconstructions outside the receptive field of a differing code (G6)
    model.eval()
    model.codebook.load_state_dict(cb)
    with torch.no_grad():
        out = model(_data(seed), mode="inference")
    lat = torch.stack([o["latent"] for o in out]).cpu()
    rec = torch.stack([o["reconstruction"] for o in out]).cpu()
    want, clear = g[tag + "eval.latent"].long(), g[tag + "eval.clear"]
    assert lat.shape == want.shape == (4, 4) + ((16, 16) if CC.CONFIGS[name]["n_layers"] == 2 else (32, 32))
    assert torch.equal(lat[clear], want[clear])
    f = 64 // lat.shape[-1]
    keep = torch.ones(4, 64, 64, dtype=torch.bool)
    for t, i, y, x in (lat != want).nonzero().tolist():
        keep[t, max(0, f * (y - 4)):f * (y + 5), max(0, f * (x - 4)):f * (x + 5)] = False
    assert float(keep.float().mean()) > 0.8
    ref = g[tag + "eval.reconstruction"]
    assert float((rec - ref).abs()[keep[:, None].expand_as(rec)].max() / ref.abs().max()) < ATOL
    return model, cb


@pytest.fixture(params=["f16x2", "f32"])
def g28_mode(request):
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode(request.param)
    yield request.param
    L.set_math_mode(before)


@pytest.mark.parametrize("name", CC.NAMES)
def test_g28_against_reference(golden, name, g28_mode):
    _run_g28(golden, name)


_AMAX_CHILD = """
import sys
sys.path[:0] = [{tests!r}, {golden!r}]
import conftest
import test_gpu_convcoders as T
from lvt_amd.hip import binding as L
assert L.AMAX_CHECK and L.get_math_mode() == "f16x2"
T._run_g28(conftest.Golden, "b")
print("amax-checked step OK")
"""


def test_g28_under_amax_check_in_a_fresh_process():
    """Every max |.| record that an engine launch of config (b) reads -- those the resample kernels and the leaky epilogues wrote
    included -- is verified against its tensor.  LVT_AMAX_CHECK is read when lvt_amd.hip.binding is imported: a child process."""
    env = dict(os.environ, LVT_AMAX_CHECK="1", LVT_MATH="f16x2")
    code = _AMAX_CHILD.format(tests=os.path.join(ROOT, "tests"), golden=os.path.join(ROOT, "tests", "golden"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "amax-checked step OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_g28_eval_fold_matches_unfolded(golden, f16x2, monkeypatch):
    from lvt_amd.hip import norm as BN
    g = golden("g28_conv_coders")
    seed = int(g["seed"])
    model, _ = conv_model("b", seed, float(g["b.scale"]))
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


# ---- the reference's tensor-level methods ---------------------------------------------------------------------------------
def test_model_surface(golden, f16x2):
    """encode / decode / inference / supervised / interpolate_first_last of the VQ-VAE and the plain auto-encoder on the two stacks."""
    from lvt_amd.utils.events import EventStorage
    g = golden("g28_conv_coders")
    seed = int(g["seed"])
    x = torch.stack([torch.from_numpy(d["image"]) for d in _data(seed)]).to(DEV)
    model, _ = conv_model("c", seed, float(g["c.scale"]))
    model.eval()
    with torch.no_grad():
        lat = model.encode(model.normalizer(x))
        assert lat.shape == (4, 4, 32, 32) and lat.dtype == torch.int64
        rec = model.decode(lat)
        assert rec.shape == (4, 3, 64, 64) and float(rec.min()) >= 0.0 and float(rec.max()) <= 1.0        # sigmoid head
        out = model(_data(seed), mode="inference")
        assert torch.equal(torch.stack([o["latent"] for o in out]), lat)
        assert rel_err(torch.stack([o["reconstruction"] for o in out]), rec.clamp(0, 1)) < 1e-6
    ae, _ = conv_model("a", seed, arch="AutoEncoderModel")
    ae.eval()
    with torch.no_grad():
        z = ae.encode(ae.normalizer(x))
        assert z.shape == (4, 256, 16, 16)
        assert ae.decode(z).shape == (4, 3, 64, 64)
        mid = ae.interpolate_first_last(ae.normalizer(x))
        assert mid.shape == (4, 3, 64, 64)
        assert rel_err(mid[0], ae.decode(z[:1])[0]) < 1e-5 and rel_err(mid[-1], ae.decode(z[-1:])[0]) < 1e-5
    ae.train()
    with EventStorage(0):
        loss = ae(_data(seed), mode="supervised")
    assert list(loss) == ["loss_ae_mse"] and bool(torch.isfinite(loss["loss_ae_mse"]))


# ---- whole-model gradients against fp64 torch ------------------------------------------------------------------------------
def _twin_forward(seq, plan, outs, h):
    """fp64 forward through a deep copy of a stack's `layers`.  A LeakyReLU takes each element's branch from the sign of the GPU's
    own activation (outs[i] of the conv in front) instead of the sign of the fp64 value: its derivative jumps at 0, so where the
    two disagree -- a value within the engine's error of 0 -- the fp64 gradient of either choice is a valid reference for its own
    choice only, and that one element moves every gradient upstream of it (measured: one such activation among 1.2 million
    shifted the first conv's weight gradient by 7e-4 of its max).  The disagreements are checked to be exactly that: fp64
    values within TOL of the layer's max of 0.  -> (output, number of elements that took the GPU's branch against fp64's)."""
    i, flips = -1, 0
    for m in seq:
        if isinstance(m, torch.nn.Conv2d):
            i += 1
            h = m(h)
        elif isinstance(m, (torch.nn.AvgPool2d, torch.nn.Upsample)):
            i += 1
            h = m(h)
        elif isinstance(m, torch.nn.LeakyReLU):
            assert plan[i].act == "leaky"
            pos = _nchw(outs[i], plan[i].cout) > 0
            differ = pos != (h.detach() > 0)
            assert float(h.detach().abs()[differ].max() if differ.any() else 0.0) <= TOL * float(h.detach().abs().max())
            flips += int(differ.sum())
            h = h * torch.where(pos, 1.0, m.negative_slope).double()
        else:
            h = m(h)
    assert i == len(plan) - 1
    return h, flips


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_whole_model_gradients_against_fp64(mode):
    """Config (a) as a plain auto-encoder on 2 frames: loss and EVERY parameter gradient against the same torch modules in fp64 on
    the CPU (the module tree is the reference's, so a deep copy of `layers` in double IS the torch model; see _twin_forward for
    the one liberty taken at the LeakyReLU kinks).  Independent of G28.
    Bound: an engine launch is within 2e-5 of its output's max (TOL above); the gradient of the first layer has passed through the
    26 launches of the forward and backward chains, whose errors add at worst linearly: 26 x 2e-5 ~ 5e-4 of each gradient's max.
    Measured on the fp64 signs alone, before the kinks were handled: f16x2 at most 4.1e-7 (no element differed), f32 7.0e-4 on
    the first encoder conv with one element differing behind the encoder's fourth conv and at most 5.9e-7 downstream of it."""
    from lvt_amd.hip import binding as L, convnet
    from lvt_amd.modeling import convstack
    from lvt_amd.utils.events import EventStorage
    before = L.get_math_mode()
    L.set_math_mode(mode)
    try:
        seed = 77
        model, _ = conv_model("a", seed, arch="AutoEncoderModel")
        model.train()
        data = _data(seed, 2)
        with EventStorage(0):
            loss = model(data, mode="supervised")["loss_ae_mse"]
        loss.backward()
        # the activations of that pass again (the kernels are deterministic), layer by layer
        with torch.no_grad():
            x_cl = model._preprocess_cl(data)[0]
            e_outs, _ = convnet.stack_forward(model.encoder._plan, x_cl, convstack.plan_params(model.encoder._owners))
            d_outs, _ = convnet.stack_forward(model.generator._plan, e_outs[-1], convstack.plan_params(model.generator._owners))
    finally:
        L.set_math_mode(before)
    enc = copy.deepcopy(model.encoder.layers).cpu().double()
    dec = copy.deepcopy(model.generator.layers).cpu().double()
    for p in list(enc.parameters()) + list(dec.parameters()):
        p.grad = None
    x = (torch.stack([torch.from_numpy(d["image"]) for d in data]).double() - 0.5) / 0.5
    z, f1 = _twin_forward(enc, model.encoder._plan, e_outs, x)
    y, f2 = _twin_forward(dec, model.generator._plan, d_outs, z)
    print("elements on the GPU's side of a LeakyReLU kink against fp64's: %d" % (f1 + f2))
    assert f1 + f2 <= 20                       # of 1.2 million: a handful at most lie that close to 0
    assert rel_err(_nchw(d_outs[-1], 3), y) < 26 * TOL
    ref = F.mse_loss(y, x)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-5 * float(ref)
    n = 0
    for part, twin in ((model.encoder.layers, enc), (model.generator.layers, dec)):
        for (k, p), (k2, q) in zip(part.named_parameters(), twin.named_parameters()):
            assert k == k2 and p.grad is not None
            err = rel_err(p.grad, q.grad)
            print("%-12s %.2e" % (k, err))
            assert err < 5e-4, k
            n += 1
    assert n == 2 * (7 + 6)


# ---- a Res stack issues the calls it issued before -------------------------------------------------------------------------
_HOST_ONLY = ("_bytes", "_uses_", "_fuses_", "_supported", "_is_gather", "lvt_last_error", "lvt_version", "lvt_device_info")
_FLAG_ARG = {"lvt_conv3d_fwd": 7, "lvt_conv3d_fwd_parity": 7, "lvt_conv3d_bwd_data": 7, "lvt_conv3d_bwd_data_phases": 7,
             "lvt_bn_apply": 6}


class _Recorder:
    """Stands in for the ctypes handle: every enqueued entry point is logged by name, the engine's conv passes with their flags."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lvt_") or any(s in name for s in _HOST_ONLY):
            return fn

        def logged(*a):
            self._calls.append("%s:%d" % (name, a[_FLAG_ARG[name]]) if name in _FLAG_ARG else name)
            return fn(*a)
        return logged


def record_res_stack_calls(norm):
    """C-ABI calls of one forward + backward through ResEncoder and ResDecoder of PR-DVQVAE2 (2 frames, f16x2 arithmetic)."""
    from lvt_amd.hip import binding as L
    from lvt_amd.modeling import build_model
    from util_models import vqvae_cfg
    cfg = vqvae_cfg(DEV)
    cfg.MODEL.ENCODER.NORM = cfg.MODEL.GENERATOR.NORM = norm
    torch.manual_seed(3)
    model = build_model(cfg)
    model.train()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    before, real, calls = L.get_math_mode(), L.lib, []
    L.set_math_mode("f16x2")
    handle = real()
    L.lib = lambda: _Recorder(handle, calls)
    try:
        r = model.generator(model.encoder(x))
        r.backward(torch.ones_like(r))
        torch.cuda.synchronize()
    finally:
        L.lib = real
        L.set_math_mode(before)
    return calls


# Recorded from the commit before the conv coders with record_res_stack_calls (same function, that commit's package and library):
# flags are decimal, 262144 = LVT_MATH_F16X2, + 2097152 = LVT_CONV_WEIGHT_IMAGE, low bits = LVT_EPI_*.
RES_STACK_CALLS = {
    '': """
        lvt_to_channels_last lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_conv3d_pack_weights_multi
        lvt_conv3d_weight_images lvt_conv3d_fwd:262149 lvt_conv3d_fwd_parity:2359301 lvt_conv3d_fwd:2359301
        lvt_conv3d_fwd:2359301 lvt_conv3d_fwd:262151 lvt_conv3d_fwd:2359301 lvt_conv3d_fwd:262147 lvt_to_channels_first
        lvt_to_channels_last lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_conv3d_pack_weights_multi
        lvt_conv3d_weight_images lvt_conv3d_fwd:2359301 lvt_conv3d_fwd:2359301 lvt_conv3d_fwd:262151 lvt_conv3d_fwd:2359301
        lvt_conv3d_fwd:262151 lvt_conv3d_bwd_data_phases:2359301 lvt_convt4_fwd_act lvt_to_channels_first lvt_to_channels_last
        lvt_tanh_bwd lvt_conv3d_bwd_weight lvt_colsum lvt_conv3d_fwd:262160 lvt_conv3d_bwd_weight
        lvt_conv3d_fwd_parity:2359312 lvt_conv3d_bwd_weight lvt_conv3d_bwd_data:262160 lvt_conv3d_bwd_weight
        lvt_conv3d_fwd:2359314 lvt_conv3d_bwd_weight lvt_conv3d_bwd_data:262160 lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359314
        lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359296 lvt_to_channels_first lvt_to_channels_last lvt_conv3d_bwd_weight
        lvt_conv3d_bwd_data:262160 lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359314 lvt_conv3d_bwd_weight
        lvt_conv3d_bwd_data:262160 lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359314 lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359312
        lvt_conv3d_bwd_weight lvt_conv3d_bwd_data_phases:2359312 lvt_conv3d_bwd_weight
    """,
    'BN': """
        lvt_to_channels_last lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_conv3d_pack_weights_multi
        lvt_conv3d_weight_images lvt_conv3d_fwd:262144 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4
        lvt_conv3d_fwd_parity:2359296 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4 lvt_conv3d_fwd:2359296 lvt_bn_stats
        lvt_bn_finalize lvt_bn_apply:4 lvt_conv3d_fwd:2359296 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4
        lvt_conv3d_fwd:262144 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4 lvt_conv3d_fwd:2359296 lvt_bn_stats lvt_bn_finalize
        lvt_bn_apply:4 lvt_conv3d_fwd:262144 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:0 lvt_to_channels_first
        lvt_to_channels_last lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_amax lvt_conv3d_pack_weights_multi
        lvt_conv3d_weight_images lvt_conv3d_fwd:2359296 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4 lvt_conv3d_fwd:2359296
        lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4 lvt_conv3d_fwd:262144 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4
        lvt_conv3d_fwd:2359296 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4 lvt_conv3d_fwd:262144 lvt_bn_stats lvt_bn_finalize
        lvt_bn_apply:4 lvt_conv3d_bwd_data_phases:2359296 lvt_bn_stats lvt_bn_finalize lvt_bn_apply:4 lvt_convt4_fwd_act
        lvt_to_channels_first lvt_to_channels_last lvt_tanh_bwd lvt_conv3d_bwd_weight lvt_colsum lvt_conv3d_fwd:262160
        lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_fwd_parity:2359312 lvt_bn_bwd_reduce
        lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_bwd_data:262160 lvt_bn_bwd_reduce lvt_bn_bwd_apply
        lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359314 lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight
        lvt_conv3d_bwd_data:262160 lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359314
        lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359296 lvt_to_channels_first
        lvt_to_channels_last lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_bwd_data:262160
        lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359314 lvt_bn_bwd_reduce lvt_bn_bwd_apply
        lvt_conv3d_bwd_weight lvt_conv3d_bwd_data:262160 lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight
        lvt_conv3d_fwd:2359314 lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_fwd:2359312
        lvt_bn_bwd_reduce lvt_bn_bwd_apply lvt_conv3d_bwd_weight lvt_conv3d_bwd_data_phases:2359312 lvt_bn_bwd_reduce
        lvt_bn_bwd_apply lvt_conv3d_bwd_weight
    """,
}


@pytest.mark.parametrize("norm", ["", "BN"])
def test_res_stack_issues_the_same_calls_as_before(norm):
    assert record_res_stack_calls(norm) == RES_STACK_CALLS[norm].split()


# ---- tools/train_net.py -----------------------------------------------------------------------------------------------------
def test_train_net_runs_the_conv_coders(tmp_path):
    out = str(tmp_path / "vq")
    r = subprocess.run([sys.executable, "tools/train_net.py", "--config-file", "configs/vqvae/PR-DVQVAE2.yaml", "--synthetic",
                        "--max-iter", "6", "OUTPUT_DIR", out, "SOLVER.IMS_PER_BATCH", "4", "SOLVER.MAX_ITER", "6",
                        "MODEL.ENCODER.NAME", "ConvEncoder", "MODEL.ENCODER.NF", "32", "MODEL.ENCODER.N_LAYERS", "2",
                        "MODEL.ENCODER.OUT_CHANNELS", "256", "MODEL.GENERATOR.NAME", "ConvDecoder", "MODEL.GENERATOR.IN_CHANNELS", "256",
                        "MODEL.GENERATOR.NF", "32", "MODEL.GENERATOR.N_LAYERS", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    # (the trainer raises FloatingPointError on a loss that is not finite: a zero exit status covers all 6 iterations)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "loss_reconstruction" in r.stdout + r.stderr
    ck = torch.load(os.path.join(out, "netG", "model_final.pth"))
    assert sorted({int(k.split(".")[1]) for k in ck["model"]}) == [0, 2, 5, 7, 10, 11]
    assert all(bool(torch.isfinite(v).all()) for v in ck["model"].values())
