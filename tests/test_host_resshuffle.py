"""ResShuffleDecoder, host side (no GPU): the registry, state-dict keys, shapes and init checksums against fixture G29 (captured
from the reference by tests/golden/make_golden_shuffle.py), the module tree child by child for both strides, the plan the
conv-stack executor runs (built by the plan builder it shares with ResDecoder), the refusals and the optimizer's parameter groups."""
import os
import random

import numpy as np
import pytest
import torch
from torch import nn

import shuffle_cfg as SC
from conftest import ROOT
from test_pins import _pins

PIN_SEED = 29871897          # tests/golden/make_golden_shuffle.py


def _cfg(name, **over):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    return SC.apply(cfg, dict(SC.overrides(name), **over))


def _model(name, **over):
    from lvt_amd.modeling import build_model
    torch.manual_seed(PIN_SEED)
    np.random.seed(PIN_SEED)
    random.seed(PIN_SEED)
    return build_model(_cfg(name, **over))


def _decoder(norm="", act="tanh", stride=4, n_layers=2, spectral=False):
    from lvt_amd.modeling.generator import ResShuffleDecoder
    return ResShuffleDecoder(256, 64, 32, 3, norm, spectral, n_layers, act, stride=stride)


def test_registry_resolves_the_name():
    from lvt_amd.modeling import GENERATOR_REGISTRY
    from lvt_amd.modeling.generator import ResDecoder, ResShuffleDecoder
    assert GENERATOR_REGISTRY.get("ResShuffleDecoder") is ResShuffleDecoder
    assert GENERATOR_REGISTRY.get("ResDecoder") is ResDecoder and not issubclass(ResShuffleDecoder, ResDecoder)
    assert isinstance(_model("p").generator, ResShuffleDecoder)


@pytest.mark.parametrize("name", SC.NAMES)
def test_keys_shapes_and_init_checksums_match_reference(golden, name):
    g = golden("g29_res_shuffle")
    model = _model(name)
    for part in ("encoder", "generator"):
        sd = getattr(model, part).state_dict()
        assert list(sd.keys()) == [str(k) for k in g["%s.%s.keys" % (name, part)]], part
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["%s.%s.shapes" % (name, part)]]
        names, rows = _pins(sd)
        assert names == [str(k) for k in g["%s.%s.pin_names" % (name, part)]]
        np.testing.assert_allclose(rows, g["%s.%s.pins" % (name, part)].numpy(), rtol=1e-12, atol=1e-12, err_msg=part)
    sd = model.generator.state_dict()
    sub = ".0" if SC.CONFIGS[name]["norm"] else ""
    assert tuple(sd["layers.4%s.weight" % sub].shape) == (512, 256, 3, 3) and tuple(sd["layers.7.weight"].shape) == (12, 128, 3, 3)
    assert "layers.7.bias" in sd and ("layers.4.0.bias" not in sd) and ("layers.4.bias" in sd) == (not sub)


def _kinds(seq):
    out = []
    for m in seq:
        if isinstance(m, nn.Sequential):
            out.append((type(m[0]).__name__, type(m[1]).__name__))
        else:
            out.append(type(m).__name__)
    return out


@pytest.mark.parametrize("norm", ["", "BN"])
@pytest.mark.parametrize("stride", [4, 2])
def test_module_tree_child_by_child(stride, norm):
    d = _decoder(norm=norm, stride=stride)
    conv = ("Conv2d", "BatchNorm2d") if norm else "Conv2d"
    tail = [conv, "PixelShuffle", "ReLU", "Conv2d", "PixelShuffle"] if stride == 4 else [conv, "PixelShuffle"]
    assert _kinds(d.layers) == [conv, "ResBlock", "ResBlock", "ReLU"] + tail + ["Tanh"]
    mods = list(d.layers)
    first = mods[0][0] if norm else mods[0]
    assert (first.in_channels, first.out_channels, first.kernel_size, first.stride, first.padding) == (256, 64, (3, 3), (1, 1), (1, 1))
    up = mods[4][0] if norm else mods[4]
    want = (64, 128) if stride == 4 else (64, 12)
    assert (up.in_channels, up.out_channels, up.kernel_size, up.stride, up.padding) == want + ((3, 3), (1, 1), (1, 1))
    assert (up.bias is None) == bool(norm)
    for m in mods:
        if isinstance(m, nn.PixelShuffle):
            assert m.upscale_factor == 2
        if isinstance(m, nn.ReLU):
            assert m.inplace
    if stride == 4:
        last = mods[7]
        assert (last.in_channels, last.out_channels, last.kernel_size, last.padding) == (32, 12, (3, 3), (1, 1))
        assert last.bias is not None                 # never normalised
    assert (d.in_channels, d.out_channels) == (256, 3)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("norm", ["", "BN"])
def test_plan_of_the_stride_4_stack(norm, act):
    d = _decoder(norm=norm, act=act)
    plan = d._plan
    kind = "bn" if norm else ""
    assert [ly.kind for ly in plan] == ["conv", "conv", "conv", "conv", "conv", "conv", "shuffle", "conv", "shuffle"]
    # a ResBlock's first op is an in-place ReLU, so the layer in front of one stores its output rectified (act_after), exactly as
    # in ResDecoder's plan; the convolution in front of a shuffle has no activation, the shuffle carries the one behind it
    assert [ly.act for ly in plan] == ["relu", "relu", "relu", "relu", "relu", "", "relu", "", act]
    assert [ly.res_from for ly in plan] == [-1, -1, 0, -1, 2, -1, -1, -1, -1]
    assert [ly.kernel for ly in plan] == [(1, 3, 3), (1, 3, 3), (1, 1, 1), (1, 3, 3), (1, 1, 1), (1, 3, 3), None, (1, 3, 3), None]
    assert [ly.norm for ly in plan] == [kind] * 6 + ["", "", ""]
    assert [(ly.cin, ly.cout) for ly in plan[5:]] == [(64, 128), (128, 32), (32, 12), (12, 3)]
    assert [ly.resamples for ly in plan] == [ly.kind == "shuffle" for ly in plan]
    assert [m is None for m in d._owners] == [ly.kind == "shuffle" for ly in plan]
    if norm:
        assert [m is None for m in d._norms] == [False] * 6 + [True] * 3
    else:
        assert d._norms is None


def test_plan_of_the_stride_2_stack_and_without_activation():
    d = _decoder(norm="BN", act="", stride=2, n_layers=1)
    assert [(ly.kind, ly.act, ly.norm) for ly in d._plan] == [("conv", "relu", "bn"), ("conv", "relu", "bn"), ("conv", "relu", "bn"),
                                                             ("conv", "", "bn"), ("shuffle", "", "")]
    assert isinstance(list(d.layers)[-1], nn.PixelShuffle)


def test_res_decoder_plan_is_unchanged():
    from lvt_amd.modeling.generator import ResDecoder
    d = ResDecoder(256, 64, 32, 3, "", False, 2, "tanh", stride=4)
    assert [ly.kind for ly in d._plan] == ["conv"] * 5 + ["convT", "convT"]
    assert [ly.act for ly in d._plan] == ["relu", "relu", "relu", "relu", "relu", "relu", "tanh"]
    assert all(m is not None for m in d._owners) and not any(ly.resamples for ly in d._plan)


def test_other_upscale_factors_refused():
    d = _decoder()
    d.layers[5] = nn.PixelShuffle(3)
    with pytest.raises(NotImplementedError, match="PixelShuffle"):
        d._build_plan()


@pytest.mark.parametrize("bad", ["IN", "GN", "nnSyncBN"])
def test_unsupported_norms_refused(bad):
    from lvt_amd.modeling.generator import ResDecoder
    with pytest.raises(NotImplementedError, match="BN.*SyncBN.*FrozenBN"):
        ResDecoder(256, 64, 32, 3, bad, False, 2, "tanh", stride=4)
    with pytest.raises(NotImplementedError, match="BN.*SyncBN.*FrozenBN"):
        _decoder(norm=bad)
    with pytest.raises(NotImplementedError, match="BN.*SyncBN.*FrozenBN"):
        _model("p", **{"MODEL.GENERATOR.NORM": bad})


def test_spectral_norm_out_activation_and_stride_refused_like_res_decoder():
    from lvt_amd.modeling.generator import ResDecoder
    with pytest.raises(NotImplementedError, match="spectral"):
        ResDecoder(256, 64, 32, 3, "", True, 2, "tanh", stride=4)
    with pytest.raises(NotImplementedError, match="spectral"):
        _decoder(spectral=True)
    for cls in (ResDecoder, type(_decoder())):
        with pytest.raises(ValueError):
            cls(256, 64, 32, 3, "", False, 2, "relu", stride=4)
        with pytest.raises(ValueError):
            cls(256, 64, 32, 3, "", False, 2, "tanh", stride=3)
    with pytest.raises(ValueError):
        _model("p", **{"MODEL.GENERATOR.OUT_ACTIVATION": "relu"})


def test_from_config_kwargs():
    from lvt_amd.modeling.generator import ResShuffleDecoder
    cfg = _cfg("p")
    assert isinstance(list(ResShuffleDecoder.from_config(cfg).layers)[-1], nn.Tanh)
    assert isinstance(list(ResShuffleDecoder.from_config(cfg, out_activation="sigmoid").layers)[-1], nn.Sigmoid)
    d = ResShuffleDecoder.from_config(cfg, out_activation="", stride=2)
    assert isinstance(list(d.layers)[-1], nn.PixelShuffle) and len(d._plan) == 7
    with pytest.raises(ValueError):
        ResShuffleDecoder.from_config(cfg, stride=8)


def test_optimizer_param_groups_give_the_norm_decay_to_bn():
    from lvt_amd.solver import build_optimizer
    cfg = _cfg("b", **{"SOLVER.WEIGHT_DECAY.NORM_G": 0.125, "SOLVER.WEIGHT_DECAY.BASE_G": 0.5, "SOLVER.WEIGHT_DECAY.BIAS_G": 0.25})
    model = _model("b")
    opt = build_optimizer([model.encoder, model.generator], cfg, "_G")
    want = []
    for part in (model.encoder, model.generator):
        for m in part.modules():
            for key, p in m.named_parameters(recurse=False):
                want.append((p, 0.125 if isinstance(m, nn.BatchNorm2d) else (0.25 if key == "bias" else 0.5)))
    got = [(g["params"][0], g["weight_decay"]) for g in opt.param_groups]
    assert len(got) == len(want)
    for (p, d), (q, e) in zip(got, want):
        assert p is q and d == e
    bn = model.generator.layers[4][1]
    decay = {id(p): d for p, d in got}
    assert decay[id(bn.weight)] == decay[id(bn.bias)] == 0.125
    assert decay[id(model.generator.layers[7].weight)] == 0.5 and decay[id(model.generator.layers[7].bias)] == 0.25
