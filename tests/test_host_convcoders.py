"""ConvEncoder / ConvDecoder, host side (no GPU): registries, state-dict keys, shapes and init checksums against fixture G28
(captured from the reference by tests/golden/make_golden_convcoders.py), the module tree child by child, the plan the conv-stack
executor runs, the refusals, mixing with the Res family and the optimizer's parameter groups."""
import os
import random

import numpy as np
import pytest
import torch
from torch import nn

import convcoders_cfg as CC
from conftest import ROOT
from test_pins import _pins

PIN_SEED = 29871897          # tests/golden/make_golden_convcoders.py


def _cfg(name, **over):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    return CC.apply(cfg, dict(CC.overrides(name), **over))


def _model(name, **over):
    from lvt_amd.modeling import build_model
    torch.manual_seed(PIN_SEED)
    np.random.seed(PIN_SEED)
    random.seed(PIN_SEED)
    return build_model(_cfg(name, **over))


def test_registries_resolve_both_names():
    from lvt_amd.modeling import ENCODER_REGISTRY, GENERATOR_REGISTRY
    from lvt_amd.modeling.encoder import ConvEncoder
    from lvt_amd.modeling.generator import ConvDecoder
    assert ENCODER_REGISTRY.get("ConvEncoder") is ConvEncoder
    assert GENERATOR_REGISTRY.get("ConvDecoder") is ConvDecoder


@pytest.mark.parametrize("name", CC.NAMES)
def test_keys_shapes_and_init_checksums_match_reference(golden, name):
    g = golden("g28_conv_coders")
    model = _model(name)
    for part in ("encoder", "generator"):
        sd = getattr(model, part).state_dict()
        assert list(sd.keys()) == [str(k) for k in g["%s.%s.keys" % (name, part)]], part
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["%s.%s.shapes" % (name, part)]]
        names, rows = _pins(sd)
        assert names == [str(k) for k in g["%s.%s.pin_names" % (name, part)]]
        np.testing.assert_allclose(rows, g["%s.%s.pins" % (name, part)].numpy(), rtol=1e-12, atol=1e-12, err_msg=part)


def test_decoder_keys_of_the_plain_config():
    dec = _model("a").generator
    assert sorted({int(k.split(".")[1]) for k in dec.state_dict()}) == [0, 2, 5, 7, 10, 11]
    dec = _model("b").generator
    keys = list(dec.state_dict())
    assert "layers.0.0.weight" in keys and "layers.0.1.running_var" in keys and "layers.0.0.bias" not in keys
    assert "layers.10.weight" in keys and "layers.11.bias" in keys          # the last two are never normalised


def _kinds(seq):
    out = []
    for m in seq:
        if isinstance(m, nn.Sequential):
            out.append((type(m[0]).__name__, type(m[1]).__name__))
        else:
            out.append(type(m).__name__)
    return out


@pytest.mark.parametrize("name", CC.NAMES)
def test_module_tree_child_by_child(name):
    c = CC.CONFIGS[name]
    model = _model(name)
    conv = ("Conv2d", "BatchNorm2d") if c["norm"] else "Conv2d"
    lk = "LeakyReLU"
    want_e = [conv, lk] + [conv, lk, conv, lk, "AvgPool2d"] * c["n_layers"] + [conv, lk, conv]
    want_d = [conv, lk, conv, lk, "Upsample"] * c["n_layers"] + ["Conv2d", "Conv2d", {"tanh": "Tanh", "sigmoid": "Sigmoid"}[c["act"]]]
    assert _kinds(model.encoder.layers) == want_e
    assert _kinds(model.generator.layers) == want_d
    for m in list(model.encoder.layers) + list(model.generator.layers):
        if isinstance(m, nn.LeakyReLU):
            assert m.negative_slope == 0.2 and m.inplace
        if isinstance(m, nn.AvgPool2d):
            assert m.kernel_size == 2 and "AvgPool2d(kernel_size=2, stride=2, padding=0)" == repr(m)
        if isinstance(m, nn.Upsample):
            assert m.scale_factor == 2.0 and m.mode == "nearest" and repr(m) == repr(nn.Upsample(scale_factor=2))
    # channel widths: nf << i on the way down, nf << scale on the way up; the decoder's last two convs both read nf channels
    nf, n = c["nf"], c["n_layers"]
    first = model.encoder.layers[0]
    first = first[0] if c["norm"] else first
    assert (first.in_channels, first.out_channels, first.kernel_size, first.padding) == (3, nf, (3, 3), (1, 1))
    last2 = list(model.generator.layers)[-3:-1]
    assert [(m.in_channels, m.out_channels) for m in last2] == [(nf, nf), (nf, 3)] and all(m.bias is not None for m in last2)
    assert (model.encoder.in_channels, model.encoder.out_channels) == (3, 256)
    assert (model.generator.in_channels, model.generator.out_channels) == (256, 3)
    widest = list(model.encoder.layers)[-3]
    widest = widest[0] if c["norm"] else widest
    assert widest.out_channels == nf << n


@pytest.mark.parametrize("name", CC.NAMES)
def test_plan_of_the_stacks(name):
    c = CC.CONFIGS[name]
    model = _model(name)
    kind = "bn" if c["norm"] else ""
    e, d = model.encoder._plan, model.generator._plan
    assert [ly.kind for ly in e] == ["conv"] + ["conv", "conv", "pool"] * c["n_layers"] + ["conv", "conv"]
    assert [ly.act for ly in e] == ["leaky"] + ["leaky", "leaky", ""] * c["n_layers"] + ["leaky", ""]
    assert [ly.norm for ly in e] == [kind] + [kind, kind, ""] * c["n_layers"] + [kind, kind]
    assert [ly.kind for ly in d] == ["conv", "conv", "up"] * c["n_layers"] + ["conv", "conv"]
    assert [ly.act for ly in d] == ["leaky", "leaky", ""] * c["n_layers"] + ["", c["act"]]
    assert [ly.norm for ly in d] == [kind, kind, ""] * c["n_layers"] + ["", ""]
    assert all(ly.res_from == -1 for ly in e + d)
    # parameter-less layers hold a place in every per-layer list
    assert [m is None for m in model.encoder._owners] == [ly.kind == "pool" for ly in e]
    assert [m is None for m in model.generator._owners] == [ly.kind == "up" for ly in d]
    if c["norm"]:
        assert [m is None for m in model.encoder._norms] == [ly.kind == "pool" for ly in e]
    else:
        assert model.encoder._norms is None and model.generator._norms is None


@pytest.mark.parametrize("norm", ["BN", "SyncBN", "FrozenBN"])
def test_supported_norms_build(norm):
    from lvt_amd.modeling import convstack
    model = _model("a", **{"MODEL.ENCODER.NORM": norm, "MODEL.GENERATOR.NORM": norm})
    cls = {"BN": nn.BatchNorm2d, "SyncBN": convstack.NaiveSyncBatchNorm, "FrozenBN": convstack.FrozenBatchNorm2d}[norm]
    assert type(model.encoder.layers[0][1]) is cls and type(model.generator.layers[2][1]) is cls
    assert model.encoder.layers[0][0].bias is None


@pytest.mark.parametrize("bad", ["IN", "GN", "StdN", "nnSyncBN"])
def test_unsupported_norms_refused(bad):
    with pytest.raises(NotImplementedError, match="BN.*SyncBN.*FrozenBN"):
        _model("a", **{"MODEL.ENCODER.NORM": bad})
    with pytest.raises(NotImplementedError, match="BN.*SyncBN.*FrozenBN"):
        _model("a", **{"MODEL.GENERATOR.NORM": bad})


def test_spectral_refused():
    with pytest.raises(NotImplementedError, match="spectral"):
        _model("a", **{"MODEL.ENCODER.SPECTRAL": True})
    with pytest.raises(NotImplementedError, match="spectral"):
        _model("a", **{"MODEL.GENERATOR.SPECTRAL": True})


@pytest.mark.parametrize("act", ["relu", "softmax", "Tanh"])
def test_unknown_out_activation_is_a_value_error(act):
    with pytest.raises(ValueError):
        _model("a", **{"MODEL.ENCODER.OUT_ACTIVATION": act})
    with pytest.raises(ValueError):
        _model("a", **{"MODEL.GENERATOR.OUT_ACTIVATION": act})


@pytest.mark.parametrize("act,cls", [("", None), ("sigmoid", nn.Sigmoid), ("tanh", nn.Tanh)])
def test_out_activations(act, cls):
    model = _model("a", **{"MODEL.ENCODER.OUT_ACTIVATION": act, "MODEL.GENERATOR.OUT_ACTIVATION": act})
    for part in (model.encoder, model.generator):
        last = list(part.layers)[-1]
        assert isinstance(last, nn.Conv2d) if cls is None else type(last) is cls
        assert part._plan[-1].act == act


def test_decoder_without_scales_needs_matching_widths():
    from lvt_amd.modeling.generator import ConvDecoder
    with pytest.raises(ValueError, match="IN_CHANNELS == NF"):
        ConvDecoder(256, 32, 3, "", False, 0, "tanh")
    d = ConvDecoder(32, 32, 3, "", False, 0, "tanh")
    assert [ly.kind for ly in d._plan] == ["conv", "conv"] and list(d.state_dict()) == [
        "layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias"]


def test_mixes_with_the_res_family():
    from lvt_amd.modeling.encoder import ConvEncoder, ResEncoder
    from lvt_amd.modeling.generator import ConvDecoder, ResDecoder
    m = _model("a", **{"MODEL.ENCODER.NAME": "ResEncoder", "MODEL.ENCODER.NF": 256, "MODEL.ENCODER.RES_CHANNELS": 128})
    assert isinstance(m.encoder, ResEncoder) and isinstance(m.generator, ConvDecoder)
    m = _model("a", **{"MODEL.GENERATOR.NAME": "ResDecoder", "MODEL.GENERATOR.NF": 256, "MODEL.GENERATOR.RES_CHANNELS": 128})
    assert isinstance(m.encoder, ConvEncoder) and isinstance(m.generator, ResDecoder)


@pytest.mark.parametrize("name", ["a", "b"])
def test_optimizer_param_groups_follow_module_order(name):
    from lvt_amd.solver import build_optimizer
    cfg = _cfg(name, **{"SOLVER.WEIGHT_DECAY.NORM_G": 0.125, "SOLVER.WEIGHT_DECAY.BASE_G": 0.5, "SOLVER.WEIGHT_DECAY.BIAS_G": 0.25})
    model = _model(name)
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
    n_conv = 7 + 6
    assert len(got) == (2 * n_conv if name == "a" else n_conv + 2 * (7 + 4) + 2)


def test_non_default_slope_refused():
    from lvt_amd.modeling import convstack
    with pytest.raises(NotImplementedError, match="0.2"):
        convstack.plain_plan(nn.Sequential(nn.Conv2d(4, 4, 3, 1, 1), nn.LeakyReLU(0.1), nn.Conv2d(4, 4, 3, 1, 1)))
