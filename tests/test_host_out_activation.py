"""Output activations of the conv stacks, host side (no GPU): ResEncoder / ResDecoder build with every OUT_ACTIVATION of the
reference ("", "sigmoid", "tanh"), their child list ends as the reference's does, the state-dict keys do not depend on the
activation, the engine plan carries it on the last layer only, and an unknown string is a ValueError.  The child and key
lists are also compared with fixture G27 (captured from the reference)."""
import os

import pytest
from torch import nn

from conftest import ROOT

ACTS = ("", "sigmoid", "tanh")
LAST = {"": None, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}


def _encoder(act, stride=4, norm="", n_layers=2):
    from lvt_amd.modeling.encoder.resencoder import ResEncoder
    return ResEncoder(in_channels=3, nf=32, res_channels=16, norm=norm, use_spectral_norm=False, n_layers=n_layers,
                      out_activation=act, stride=stride)


def _decoder(act, stride=4, norm="", n_layers=2):
    from lvt_amd.modeling.generator.resdecoder import ResDecoder
    return ResDecoder(in_channels=32, nf=32, res_channels=16, out_channels=3, norm=norm, use_spectral_norm=False,
                      n_layers=n_layers, out_activation=act, stride=stride)


@pytest.mark.parametrize("build,shipped", [(_encoder, ""), (_decoder, "tanh")])
@pytest.mark.parametrize("norm", ["", "BN"])
@pytest.mark.parametrize("stride", [2, 4])
@pytest.mark.parametrize("act", ACTS)
def test_children_and_state_dict_keys(build, shipped, norm, stride, act):
    m, base = build(act, stride, norm), build(shipped, stride, norm)
    last = list(m.layers)[-1]
    if LAST[act] is None:
        assert not isinstance(last, (nn.Sigmoid, nn.Tanh))
    else:
        assert type(last) is LAST[act]
        assert not list(last.state_dict())
    # the activation is one more child at the end, nothing else moves
    n_base = len(base.layers) - (1 if shipped else 0)
    assert len(m.layers) == n_base + (1 if act else 0)
    assert [type(c) for c in list(m.layers)[:n_base]] == [type(c) for c in list(base.layers)[:n_base]]
    assert list(m.state_dict().keys()) == list(base.state_dict().keys())
    # the plan: the activation sits on the last engine layer and nowhere else
    assert m._plan[-1].act == act
    assert all(ly.act in ("", "relu") for ly in m._plan[:-1])


@pytest.mark.parametrize("act", ACTS)
def test_no_resblocks(act):
    """N_LAYERS 0: the encoder then ends in its 3x3 conv, the decoder is unchanged behind the ReLU."""
    enc, dec = _encoder(act, n_layers=0), _decoder(act, n_layers=0)
    assert enc._plan[-1].act == act and enc._plan[-1].kernel == (1, 3, 3) and enc._plan[-1].res_from == -1
    assert dec._plan[-1].act == act and dec._plan[-1].kind == "convT"


@pytest.mark.parametrize("build", [_encoder, _decoder])
@pytest.mark.parametrize("act", ["softmax", "Tanh", "gelu", None])
def test_unknown_activation_is_a_value_error(build, act):
    with pytest.raises(ValueError):
        build(act)


def test_relu_terminated_stacks_stay_refused():
    """The reference's encoder also knows "relu" (its decoder does not); a ReLU-terminated stack has no backward here."""
    with pytest.raises(NotImplementedError):
        _encoder("relu")
    with pytest.raises(ValueError):
        _decoder("relu")


def _cfg(norm, enc_act, dec_act):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.ENCODER.NORM = cfg.MODEL.GENERATOR.NORM = norm
    cfg.MODEL.ENCODER.OUT_ACTIVATION, cfg.MODEL.GENERATOR.OUT_ACTIVATION = enc_act, dec_act
    return cfg


def test_build_model_matches_reference_tree(golden):
    """Child class names of `layers` and state-dict keys of both stacks, per combination of G27."""
    from lvt_amd.modeling import build_model
    g = golden("g27_out_activation")
    for combo in g["combos"]:
        tag, norm, enc_act, dec_act = str(combo).split("|")
        model = build_model(_cfg(norm, enc_act, dec_act))
        for part in ("encoder", "generator"):
            mod = getattr(model, part)
            assert [type(c).__name__ for c in mod.layers] == [str(c) for c in g["%s.%s.children" % (tag, part)]], (tag, part)
            assert list(mod.state_dict().keys()) == [str(k) for k in g["%s.%s.keys" % (tag, part)]], (tag, part)


def test_from_config_honours_the_out_activation_kwarg():
    from lvt_amd.modeling.generator.resdecoder import ResDecoder
    cfg = _cfg("", "", "tanh")
    assert isinstance(list(ResDecoder.from_config(cfg).layers)[-1], nn.Tanh)
    assert isinstance(list(ResDecoder.from_config(cfg, out_activation="sigmoid").layers)[-1], nn.Sigmoid)
    assert isinstance(list(ResDecoder.from_config(cfg, out_activation="").layers)[-1], nn.ConvTranspose2d)


def test_abi_declares_the_sigmoid_entries():
    from lvt_amd.hip import binding as L
    text = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    assert "#define LVT_EPI_SIGMOID   %d " % L.EPI_SIGMOID in text
    assert L.EPI_SIGMOID & (L.EPI_BIAS | L.EPI_RESIDUAL | L.EPI_RELU | L.EPI_TANH | L.EPI_MASK | L.EPI_ACCUM | L.EPI_PLANES) == 0
    assert {"lvt_sigmoid_bwd", "lvt_convt4_fwd_act", "lvt_convt4_fwd"} <= set(L.declared_symbols())
    assert [L.epi_pad(n) for n in range(4)] == [n << 24 for n in range(4)]
    with pytest.raises(ValueError):
        L.epi_pad(4)
