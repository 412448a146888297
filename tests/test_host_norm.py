"""Batch-normalised conv stacks, host side (no GPU): the module tree, state-dict keys, init checksums and optimizer param
groups of ResEncoder / ResDecoder for NORM "BN", "SyncBN" and "FrozenBN" against fixture G26 (captured from the
reference), and the refusal of the norms that are not implemented."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_pins import _pins

NORMS = ("BN", "SyncBN", "FrozenBN")
PIN_SEED = 29871897          # tests/golden/make_golden_norm.py


def _cfg(norm, enc_norm=None, gen_norm=None, **over):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.ENCODER.NORM = norm if enc_norm is None else enc_norm
    cfg.MODEL.GENERATOR.NORM = norm if gen_norm is None else gen_norm
    for k, v in over.items():
        node = cfg
        ks = k.split(".")
        for s in ks[:-1]:
            node = node[s]
        node[ks[-1]] = v
    return cfg


def _model(norm, **kw):
    from lvt_amd.modeling import build_model
    torch.manual_seed(PIN_SEED)
    np.random.seed(PIN_SEED)
    random.seed(PIN_SEED)
    return build_model(_cfg(norm, **kw))


@pytest.mark.parametrize("norm", NORMS)
def test_state_dict_keys_and_shapes_match_reference(golden, norm):
    g = golden("g26_batchnorm")
    tag = "FrozenBN" if norm == "FrozenBN" else "BN"        # NaiveSyncBatchNorm is an nn.BatchNorm2d: the same keys
    model = _model(norm)
    for part in ("encoder", "generator"):
        sd = getattr(model, part).state_dict()
        assert list(sd.keys()) == [str(k) for k in g["%s.%s.keys" % (tag, part)]], part
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["%s.%s.shapes" % (tag, part)]]


@pytest.mark.parametrize("norm", ("BN", "FrozenBN"))
def test_init_checksums_match_reference(golden, norm):
    g = golden("g26_batchnorm")
    model = _model(norm)
    for part in ("encoder", "generator"):
        names, rows = _pins(getattr(model, part).state_dict())
        assert names == [str(k) for k in g["%s.%s.pin_names" % (norm, part)]]
        want = g["%s.%s.pins" % (norm, part)].numpy()
        np.testing.assert_allclose(rows, want, rtol=1e-12, atol=1e-12, err_msg=part)


@pytest.mark.parametrize("norm", NORMS)
def test_module_tree(norm):
    from torch import nn
    from lvt_amd.modeling import convstack
    model = _model(norm)
    enc, dec = model.encoder, model.generator
    cls = {"BN": nn.BatchNorm2d, "SyncBN": convstack.NaiveSyncBatchNorm, "FrozenBN": convstack.FrozenBatchNorm2d}[norm]
    first = enc.layers[0]
    assert isinstance(first, nn.Sequential) and first[0].bias is None and type(first[1]) is cls
    assert isinstance(enc.layers[5].block[3][1], cls)
    # the decoder's last ConvTranspose is not normalised, the middle one is
    assert isinstance(dec.layers[6], nn.ConvTranspose2d) and dec.layers[6].bias is not None
    assert isinstance(dec.layers[4], nn.Sequential) and isinstance(dec.layers[4][0], nn.ConvTranspose2d)
    norms = [ly.norm for ly in enc._plan]
    kind = {"BN": "bn", "SyncBN": "syncbn", "FrozenBN": "frozen"}[norm]
    assert norms == [kind] * 7
    assert [ly.norm for ly in dec._plan] == [kind] * 6 + [""]
    # the residual is added after the second norm of a block: the 1x1 layer carries both
    assert enc._plan[4].res_from == 2 and enc._plan[4].norm == kind
    if norm == "FrozenBN":
        assert not list(first[1].parameters()) and first[1]._version == 3
        assert set(dict(first[1].named_buffers())) == {"weight", "bias", "running_mean", "running_var"}


def test_plain_config_unchanged():
    from torch import nn
    model = _model("")
    assert isinstance(model.encoder.layers[0], nn.Conv2d) and model.encoder.layers[0].bias is not None
    assert model.encoder._norms is None and model.generator._norms is None
    assert all(ly.norm == "" for ly in model.encoder._plan + model.generator._plan)


def test_encoder_and_generator_set_separately():
    model = _model("", enc_norm="BN", gen_norm="")
    assert all(ly.norm == "bn" for ly in model.encoder._plan)
    assert all(ly.norm == "" for ly in model.generator._plan)


@pytest.mark.parametrize("norm", ("BN", "FrozenBN"))
def test_stride2_and_four_blocks(norm):
    from lvt_amd.modeling.encoder.resencoder import ResEncoder
    from lvt_amd.modeling.generator.resdecoder import ResDecoder
    e = ResEncoder(3, 64, 32, norm, False, 4, "", 2)
    assert len(e._plan) == 2 + 2 * 4 and all(ly.norm for ly in e._plan)
    d = ResDecoder(64, 64, 32, 3, norm, False, 4, "tanh", 2)
    # at stride 2 the only ConvTranspose is normalised, as in the reference
    assert d._plan[-1].kind == "convT" and d._plan[-1].norm and d._plan[-1].act == "tanh"


@pytest.mark.parametrize("norm", ("BN", "SyncBN"))
def test_norm_params_in_weight_decay_norm_groups(norm):
    from lvt_amd.solver import build_optimizer
    cfg = _cfg(norm, **{"SOLVER.WEIGHT_DECAY.NORM_G": 0.125, "SOLVER.WEIGHT_DECAY.BASE_G": 0.5,
                        "SOLVER.WEIGHT_DECAY.BIAS_G": 0.25})
    model = _model(norm)
    opt = build_optimizer([model.encoder, model.generator], cfg, "_G")
    # one group per parameter in module-traversal order (the reference's solver/build.py), norm affine at NORM decay
    want = []
    for part in (model.encoder, model.generator):
        for m in part.modules():
            for key, p in m.named_parameters(recurse=False):
                want.append((p, 0.125 if isinstance(m, torch.nn.BatchNorm2d) else (0.25 if key == "bias" else 0.5)))
    got = [(g["params"][0], g["weight_decay"]) for g in opt.param_groups]
    assert len(got) == len(want)
    for (p, d), (q, e) in zip(got, want):
        assert p is q and d == e
    n_norm = sum(1 for _, d in got if d == 0.125)
    assert n_norm == 2 * (7 + 6)


def test_frozen_has_no_parameters_in_optimizer():
    from lvt_amd.solver import build_optimizer
    cfg = _cfg("FrozenBN")
    model = _model("FrozenBN")
    opt = build_optimizer([model.encoder, model.generator], cfg, "_G")
    assert len(opt.param_groups) == sum(1 for _ in model.encoder.parameters()) + sum(1 for _ in model.generator.parameters())
    assert len(opt.param_groups) == 7 + 6 + 1 * 2       # bias-less convs; the last ConvTranspose keeps its bias


def test_frozen_state_dict_version_upgrade():
    from lvt_amd.modeling import convstack
    m = convstack.FrozenBatchNorm2d(4)
    sd = {"weight": torch.ones(4), "bias": torch.zeros(4), "running_mean": torch.zeros(4), "running_var": torch.full((4,), 2.0)}
    sd = type(m.state_dict())(sd)
    sd._metadata = {"": {"version": 2}}
    m.load_state_dict(sd)
    assert torch.allclose(m.running_var, torch.full((4,), 2.0 - 1e-5))


@pytest.mark.parametrize("bad", ["IN", "GN", "StdN", "nnSyncBN"])
def test_unsupported_norms_refused(bad):
    with pytest.raises(NotImplementedError, match="BN.*SyncBN.*FrozenBN"):
        _model(bad)
    with pytest.raises(NotImplementedError, match="BN.*SyncBN.*FrozenBN"):
        _model("", enc_norm="", gen_norm=bad)


def test_spectral_refused():
    with pytest.raises(NotImplementedError, match="spectral"):
        _model("BN", **{"MODEL.ENCODER.SPECTRAL": True})
