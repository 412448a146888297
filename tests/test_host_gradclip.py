"""Host side of gradient clipping (SOLVER.CLIP_GRADIENTS): config keys, the clipper factory's refusals, the C-ABI table."""
import glob
import os
import re

import pytest

from conftest import ROOT


def _cfg(**clip):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    for k, v in clip.items():
        cfg.SOLVER.CLIP_GRADIENTS[k] = v
    return cfg


def test_defaults_and_shipped_yamls():
    from lvt_amd.config import get_cfg
    c = get_cfg().SOLVER.CLIP_GRADIENTS
    assert c.ENABLED is False and c.CLIP_TYPE == "norm" and c.CLIP_VALUE == 1.0 and c.NORM_TYPE == 2.0
    yamls = sorted(glob.glob(os.path.join(ROOT, "configs", "*", "*.yaml")))
    assert len(yamls) == 7
    for path in yamls:
        cfg = get_cfg()
        cfg.merge_from_file(path)
        assert cfg.SOLVER.CLIP_GRADIENTS.ENABLED is False, path
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "value",
                         "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", "0.5"])
    c = cfg.SOLVER.CLIP_GRADIENTS
    assert c.ENABLED is True and c.CLIP_TYPE == "value" and c.CLIP_VALUE == 0.5


def test_disabled_builds_no_clipper():
    from lvt_amd.solver.build import build_grad_clipper
    assert build_grad_clipper(_cfg(), []) is None
    assert build_grad_clipper(_cfg(CLIP_TYPE="value", CLIP_VALUE=0.5), []) is None


@pytest.mark.parametrize("enabled", [False, True])
@pytest.mark.parametrize("bad", [{"CLIP_TYPE": "foo"}, {"NORM_TYPE": 1.0}, {"CLIP_VALUE": 0}, {"CLIP_VALUE": -1.0},
                                 {"NORM_TYPE": float("inf")}])
def test_bad_settings_are_value_errors(bad, enabled):
    from lvt_amd.solver.build import build_grad_clipper
    with pytest.raises(ValueError):
        build_grad_clipper(_cfg(ENABLED=enabled, **bad), [])


def test_clipper_refuses_optimizers_without_the_fused_step():
    """Clipping happens inside the fused step kernels: handing the clipper a torch optimizer is an error, not a fallback."""
    import torch
    from lvt_amd.hip import LvtError
    from lvt_amd.solver.build import build_grad_clipper
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(LvtError):
        build_grad_clipper(_cfg(ENABLED=True), [{"optimizer": opt}])


def test_set_grad_clip_is_consumed_once():
    import torch
    from lvt_amd.solver.fused import FusedAdam
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError):
        opt.set_grad_clip(None, 0.0)
    opt.set_grad_clip(None, 0.5)
    assert opt._take_clip() == (None, 0.5) and opt._take_clip() is None


def test_abi_table_and_version():
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    version = int(re.search(r"int lvt_version\(void\);\s*/\*\s*(\d+)\s*=", header).group(1))
    assert L.ABI_VERSION == version == 680 == L.lib().lvt_version()
    assert "`lvt_version()` == %d" % version in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    new = {"lvt_grad_sqnorm_partials", "lvt_grad_sqnorm", "lvt_grad_clip_coef", "lvt_adam_step_scaled",
           "lvt_rmsprop_step_scaled"}
    assert new <= set(L.declared_symbols())
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, header), name
    # argument validation comes before any device work
    lib = L.lib()
    e = (L.GradEntry * 2)()
    assert lib.lvt_grad_sqnorm_partials(e, 2) == -1                      # null gradient
    e[0].g, e[0].n, e[1].g, e[1].n = 4096, 16385, 8192 + 4, 16384
    assert lib.lvt_grad_sqnorm_partials(e, 2) == 3                       # 16385 elements end one element into a second chunk
    assert lib.lvt_grad_sqnorm(e, 2, 256, 2, None) == -1 and b"partials" in lib.lvt_last_error()
    assert lib.lvt_grad_clip_coef(256, 3, 0.0, 512, None, None) == -1 and b"max_norm" in lib.lvt_last_error()
    o = (L.OptEntry * 1)()
    assert lib.lvt_adam_step_scaled(o, 1, 0.9, 0.9, 1e-8, 1, None, 0.0, None) == -1
    assert lib.lvt_rmsprop_step_scaled(o, 1, 0.9, 1e-8, 0.0, None, -1.0, None) == -1
