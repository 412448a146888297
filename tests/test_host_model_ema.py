"""Host side of the Polyak-averaged weights (SOLVER.MODEL_EMA): config keys, the factory's refusals, the decay schedule, the
C-ABI table, the optimizer's state dict and the naming of the averaged checkpoint twins."""
import ctypes as C
import glob
import math
import os
import re

import pytest
import torch

from conftest import ROOT


def _cfg(**ema):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    for k, v in ema.items():
        cfg.SOLVER.MODEL_EMA[k] = v
    return cfg


def test_defaults_and_shipped_yamls():
    from lvt_amd.config import get_cfg
    c = get_cfg().SOLVER.MODEL_EMA
    assert c.ENABLED is False and c.DECAY == 0.9999 and c.WARMUP is True
    yamls = sorted(glob.glob(os.path.join(ROOT, "configs", "*", "*.yaml")))
    assert len(yamls) == 7
    for path in yamls:
        cfg = get_cfg()
        cfg.merge_from_file(path)
        assert cfg.SOLVER.MODEL_EMA.ENABLED is False, path
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.MODEL_EMA.ENABLED", "True", "SOLVER.MODEL_EMA.DECAY", "0.99", "SOLVER.MODEL_EMA.WARMUP", "False"])
    c = cfg.SOLVER.MODEL_EMA
    assert c.ENABLED is True and c.DECAY == 0.99 and c.WARMUP is False


def test_disabled_builds_nothing():
    from lvt_amd.solver.build import build_model_ema
    assert build_model_ema(_cfg(), []) is None
    assert build_model_ema(_cfg(DECAY=0.5, WARMUP=False), []) is None


@pytest.mark.parametrize("enabled", [False, True])
@pytest.mark.parametrize("decay", [1.0, -0.1, float("nan")])
def test_bad_decay_is_a_value_error(decay, enabled):
    from lvt_amd.solver.build import build_model_ema
    with pytest.raises(ValueError):
        build_model_ema(_cfg(ENABLED=enabled, DECAY=decay), [])


def test_enable_ema_refuses_a_bad_decay():
    from lvt_amd.solver.fused import FusedAdam, FusedRMSprop
    for cls in (FusedAdam, FusedRMSprop):
        opt = cls([torch.nn.Parameter(torch.zeros(3))])
        for bad in (1.0, -0.1, float("nan"), float("inf"), 1.5):
            with pytest.raises(ValueError):
                opt.enable_ema(bad)
        opt.enable_ema(0.0)
        opt.enable_ema(0.9999, warmup=False)


def test_model_ema_refuses_optimizers_without_the_fused_step():
    from lvt_amd.hip import LvtError
    from lvt_amd.solver.build import build_model_ema
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(LvtError):
        build_model_ema(_cfg(ENABLED=True), [{"optimizer": opt}])


def test_decay_schedule():
    from lvt_amd.solver.ema import ema_decay_at
    assert ema_decay_at(0, 0.9999, True) == 0.1
    assert ema_decay_at(1, 0.9999, True) == 2.0 / 11.0
    assert ema_decay_at(80, 0.9999, True) == 0.9
    assert ema_decay_at(10 ** 9, 0.9999, True) == 0.9999
    assert ema_decay_at(0, 0.05, True) == 0.05                       # the warm-up never raises the decay above DECAY
    for t in (0, 1, 1000):
        assert ema_decay_at(t, 0.9999, False) == 0.9999
    # monotone, and DECAY from the step where (1 + t) / (10 + t) reaches it: t = (10 d - 1) / (1 - d)
    vals = [ema_decay_at(t, 0.99, True) for t in range(2000)]
    assert all(b >= a for a, b in zip(vals, vals[1:]))
    first = next(t for t, v in enumerate(vals) if v == 0.99)
    assert first == math.ceil((10 * 0.99 - 1) / (1 - 0.99) - 1e-9)


def test_abi_table_and_argument_validation():
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    new = {"lvt_adam_step_ema", "lvt_rmsprop_step_ema", "lvt_ema_swap"}
    assert new <= set(L.declared_symbols())
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in text, name
    lib = L.lib()
    sigs = lib._lvt_sigs
    vp, ci, cf, cll, P = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.POINTER
    # the header's argument lists: (entries, ema, n, beta1, beta2, eps, step, w, gscale, clamp, stream) and so on
    assert sigs["lvt_adam_step_ema"] == (ci, [P(L.OptEntry), P(vp), ci, cf, cf, cf, ci, cf, vp, cf, vp])
    assert sigs["lvt_rmsprop_step_ema"] == (ci, [P(L.OptEntry), P(vp), ci, cf, cf, cf, cf, vp, cf, vp])
    assert sigs["lvt_ema_swap"] == (ci, [P(vp), P(vp), P(cll), ci, vp])
    assert re.search(r"lvt_adam_step_ema\(const lvt_opt_entry \*entries, float \*const \*ema, int n, float beta1, float beta2, "
                     r"float eps, int step,\s*float w, const lvt_clip_record \*gscale, float clamp, void \*stream\)", header)
    assert re.search(r"lvt_rmsprop_step_ema\(const lvt_opt_entry \*entries, float \*const \*ema, int n, float alpha, float eps, "
                     r"float momentum,\s*float w, const lvt_clip_record \*gscale, float clamp, void \*stream\)", header)
    assert re.search(r"lvt_ema_swap\(float \*const \*a, float \*const \*b, const long long \*counts, int n, void \*stream\)", header)
    assert C.sizeof(L.OptEntry) == 48                                 # lvt_opt_entry is public ABI and did not grow
    # argument validation comes before any device work (no GPU here: a launch would fail differently)
    o = (L.OptEntry * 1)()
    o[0].p, o[0].g, o[0].s0, o[0].s1, o[0].n = 4096, 8192, 12288, 16384, 8
    sh = (vp * 1)(20480)
    null = (vp * 1)(None)
    assert lib.lvt_adam_step_ema(o, None, 1, 0.9, 0.9, 1e-8, 1, 0.1, None, 0.0, None) == -1
    assert lib.lvt_adam_step_ema(o, null, 1, 0.9, 0.9, 1e-8, 1, 0.1, None, 0.0, None) == -1
    assert b"shadow" in lib.lvt_last_error()
    assert lib.lvt_adam_step_ema(o, sh, 1, 0.9, 0.9, 1e-8, 0, 0.1, None, 0.0, None) == -1         # step 0
    assert lib.lvt_adam_step_ema(o, sh, 1, 0.9, 0.9, 1e-8, 1, 1.5, None, 0.0, None) == -1         # w outside [0, 1]
    assert lib.lvt_adam_step_ema(o, sh, 1, 0.9, 0.9, 1e-8, 1, float("nan"), None, 0.0, None) == -1
    assert lib.lvt_adam_step_ema(o, sh, 1, 0.9, 0.9, 1e-8, 1, 0.1, None, -1.0, None) == -1        # negative clamp
    assert lib.lvt_adam_step_ema(o, sh, 1, 0.9, 0.9, 1e-8, 1, 0.1, 4096 + 4, 0.0, None) == -1     # misaligned record
    assert lib.lvt_rmsprop_step_ema(o, null, 1, 0.9, 1e-8, 0.0, 0.1, None, 0.0, None) == -1
    assert lib.lvt_rmsprop_step_ema(o, (vp * 1)(4096), 1, 0.9, 1e-8, 0.0, 0.1, None, 0.0, None) == -1     # the parameter itself
    assert lib.lvt_rmsprop_step_ema(o, sh, 0, 0.9, 1e-8, 0.0, 0.1, None, 0.0, None) == -1
    a, b, n = (vp * 1)(4096), (vp * 1)(8192), (cll * 1)(8)
    assert lib.lvt_ema_swap(a, null, n, 1, None) == -1 and b"ema_swap" in lib.lvt_last_error()
    assert lib.lvt_ema_swap(a, b, (cll * 1)(0), 1, None) == -1
    assert lib.lvt_ema_swap(a, a, n, 1, None) == -1
    assert lib.lvt_ema_swap(a, (vp * 1)(4096 + 16), n, 1, None) == -1                              # 8 floats from 4096 overlap 4112
    assert lib.lvt_ema_swap(a, (vp * 1)(8192 + 2), n, 1, None) == -1
    assert lib.lvt_ema_swap(None, b, n, 1, None) == -1 and lib.lvt_ema_swap(a, b, None, 1, None) == -1


def test_a_bad_entry_behind_the_first_launch_is_refused_before_any_launch():
    """70 entries are two launches (64 + 6).  Entry 66 is bad: the call must name it and return LVT_EINVAL -- had the first 64
    been launched before the table was read to its end, the launch (of fake pointers; without a GPU, of anything) would have
    failed differently, or worse, run."""
    from lvt_amd.hip import binding as L
    lib = L.lib()
    vp, cll = C.c_void_p, C.c_longlong
    n, bad = 70, 66
    at = lambda i, k: ((i + 1) << 20) + 4096 * k                     # noqa: E731  (stream k of tensor i: 1 MB apart, 16-byte aligned)
    o = (L.OptEntry * n)()
    for i in range(n):
        o[i].p, o[i].g, o[i].s0, o[i].s1, o[i].n, o[i].lr = at(i, 0), at(i, 1), at(i, 2), at(i, 3), 8, 1e-3
    o[bad].g = None
    sh = (vp * n)(*[at(i, 4) for i in range(n)])
    for name, call in (("adam_step", lambda: lib.lvt_adam_step(o, n, 0.9, 0.9, 1e-8, 1, None)),
                       ("rmsprop_step_scaled", lambda: lib.lvt_rmsprop_step_scaled(o, n, 0.9, 1e-8, 0.0, None, 0.5, None)),
                       ("adam_step_ema", lambda: lib.lvt_adam_step_ema(o, sh, n, 0.9, 0.9, 1e-8, 1, 0.1, None, 0.0, None))):
        assert call() == -1, name
        err = lib.lvt_last_error()
        assert b"66" in err and name.encode() in err, err
    a, b = (vp * n)(*[at(i, 0) for i in range(n)]), (vp * n)(*[at(i, 1) for i in range(n)])
    b[bad] = at(bad, 0) + 16                                          # b[66] starts 16 bytes into the 32 of a[66]
    assert lib.lvt_ema_swap(a, b, (cll * n)(*[8] * n), n, None) == -1
    err = lib.lvt_last_error()
    assert b"66" in err and b"ema_swap" in err, err


def test_shadow_table_refuses_a_wrong_count():
    """The pointer table handed to the `_ema` entry points has one shadow per entry: anything else is an error, not a launch."""
    from lvt_amd.hip import LvtError
    from lvt_amd.solver.fused import _shadows
    p = torch.zeros(3)
    ents = [(p, p, p, p, 1e-3, 0.0)] * 2
    with pytest.raises(LvtError):
        _shadows([p], ents)
    with pytest.raises(LvtError):
        _shadows([None, None], ents)


def test_state_dict_carries_the_shadows_and_loads_into_torch():
    from lvt_amd.solver.fused import FusedAdam
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    opt = FusedAdam(ps, 1e-3)
    for p in ps:                                            # state as a step would have made it (no step on the CPU)
        opt.state[p] = {"step": 1, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    assert all("ema" not in opt.state[p] for p in ps)
    opt.enable_ema(0.999)
    for p in ps:
        e = opt.state[p]["ema"]
        assert torch.equal(e, p.detach()) and e.data_ptr() != p.data_ptr() and not e.requires_grad
    sd = opt.state_dict()
    assert len(sd["state"]) == 2
    for i, p in enumerate(ps):
        assert set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
        assert torch.equal(sd["state"][i]["ema"], p.detach())
    ref = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], 1e-3)
    ref.load_state_dict(sd)
    assert all("ema" in st for st in ref.state.values()) and len(ref.state) == 2
    # and back into a fused optimizer, which then owns shadows without another enable_ema clone
    again = FusedAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], 1e-3)
    again.load_state_dict(sd)
    kept = [st["ema"] for st in again.state.values()]
    again.enable_ema(0.999)
    assert all(a is b for a, b in zip(kept, [st["ema"] for st in again.state.values()]))
    # a parameter without state gets no shadow before its state exists
    lone = FusedAdam([torch.nn.Parameter(torch.zeros(3))])
    lone.enable_ema(0.5)
    assert len(lone.state_dict()["state"]) == 0
    # a CPU parameter is refused by the step, as without averaging
    from lvt_amd.hip import LvtError
    lone.param_groups[0]["params"][0].grad = torch.zeros(3)
    with pytest.raises(LvtError):
        lone.step()


def test_twin_naming_and_untouched_marker(tmp_path):
    from lvt_amd.solver.ema import ema_twin
    from lvt_amd.utils.checkpoint import Checkpointer, PeriodicCheckpointer
    assert ema_twin("/a/b/model_0000099.pth") == "/a/b/model_0000099_ema.pth"
    assert ema_twin("model_final.pth") == "model_final_ema.pth"
    module = torch.nn.Linear(3, 2)
    ck = Checkpointer(module, str(tmp_path / "netG"))
    pc = PeriodicCheckpointer(ck, 2, max_iter=4)
    assert pc.due(0) == [] and pc.due(1) == ["model_0000001"] and pc.due(3) == ["model_0000003", "model_final"]
    for it in range(4):
        pc.step(it)
        with torch.no_grad():
            module.weight.add_(1.0)                         # stands for the swap: the twin records the module as it is now
        pc.step_twin(it, ema_updates=it + 1)
        with torch.no_grad():
            module.weight.sub_(1.0)
    names = sorted(os.listdir(str(tmp_path / "netG")))
    assert names == ["last_checkpoint", "model_0000001.pth", "model_0000001_ema.pth", "model_0000003.pth", "model_0000003_ema.pth",
                     "model_final.pth", "model_final_ema.pth"]
    assert open(str(tmp_path / "netG" / "last_checkpoint")).read() == "model_final.pth"
    assert ck.get_checkpoint_file() == str(tmp_path / "netG" / "model_final.pth")
    live = torch.load(str(tmp_path / "netG" / "model_final.pth"))
    twin = torch.load(ema_twin(ck.get_checkpoint_file()))
    assert set(twin) == {"model", "iteration", "ema_updates"} and twin["iteration"] == 3 and twin["ema_updates"] == 4
    assert list(twin["model"]) == list(live["model"])
    assert torch.equal(twin["model"]["weight"], live["model"]["weight"] + 1.0)
    assert torch.equal(twin["model"]["bias"], live["model"]["bias"])
    # a twin is an ordinary checkpoint for a module of the same kind
    other = Checkpointer(torch.nn.Linear(3, 2), str(tmp_path / "other"))
    other.load(ema_twin(ck.get_checkpoint_file()))
    assert torch.equal(other.model.weight, twin["model"]["weight"])
