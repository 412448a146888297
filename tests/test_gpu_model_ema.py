"""Polyak-averaged weights inside the fused optimizers (lvt_adam_step_ema / lvt_rmsprop_step_ema / lvt_ema_swap,
solver/ema.py): the shadows against an fp64 replay, the untouched optimizer trajectory, clipped and skipped steps, the swap,
and the Trainer / train_net wiring."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["adam", "rmsprop", "rmsprop_nomom"]
STEPS = 12
LENGTHS = [1, 3, 4, 1023, 16384, 16385, 40003]     # below / at / one past a 16384-element chunk, odd, three chunks
OFF_P, OFF_E = len(LENGTHS), len(LENGTHS) + 1      # the tensors whose parameter / shadow start 4 bytes off a 16-byte boundary
SHAPES = [(n,) for n in LENGTHS] + [(1000,), (2000,)] + [(3 + i % 5, 4) for i in range(70)]       # 79 tensors: two launches


def _init(i):
    return torch.randn(SHAPES[i], generator=torch.Generator().manual_seed(7000 + i))


def _grad(step, i):
    return torch.randn(SHAPES[i], generator=torch.Generator().manual_seed(100 * step + i))


def _off_view(t):
    """A copy of `t` on the device that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _make(kind, ema, warmup=True, decay=0.999):
    """Parameters and a fused optimizer over SHAPES: three learning rates, weight decay on every other tensor.  With `ema`,
    the shadow of tensor OFF_E is handed over through the optimizer's state, 4 bytes off a 16-byte boundary."""
    from lvt_amd.solver.fused import FusedAdam, FusedRMSprop
    ps = [torch.nn.Parameter(_off_view(_init(i)) if i == OFF_P else _init(i).to(DEV)) for i in range(len(SHAPES))]
    groups = [{"params": [p], "lr": 1e-2 * (1 + i % 3), "weight_decay": 0.0 if i % 2 else 1e-3} for i, p in enumerate(ps)]
    if kind == "adam":
        opt = FusedAdam(groups, 1e-2, betas=(0.9, 0.9))
    else:
        opt = FusedRMSprop(groups, 1e-2, alpha=0.95, momentum=0.9 if kind == "rmsprop" else 0.0)
    if ema:
        p = ps[OFF_E]
        st = {"step": 0}
        names = ("exp_avg", "exp_avg_sq") if kind == "adam" else (("square_avg", "momentum_buffer") if kind == "rmsprop" else ("square_avg",))
        for name in names:
            st[name] = torch.zeros_like(p)
        st["ema"] = _off_view(p.detach().cpu())
        opt.state[p] = st
        opt.enable_ema(decay, warmup)
        assert opt.state[p]["ema"].data_ptr() % 16 == 4
    return ps, opt


def _set_grads(ps, step):
    for i, p in enumerate(ps):
        p.grad = None if (i == 4 and step % 2) else _grad(step, i).to(DEV)        # tensor 4 gets no gradient on odd steps


def _state_tensors(opt, ps, skip=("ema",)):
    return [v for p in ps for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v) and k not in skip]


def _shadows(opt, ps):
    return [opt.state[p]["ema"] for p in ps]


def _run(kind, ema, steps=STEPS, clip=None, trace=False):
    """-> (params, optimizer, [per step: list of CPU copies of every parameter] if trace)."""
    ps, opt = _make(kind, ema)
    hist = []
    for step in range(steps):
        _set_grads(ps, step)
        if clip is not None:
            opt.set_grad_clip(*clip)
        opt.step()
        if trace:
            hist.append([p.detach().cpu() for p in ps])
    return ps, opt, hist


def _record(coef, skip=0):
    rec = torch.zeros(4, dtype=torch.float32, device=DEV)            # lvt_clip_record {norm, coef, skip, reserved}
    rec[0], rec[1] = 1.0, coef
    rec.view(torch.int32)[2] = skip
    return rec


def _check_against_fp64(kind, clip):
    """Replays E_k = E_{k-1} + w_k (P_k - E_{k-1}) in fp64 from E_0 = P_0 on the parameters the GPU produced, and checks the
    shadows after every step: |e_k - E_k| <= k 2^-21 A, A the largest |p| or |e| the TENSOR has seen so far.  Per update the
    kernel rounds p - e (<= 2A 2^-24, then scaled by w <= 0.9), the fused multiply-add (<= A 2^-24) and w itself (2^-24
    relative, on |p - e| <= 2A): under 5 A 2^-24 = 0.625 A 2^-21, and a decay <= 1 does not amplify what came before."""
    from lvt_amd.solver.ema import ema_decay_at
    ps, opt = _make(kind, True)
    ref = [_init(i).double() for i in range(len(SHAPES))]
    amax = [float(r.abs().max()) for r in ref]
    updates = [0] * len(SHAPES)           # a tensor without a gradient is not in the launch: its shadow waits
    worst = 0.0
    for step in range(STEPS):
        _set_grads(ps, step)
        if clip is not None:
            opt.set_grad_clip(*clip)
        opt.step()
        w = 1.0 - ema_decay_at(step, 0.999, True)
        for i, p in enumerate(ps):
            if p.grad is None:
                assert i == 4
                continue
            updates[i] += 1
            pk = p.detach().cpu().double()
            ref[i] = ref[i] + w * (pk - ref[i])
            e = opt.state[p]["ema"].cpu().double()
            amax[i] = max(amax[i], float(pk.abs().max()), float(e.abs().max()))
            err = float((e - ref[i]).abs().max())
            bound = updates[i] * 2.0 ** -21 * amax[i]
            worst = max(worst, err / bound)
            assert err <= bound, (kind, step, i, err, bound)
    assert opt.ema_updates == STEPS
    print("%s: worst |e - E| / bound over %d steps: %.3f" % (kind, STEPS, worst))
    return ps, opt


def _check_trajectory(kind, clip):
    pa, oa, _ = _run(kind, True, clip=clip)
    pb, ob, _ = _run(kind, False, clip=clip)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), i
    sa, sb = _state_tensors(oa, pa), _state_tensors(ob, pb)
    assert len(sa) == len(sb) == len(SHAPES) * (1 if kind == "rmsprop_nomom" else 2)
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)
    assert all("ema" not in ob.state[p] for p in pb)
    # the average did move, and is not the parameter
    assert all(not torch.equal(e, p) for e, p in zip(_shadows(oa, pa), pa))


# ---- 1. the shadows against fp64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_shadows_against_fp64(kind):
    _check_against_fp64(kind, None)


# ---- 2. the optimizer's own trajectory is untouched ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_trajectory_is_untouched(kind):
    _check_trajectory(kind, None)


# ---- 3. clipping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_clipped_step(kind):
    """A record with coef = 0.5: the same two checks against the `_scaled` step."""
    clip = (_record(0.5), 0.0)
    _check_against_fp64(kind, clip)
    _check_trajectory(kind, clip)
    # and the clip did bind: an unclipped run differs
    pa, _, _ = _run(kind, True, steps=2, clip=clip)
    pc, _, _ = _run(kind, True, steps=2)
    assert not torch.equal(pa[5], pc[5])


@pytest.mark.parametrize("kind", KINDS)
def test_clamp_only(kind):
    clip = (None, 0.5)
    _check_against_fp64(kind, clip)
    _check_trajectory(kind, clip)
    pa, _, _ = _run(kind, True, steps=2, clip=clip)
    pc, _, _ = _run(kind, True, steps=2)
    assert not torch.equal(pa[5], pc[5])


@pytest.mark.parametrize("kind", KINDS)
def test_skipped_step_keeps_every_bit(kind):
    ps, opt, _ = _run(kind, True, steps=2)
    before_p = [p.detach().clone() for p in ps]
    before_s = [s.clone() for s in _state_tensors(opt, ps, skip=())]
    assert len(before_s) == len(SHAPES) * (2 if kind == "rmsprop_nomom" else 3)       # the shadows are among them
    _set_grads(ps, 2)
    opt.set_grad_clip(_record(0.0, skip=1), 0.0)
    opt.step()
    for a, b in zip(ps, before_p):
        assert torch.equal(a, b)
    for a, b in zip(_state_tensors(opt, ps, skip=()), before_s):
        assert torch.equal(a, b)
    assert opt.ema_updates == 3                      # the host has counted the skipped step
    _set_grads(ps, 3)
    opt.step()
    assert not torch.equal(ps[0], before_p[0]) and not torch.equal(opt.state[ps[0]]["ema"], before_s[0])


# ---- 4. bit reproducibility ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_bit_reproducible(kind):
    p1, o1, _ = _run(kind, True)
    p2, o2, _ = _run(kind, True)
    for a, b in zip(_shadows(o1, p1), _shadows(o2, p2)):
        assert torch.equal(a, b)


# ---- 5. the swap ---------------------------------------------------------------------------------------------------------------
def test_swap_kernel_exchanges_and_restores():
    """lvt_ema_swap on the tensor set (scalar and float4 lanes, > 64 pairs): exchanged once, restored by the second call."""
    from lvt_amd.hip import binding as L
    a = [_off_view(_init(i)) if i == OFF_P else _init(i).to(DEV) for i in range(len(SHAPES))]
    b = [_off_view(_grad(0, i)) if i == OFF_E else _grad(0, i).to(DEV) for i in range(len(SHAPES))]
    a0, b0 = [t.clone() for t in a], [t.clone() for t in b]
    n = len(a)
    pa, pb, cnt = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_longlong * n)()
    for i in range(n):
        pa[i], pb[i], cnt[i] = a[i].data_ptr(), b[i].data_ptr(), a[i].numel()
    L.check(L.lib().lvt_ema_swap(pa, pb, cnt, n, L.stream_ptr()), "lvt_ema_swap")
    for i in range(n):
        assert torch.equal(a[i], b0[i]) and torch.equal(b[i], a0[i]), i
    L.check(L.lib().lvt_ema_swap(pa, pb, cnt, n, L.stream_ptr()), "lvt_ema_swap")
    for i in range(n):
        assert torch.equal(a[i], a0[i]) and torch.equal(b[i], b0[i]), i


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_averaged_swaps_and_restores(kind):
    from lvt_amd.hip import LvtError
    from lvt_amd.solver.ema import ModelEma
    ps, opt, _ = _run(kind, True, steps=3)
    ema = ModelEma([{"optimizer": opt}], 0.999, True)
    assert opt.ema_updates == 3 and ema.updates == 3            # enabling again keeps shadows and count
    live = [p.detach().clone() for p in ps]
    avg = [e.clone() for e in _shadows(opt, ps)]
    ptrs = [p.data_ptr() for p in ps]
    with ema.averaged():
        for i, p in enumerate(ps):
            assert torch.equal(p, avg[i]) and torch.equal(opt.state[p]["ema"], live[i]), i
        with pytest.raises(LvtError):
            with ema.averaged():
                pass
    for i, p in enumerate(ps):
        assert torch.equal(p, live[i]) and torch.equal(opt.state[p]["ema"], avg[i]), i
    assert ptrs == [p.data_ptr() for p in ps]                   # contents moved, pointers did not


def _vq_trained(steps=2):
    """A small VQ-VAE (PR-DVQVAE2 on 2 frames), `steps` optimizer steps with averaging on -> (model, ModelEma, batch)."""
    import seeded
    from util_models import vqvae_cfg, vqvae_seeded
    from lvt_amd.solver.ema import ModelEma
    from lvt_amd.utils.events import EventStorage
    model, _, _, _ = vqvae_seeded(21, scale=0.05, device=DEV)
    model.train()
    optimizers, _ = model.configure_optimizers_and_checkpointers()
    ema = ModelEma(optimizers, 0.9, True)
    x = seeded.seeded_input("model_ema", (2, 3, 64, 64), 22)
    batch = [{"image": x[i].numpy()} for i in range(2)]
    with EventStorage(0):
        for _ in range(steps):
            sum(model(batch, mode="supervised").values()).backward()
            for o in optimizers:
                o["optimizer"].step()
            for o in optimizers:
                o["optimizer"].zero_grad()
    return model, ema, batch, vqvae_cfg


@pytest.mark.parametrize("amax_check", [False, True])
def test_forward_under_averaged_equals_a_model_loaded_from_the_twin(amax_check):
    """The forward under `averaged()` is the forward of a fresh model that loaded the averaged state dicts; in f16x2 mode under
    LVT_AMAX_CHECK, so that a max-|.| record that survived the swap would be caught."""
    from lvt_amd.hip import binding as L
    from lvt_amd.modeling import build_model
    assert L.get_math_mode() == "f16x2"
    model, ema, batch, vqvae_cfg = _vq_trained()
    model.eval()
    old = L.AMAX_CHECK
    L.AMAX_CHECK = amax_check
    try:
        with torch.no_grad():
            live = model(batch, mode="inference")
            with ema.averaged():
                sd = {name: {k: v.clone() for k, v in getattr(model, name).state_dict().items()}
                      for name in ("encoder", "generator", "codebook")}
                avg = model(batch, mode="inference")
            again = model(batch, mode="inference")
            fresh = build_model(vqvae_cfg(DEV))
            for name, state in sd.items():
                getattr(fresh, name).load_state_dict(state)
            fresh.eval()
            twin = fresh(batch, mode="inference")
    finally:
        L.AMAX_CHECK = old
    for a, b, c, d in zip(avg, twin, live, again):
        for k in ("reconstruction", "latent"):
            assert torch.equal(a[k], b[k]), k
            assert torch.equal(c[k], d[k]), k                       # and the live weights are back
        assert not torch.equal(a["reconstruction"], c["reconstruction"])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lvt_amd.hip import LvtError
    from lvt_amd.hip import binding as L
    from lvt_amd.solver.fused import FusedAdam, _entries, _shadows as shadow_table
    p = torch.nn.Parameter(torch.zeros(8, device=DEV))
    opt = FusedAdam([p], 1e-3)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            opt.enable_ema(bad)
    g, m, v = torch.ones(8, device=DEV), torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    ents = [(p, g, m, v, 1e-3, 0.0)]
    with pytest.raises(LvtError):                                # one shadow too many
        shadow_table([torch.zeros(8, device=DEV)] * 2, ents)
    with pytest.raises(LvtError):                                # a shadow of another size
        shadow_table([torch.zeros(4, device=DEV)], ents)
    null = (C.c_void_p * 1)(None)
    rc = L.lib().lvt_adam_step_ema(_entries(ents), null, 1, 0.9, 0.999, 1e-8, 1, 0.1, None, 0.0, L.stream_ptr())
    assert rc == -1
    with pytest.raises(LvtError):
        L.check(rc, "lvt_adam_step_ema")
    torch.cuda.synchronize()
    assert float(p.detach().abs().max()) == 0.0 and float(m.abs().max()) == 0.0        # nothing was launched


# ---- 7. through the Trainer and train_net ----------------------------------------------------------------------------------------
def test_trainer_respects_accumulation_and_resumes_from_the_twin(tmp_path):
    import seeded
    from util_models import vqvae_cfg
    from lvt_amd.engine.trainer import Trainer
    from lvt_amd.modeling import build_model
    from lvt_amd.solver.ema import ema_twin

    def trainer(nbatches):
        cfg = vqvae_cfg(DEV)
        cfg.OUTPUT_DIR = str(tmp_path)
        cfg.SOLVER.MAX_ITER = 4
        cfg.SOLVER.CHECKPOINT_PERIOD = 10 ** 6
        cfg.SOLVER.ACCUMULATION_STEPS = 2
        cfg.SOLVER.MODEL_EMA.ENABLED = True
        cfg.SOLVER.MODEL_EMA.DECAY = 0.9
        torch.manual_seed(11)
        model = build_model(cfg)
        x = seeded.seeded_input("model_ema", (2, 3, 64, 64), 12)
        batch = [{"image": x[i].numpy()} for i in range(2)]
        return Trainer(cfg, model, iter([batch] * nbatches), log_period=10 ** 6)

    t = trainer(4)
    assert t.model_ema is not None and len(t.model_ema.optimizers) == 2
    t.train()
    assert [o["optimizer"].ema_updates for o in t.optimizers] == [2, 2]         # 4 iterations, a step every second one
    for sub in ("netE", "netG"):
        live = os.path.join(str(tmp_path), sub, "model_final.pth")
        assert open(os.path.join(str(tmp_path), sub, "last_checkpoint")).read() == "model_final.pth"
        twin = torch.load(ema_twin(live))
        assert twin["ema_updates"] == 2 and twin["iteration"] == 3
    assert not os.path.exists(os.path.join(str(tmp_path), "netC", "model_final_ema.pth"))       # no optimizer: no twin
    shadows = {k: v.clone() for k, v in t.model_ema.shadows(t.model.encoder).items()}
    live = {k: v.detach().clone() for k, v in t.model.encoder.named_parameters()}
    # a new trainer on the same directory: the live weights and the shadows come back, and the schedule goes on
    r = trainer(1)
    r.resume_or_load(resume=True)
    assert [o["optimizer"].ema_updates for o in r.optimizers] == [2, 2]
    got = r.model_ema.shadows(r.model.encoder)
    assert set(got) == set(shadows) == set(live)
    for k in shadows:
        assert torch.equal(got[k], shadows[k]), k
        assert torch.equal(dict(r.model.encoder.named_parameters())[k], live[k]), k
    assert any(not torch.equal(shadows[k], live[k]) for k in shadows)


def test_train_net_writes_and_evaluates_the_averaged_twins(tmp_path):
    out = str(tmp_path / "vq")
    base = [sys.executable, "tools/train_net.py", "--config-file", "configs/vqvae/PR-DVQVAE2.yaml", "--synthetic"]
    opts = ["OUTPUT_DIR", out, "SOLVER.IMS_PER_BATCH", "4", "SOLVER.MODEL_EMA.ENABLED", "True"]
    r = subprocess.run(["timeout", "-k", "10", "600"] + base + ["--max-iter", "3"] + opts + ["SOLVER.MAX_ITER", "3"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for sub in ("netE", "netG"):
        live = torch.load(os.path.join(out, sub, "model_final.pth"))
        twin = torch.load(os.path.join(out, sub, "model_final_ema.pth"))
        assert set(twin) == {"model", "iteration", "ema_updates"} and twin["ema_updates"] == 3
        assert list(twin["model"]) == list(live["model"])
        floats = [k for k, v in live["model"].items() if v.is_floating_point() and v.numel() > 1]
        assert floats
        for k in floats:
            assert not torch.equal(twin["model"][k], live["model"][k]), k           # (this config has no float buffers)
        for k in set(live["model"]) - set(floats):
            assert torch.equal(twin["model"][k], live["model"][k]), k
        assert open(os.path.join(out, sub, "last_checkpoint")).read() == "model_final.pth"
    assert not os.path.exists(os.path.join(out, "netC", "model_final_ema.pth"))         # the EMA codebook has no optimizer
    weights = []
    for key, sub in (("MODEL.ENCODER.WEIGHTS", "netE"), ("MODEL.GENERATOR.WEIGHTS", "netG"), ("MODEL.CODEBOOK.WEIGHTS", "netC")):
        weights += [key, os.path.join(out, sub, "model_final.pth")]
    r = subprocess.run(["timeout", "-k", "10", "600"] + base + ["--eval-only", "--eval-batches", "1"] + opts + weights,
                       cwd=ROOT, capture_output=True, text=True)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "evaluation results" in log
    for sub in ("netE", "netG"):
        assert "loading averaged weights %s" % os.path.join(out, sub, "model_final_ema.pth") in log
    assert "netC/model_final_ema.pth" not in log
