"""Gradient clipping inside the fused optimizers (solver/clip.py, lvt_grad_sqnorm / lvt_grad_clip_coef / lvt_*_step_scaled):
the global norm against fp64, clipped steps against torch.nn.utils.clip_grad_* + torch.optim, the non-finite skip, and the
Trainer / data-parallel wiring."""
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from conftest import rel_err
from test_gpu_optim import _params as _optim_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["adam", "rmsprop", "rmsprop_nomom"]
OFFSET = -1          # index of the parameter whose gradient is a view one element into its storage


def _params(seed):
    """The tensors of test_gpu_optim (> 64 of them, sizes 1, 5, 100000, ragged), one that ends one element into a second
    16384-element chunk, and one more whose GRADIENT will be 4-byte aligned only."""
    g = torch.Generator().manual_seed(seed + 1000)
    return _optim_params(seed) + [torch.randn(16385, generator=g), torch.randn(1000, generator=g)]


SHAPES = [tuple(p.shape) for p in _params(0)]


def _grad(step, i, scale=1.0):
    return scale * torch.randn(SHAPES[i], generator=torch.Generator().manual_seed(100 * step + i))


def _grads(step, scale=1.0):
    """index -> CPU gradient of one step; parameter 4 gets none on odd steps (as in test_fused_matches_torch)."""
    return {i: _grad(step, i, scale) for i in range(len(SHAPES)) if not (i == 4 and step % 2)}


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))


def _set_grads(params, grads, offset_view=True):
    n = len(params)
    for i, p in enumerate(params):
        g = grads.get(i)
        if g is None:
            p.grad = None
        elif offset_view and i == n + OFFSET:
            buf = torch.empty(g.numel() + 1, device=DEV)
            view = buf[1:].view(g.shape)
            view.copy_(g)
            assert view.data_ptr() % 16 == 4
            p.grad = view
        else:
            p.grad = g.to(DEV)


def _groups(ps):
    return [{"params": [p], "lr": 1e-2 * (1 + i % 3), "weight_decay": 0.0 if i % 2 else 1e-3} for i, p in enumerate(ps)]


def _make(kind, fused, seed=0):
    from lvt_amd.solver.fused import FusedAdam, FusedRMSprop
    ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in _params(seed)]
    if kind == "adam":
        cls = FusedAdam if fused else torch.optim.Adam
        return ps, cls(_groups(ps), 1e-2, betas=(0.9, 0.9))
    cls = FusedRMSprop if fused else torch.optim.RMSprop
    return ps, cls(_groups(ps), 1e-2, alpha=0.95, momentum=0.9 if kind == "rmsprop" else 0.0)


def _state_tensors(opt, params):
    return [v for p in params for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]


def _clipper(opt, clip_type, value):
    from lvt_amd.solver.clip import GradClipper
    return GradClipper([opt], clip_type, value, 2.0)


# ---- 1. the norm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e25])
def test_norm_against_fp64(scale):
    """fp64 squares and sums: neither 1e25 (squares overflow fp32) nor 1e-30 (squares vanish in fp32) loses the norm.  Bound
    2^-22: two fp32 roundings of an fp64 result whose own error is around 1e-10."""
    ps, opt = _make("adam", True)
    grads = _grads(0, scale)
    _set_grads(ps, grads)
    clip = _clipper(opt, "norm", 1.0)
    clip.prepare()
    ref = _norm64(grads)
    got = float(clip.norm)
    print("scale %g: norm %.9g, fp64 %.9g, rel %.3g" % (scale, got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 2.0 ** -22 * ref
    assert int(clip.skip) == 0 and int(clip.skipped) == 0


# ---- 2. a clip that does not bind changes nothing -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_inactive_clip_is_exact(kind):
    pa, oa = _make(kind, True)
    pb, ob = _make(kind, True)
    clip = _clipper(oa, "norm", 1e9)
    for step in range(5):
        grads = _grads(step)
        _set_grads(pa, grads)
        _set_grads(pb, grads)
        clip.prepare()
        assert float(clip.coef) == 1.0
        oa.step(); ob.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    sa, sb = _state_tensors(oa, pa), _state_tensors(ob, pb)
    assert len(sa) == len(sb) > 0
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)


# ---- 3. / 4. clipped steps against torch ----------------------------------------------------------------------------------------
def _run_fused(kind, clip_type, value, steps):
    """-> (params, optimizer, clipper, [coef per step], [record per step])."""
    pa, oa = _make(kind, True)
    clip = _clipper(oa, clip_type, value)
    coefs, records = [], []
    for step in range(steps):
        _set_grads(pa, _grads(step))
        clip.prepare()
        if clip_type == "norm":
            coefs.append(float(clip.coef))
            records.append(clip.record.clone())
        oa.step()
    return pa, oa, clip, coefs, records


def _run_torch(kind, clip_type, value, steps):
    pb, ob = _make(kind, False)
    for step in range(steps):
        _set_grads(pb, _grads(step), offset_view=False)
        have = [p for p in pb if p.grad is not None]
        if clip_type == "norm":
            torch.nn.utils.clip_grad_norm_(have, value)
        else:
            torch.nn.utils.clip_grad_value_(have, value)
        ob.step()
    return pb, ob


@pytest.mark.parametrize("kind", KINDS)
def test_active_norm_clip_matches_torch(kind):
    max_norm = 0.3 * _norm64(_grads(0))
    pa, oa, clip, coefs, _ = _run_fused(kind, "norm", max_norm, 5)
    pb, ob = _run_torch(kind, "norm", max_norm, 5)
    print("coef per step:", coefs)
    assert len(coefs) == 5 and all(c < 1.0 for c in coefs)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert rel_err(a, b) < 2e-6, i
    assert int(clip.skipped) == 0
    assert set(oa.state_dict()["state"][0].keys()) == set(ob.state_dict()["state"][0].keys())


@pytest.mark.parametrize("kind", KINDS)
def test_value_clip_matches_torch(kind):
    pa, oa, clip, _, _ = _run_fused(kind, "value", 0.5, 5)
    pb, ob = _run_torch(kind, "value", 0.5, 5)
    assert clip.norm is None                     # no norm pass in this mode
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert rel_err(a, b) < 2e-6, i
    # and the clamp did bind: an unclipped run differs
    pc, oc = _make(kind, True)
    for step in range(5):
        _set_grads(pc, _grads(step))
        oc.step()
    assert max(rel_err(a, c) for a, c in zip(pa, pc)) > 1e-4


# ---- 5. a gradient that is not finite skips the step ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_non_finite_gradient_skips_the_step(kind):
    max_norm = 0.3 * _norm64(_grads(0))
    pa, oa = _make(kind, True)
    clip = _clipper(oa, "norm", max_norm)
    _set_grads(pa, _grads(0))
    clip.prepare(); oa.step()                                        # a finite step first: the state tensors are non-trivial
    assert int(clip.skip) == 0
    last = len(pa) - 1
    for n, (idx, pos, bad) in enumerate([(last, -1, float("nan")), (0, 0, float("inf"))], 1):
        grads = _grads(n)
        grads[idx].view(-1)[pos] = bad
        before_p = [p.detach().clone() for p in pa]
        before_s = [s.clone() for s in _state_tensors(oa, pa)]
        _set_grads(pa, grads)
        clip.prepare(); oa.step()
        for a, b in zip(pa, before_p):
            assert torch.equal(a, b)
        for a, b in zip(_state_tensors(oa, pa), before_s):
            assert torch.equal(a, b)
        assert int(clip.skipped) == n and int(clip.skip) == 1 and float(clip.coef) == 0.0
    # a finite step afterwards
    before_p = [p.detach().clone() for p in pa]
    grads = _grads(3)
    _set_grads(pa, grads)
    clip.prepare(); oa.step()
    assert int(clip.skip) == 0 and int(clip.skipped) == 2 and 0.0 < float(clip.coef) < 1.0
    if kind == "adam":       # its bias correction has counted the skipped steps: no torch twin, but finite and moved
        for i, (a, b) in enumerate(zip(pa, before_p)):
            assert bool(torch.isfinite(a).all()), i
            assert torch.equal(a, b) == (i not in grads), i          # (parameter 4 has no gradient on this step and stays)
        return
    # RMSprop's update does not read the step count: equal to torch's optimizer that simply did not take the bad steps
    pb, ob = _make(kind, False)
    for step in (0, 3):
        _set_grads(pb, _grads(step), offset_view=False)
        torch.nn.utils.clip_grad_norm_([p for p in pb if p.grad is not None], max_norm)
        ob.step()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert rel_err(a, b) < 2e-6, i


# ---- 6. p.grad keeps the unclipped gradient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip_type,value", [("norm", None), ("value", 0.5)])
def test_grad_is_untouched(clip_type, value):
    value = 0.3 * _norm64(_grads(0)) if value is None else value
    pa, oa = _make("adam", True)
    clip = _clipper(oa, clip_type, value)
    _set_grads(pa, _grads(0))
    copies = [p.grad.clone() for p in pa]
    before = [p.detach().clone() for p in pa]
    clip.prepare(); oa.step()
    for p, c, b in zip(pa, copies, before):
        assert torch.equal(p.grad, c)
        assert not torch.equal(p, b)


# ---- 7. bit reproducibility ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_bit_reproducible(kind):
    max_norm = 0.3 * _norm64(_grads(0))
    p1, o1, _, _, r1 = _run_fused(kind, "norm", max_norm, 1)
    p2, o2, _, _, r2 = _run_fused(kind, "norm", max_norm, 1)
    assert torch.equal(r1[0].view(torch.int32), r2[0].view(torch.int32))
    for a, b in zip(p1, p2):
        assert torch.equal(a, b)
    for a, b in zip(_state_tensors(o1, p1), _state_tensors(o2, p2)):
        assert torch.equal(a, b)


# ---- 8. one norm over all optimizers, through the Trainer ---------------------------------------------------------------------------
def _vq_trainer(out_dir, clip_value=None, nbatches=1):
    """Trainer on PR-DVQVAE2 with seeded weights (4 frames per step); clipping enabled iff clip_value is given."""
    import seeded
    from util_models import vqvae_cfg
    from lvt_amd.engine.trainer import Trainer
    from lvt_amd.modeling import build_model
    cfg = vqvae_cfg(DEV)
    cfg.OUTPUT_DIR = str(out_dir)
    cfg.SOLVER.CHECKPOINT_PERIOD = 10 ** 6
    if clip_value is not None:
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = clip_value
    torch.manual_seed(11)
    model = build_model(cfg)
    model.encoder.load_state_dict(seeded.seeded_params(seeded.VQVAE_ENCODER_SHAPES, 11, "enc."))
    model.generator.load_state_dict(seeded.seeded_params(seeded.VQVAE_DECODER_SHAPES, 11, "dec."))
    model.codebook.load_state_dict(seeded.seeded_codebook_state(11, scale=0.05))
    x = seeded.seeded_input("gradclip", (4, 3, 64, 64), 12)
    batch = [{"image": x[i].numpy()} for i in range(4)]
    return Trainer(cfg, model, iter([batch] * nbatches), log_period=10 ** 6), batch


def test_trainer_clips_one_norm_over_all_optimizers(tmp_path):
    from lvt_amd.utils.events import EventStorage
    tb, batch = _vq_trainer(tmp_path)
    assert tb.clipper is None
    assert len(tb.optimizers) == 2                       # netE and netG: the norm has to span both
    with EventStorage(0):
        sum(tb.model(batch, mode="supervised").values()).backward()
    params_b = list(tb.model.encoder.parameters()) + list(tb.model.generator.parameters())
    norm = math.sqrt(sum(float((p.grad.double().cpu() ** 2).sum()) for p in params_b))
    c = 0.5 * norm
    coef = c / (norm + 1e-6)
    with torch.no_grad():
        for p in params_b:
            p.grad.mul_(coef)
    for item in tb.optimizers:
        item["optimizer"].step()

    ta, _ = _vq_trainer(tmp_path, clip_value=c)
    assert ta.clipper is not None and len(ta.clipper.optimizers) == 2
    with EventStorage(0):
        ta.run_step()
    params_a = list(ta.model.encoder.parameters()) + list(ta.model.generator.parameters())
    got = float(ta.clipper.norm)
    print("trainer grad norm %.9g, fp64 %.9g, coef %.6f" % (got, norm, float(ta.clipper.coef)))
    assert abs(got - norm) <= 1e-5 * norm
    assert abs(float(ta.clipper.coef) - 0.5) < 1e-4
    assert len(params_a) == len(params_b) > 0
    for i, (a, b) in enumerate(zip(params_a, params_b)):
        assert rel_err(a, b) < 2e-6, i


def test_trainer_skips_a_poisoned_step_and_logs_it(tmp_path, caplog):
    """A NaN in ONE gradient of the encoder: neither optimizer touches its parameters; the next iteration trains, and the log
    line carries the gradient norm and the skip counter."""
    import logging
    from lvt_amd.utils.events import EventStorage
    ta, _ = _vq_trainer(tmp_path, clip_value=1e-3, nbatches=2)
    params = list(ta.model.encoder.parameters()) + list(ta.model.generator.parameters())
    poison = [True]
    ta.model.encoder.layers[0].weight.register_hook(lambda g: g * float("nan") if poison[0] else g)
    before = [p.detach().clone() for p in params]
    with EventStorage(0):
        ta.run_step()
    assert int(ta.clipper.skipped) == 1 and int(ta.clipper.skip) == 1
    for a, b in zip(params, before):
        assert torch.equal(a, b)
    poison[0] = False
    ta.start_iter = 1
    with caplog.at_level(logging.INFO, logger="lvt_amd"):
        ta.train(max_iter=2)
    assert int(ta.clipper.skipped) == 1 and int(ta.clipper.skip) == 0 and 0.0 < float(ta.clipper.coef) < 1.0
    assert all(bool(torch.isfinite(a).all()) for a in params)
    assert not torch.equal(params[0], before[0]) and not torch.equal(params[-1], before[-1])
    assert sum(int(not torch.equal(a, b)) for a, b in zip(params, before)) > 0.9 * len(params)
    line =[r.getMessage() for r in caplog.records if "grad_norm" in r.getMessage()]
    assert len(line) == 1 and "skipped_steps: 1.00000" in line[0], caplog.text


# ---- 9. under an active gradient reducer ----------------------------------------------------------------------------------------
def _reducer_worker(port, ret):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from test_gpu_dp import _vt_batches, _vt_cfg
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        from lvt_amd.engine.grad_reducer import BucketedGradReducer
        from lvt_amd.modeling import build_model
        from lvt_amd.solver.clip import GradClipper
        from lvt_amd.utils.events import EventStorage
        cfg = _vt_cfg(2)
        batch = next(_vt_batches(cfg, [0], 2, 1))

        def one_step(reducer, max_norm):
            torch.manual_seed(5)
            model = build_model(cfg)
            model.train()
            optimizers, _ = model.configure_optimizers_and_checkpointers()
            views = 0
            if reducer:
                model._reducers = [BucketedGradReducer(model.model.parameters(), bucket_bytes=4 << 20, reduce_single_rank=True)]
            with EventStorage(0):
                model(batch, mode="supervised")["loss_cross_entropy"].backward()
            model.finish_gradient_sync()
            if reducer:
                red = model._reducers[0]
                views = sum(int(p.grad is not None and p.grad.data_ptr() == red._slot[p][1].data_ptr()) for p in red.params)
            grads = [p.grad for p in model.model.parameters() if p.grad is not None]
            norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
            clip = GradClipper([o["optimizer"] for o in optimizers], "norm", max_norm or 0.5 * norm, 2.0)
            clip.prepare()
            for o in optimizers:
                o["optimizer"].step()
            torch.cuda.synchronize()
            out = {n: p.detach().clone() for n, p in model.model.named_parameters()}
            for r in model._reducers:
                r.remove()
            return out, norm, float(clip.norm), float(clip.coef), views, len(grads)

        plain, norm, norm_p, coef_p, _, n = one_step(False, None)
        reduced, _, norm_r, coef_r, views, _ = one_step(True, 0.5 * norm)
        worst = max(rel_err(reduced[k], plain[k]) for k in plain)
        ret["out"] = (worst, norm, norm_p, norm_r, coef_p, coef_r, views, n)
    finally:
        dist.destroy_process_group()


def test_clipped_step_under_active_reducer():
    """One clipped DSFVT step with the gradients living in the buckets of an active reducer (one-rank `nccl` group, as
    test_reducer_on_rccl_backend_single_rank drives it) equals the same step without a reducer."""
    from test_gpu_dp import _free_port
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    p = ctx.Process(target=_reducer_worker, args=(_free_port(), ret))
    p.start()
    p.join(300)
    if p.is_alive():                               # a hung child fails the test once; it is not waited for or retried
        p.kill()
        p.join()
    assert p.exitcode == 0
    worst, norm, norm_p, norm_r, coef_p, coef_r, views, n = ret["out"]
    print("worst %.3g norm %.9g / %.9g / %.9g coef %.6f / %.6f, %d of %d gradients in buckets" %
          (worst, norm, norm_p, norm_r, coef_p, coef_r, views, n))
    assert views > 0.9 * n                         # the norm pass and the step read the bucket slots
    assert coef_p < 1.0 and coef_r < 1.0
    assert abs(norm_r - norm) <= 1e-5 * norm
    assert worst < 2e-6
