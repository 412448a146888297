"""SyncBN (the reference's NaiveSyncBatchNorm) across ranks: two ranks share cuda:0 over gloo (as tests/test_gpu_dp.py),
each with half of the batch, against one process running BN on the whole batch; and SyncBN at world size 1 against BN."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import rel_err

pytestmark = pytest.mark.gpu
NFRAMES = 8
SCALE = 0.2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _paths():
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _frames(lo, hi):
    import seeded
    return [{"image": seeded.seeded_input("g26dp.f%d" % i, (3, 64, 64), 26).numpy()} for i in range(lo, hi)]


def _step(model, data):
    """One supervised forward + backward; then a no-grad train-mode encoder pass (batch statistics) for the outputs."""
    from lvt_amd.utils.events import EventStorage
    with EventStorage(0):
        losses = model(data, mode="supervised")
    sum(losses.values()).backward()
    model.finish_gradient_sync()
    buffers = {n: b.detach().cpu().clone() for n, b in model.named_buffers() if "layers" in n}
    x = torch.stack([torch.from_numpy(d["image"]) for d in data]).to(model.device)
    with torch.no_grad():
        z = model.encoder(model.normalizer(x)).cpu()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().clone() for n, p in list(model.encoder.named_parameters()) +
             [("g." + n, p) for n, p in model.generator.named_parameters()] if p.grad is not None}
    return {"loss": {k: float(v.detach()) for k, v in losses.items()}, "buffers": buffers, "z": z, "grads": grads}


def _worker(rank, world, port, ret):
    _paths()
    from test_gpu_norm import norm_model
    from lvt_amd.hip import binding as L
    L.set_math_mode("f32")               # both sides on plain fp32 MFMA: differences are summation order only
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model, _ = norm_model("SyncBN", SCALE)
        model.train()
        model.wrap_parallel(device_ids=[0], broadcast_buffers=False)
        half = NFRAMES // world
        ret[rank] = _step(model, _frames(rank * half, (rank + 1) * half))
    finally:
        dist.destroy_process_group()


def _rows(name):
    """Rows (N*H*W) that the norm layer `name` of a 64x64 frame batch normalises over."""
    hw = 32 * 32 if name in ("encoder.layers.0.1", "generator.layers.4.1") else 16 * 16
    return NFRAMES * hw


@pytest.fixture
def f32_math():
    from lvt_amd.hip import binding as L
    before = L.get_math_mode()
    L.set_math_mode("f32")
    yield
    L.set_math_mode(before)


def test_syncbn_two_ranks_equal_bn_on_the_whole_batch(f32_math):
    """In f32 arithmetic on both sides, so that the bounds are fp32-class: a cross-rank backward that missed the all-reduce
    of (sum g, sum g xhat), or a forward that missed the statistics', is off by percents in the BN parameters' gradients."""
    from test_gpu_norm import norm_model
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    a, b = ret[0], ret[1]
    model, _ = norm_model("BN", SCALE)
    rv0 = {n: t.detach().cpu().clone() for n, t in model.named_buffers() if n.endswith("running_var")}
    model.train()
    one = _step(model, _frames(0, NFRAMES))
    # forward outputs: the two halves are the whole batch's
    assert rel_err(torch.cat([a["z"], b["z"]]), one["z"]) < 1e-5
    for k in ("loss_reconstruction", "loss_commitment"):
        mean = 0.5 * (a["loss"][k] + b["loss"][k])
        assert abs(mean - one["loss"][k]) < 1e-5 * abs(one["loss"][k]), k
    # averaged parameter gradients (gamma and beta through the bucketed reducer like every parameter)
    assert a["grads"].keys() == one["grads"].keys()
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
        assert rel_err(a["grads"][k], one["grads"][k]) < 1e-4, k
    for n, t in one["buffers"].items():
        for r in (a, b):
            got = r["buffers"][n]
            if n.endswith("num_batches_tracked"):
                assert int(got) == 0 and int(t) == 1, n           # not counted by the cross-rank form
            elif n.endswith("running_mean"):
                assert rel_err(got, t) < 1e-5, n
            elif n.endswith("running_var"):
                # BN stores 0.9 rv0 + 0.1 var * n / (n - 1); SyncBN the biased var
                nrows = _rows(n.rsplit(".", 1)[0])
                var_u = (t.double() - 0.9 * rv0[n].double()) / 0.1
                want = 0.9 * rv0[n].double() + 0.1 * var_u * (nrows - 1) / nrows
                assert rel_err(got, want) < 1e-5, n


def test_syncbn_world_size_one_is_bn_bit_for_bit():
    from test_gpu_norm import norm_model
    out = {}
    for norm in ("BN", "SyncBN"):
        model, _ = norm_model(norm, SCALE)
        model.train()
        out[norm] = _step(model, _frames(0, 4))
    a, b = out["BN"], out["SyncBN"]
    assert a["loss"] == b["loss"]
    assert torch.equal(a["z"], b["z"])
    for part in ("grads", "buffers"):
        assert a[part].keys() == b[part].keys()
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), k
