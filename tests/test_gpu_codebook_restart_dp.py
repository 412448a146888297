"""Codebook restart across ranks: two ranks share cuda:0 over gloo (as tests/test_gpu_norm_dp.py), each quantising its half of
a z, against one process on the whole z.  The quantiser alone, so no encoder index flips enter."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import rel_err

pytestmark = pytest.mark.gpu
NUM, K, D = 2, 64, 16
P = 4
NFRAMES = K + 4                  # R = 4 K + 16 rows, 2 K + 8 per rank
PASSES = 2
SEED = 9


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


def _inputs():
    """(z per pass, [(w, rs)] per codebook): a quarter of the codes 1e3 away with running_size 0, the others running_size 10."""
    g = torch.Generator()
    g.manual_seed(77)
    zs = [torch.randn(NFRAMES, 1, 2, 2, NUM * D, generator=g) for _ in range(PASSES)]
    state = []
    for _ in range(NUM):
        w = torch.randn(K, D, generator=g)
        rs = torch.full((K,), 10.0)
        w[0::4] += 1e3
        rs[0::4] = 0.0
        state.append((w, rs))
    return zs, state


def _run(lo, hi):
    """PASSES train passes of a restart-enabled quantiser on frames [lo, hi) of every z -> its state on the CPU."""
    from lvt_amd.modeling.vq import DVQEmbedding
    zs, state = _inputs()
    q = DVQEmbedding(NUM, K, NUM * D, True).to("cuda")
    q.enable_restart(1.0, SEED)
    q.train()
    with torch.no_grad():
        for v, (w, rs) in zip(q.ve, state):
            v.embedding.weight.data.copy_(w)
            v.running_size.copy_(rs)
            v.running_sum.copy_(w * rs[:, None])
    passes = []
    for z in zs:
        q.straight_through_cl(z[lo:hi].to("cuda").contiguous())
        idx = q.last_indices.cpu()                                         # (of the rows this process saw)
        passes.append({"w": torch.stack([v.embedding.weight.detach().cpu() for v in q.ve]),
                       "rs": torch.stack([v.running_size.cpu() for v in q.ve]),
                       "rsum": torch.stack([v.running_sum.cpu() for v in q.ve]),
                       "health": q.restart_health.cpu().clone(),
                       "counts": torch.stack([torch.bincount(idx[:, i].reshape(-1), minlength=K) for i in range(NUM)])})
    return {"passes": passes, "total": q.restart_total.cpu().clone(), "pass": int(q.restart_pass)}


def _worker(rank, world, port, ret):
    _paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lvt_amd.modeling.vq import vq_embedding as M
        calls = [0]
        real = M.all_reduce_sum_async_

        def counted(t, group=None):
            calls[0] += 1
            return real(t, group)
        M.all_reduce_sum_async_ = counted
        half = NFRAMES // world
        out = _run(rank * half, (rank + 1) * half)
        out["collectives"] = calls[0]
        ret[rank] = out
    finally:
        dist.destroy_process_group()


def test_two_ranks_restart_the_codes_one_process_restarts():
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
    one = _run(0, NFRAMES)
    assert a["collectives"] == b["collectives"] == PASSES                  # ONE collective per pass: statistics and candidates
    assert a["pass"] == b["pass"] == one["pass"] == PASSES
    assert torch.equal(a["total"], b["total"]) and torch.equal(a["total"], one["total"])
    nfresh = 0
    for pa, pb, p1 in zip(a["passes"], b["passes"], one["passes"]):
        for key in ("w", "rs", "rsum", "health"):
            assert torch.equal(pa[key], pb[key]), key                      # the ranks stay bit-identical
        assert torch.equal(pa["health"][:, 1:], p1["health"][:, 1:])       # dead, restarted: exact
        assert rel_err(pa["health"][:, 0], p1["health"][:, 0]) < 1e-5
        assert torch.equal(pa["counts"] + pb["counts"], p1["counts"])
        # codes this pass restarted won no row and hold exactly the threshold in running_size (an unused code that was not
        # restarted holds 0.99 of a value that is not 1 / 0.99 here): the same rows, copied -- bit-equal across the two runs
        fresh = (p1["counts"] == 0) & (p1["rs"] == 1.0)
        assert torch.equal(fresh.sum(1).float(), p1["health"][:, 2])
        assert torch.equal(fresh, (p1["counts"] == 0) & (pa["rs"] == 1.0))
        assert torch.equal(pa["w"][fresh], p1["w"][fresh]) and torch.equal(pa["rsum"][fresh], p1["rsum"][fresh])
        for key in ("w", "rs", "rsum"):
            assert rel_err(pa[key][~fresh], p1[key][~fresh]) < 1e-5, key
        nfresh += int(fresh.sum())
    assert nfresh == int(one["total"].sum()) >= NUM * K // 4               # (every far code in the first pass)
