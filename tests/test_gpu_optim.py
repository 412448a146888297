"""Fused multi-tensor Adam / RMSprop vs torch.optim on the GPU (same gradients, 5 steps)."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(70, 33), (5,), (3, 4, 5, 6), (100000,), (1,)] + [(17, 3)] * 70      # > 64 tensors, ragged sizes
    return [torch.randn(*s, generator=g) for s in shapes]


@pytest.mark.parametrize("kind", ["adam", "rmsprop", "rmsprop_nomom"])
def test_fused_matches_torch(kind):
    from lvt_amd.solver.fused import FusedAdam, FusedRMSprop
    dev = "cuda:0"
    a = [torch.nn.Parameter(p.clone().to(dev)) for p in _params(0)]
    b = [torch.nn.Parameter(p.clone().to(dev)) for p in _params(0)]
    groups = lambda ps: [{"params": [p], "lr": 1e-2 * (1 + i % 3), "weight_decay": 0.0 if i % 2 else 1e-3}
                         for i, p in enumerate(ps)]      # noqa: E731  (one group per parameter, like the reference)
    if kind == "adam":
        oa, ob = FusedAdam(groups(a), 1e-2, betas=(0.9, 0.9)), torch.optim.Adam(groups(b), 1e-2, betas=(0.9, 0.9))
    else:
        mom = 0.9 if kind == "rmsprop" else 0.0
        oa = FusedRMSprop(groups(a), 1e-2, alpha=0.95, momentum=mom)
        ob = torch.optim.RMSprop(groups(b), 1e-2, alpha=0.95, momentum=mom)
    for step in range(5):
        for i, (pa, pb) in enumerate(zip(a, b)):
            g = torch.randn(pa.shape, generator=torch.Generator().manual_seed(100 * step + i)).to(dev)
            if i == 4 and step % 2:          # a parameter that sometimes receives no gradient
                pa.grad = pb.grad = None
                continue
            pa.grad, pb.grad = g.clone(), g.clone()
        oa.step(); ob.step()
    for pa, pb in zip(a, b):
        assert rel_err(pa, pb) < 2e-6
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert set(sa[0].keys()) == set(sb[0].keys())


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_two_keys_and_two_step_counts_in_one_optimizer(kind):
    """Launch grouping and order: one optimizer whose groups carry two hyper-parameter keys, 70 ragged tensors each (two launches
    per batch), half of each key's tensors joining at step 3, so that every `step()` from there on launches two step counts
    times two keys.  Against torch built with the same groups, and bit for bit against a second run."""
    from lvt_amd.solver.fused import FusedAdam, FusedRMSprop
    dev = "cuda:0"
    if kind == "adam":
        keys, fused, ref = [dict(betas=(0.9, 0.9), eps=1e-8), dict(betas=(0.8, 0.95), eps=1e-6)], FusedAdam, torch.optim.Adam
    else:
        keys, fused, ref = [dict(alpha=0.95, momentum=0.9), dict(alpha=0.9, momentum=0.0)], FusedRMSprop, torch.optim.RMSprop
    # parameter i: tensor i // 2 of key i % 2 (the keys alternate, one group per parameter, like the reference)
    init = [t for pair in zip(_params(1)[:70], _params(2)[:70]) for t in pair]
    late = [(i // 2) % 2 == 1 for i in range(len(init))]
    grads = [[torch.randn(t.shape, generator=torch.Generator().manual_seed(1000 * step + i)).to(dev) for i, t in enumerate(init)]
             for step in range(5)]

    def run(cls):
        ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
        opt = cls([dict(params=[p], lr=1e-2 * (1 + i % 3), weight_decay=0.0 if (i // 2) % 2 else 1e-3, **keys[i % 2])
                   for i, p in enumerate(ps)], 1e-2)
        for step in range(5):
            for i, p in enumerate(ps):
                p.grad = None if late[i] and step < 2 else grads[step][i].clone()
            opt.step()
        return ps, opt

    (a, oa), (a2, oa2), (b, _) = run(fused), run(fused), run(ref)
    assert sorted(int(oa.state[p]["step"]) for p in a[:4]) == [3, 3, 5, 5]
    for pa, pb in zip(a, b):
        assert rel_err(pa, pb) < 2e-6
    for pa, pa2 in zip(a, a2):
        assert torch.equal(pa, pa2)
        sa, sa2 = oa.state[pa], oa2.state[pa2]
        assert set(sa) == set(sa2)
        for k, v in sa.items():
            assert torch.equal(v, sa2[k]) if torch.is_tensor(v) else v == sa2[k], k
