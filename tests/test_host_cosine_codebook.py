"""Host side of the cosine codebook lookup (MODEL.CODEBOOK.COSINE): the config key, the model's refusals, state-dict
keys and the unit-row init, the rule of lvt_amd/modeling/vq/cosine.py in float64 against torch autograd, the share of rows the
margin rule leaves out on the unit sphere (the 2 % the GPU tests allow), and the C-ABI table."""
import glob
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_err


def _cfg(num=4, cosine=None, **kw):
    from lvt_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/vqvae/PR-DVQVAE2.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.CODEBOOK.NUM = num
    if cosine is not None:
        cfg.MODEL.CODEBOOK.COSINE = cosine
    for k, v in kw.items():
        cfg.MODEL.CODEBOOK[k] = v
    return cfg


def test_default_and_shipped_yamls():
    from lvt_amd.config import get_cfg
    assert get_cfg().MODEL.CODEBOOK.COSINE is False
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*", "*.yaml"))):
        cfg = get_cfg()
        cfg.merge_from_file(path)
        assert cfg.MODEL.CODEBOOK.COSINE is False, path
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.CODEBOOK.COSINE", "True"])
    assert cfg.MODEL.CODEBOOK.COSINE is True


@pytest.mark.parametrize("num", [4, 1])
def test_state_dict_keys_shapes_and_unit_rows(num):
    from lvt_amd.modeling import build_model
    torch.manual_seed(0)
    off = build_model(_cfg(num))                        # the key left at its default
    off2 = build_model(_cfg(num, cosine=False))
    on = build_model(_cfg(num, cosine=True))
    assert off.codebook.cosine is False and off2.codebook.cosine is False and on.codebook.cosine is True
    # off: the module tree and the state dict the quantiser has always had (the reference's names)
    pre = ["ve.%d." % i for i in range(num)] if num > 1 else [""]
    want = [p + k for p in pre for k in ("running_size", "running_sum", "embedding.weight")]
    assert sorted(off.codebook.state_dict().keys()) == sorted(want)
    tree = [n for n, _ in off.named_modules()]
    assert tree == [n for n, _ in off2.named_modules()] == [n for n, _ in on.named_modules()]
    sd_off, sd_on = off.state_dict(), on.state_dict()
    assert list(sd_off.keys()) == list(sd_on.keys()) == list(off2.state_dict().keys())
    assert [tuple(v.shape) for v in sd_off.values()] == [tuple(v.shape) for v in sd_on.values()]
    assert [n for n, _ in off.named_buffers()] == [n for n, _ in on.named_buffers()]
    K = on.cfg.MODEL.CODEBOOK.SIZE
    for k, v in on.codebook.state_dict().items():
        if k.endswith("embedding.weight") or k.endswith("running_sum"):
            assert float((v.double().norm(dim=-1) - 1).abs().max()) <= 1e-6, k
        else:
            assert bool((v == 0).all()), k
    for k, v in off.codebook.state_dict().items():
        if k.endswith("embedding.weight"):
            assert float(v.abs().max()) <= 1.0 / K, k          # the reference's uniform(-1/K, 1/K) init, untouched
    w = [v for k, v in on.codebook.state_dict().items() if k.endswith("embedding.weight")]
    s = [v for k, v in on.codebook.state_dict().items() if k.endswith("running_sum")]
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(w, s))
    # checkpoints of the two kinds load into each other strictly (telling them apart is the user's business)
    on.codebook.load_state_dict(off.codebook.state_dict())


@pytest.mark.parametrize("num", [4, 1])
def test_refusals(num):
    from lvt_amd.modeling import build_model
    from lvt_amd.modeling.vq import DVQEmbedding, SingleVQEmbedding
    with pytest.raises(ValueError) as e:
        build_model(_cfg(num, cosine=True, EMA=False))
    assert "MODEL.CODEBOOK.COSINE" in str(e.value) and "MODEL.CODEBOOK.EMA" in str(e.value)
    assert build_model(_cfg(num, cosine=False, EMA=False)).codebook.cosine is False
    with pytest.raises(ValueError):
        DVQEmbedding(2, 64, 32, False, cosine=True)
    with pytest.raises(ValueError):
        SingleVQEmbedding(64, 128, False, cosine=True)
    with pytest.raises(NotImplementedError) as e:
        SingleVQEmbedding(64, 2048, True, cosine=True)
    assert "MODEL.CODEBOOK.COSINE" in str(e.value)
    assert SingleVQEmbedding(64, 2048, True).cosine is False                    # refused under COSINE only
    assert SingleVQEmbedding(64, 1024, True, cosine=True).cosine is True
    for d in (16, 48, 256):
        assert DVQEmbedding(2, 64, 2 * d, True, cosine=True).cosine is True


def test_normalise_cl_is_the_identity_when_off():
    from lvt_amd.modeling.vq import DVQEmbedding, SingleVQEmbedding
    z = torch.randn(2, 1, 4, 4, 128)
    for q in (DVQEmbedding(2, 64, 128, True), SingleVQEmbedding(64, 128, True)):
        assert q.normalise_cl(z) is z                                           # no launch: a CPU tensor would be refused


# ---- the rule (lvt_amd/modeling/vq/cosine.py) in float64 ---------------------------------------------------------------------
def _rows(rows, G, d, seed):
    return torch.randn(rows, G * d, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("G,d", [(4, 64), (3, 48), (1, 256)])
def test_normalise_is_idempotent_and_unit(G, d):
    from lvt_amd.modeling.vq import cosine as C
    z = _rows(50, G, d, 1) * 3.0
    u = C.normalise(z, d)
    assert float((u.view(50, G, d).norm(dim=-1) - 1).abs().max()) < 1e-14
    assert rel_err(C.normalise(u, d), u) < 1e-15
    assert C.normalise(z.float(), d).dtype == torch.float32                  # (works in the dtype it is handed)
    assert rel_err(C.inverse_norm(z, d), 1.0 / z.view(50, G, d).norm(dim=-1)) < 1e-15


@pytest.mark.parametrize("G,d", [(4, 64), (3, 48), (1, 256)])
def test_closed_form_backward_equals_autograd(G, d):
    """Random rows, a zero group and a group of norm 1e-13 (below eps: clamped), each in a tensor of its own -- the clamped
    gradients are g * 1e12 and would swamp a max-relative error."""
    from lvt_amd.modeling.vq import cosine as C
    zero = _rows(3, G, d, 3)
    zero[1, :d] = 0
    tiny = _rows(3, G, d, 4)
    tiny[2, -d:] = F.normalize(tiny[2, -d:], dim=0) * 1e-13
    for z in (_rows(40, G, d, 2), zero, tiny, zero[1:2, :d], tiny[2:3, -d:]):
        g = torch.randn(z.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        leaf = z.clone().requires_grad_(True)
        F.normalize(leaf.view(z.shape[0], -1, d), dim=-1, eps=1e-12).flatten(-2).backward(g)
        mine = C.normalise_backward(g, z, d)
        assert torch.isfinite(mine).all()
        assert rel_err(mine, leaf.grad) < 1e-12
        # the same through cosine.normalise itself
        leaf2 = z.clone().requires_grad_(True)
        C.normalise(leaf2, d).backward(g)
        assert rel_err(leaf2.grad, leaf.grad) < 1e-12
    # what the clamped branch is: r g with r = 1 / eps
    g = torch.ones(1, d, dtype=torch.float64)
    assert torch.equal(C.normalise_backward(g, torch.zeros(1, d, dtype=torch.float64), d), g / 1e-12)


def test_nearest_breaks_ties_to_the_lowest_code():
    from lvt_amd.modeling.vq import cosine as C
    e = F.normalize(_rows(64, 1, 16, 6), dim=-1)
    e[40] = e[7]
    e[63] = e[7]
    idx = C.nearest(e.clone(), e)
    want = torch.arange(64)
    want[40] = want[63] = 7
    assert torch.equal(idx, want)


@pytest.mark.parametrize("num,K,d", [(4, 64, 64), (1, 128, 256), (2, 64, 48)])
def test_reference_step_keeps_unit_rows(num, K, d):
    """normalise, search, EMA by the reference's formula, normalise codes: three passes in float64."""
    from lvt_amd.modeling.vq import cosine as C
    gen = torch.Generator().manual_seed(num * K + d)
    w = torch.stack([C.init_((torch.rand(K, d, dtype=torch.float64, generator=gen) * 2 - 1) / K) for _ in range(num)])
    rs, rsum = torch.zeros(num, K, dtype=torch.float64), w.clone()
    for it in range(3):
        z = torch.randn(300, num * d, dtype=torch.float64, generator=gen) * 2.0
        out = C.step(w, rs, rsum, z, beta=0.25)
        u = out["u"]
        assert rel_err(u, F.normalize(z.view(300, num, d), dim=-1).flatten(-2)) < 1e-15
        for i in range(num):
            ui = u[:, d * i:d * (i + 1)]
            dist = ((ui[:, None, :] - w[i][None]) ** 2).sum(-1)
            assert torch.equal(out["idx"][:, i], dist.argmin(1)), (it, i)
            assert torch.equal(out["z_q_st"][:, d * i:d * (i + 1)], w[i][out["idx"][:, i]])        # the PRE-update codebook
            assert torch.equal(out["z_q_bar"][:, d * i:d * (i + 1)], out["weight"][i][out["idx"][:, i]])
            # the reference's EMA (vq_embedding.py:46-59) on the rows u, then unit rows; the buffers are not normalised
            cnt = torch.bincount(out["idx"][:, i], minlength=K).double()
            tot = torch.zeros(K, d, dtype=torch.float64).index_add_(0, out["idx"][:, i], ui)
            assert rel_err(out["running_size"][i], rs[i] * 0.99 + 0.01 * cnt) < 1e-15
            assert rel_err(out["running_sum"][i], rsum[i] * 0.99 + 0.01 * tot) < 1e-15
            n = out["running_size"][i].sum()
            raw = out["running_sum"][i] / ((out["running_size"][i] + 1e-5) / (n + K * 1e-5) * n).unsqueeze(1)
            assert rel_err(out["weight"][i], F.normalize(raw, dim=-1)) < 1e-15
        assert float((out["weight"].norm(dim=-1) - 1).abs().max()) < 1e-14
        assert float((out["running_sum"].norm(dim=-1) - 1).abs().max()) > 1e-3
        want = 0.25 * ((u - out["z_q_bar"]) ** 2).mean()
        assert abs(float(out["loss_commitment"]) - float(want)) < 1e-15
        assert float(out["loss_commitment"]) <= 0.25 * 4.0 / d + 1e-12          # bounded: |u - e|^2 <= 4 per sub-vector
        w, rs, rsum = out["weight"], out["running_size"], out["running_sum"]


def test_step_gradient_passes_straight_through_and_commitment_to_z():
    from lvt_amd.modeling.vq import cosine as C
    gen = torch.Generator().manual_seed(9)
    num, K, d = 2, 64, 32
    w = F.normalize(torch.randn(num, K, d, dtype=torch.float64, generator=gen), dim=-1)
    z = torch.randn(20, num * d, dtype=torch.float64, generator=gen).requires_grad_(True)
    g_st = torch.randn(20, num * d, dtype=torch.float64, generator=gen)
    out = C.step(w, torch.ones(num, K, dtype=torch.float64), w.clone(), z, beta=0.5)
    ((out["z_q_st"] * g_st).sum() + out["loss_commitment"]).backward()
    u = out["u"].detach()
    g_u = g_st + 0.5 * 2.0 * (u - out["z_q_bar"]) / u.numel()
    assert rel_err(z.grad, C.normalise_backward(g_u, z.detach(), d)) < 1e-12


@pytest.mark.parametrize("K,d", [(64, 16), (512, 64), (2048, 64), (512, 256), (2048, 16), (128, 48)])
def test_margin_rule_leaves_out_few_rows_on_the_unit_sphere(K, d):
    """The headroom of the 2 % that the GPU tests allow util_models.margin_ok(rel=1e-4) to leave out: 8192 normalised normal rows
    against normalised normal codes.  Measured with this seed: 0.073 % (64, 16), 0.183 % (512, 64), 0.293 % (2048, 64),
    0.635 % (512, 256), 0.269 % (2048, 16), 0.256 % (128, 48).  (512, 256) is the tightest: eight other seeds gave 0.38 % to
    0.61 %, mean 0.51 % -- a quarter of the bound asserted here and on the device."""
    from util_models import margin_ok
    gen = torch.Generator().manual_seed(K + d)
    u = F.normalize(torch.randn(8192, d, generator=gen), dim=-1)
    e = F.normalize(torch.randn(K, d, generator=gen), dim=-1)
    out = 1.0 - float(margin_ok(u, e, rel=1e-4).float().mean())
    print("margin rule leaves out %.3f %% at K=%d d=%d" % (100 * out, K, d))
    assert out <= 0.02


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_table_and_argument_validation():
    from lvt_amd.hip import binding as L
    header = open(os.path.join(ROOT, "include", "lvt_hip.h")).read()
    assert L.ABI_VERSION == 680 == L.lib().lvt_version()
    new = {"lvt_l2norm_groups_fwd", "lvt_l2norm_groups_bwd"}
    assert new <= set(L.declared_symbols())
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in text, name
    lib = L.lib()
    p = 4096                                                               # a non-null, 16-byte aligned address
    ok = dict(x=p, rows=8, G=4, d=64, eps=1e-12, y=p, inv=p, am=None)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.lvt_l2norm_groups_fwd(a["x"], a["rows"], a["G"], a["d"], a["eps"], a["y"], a["inv"], a["am"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.lvt_l2norm_groups_bwd(a["x"], a["y"], a["inv"], a["rows"], a["G"], a["d"], a["eps"], a["x"], a["am"], None)
    bad_geometry = (dict(rows=0), dict(rows=-3), dict(G=0), dict(d=0), dict(d=8), dict(d=24), dict(d=1040), dict(d=2048, G=1),
                    dict(G=5, d=1024), dict(G=65, d=64), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")),
                    dict(eps=float("nan")))
    for bad in bad_geometry + (dict(x=None), dict(y=None), dict(x=p + 4), dict(y=p + 8), dict(inv=p + 2), dict(am=p + 1)):
        assert fwd(**bad) == -1, bad
        assert b"lvt_l2norm_groups_fwd" in lib.lvt_last_error(), bad
    for bad in bad_geometry + (dict(x=None), dict(y=None), dict(inv=None), dict(x=p + 4), dict(y=p + 8), dict(inv=p + 2),
                               dict(am=p + 1)):
        assert bwd(**bad) == -1, bad
        assert b"lvt_l2norm_groups_bwd" in lib.lvt_last_error(), bad


def test_wrappers_refuse_cpu_tensors_and_bad_widths():
    from lvt_amd.hip import binding as L, l2norm
    with pytest.raises(L.LvtError):
        l2norm.l2norm_groups_fwd(torch.zeros(4, 64), 64)
    with pytest.raises(L.LvtError):
        l2norm.l2norm_groups_bwd(torch.zeros(4, 64), torch.zeros(4, 64), torch.zeros(4, 1), 64)
